"""Host side of the fused BDQ update on a prioritised batch (pbn_bdq_learn_per; no GPU): the entry
is exported and declared, refuses bad arguments before it looks at the net or touches a device,
and FusedBDQUpdate / BDQLearner refuse bad arguments by name."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from pbn_rl_amd import _lib
from pbn_rl_amd.replay import BDQLearner, FusedBDQUpdate

EINVAL = -22
P = 0x10000     # a non-null, 16-byte aligned address: every call below must return before using it


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _learn_per(lib, B=32, K=3, w=P, prio=P):
    """pbn_bdq_learn_per with a null net and fake buffers.  The entry checks its own arguments and
    the shape arguments that need no net first, so a call that gets as far as the net fails there."""
    rc = lib.pbn_bdq_learn_per(None, B, P, 1024, P, P, P, P, K, P, P, P, P, P, P, P, P, P, 1e-4, 0.9, 0.999, 1e-8,
                               0.999, 1.0, 0.01, P, 1 << 30, P, None, w, 1e-5, prio, None, None)
    return rc, lib.pbn_last_error().decode()


def test_entry_is_exported_and_declared(lib):
    assert hasattr(lib, "pbn_bdq_learn_per") and "pbn_bdq_learn_per" in _lib.EXPORTS
    decl = _lib.declared()["pbn_bdq_learn_per"]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r" T pbn_bdq_learn_per$", out, re.M)
    assert decl.restype is ctypes.c_int and len(decl.params) == len(lib.pbn_bdq_learn_per.argtypes) == 34
    assert lib.pbn_abi_version() == 11


@pytest.mark.parametrize("bad,msg", [
    (dict(w=None), "d_weights"), (dict(prio=None), "d_priority"), (dict(w=P + 2), "d_weights"),
    (dict(prio=P + 2), "d_priority"), (dict(B=24), "batch"), (dict(K=8), "n_branches"),
])
def test_entry_rejects_bad_arguments(lib, bad, msg):
    rc, err = _learn_per(lib, **bad)
    assert rc == EINVAL and msg in err, (bad, err)


def test_good_arguments_reach_the_net(lib):
    """With nothing else wrong the call fails at the null net: the rejections above came first."""
    rc, err = _learn_per(lib)
    assert rc == EINVAL and "net" in err, err
    # pbn_bdq_learn keeps its behaviour
    rc = lib.pbn_bdq_learn(None, 32, P, 1024, P, P, P, P, 3, P, P, P, P, P, P, P, P, P, 1e-4, 0.9, 0.999, 1e-8, 0.999,
                           1.0, 0.01, P, 1 << 30, P, None, None, None)
    assert rc == EINVAL and "net" in lib.pbn_last_error().decode()


def test_update_validates_its_weight_arguments():
    """FusedBDQUpdate.update's check of weights / priorities_out (the class itself needs a GPU)."""
    check = FusedBDQUpdate.check_per_args
    B, dev = 32, torch.device("cpu")
    w, p = torch.ones(B), torch.empty(B)
    check(B, dev, None, None)
    check(B, dev, w, p)
    with pytest.raises(ValueError, match="priorities_out"):
        check(B, dev, w, None)
    with pytest.raises(ValueError, match="weights"):
        check(B, dev, None, p)
    for bad in (torch.ones(B, dtype=torch.float64), torch.ones(B + 1), torch.ones(B, 1), torch.ones(2 * B)[::2],
                [1.0] * B):
        with pytest.raises(ValueError, match="^weights"):
            check(B, dev, bad, p)
    for bad in (torch.empty(B, dtype=torch.float16), torch.empty(B - 1), torch.empty(1, B), torch.empty(2 * B)[::2]):
        with pytest.raises(ValueError, match="^priorities_out"):
            check(B, dev, w, bad)
    with pytest.raises(ValueError, match="^weights"):      # host tensors for a device update
        check(B, torch.device("cuda", 0), w, p)


def test_learner_refuses_a_fused_update_without_a_gpu_env():
    for kw in (dict(fused=True), dict(fused=True, prioritised=True)):
        with pytest.raises(ValueError, match="fused update"):
            BDQLearner(None, **kw)
