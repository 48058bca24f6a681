"""The captured DDQN-PER frame without a GPU: ``DDQNLearner.capture()``'s refusals (raised before
anything touches the device), and pbn_ddqn_schedule's declaration, binding and argument checks."""
import ctypes
import os

import pytest
import torch

from pbn_rl_amd import _lib
from pbn_rl_amd.ddqn import DDQNLearner
from tests.test_ddqn_host import StubEnv


def _learner(**kw):
    torch.manual_seed(0)
    args = dict(net_arch=[(8, 8)], total_frames=10, capacity=64, batch_size=16, prioritised=False, fused=False)
    args.update(kw)
    return DDQNLearner(StubEnv(), **args)


def test_capture_needs_graphable():
    lr = _learner()
    assert lr.graphable is False
    with pytest.raises(ValueError, match="graphable=True"):
        lr.capture()
    with pytest.raises(ValueError, match="capture\\(\\) first"):
        lr.run(3)


def test_capture_refuses_the_pytorch_update_and_uniform_replay():
    lr = _learner(graphable=True)
    with pytest.raises(ValueError) as e:
        lr.capture()
    assert "fused: " in str(e.value) and "prioritised: " in str(e.value)
    assert "train_frequency" not in str(e.value) and "per_max_beta" not in str(e.value)
    assert lr.frames == 0 and lr._graph is None


def test_capture_refuses_a_train_frequency_other_than_one():
    lr = _learner(graphable=True, train_frequency=2)
    with pytest.raises(ValueError, match="train_frequency: .*not every 2"):
        lr.capture()


def test_capture_refuses_each_argument_alone():
    """One wrong argument at a time, on a learner whose other attributes say fused and prioritised
    (a CPU stub cannot construct those; the check reads only these attributes)."""
    for attr, value, name in (("fused", None, "fused: "), ("prioritised", False, "prioritised: "),
                              ("train_frequency", 4, "train_frequency: "), ("per_max_beta", 0.9, "per_max_beta: ")):
        lr = _learner(graphable=True)
        lr.fused, lr.prioritised = object(), True
        lr._check_capturable()                      # this one would be taken
        setattr(lr, attr, value)
        with pytest.raises(ValueError) as e:
            lr._check_capturable()
        msg = str(e.value)
        assert name in msg, (attr, msg)
        assert [n for n in ("fused: ", "prioritised: ", "train_frequency: ", "per_max_beta: ") if n in msg] == [name]


def test_eager_frames_are_unchanged_by_graphable():
    a, b = _learner(graphable=False), _learner(graphable=True)
    for _ in range(6):
        ra, da = a.frame()
        rb, db = b.frame()
        assert torch.equal(ra, rb) and torch.equal(da, db)
    assert (a.epsilon, a.beta, a.frames, a.updates, a.syncs) == (b.epsilon, b.beta, b.frames, b.updates, b.syncs)
    assert all(torch.equal(x, y) for x, y in zip(a.q.state_dict().values(), b.q.state_dict().values()))


# ---- the export ------------------------------------------------------------------------------------
def _declared_params(name):
    """The parameter list of ``name``'s declaration in include/pbn_env.h, as the header spells it."""
    assert name in _lib.declared(), f"{name} is not declared in pbn_env.h"
    return list(_lib.declared()[name].ctext)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_schedule_is_declared_and_bound_with_matching_arguments(lib):
    assert "pbn_ddqn_schedule" in _lib.EXPORTS
    params = _declared_params("pbn_ddqn_schedule")
    bound = lib.pbn_ddqn_schedule.argtypes
    assert len(params) == len(bound) == 12
    assert lib.pbn_ddqn_schedule.restype is ctypes.c_int
    for p, t in zip(params, bound):
        if "*" in p:
            assert t is ctypes.c_void_p, p
        elif p.startswith("double"):
            assert t is ctypes.c_double, p
        else:
            assert p.startswith("int64_t") and t is ctypes.c_int64, p
    # the precedent: the exports this one sits beside are bound with their declared counts too
    for name in ("pbn_ddqn_learn", "pbn_dqn_flipmask_from_state", "pbn_replay_advance"):
        assert len(_declared_params(name)) == len(getattr(lib, name).argtypes), name
    assert lib.pbn_abi_version() == 11


def test_schedule_rejects_bad_arguments_before_the_device(lib):
    err = lambda: lib.pbn_last_error().decode()  # noqa: E731
    ok = dict(beta=64, inc=0.05, step=128, base=1, every=4, tp=4096, p=8192, n=1024, ti=16384, i=32768, ni=2048)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.pbn_ddqn_schedule(a["beta"], a["inc"], a["step"], a["base"], a["every"], a["tp"], a["p"], a["n"],
                                     a["ti"], a["i"], a["ni"], None)

    assert call(beta=None) == -22 and "null d_beta or d_step" in err()
    assert call(step=None) == -22 and "null d_beta or d_step" in err()
    assert call(beta=68) == -22 and "8-byte aligned" in err()
    assert call(every=0) == -22 and "target_update >= 1" in err()
    assert call(n=1022) == -22 and "multiples of 4" in err()
    assert call(ni=0) == -22 and "multiples of 4" in err()
    assert call(tp=None) == -22 and "null buffer" in err()
    assert call(i=32772) == -22 and "16-byte aligned" in err()
    assert call(tp=8192 + 2048) == -22 and "overlaps its source" in err()
