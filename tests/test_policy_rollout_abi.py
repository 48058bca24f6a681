"""pbn_rollout_dqn in the C-ABI (no GPU needed): the symbol is exported under an unchanged ABI
version, and a null net and the argument errors that need no net are rejected, each with its
reason, before any device call."""
import ctypes
import os
import re
import subprocess

import pytest

from pbn_rl_amd import _lib


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def call(lib, **over):
    a = dict(net=None, seed=0, step=0, env_offset=0, n_envs=32, n_steps=2, mode=_lib.MODE_AUTORESET, state=None,
             target=None, t=None, h0=8, h1=8, image=None, epsilon=0.0, flipmask=None, actions=None, obs=None,
             final_state=None, reward=None, flags=None, updates=None, stream=None)
    a.update(over)
    return lib.pbn_rollout_dqn(*a.values()), lib.pbn_last_error().decode()


def test_rollout_dqn_is_exported_and_the_abi_version_stays(lib):
    assert "pbn_rollout_dqn" in _lib.EXPORTS
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert "pbn_rollout_dqn" in set(re.findall(r" T (\w+)$", out, re.M))
    decl = _lib.declared()["pbn_rollout_dqn"]
    assert hasattr(lib, "pbn_rollout_dqn") and tuple(lib.pbn_rollout_dqn.argtypes) == decl.argtypes
    assert decl.restype is ctypes.c_int and len(decl.params) == 22
    assert lib.pbn_abi_version() == 11


def test_rollout_dqn_rejects_a_null_net(lib):
    assert call(lib) == (-22, "null net")
    assert call(lib, n_steps=0) == (-22, "null net")


@pytest.mark.parametrize("over,msg", [
    (dict(mode=_lib.MODE_AUTORESET | _lib.MODE_RANDOM_ACTIONS), "the policy chooses the actions"),
    (dict(mode=8), "unknown mode bits"),
    (dict(h0=65), "hidden widths must be 1..64"),
    (dict(h1=0), "hidden widths must be 1..64"),
    (dict(n_steps=-1), "n_steps < 0"),
    (dict(n_envs=33), "n_envs and env_offset must be multiples of 32"),
    (dict(n_envs=-32), "n_envs < 0"),
    (dict(env_offset=16), "n_envs and env_offset must be multiples of 32"),
    (dict(n_envs=1 << 30), "n_envs must be below 2^30"),
    (dict(epsilon=float("nan")), "epsilon must be in [0, 1]"),
], ids=lambda v: None if isinstance(v, str) else "-".join(f"{k}={x}" for k, x in v.items()))
def test_rollout_dqn_rejects_with_the_reason(lib, over, msg):
    rc, err = call(lib, **over)
    assert rc == -22 and msg in err, (rc, err)
