"""The per-step output stores of the pipelined rollout kernel (pbn_rollout_pipe): every output
row is written through a buffer descriptor that covers one step's row of one state word, built
once and advanced per step; a null optional output is a descriptor of zero records, and a lane
of an invalid group is dropped by the descriptor's range check instead of an EXEC mask.

What can go wrong there shows at the smallest sizes: one block whose upper half is invalid
(32 envs), a full block (64), an odd group count (96: the last block is half valid), the
peeled first and last iterations and both slot parities (1, 2, 3 steps), every combination of
the optional outputs, and multi-word states (rows of words 1.. are the descriptor moved on).
Every output is compared bit for bit with the CPU oracle, and every output buffer is a view cut
from one arena pre-filled with a canary, with a canary stretch before and after it: a store the
range check should have dropped lands in the next row (caught by the comparison) or, from the
last row, in the canary behind it.  (Within one output the layout [step][word][env] is
contiguous, so there is no room for canaries between the words' rows.)

m47's wide functions are lowered to gates, which the wave kernel runs: it is here as the two-word
network the suite bundles; the two-word instance of the pipelined kernel is reached by the
synthetic 45-node network.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from oracle import oracle
from pbn_rl_amd import _lib
from pbn_rl_amd.attractors import load_attractors
from pbn_rl_amd.network import load_network
from pbn_rl_amd.spec import EnvSpec
from pbn_rl_amd.vector_env import VectorPBNEnv

from .synthetic import random_spec

CANARY = 0xA5
PAD = 256          # canary bytes around every output: more than one block's 64 lanes x 4 bytes
SEED, OFFSET = 977, 64
NETS = ["pbn7", "m47", "pbn70", "synth45"]   # 1, 2 (gates: wave kernel), 3, 2 (pipelined) state words


def make_spec(name):
    kw = dict(perturbation=0.05, horizon=2)   # truncation and autoreset inside three steps
    if name == "synth45":
        return random_spec(45, 23, max_funcs=3, **kw)
    return EnvSpec(load_network(name), load_attractors(name), **kw)


def u32(x: torch.Tensor) -> np.ndarray:
    return x.cpu().numpy().view(np.uint32)


class Arena:
    """Output buffers of an R-step rollout cut from one canary-filled byte tensor."""

    def __init__(self, env, R, keep_obs, keep_final):
        W, n = env.words, env.n_alloc
        shapes = {"flipmask": ((R, W, n), torch.int32), "reward": ((R, n), torch.float32),
                  "flags": ((R, n), torch.uint8)}
        if keep_obs:
            shapes["obs"] = ((R, W, n), torch.int32)
        if keep_final:
            shapes["final_state"] = ((R, W, n), torch.int32)
        size, spans = PAD, {}
        for key, (shape, dt) in shapes.items():
            nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dt).element_size()
            spans[key] = (size, nbytes)
            size += (nbytes + PAD + 15) // 16 * 16   # 16-byte aligned views
        self.bytes = torch.full((size,), CANARY, dtype=torch.uint8, device=env.device)
        self.data = np.zeros(size, dtype=bool)
        self.out = {"_n_steps": R, "obs": None, "final_state": None, "updates": None}
        for key, (shape, dt) in shapes.items():
            lo, nbytes = spans[key]
            self.out[key] = self.bytes[lo:lo + nbytes].view(dt).view(*shape)
            self.data[lo:lo + nbytes] = True

    def check_canaries(self, tag):
        got = self.bytes.cpu().numpy()
        bad = np.flatnonzero(~self.data & (got != CANARY))
        assert bad.size == 0, f"{tag}: canary bytes overwritten at {bad[:8]}"


def rollout_against_oracle(env, spec, R, keep_obs, keep_final, given, tag, copy=None):
    """One R-step rollout from a fresh reset into canary-fenced buffers == R oracle steps."""
    n, W = env.n_alloc, spec.words
    env.step_index = 0
    env.reset(SEED)
    st, tg, t = oracle.reset(spec, SEED, 0, OFFSET, n)
    mode = 1 if given else 3
    flips = fm = None
    if given:
        rng = np.random.default_rng(R * 131 + n)
        flips = rng.integers(0, 2 ** 32, size=(R, W, n), dtype=np.uint64).astype(np.uint32) & np.uint32(0x04010020)
        if spec.n % 32:
            flips[:, W - 1] &= np.uint32((1 << (spec.n % 32)) - 1)
        fm = torch.from_numpy(flips.view(np.int32)).to(env.device)
    arena = Arena(env, R, keep_obs, keep_final)
    out = env.rollout(R, flipmasks=fm, random_actions=not given, keep_obs=keep_obs, keep_final=keep_final,
                      out=arena.out, copy=copy)
    assert out is arena.out
    torch.cuda.synchronize()
    for k in range(R):
        flip = np.zeros((W, n), np.uint32) if flips is None else flips[k]
        ref = oracle.step(spec, SEED, 1 + k, OFFSET, st, flip, tg, t, mode)
        at = f"{tag} step {k}"
        if keep_obs:
            assert np.array_equal(u32(out["obs"][k]), st), at + " obs"
        if keep_final:
            assert np.array_equal(u32(out["final_state"][k]), ref["final_state"]), at + " final_state"
        assert np.array_equal(out["flags"][k].cpu().numpy(), ref["flags"]), at + " flags"
        assert np.array_equal(u32(out["reward"][k]), ref["reward"].view(np.uint32)), at + " reward"
        assert np.array_equal(u32(out["flipmask"][k]), ref["flipmask"]), at + " flipmask"
        st, tg, t = ref["state_out"], ref["target"], ref["t"]
    assert np.array_equal(u32(env.state), st), tag + " state"
    assert np.array_equal(env.target.cpu().numpy(), tg), tag + " target"
    assert np.array_equal(env.t.cpu().numpy(), t), tag + " t"
    arena.check_canaries(tag)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NETS)
def test_rollout_stores_match_oracle_and_keep_canaries(name):
    """32 / 64 / 96 envs x 1 / 2 / 3 steps x every keep_obs / keep_final combination x in-kernel
    actions and given flip masks."""
    spec = make_spec(name)
    for n in (32, 64, 96):
        env = VectorPBNEnv(spec, n, seed=SEED, env_offset=OFFSET, autoreset=True)
        for R, keep_obs, keep_final, given in itertools.product((1, 2, 3), (False, True), (False, True),
                                                                (False, True)):
            rollout_against_oracle(env, spec, R, keep_obs, keep_final, given,
                                   f"{name} n={n} R={R} obs={keep_obs} final={keep_final} given={given}")
        env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pbn7", "pbn70"])
def test_rollout_rows_are_the_steps_rows(name):
    """Row t of a launch holds step t: a 3-step rollout, then a 2-step rollout into fresh buffers,
    against the same five steps taken as pbn_step launches."""
    spec, n = make_spec(name), 96
    env = VectorPBNEnv(spec, n, seed=SEED, env_offset=OFFSET, autoreset=True)
    one = VectorPBNEnv(spec, n, seed=SEED, env_offset=OFFSET, autoreset=True)
    env.reset()
    one.reset()
    for R in (3, 2):
        arena = Arena(env, R, True, True)
        out = env.rollout(R, random_actions=True, keep_obs=True, keep_final=True, out=arena.out)
        torch.cuda.synchronize()
        for k in range(R):
            before = u32(one.state).copy()
            state, reward, flags = one.step_flipmask(random_actions=True)
            at = f"{name} R={R} row {k}"
            assert np.array_equal(u32(out["obs"][k]), before), at + " obs"
            assert np.array_equal(u32(out["final_state"][k]), u32(one.final_state)), at + " final_state"
            assert np.array_equal(u32(out["reward"][k]), u32(reward)), at + " reward"
            assert np.array_equal(out["flags"][k].cpu().numpy(), flags.cpu().numpy()), at + " flags"
            assert np.array_equal(u32(out["flipmask"][k]), u32(one.flipmask)), at + " flipmask"
        assert np.array_equal(u32(env.state), u32(one.state)), f"{name} R={R} state"
        arena.check_canaries(f"{name} R={R}")
    env.close()
    one.close()


@pytest.mark.gpu
def test_rollout_stores_with_ride_copy():
    """The ride-along copy is a fourth wave per block that leaves before the step loops: the
    three roles still meet at every barrier, and the copy arrives whole."""
    spec, n = make_spec("pbn7"), 96
    env = VectorPBNEnv(spec, n, seed=SEED, env_offset=OFFSET, autoreset=True)
    src = torch.arange(4096, dtype=torch.int32, device=env.device) * 2654435 + 7
    dst = torch.zeros_like(src)
    rollout_against_oracle(env, spec, 3, True, True, False, "ride copy", copy=(dst, src))
    assert torch.equal(dst, src)
    env.close()


def test_rollout_buffers_without_optional_outputs_host():
    """No GPU: rollout_buffers with both optional outputs off leaves them None, which the binding
    passes as null pointers, and the host's argument checks do not ask for them: with every
    required buffer given the call is refused for its null net alone."""
    env = VectorPBNEnv.__new__(VectorPBNEnv)
    env.words, env.n_alloc, env.device = 3, 96, torch.device("cpu")
    out = env.rollout_buffers(2, keep_obs=False, keep_final=False)
    assert out["obs"] is None and out["final_state"] is None and out["updates"] is None
    assert out["flipmask"].shape == (2, 3, 96) and out["reward"].shape == (2, 96) and out["flags"].shape == (2, 96)
    L = _lib.load()
    state = torch.zeros(3, 96, dtype=torch.int32)
    tg = torch.zeros(96, dtype=torch.uint8)
    t = torch.zeros(96, dtype=torch.uint8)
    ptr = lambda x: x.data_ptr() if x is not None else None  # noqa: E731
    rc = L.pbn_rollout_ex(None, 1, 0, 0, 96, 2, 3, state.data_ptr(), out["flipmask"].data_ptr(), tg.data_ptr(),
                          t.data_ptr(), ptr(out["obs"]), ptr(out["final_state"]), out["reward"].data_ptr(),
                          out["flags"].data_ptr(), ptr(out["updates"]), None)
    assert rc == -22 and "null net" in L.pbn_last_error().decode()
    assert ctypes.c_void_p(ptr(out["obs"])).value is None
