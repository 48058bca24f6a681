"""The RNG waves of the pipelined rollout kernel (pbn_rollout_pipe) hold the Philox key schedule
and the 64-bit step of the call they compute (one step ahead) across their loops: the round keys
are built once per launch and the step's two words are advanced by one per step with a carry,
in loops that take two steps per trip (the second one guarded) and end with the block's last
barrier.

Every output of a rollout from a fresh reset is compared with the CPU oracle step by step, bit
for bit (obs, final_state, flipmask, reward, flags, then state, target, t), at the smallest sizes
that reach this:
  - pbn28 (env_fast, sel_fast with two thresholds, state_fast with K = 3), pbn7 and pbn70 (three
    state words: the general selection loop);
  - 32 envs (one block, its upper half invalid) and 96 (two blocks, the second half empty);
  - 1 .. 5 steps per launch: both parities of the two-step trip, a lone first step, the
    barrier-only last iteration;
  - seeds whose round keys wrap modulo 2^32 at different rounds;
  - a first step of 0, of 2^32 - 3 (the low word wraps and the high half takes the carry inside
    the launch, first on a call computed one step ahead) and of 2^48 - 3 (the 16 bits of the high
    half that the counter keeps wrap to 0);
  - env_offset 64 and 2^32 - 64, where the 96 envs straddle 2^32: the lanes of one launch differ in
    the high half of their id.
The oracle's own handling of these step and offset values is checked on the CPU against the
numpy restatement (test_oracles_agree_on_the_boundary_cases: no GPU)."""
import numpy as np
import pytest
import torch

from oracle import np_oracle, oracle
from pbn_rl_amd.attractors import load_attractors
from pbn_rl_amd.network import load_network
from pbn_rl_amd.spec import EnvSpec
from pbn_rl_amd.vector_env import VectorPBNEnv

S_SMALL, S_ONES, S_LARGE = 977, 2 ** 64 - 1, 0xC3A5C85C97CB3127
T_LO, T_HI = 2 ** 32 - 3, 2 ** 48 - 3      # first steps whose low word / kept high 16 bits wrap in a launch
OFF, OFF_HI = 64, 2 ** 32 - 64             # env_offset; the second: envs 64 .. 95 have ids >= 2^32

# (seed, first step, env_offset, steps per launch)
PLAIN = [(S_SMALL, 0, OFF, R) for R in (1, 2, 3, 4, 5)]
BOUNDARY = [(S_ONES, 0, OFF, 4), (S_LARGE, 0, OFF, 5),
            (S_SMALL, T_LO, OFF, 5), (S_LARGE, T_LO, OFF, 4),
            (S_ONES, T_HI, OFF, 5), (S_SMALL, T_HI, OFF, 4),
            (S_SMALL, 0, OFF_HI, 5), (S_ONES, 0, OFF_HI, 4),
            (S_LARGE, T_LO, OFF_HI, 5), (S_ONES, T_HI, OFF_HI, 2)]
CASES = {  # network -> envs -> cases
    "pbn28": {96: PLAIN + BOUNDARY, 32: [(S_SMALL, 0, OFF, R) for R in (1, 2, 3)] + [(S_LARGE, T_LO, OFF_HI, 4)]},
    "pbn7": {96: PLAIN + [(S_ONES, T_LO, OFF_HI, 5), (S_LARGE, T_HI, OFF, 4)], 32: [(S_SMALL, 0, OFF, 2), (S_LARGE, T_LO, OFF, 3)]},
    "pbn70": {96: PLAIN + [(S_ONES, T_LO, OFF_HI, 5), (S_LARGE, T_HI, OFF, 4)], 32: [(S_SMALL, 0, OFF, 2), (S_LARGE, T_LO, OFF, 3)]},
}


def make_spec(name):
    return EnvSpec(load_network(name), load_attractors(name), perturbation=0.05, horizon=2)


def u32(x: torch.Tensor) -> np.ndarray:
    return x.cpu().numpy().view(np.uint32)


def rollout_against_oracle(spec, n, seed, step0, offset, R, tag):
    """One R-step rollout whose first step is step0, from a reset at step 0 == R oracle steps."""
    env = VectorPBNEnv(spec, n, seed=seed, env_offset=offset, autoreset=True)
    env.reset()
    st, tg, t = oracle.reset(spec, seed, 0, offset, n)
    assert np.array_equal(u32(env.state), st), tag + " reset"
    env.step_index = step0
    out = env.rollout(R, random_actions=True, keep_obs=True, keep_final=True)
    torch.cuda.synchronize()
    zero = np.zeros((spec.words, n), np.uint32)
    for k in range(R):
        ref = oracle.step(spec, seed, step0 + k, offset, st, zero, tg, t, 3)
        at = f"{tag} step {k}"
        assert np.array_equal(u32(out["obs"][k]), st), at + " obs"
        assert np.array_equal(u32(out["final_state"][k]), ref["final_state"]), at + " final_state"
        assert np.array_equal(u32(out["flipmask"][k]), ref["flipmask"]), at + " flipmask"
        assert np.array_equal(u32(out["reward"][k]), ref["reward"].view(np.uint32)), at + " reward"
        assert np.array_equal(out["flags"][k].cpu().numpy(), ref["flags"]), at + " flags"
        st, tg, t = ref["state_out"], ref["target"], ref["t"]
    assert np.array_equal(u32(env.state), st), tag + " state"
    assert np.array_equal(env.target.cpu().numpy(), tg), tag + " target"
    assert np.array_equal(env.t.cpu().numpy(), t), tag + " t"
    assert env.step_index == step0 + R
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_rollout_matches_oracle_across_key_and_step_boundaries(name):
    spec = make_spec(name)
    for n, cases in CASES[name].items():
        for seed, step0, offset, R in cases:
            rollout_against_oracle(spec, n, seed, step0, offset, R,
                                   f"{name} n={n} seed={seed:#x} step0={step0:#x} offset={offset:#x} R={R}")


def test_cases_cover_every_axis_on_pbn28_at_96_envs():
    """No GPU: every value of every axis appears with pbn28 at 96 envs, and the boundary steps and
    the straddling offset appear at both parities of the step count."""
    cases = CASES["pbn28"][96]
    assert {c[0] for c in cases} == {S_SMALL, S_ONES, S_LARGE}
    assert {c[1] for c in cases} == {0, T_LO, T_HI}
    assert {c[2] for c in cases} == {OFF, OFF_HI}
    assert {c[3] for c in cases} == {1, 2, 3, 4, 5}
    assert any(c[1] == T_LO and c[3] == 5 for c in cases)
    for key, idx in ((T_LO, 1), (T_HI, 1), (OFF_HI, 2)):
        assert {c[3] & 1 for c in cases if c[idx] == key} == {0, 1}, key
    for name in CASES:
        assert set(CASES[name]) == {32, 96}


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracles_agree_on_the_boundary_cases(name):
    """No GPU: the C oracle accepts the boundary step and offset values and computes, there, what
    the numpy restatement computes (two implementations of the counter map's high halves)."""
    spec = make_spec(name)
    npo = np_oracle.NpPBN(spec)
    n = 96
    zero = np.zeros((spec.words, n), np.uint32)
    for seed, step0, offset in ((S_LARGE, T_LO, OFF_HI), (S_ONES, T_HI, OFF), (S_SMALL, T_HI, OFF_HI)):
        st, tg, t = oracle.reset(spec, seed, 0, offset, n)
        s2, g2, t2 = npo.reset(seed, 0, offset, n)
        assert np.array_equal(st, s2) and np.array_equal(tg, g2) and np.array_equal(t, t2)
        for k in range(5):
            ref = oracle.step(spec, seed, step0 + k, offset, st, zero, tg, t, 3)
            got = npo.step(seed, step0 + k, offset, st, zero, tg, t, 3)
            for key in ("state_out", "final_state", "reward", "flags", "target", "t", "flipmask"):
                assert np.array_equal(ref[key], got[key]), (key, seed, step0, offset, k)
            st, tg, t = ref["state_out"], ref["target"], ref["t"]
