"""pbn_rollout's pipelined kernel with the Philox prefix hoisted out of its two fast RNG loops
(csrc/philox.h philox_prefix / philox_tail, csrc/rollout_pipe.h env_fast / sel_fast) == the CPU
oracle, bit for bit.

The fast loops build, per lane and in front of the step loop, the part of every per-step call's
first three rounds that does not depend on the step's low word; that holds while the step's high
word does not change within the launch, and a launch that crosses a multiple of 2^32 takes the
general role loops.  The cases here are the ones where that can go wrong: launch lengths of both
parities of the two-step trip (and the peeled last barrier), a second launch (the prefix rebuilt
from the advanced step), the step word around its wrap and above it (a non-zero high half in
counter word 3), an env offset above 2^32 (the id's high half in the same word), other node
counts and threshold counts (the NQ = 1, 2, 3 instances of the selection loop), and the rare
fourth-flip calls, which have another counter word 2 and keep the whole call.

Every case runs pbn_rollout with in-kernel random actions, autoreset, and the per-step obs and
final states kept, and compares, for every step of every launch, obs (the state before the step),
the flip masks, the final state, reward and flags, and after every launch state, t and target
(which a launch returns once; the T = 1 launches check them at every step)."""
import numpy as np
import pytest

from oracle import oracle
from pbn_rl_amd.attractors import load_attractors
from pbn_rl_amd.network import load_network
from pbn_rl_amd.spec import EnvSpec
from pbn_rl_amd.vector_env import VectorPBNEnv

from .synthetic import random_spec

pytestmark = pytest.mark.gpu

MODE = 3   # autoreset | random actions


def make_spec(name, **kw):
    return EnvSpec(load_network(name), load_attractors(name), **kw)


def u32(x):
    return x.cpu().numpy().view(np.uint32)


def run_launches(spec, n, launches, *, seed=4242, env_offset=2048, first_step=None):
    """Launches of the given lengths, one after the other on one env, beside the oracle's steps,
    over every allocated env (``n`` rounded up to whole 32-env groups).  ``first_step``: the step
    index of the first launch (after the reset at step 0)."""
    env = VectorPBNEnv(spec, n, seed=seed, env_offset=env_offset, autoreset=True)
    env.reset()
    n = env.n_alloc   # whole 32-env groups: the kernel steps every allocated env, and so does the oracle
    st, tg, t = oracle.reset(spec, seed, 0, env_offset, n)
    assert np.array_equal(u32(env.state)[:, :n], st)
    if first_step is not None:
        env.step_index = first_step
    W = spec.words
    flip = np.zeros((W, n), np.uint32)
    flags_seen = 0
    for li, T in enumerate(launches):
        step0 = env.step_index
        out = env.rollout(T, random_actions=True, keep_obs=True, keep_final=True)
        assert env.step_index == step0 + T
        for k in range(T):
            ref = oracle.step(spec, seed, step0 + k, env_offset, st, flip, tg, t, MODE)
            tag = "launch %d step %d" % (li, k)
            assert np.array_equal(u32(out["obs"][k])[:, :n], st), tag + " obs"
            assert np.array_equal(u32(out["flipmask"][k])[:, :n], ref["flipmask"]), tag + " flip masks"
            assert np.array_equal(u32(out["final_state"][k])[:, :n], ref["final_state"]), tag + " final state"
            assert np.array_equal(out["reward"][k].cpu().numpy()[:n].view(np.uint32),
                                  ref["reward"].view(np.uint32)), tag + " reward"
            assert np.array_equal(out["flags"][k].cpu().numpy()[:n], ref["flags"]), tag + " flags"
            flags_seen |= int(np.bitwise_or.reduce(ref["flags"]))
            st, tg, t = ref["state_out"], ref["target"], ref["t"]
        assert np.array_equal(u32(env.state)[:, :n], st), "launch %d state" % li
        assert np.array_equal(env.t.cpu().numpy()[:n], t), "launch %d t" % li
        assert np.array_equal(env.target.cpu().numpy()[:n], tg), "launch %d target" % li
    env.close()
    return flags_seen


@pytest.fixture(autouse=True)
def pipelined(monkeypatch):
    monkeypatch.setenv("PBN_ROLL", "pipe")


# ---------------------------------------------------------------- launch lengths
@pytest.mark.parametrize("n_envs", [96, 33])   # one and a half blocks (an invalid half); a ragged env count
@pytest.mark.parametrize("T", [1, 2, 5])
def test_launch_lengths_and_a_second_launch(n_envs, T):
    """Both parities of the two-step trip, the peeled last barrier, and a second launch whose
    prefix is rebuilt from the advanced step index."""
    run_launches(make_spec("pbn28", perturbation=0.05, horizon=4), n_envs, [T, T], env_offset=96)


def test_single_steps_check_t_and_target_every_step():
    run_launches(make_spec("pbn28", perturbation=0.05, horizon=3), 96, [1, 1, 1, 1, 2, 1], env_offset=96)


# ---------------------------------------------------------------- the step word near its wrap
@pytest.mark.parametrize("first_step,T", [
    (2 ** 32 - 3, 8),    # crosses the boundary: the general loops
    (2 ** 32 - 40, 8),   # near it without crossing: the fast loops
    (2 ** 32 - 8, 8),    # the one-ahead call reaches 2^32 exactly: the general loops, by one
    (2 ** 32 - 9, 8),    # the last launch below it that the fast loops take
    (2 ** 32, 4),        # high word 1 from the first step
    (2 ** 33 + 5, 4),    # high word 2: reaches the prefix through counter word 3
])
def test_step_word_near_wrap(first_step, T):
    run_launches(make_spec("pbn28", perturbation=0.05, horizon=5), 96, [T, 3], first_step=first_step)


def test_step_high_word_above_16_bits():
    """Counter word 3 takes the step's bits 32..47: bits 48 and up are dropped."""
    run_launches(make_spec("pbn28", perturbation=0.05, horizon=5), 64, [4], first_step=(0x1ABCD << 32) + 7)


# ---------------------------------------------------------------- env offset
def test_env_offset_above_32_bits():
    """A non-zero hi16(id) in counter word 3 (the env draws), and lo32(G) != lo32(ge) >> 5."""
    run_launches(make_spec("pbn28", perturbation=0.05, horizon=5), 96, [5, 2], env_offset=2 ** 32 + 64 * 3)


def test_env_offset_and_step_high_halves_together():
    run_launches(make_spec("pbn28", perturbation=0.05, horizon=5), 64, [3],
                 env_offset=(0x1234 << 37) + 64 * 5, first_step=(0x4321 << 32) + 2 ** 32 - 20)


# ---------------------------------------------------------------- other networks and shapes
@pytest.mark.parametrize("name", ["pbn7", "pbn10"])
def test_small_networks(name):
    run_launches(make_spec(name, perturbation=0.05, horizon=4), 64, [5, 2])


@pytest.mark.parametrize("max_funcs", [2, 4])
def test_synthetic_threshold_counts(max_funcs):
    """At most 2 and at most 4 functions per node: the selection loop's NQ = 1 and NQ = 3
    instances (pbn28 and pbn10 run NQ = 2)."""
    spec = random_spec(31, 22, max_funcs=max_funcs, perturbation=0.05, horizon=6)
    assert max(len(f) for f in spec.network.nodes) == max_funcs
    run_launches(spec, 96, [5, 2])


@pytest.mark.parametrize("p", [0.3, 0.12])
def test_fourth_flip_calls(p):
    """High perturbation rates: most envs are perturbed and many draw further gaps.  At 0.12 the
    gap method is the bucket table, so the env draws run the fast loop and its gap_tail calls
    (another counter word 2, this step's low word: the whole call, not the prefix); at 0.3 the
    gap method takes the general loop."""
    seen = run_launches(make_spec("pbn28", perturbation=p, horizon=6), 64, [6, 1])
    assert seen & 8   # FLAG_PERTURBED
