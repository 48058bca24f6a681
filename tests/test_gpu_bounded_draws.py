"""pbn_rollout under both step laws with the env draws' trimmed bounded draws (csrc/step_law.h:
two divisions for the three action digits; the fast env loops: gap 2's uniform from the running
X) == the C oracle, bit for bit, at the corners of those forms.

Networks are tests/synthetic.py's random ones (at most three functions per node: the pipelined
kernels' usual instances; p = 0.05: the gap bucket table, so with two or more single-state
attractors the env-draw wave runs its fast loop):
  - N = 1 (n1 = 2: the largest magic, 2^31), N = 31 (n1 = 32: the last actions_mask31 size),
    N = 32 (one word past actions_mask31: the general env loop and actions_from_draw<1>) and
    N = 33 (the first two-word size: the fast loop with actions_from_draw<2>);
  - A = 2 attractors (A - 1 == 1: the pair split's no-divide arm), 3 (the largest pair magic) and
    254 (the descriptor's limit, which the generator gives at 31 nodes and up; one node has two
    states): the second draw's range A(A-1), which gap 2's uniform now follows on the chain;
  - 64 envs (one full block) and 96 (a second block with an invalid half), 3 steps;
  - one launch from step 2^32 - 2, which crosses the step word's wrap and takes the general loops.
Every output of every step is compared: obs, flip masks (the action digits), final state, reward,
flags, the update counts, and after the launch state, t and target (the pair draw).
"""
import numpy as np
import pytest

from oracle import oracle
from pbn_rl_amd.vector_env import VectorPBNEnv

from .synthetic import random_spec

pytestmark = pytest.mark.gpu

MODE = 3   # autoreset | random actions
STEPS = 3
CORNERS = [(1, 2), (31, 2), (31, 3), (31, 254), (32, 2), (32, 3), (32, 254), (33, 2), (33, 3), (33, 254)]   # (N, A)


def u32(x):
    return x.cpu().numpy().view(np.uint32)


def corner_spec(n_nodes, n_attr, settle):
    # horizon 2: episodes end (and the autoreset pair is applied) within the three steps
    spec = random_spec(n_nodes, 500 + n_nodes, n_targets=n_attr, max_funcs=3, perturbation=0.05, horizon=2,
                       settle=settle)
    assert len(spec.attractors) == n_attr and all(len(a) == 1 for a in spec.attractors)
    return spec


def run_launch(spec, n, *, first_step=None, seed=977, env_offset=64):
    """One STEPS-step launch beside the oracle's steps, over every allocated env."""
    env = VectorPBNEnv(spec, n, seed=seed, env_offset=env_offset, autoreset=True)
    env.reset()
    n = env.n_alloc
    st, tg, t = oracle.reset(spec, seed, 0, env_offset, n)
    assert np.array_equal(u32(env.state)[:, :n], st)
    if first_step is not None:
        env.step_index = first_step
    step0 = env.step_index
    flip = np.zeros((spec.words, n), np.uint32)
    out = env.rollout(STEPS, random_actions=True, keep_obs=True, keep_final=True, keep_updates=True)
    resets = 0
    for k in range(STEPS):
        ref = oracle.step(spec, seed, step0 + k, env_offset, st, flip, tg, t, MODE)
        tag = "step %d" % k
        assert np.array_equal(u32(out["obs"][k])[:, :n], st), tag + " obs"
        assert np.array_equal(u32(out["flipmask"][k])[:, :n], ref["flipmask"]), tag + " flip masks"
        assert np.array_equal(u32(out["final_state"][k])[:, :n], ref["final_state"]), tag + " final state"
        assert np.array_equal(out["reward"][k].cpu().numpy()[:n].view(np.uint32), ref["reward"].view(np.uint32)), \
            tag + " reward"
        assert np.array_equal(out["flags"][k].cpu().numpy()[:n], ref["flags"]), tag + " flags"
        assert np.array_equal(out["updates"][k].cpu().numpy().view(np.uint16)[:n], ref["updates"]), tag + " updates"
        resets += int(((ref["flags"] & 16) != 0).sum())
        st, tg, t = ref["state_out"], ref["target"], ref["t"]
    assert np.array_equal(u32(env.state)[:, :n], st), "state"
    assert np.array_equal(env.t.cpu().numpy()[:n], t), "t"
    assert np.array_equal(env.target.cpu().numpy()[:n], tg), "target"
    env.close()
    assert resets >= n   # (horizon 2: every env drew an autoreset pair that the next step shows)


@pytest.fixture(autouse=True)
def pipelined(monkeypatch):
    monkeypatch.setenv("PBN_ROLL", "pipe")


@pytest.mark.parametrize("settle", [0, 4], ids=["one_update", "settle4"])
@pytest.mark.parametrize("n_nodes,n_attr", CORNERS)
def test_corners_match_oracle(n_nodes, n_attr, settle):
    spec = corner_spec(n_nodes, n_attr, settle)
    for n_envs in (64, 96):
        run_launch(spec, n_envs)


@pytest.mark.parametrize("settle", [0, 4], ids=["one_update", "settle4"])
@pytest.mark.parametrize("n_nodes,n_attr", [(31, 3), (33, 254)])
def test_launch_across_the_step_wrap_takes_the_general_loops(n_nodes, n_attr, settle):
    run_launch(corner_spec(n_nodes, n_attr, settle), 96, first_step=2 ** 32 - 2)
