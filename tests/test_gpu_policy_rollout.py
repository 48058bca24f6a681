"""The policy rollout (pbn_rollout_dqn, BatchedDDQN.rollout): a DQN chooses every action inside the
multi-step step kernel.  Every output must equal, bit for bit, what the same number of rounds of
the acting launch (act_q) and pbn_step give from the same seed, under both step laws, and the steps
must be the CPU oracle's on the flip masks the launch emitted.  All comparisons are exact."""
import numpy as np
import pytest
import torch

from oracle import oracle
from pbn_rl_amd import _lib
from pbn_rl_amd.attractors import load_attractors
from pbn_rl_amd.ddqn import DQN, BatchedDDQN
from pbn_rl_amd.network import load_network
from pbn_rl_amd.spec import EnvSpec
from pbn_rl_amd.vector_env import VectorPBNEnv

pytestmark = pytest.mark.gpu

SEED = 23
LAUNCHES = (5, 3)
# one tile, W = 1; the reference's shape; W = 2, A = 34 crosses the 32-output tile and the lowered
# gates run eval_gate_levels in the loop; W = 3
SHAPES = [("pbn7", [(8, 8)]), ("pbn28", [(50, 50)]), ("bb33", [(50, 50)]), ("pbn70", [(64, 64)])]
IDS = ["pbn7-8x8", "pbn28-50x50", "bb33-50x50", "pbn70-64x64"]
# three groups (one block, its fourth wave idle); a second, partial block
ENVS = [96, 160]
_SPECS = {}


def make_spec(net, settle=0):
    key = (net, settle)
    if key not in _SPECS:
        kw = {"settle": settle} if settle else {}
        _SPECS[key] = EnvSpec(load_network(net), load_attractors(net), perturbation=0.0 if net == "bb33" else 0.05,
                              horizon=3, **kw)
    return _SPECS[key]


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def make_dqn(N, arch):
    torch.manual_seed(3)
    return DQN(N, N + 1, arch).cuda()


def make_env(spec, n):
    env = VectorPBNEnv(spec, n, seed=SEED)
    env.reset()
    env.target[5] = 255          # envs without a target: the forward reads no table row
    env.target[64] = 255
    return env


def twin_steps(agent, eps, n_steps):
    """n_steps rounds of the acting launch and pbn_step; the per-step records, stacked."""
    env = agent.env
    rec = {k: [] for k in ("obs", "flipmask", "actions", "final_state", "reward", "flags")}
    for _ in range(n_steps):
        rec["obs"].append(env.state.clone())
        agent.act_q(eps)
        rec["flipmask"].append(env.flipmask.clone())
        rec["actions"].append(agent.actions.clone())
        env.step_flipmask(use_current=True)
        rec["final_state"].append(env.final_state.clone())
        rec["reward"].append(env.reward.clone())
        rec["flags"].append(env.flags.clone())
    return {k: torch.stack(v) for k, v in rec.items()}


def run_pair(spec, arch, n, check_updates=False, q=None):
    """Fused launches against the twin for epsilon 0, 0.3 and 1; returns nothing, asserts.  ``q``: the
    network on the device (default: make_dqn's)."""
    q = make_dqn(spec.n, arch) if q is None else q
    actions = {}
    for eps in (0.0, 0.3, 1.0):
        env, twin_env = make_env(spec, n), make_env(spec, n)
        agent, twin = BatchedDDQN(env, q), BatchedDDQN(twin_env, q)
        assert agent.kernel and twin.kernel
        greedy = agent.q_values().argmax(1).to(torch.int32).clone()
        taken, resets, most_updates = [], 0, 0
        for n_steps in LAUNCHES:
            first = env.step_index
            pre = (env.state.clone(), env.target.clone(), env.t.clone())
            out = agent.rollout(n_steps, eps, keep_obs=True, keep_updates=check_updates)
            assert env.step_index == first + n_steps
            assert out["actions"].shape == (n_steps, env.n_alloc) and out["actions"].dtype == torch.int32
            want = twin_steps(twin, eps, n_steps)
            for key, ref in want.items():
                assert torch.equal(out[key], ref), (eps, n_steps, key)
            for key in ("state", "target", "t"):
                assert torch.equal(getattr(env, key), getattr(twin_env, key)), (eps, n_steps, key)
            assert env.step_index == twin_env.step_index
            if check_updates:
                # the same steps from the emitted flip masks: pbn_rollout_ex's update counts
                assert n == env.n_alloc
                rep = VectorPBNEnv(spec, n, seed=SEED)
                rep.set_state(*pre)
                rep.step_index = first
                got = rep.rollout(n_steps, flipmasks=out["flipmask"], keep_updates=True)
                assert torch.equal(got["updates"], out["updates"]), (eps, n_steps)
                assert torch.equal(got["final_state"], out["final_state"]), (eps, n_steps)
                most_updates = max(most_updates, int(out["updates"].max()))
                rep.close()
            resets += int(((out["flags"] & _lib.FLAG_RESET) != 0).sum())
            taken.append(out["actions"].clone())
        actions[eps] = torch.cat(taken)
        if eps == 0.0:
            assert torch.equal(actions[eps][0], greedy)
        # horizon 3: autoresets drew new targets inside the launches (the next forward reads them)
        assert resets > 0
        if check_updates and eps == 1.0:
            assert most_updates > 1      # a random flip left some env settling over several updates
        env.close()
        twin_env.close()
    assert not torch.equal(actions[1.0], actions[0.0])
    assert int(actions[1.0].min()) >= 0 and int(actions[1.0].max()) <= spec.n


@pytest.mark.parametrize("n", ENVS)
@pytest.mark.parametrize("net,arch", SHAPES, ids=IDS)
def test_fused_rollout_equals_act_then_step(net, arch, n):
    run_pair(make_spec(net), arch, n)


@pytest.mark.parametrize("net,arch,settle", [("pbn7", [(8, 8)], 9), ("bb33", [(50, 50)], 64)],
                         ids=["pbn7-settle9", "bb33-settle64"])
def test_fused_rollout_equals_act_then_step_under_the_settle_law(net, arch, settle):
    run_pair(make_spec(net, settle), arch, 96, check_updates=True)


@pytest.mark.parametrize("net,arch,settle", [("pbn7", [(8, 8)], 0), ("bb33", [(50, 50)], 0), ("pbn7", [(8, 8)], 9)],
                         ids=["pbn7", "bb33", "pbn7-settle9"])
def test_fused_rollout_steps_are_the_oracles(net, arch, settle):
    steps_are_the_oracles(make_spec(net, settle), arch)


def steps_are_the_oracles(spec, arch):
    """oracle.step on the launch's emitted flip masks, from the same reset: the launch's
    per-step outputs at every step, and the state, target and t every launch leaves."""
    n = 96
    env = make_env(spec, n)
    agent = BatchedDDQN(env, make_dqn(spec.n, arch))
    st, tg, t = oracle.reset(spec, SEED, 0, 0, n)
    assert np.array_equal(u32(env.state), st)
    tg = tg.copy()
    tg[5] = tg[64] = 255
    resets = 0
    for n_steps in (1, 3, 1, 2):
        first = env.step_index
        out = agent.rollout(n_steps, 0.3, keep_obs=True, keep_updates=True)
        for k in range(n_steps):
            assert np.array_equal(u32(out["obs"][k]), st), k
            ref = oracle.step(spec, SEED, first + k, 0, st, u32(out["flipmask"][k]), tg, t, _lib.MODE_AUTORESET)
            assert np.array_equal(u32(out["final_state"][k]), ref["final_state"]), k
            assert np.array_equal(u32(out["reward"][k]), ref["reward"].view(np.uint32)), k
            assert np.array_equal(out["flags"][k].cpu().numpy(), ref["flags"]), k
            assert np.array_equal(out["updates"][k].cpu().numpy().view(np.uint16), ref["updates"]), k
            nxt = u32(out["obs"][k + 1]) if k + 1 < n_steps else u32(env.state)
            assert np.array_equal(nxt, ref["state_out"]), k
            st, tg, t = ref["state_out"], ref["target"], ref["t"]
            resets += int(((ref["flags"] & _lib.FLAG_RESET) != 0).sum())
        assert np.array_equal(env.target.cpu().numpy(), tg)
        assert np.array_equal(env.t.cpu().numpy(), t)
    assert resets > 0        # horizon 3: autoresets drew new targets inside the launches
    env.close()


def _raw_call(env, agent, bufs, **over):
    """pbn_rollout_dqn through ctypes with one argument replaced; (rc, message)."""
    L = _lib.load()
    a = dict(net=env.net.handle, seed=env.seed, step=env.step_index, env_offset=0, n_envs=env.n_alloc, n_steps=2,
             mode=_lib.MODE_AUTORESET, state=env.state.data_ptr(), target=env.target.data_ptr(), t=env.t.data_ptr(),
             h0=agent.h0, h1=agent.h1, image=agent.image().data_ptr(), epsilon=0.0,
             flipmask=bufs["flipmask"].data_ptr(), actions=bufs["actions"].data_ptr(), obs=None,
             final_state=bufs["final_state"].data_ptr(), reward=bufs["reward"].data_ptr(),
             flags=bufs["flags"].data_ptr(), updates=None, stream=env._stream())
    a.update(over)
    rc = L.pbn_rollout_dqn(*a.values())
    return rc, L.pbn_last_error().decode()


def test_refusals_and_the_empty_launch():
    spec = make_spec("pbn7")
    env = make_env(spec, 96)
    agent = BatchedDDQN(env, make_dqn(spec.n, [(8, 8)]))
    bufs = env.rollout_buffers(2, keep_actions=True)
    for b in (bufs["flipmask"], bufs["actions"], bufs["final_state"]):
        b.fill_(0x5A5A5A5A)
    bufs["reward"].fill_(-7.5)
    bufs["flags"].fill_(0xA5)
    before = {k: v.clone() for k, v in bufs.items() if isinstance(v, torch.Tensor)}
    state, target, t = env.state.clone(), env.target.clone(), env.t.clone()
    for over, msg in [
            (dict(mode=_lib.MODE_AUTORESET | _lib.MODE_RANDOM_ACTIONS), "the policy chooses the actions"),
            (dict(mode=4), "unknown mode bits"),
            (dict(image=None), "null buffer"),
            (dict(h0=65), "hidden widths must be 1..64"),
            (dict(n_steps=-1), "n_steps < 0"),
            (dict(n_envs=33), "n_envs and env_offset must be multiples of 32"),
            (dict(epsilon=1.5), "epsilon must be in [0, 1]")]:
        rc, err = _raw_call(env, agent, bufs, **over)
        assert rc == -22 and msg in err, (over, rc, err)
    rc, _ = _raw_call(env, agent, bufs, n_steps=0)
    assert rc == 0
    rc, _ = _raw_call(env, agent, bufs, n_envs=0)
    assert rc == 0
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(bufs[k], v), k          # nothing was written, by the refusals or the no-ops
    assert torch.equal(env.state, state) and torch.equal(env.target, target) and torch.equal(env.t, t)
    with pytest.raises(ValueError, match="one hidden Linear"):
        BatchedDDQN(env, agent.q, kernel=False).rollout(2)
    env.close()
