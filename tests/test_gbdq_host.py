"""The GBDQ agent without a GPU (pbn_rl_amd/gbdq.py; DESIGN.md "GBDQ"): the edge list against the
reference's routine, the module tree against the reference's state_dict, EdgeConv against a per-edge
loop, the per-env BatchNorm mode against B = 1 forwards, gbdq_update against the same arithmetic
longhand, the split replay's CPU partition against numpy, and the learner's bit-equal resume."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from pbn_rl_amd.gbdq import (BatchedGBDQ, EdgeConv, GBDQLearner, GraphBranchingQNetwork, SplitDeviceReplay, edge_csr,
                             edge_index, front_supported, gbdq_update)
from tests import gbdq_cases as gc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("name", ["pbn7", "pbn28", "bb33", "hub"])
def test_edge_index_equals_the_reference_routine(name):
    spec = gc.named_spec(name)
    want = gc.ref_adj_list(spec)
    got = edge_index(spec)
    assert got.dtype == torch.long and torch.equal(got, want)
    assert int(got.max()) < spec.n      # never a gate of a lowered network


def test_hub_network_has_the_duplicate_self_pair_and_the_hub():
    spec = gc.hub_spec(9)
    e = edge_index(spec)
    pairs = list(zip(e[0].tolist(), e[1].tolist()))
    assert pairs[:2] == [(0, 0), (0, 0)]                       # node 0 lists itself: its self pair twice
    assert pairs.count((3, 3)) == 2
    assert int((e[1] == 0).sum()) == 9 + 1                      # in-degree N + 1
    start, src = edge_csr(e, 9)
    assert start.tolist()[:2] == [0, 10] and src[:10].tolist() == [0, 0, 1, 2, 3, 4, 5, 6, 7, 8]
    assert int(start[-1]) == e.shape[1]


# ------------------------------------------------------------------------------------ the module tree
def test_state_dict_keys_and_shapes_match_the_reference():
    """golden/gbdq_state_dict.json: the keys and shapes that gbdq_model/network.py's
    GraphBranchingQNetwork(7, 8, 5) registers, in order (read off its text; EdgeConv keeps its
    module as ``nn``)."""
    with open(os.path.join(GOLDEN, "gbdq_state_dict.json")) as f:
        want = [(k, tuple(s)) for k, s in json.load(f)]
    q = GraphBranchingQNetwork(7, 8, 5)
    got = [(k, tuple(v.shape)) for k, v in q.state_dict().items()]
    assert got == want
    ref_sd = {k: torch.full(s, 0.25, dtype=torch.int64 if k.endswith("num_batches_tracked") else torch.float32)
              for k, s in want}
    q.load_state_dict(ref_sd, strict=True)
    assert q.gconv2.nn[0].weight is q.conv_model2[0].weight      # shared, as the reference shares them
    assert float(q.adv_heads[4][4].bias[3].detach()) == 0.25


# ------------------------------------------------------------------------------------ EdgeConv
def test_edgeconv_equals_a_per_edge_loop():
    torch.manual_seed(3)
    spec = gc.hub_spec(6)
    e = edge_index(spec)
    mlp = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.ReLU(), torch.nn.Linear(5, 4)).double()
    conv = EdgeConv(mlp)
    x = torch.randn(3, 6, 3, dtype=torch.float64)
    want = torch.zeros(3, 6, 4, dtype=torch.float64)
    for b in range(3):
        for k in range(e.shape[1]):
            j, i = int(e[0, k]), int(e[1, k])                   # source -> target
            want[b, i] += mlp(torch.cat([x[b, i], x[b, j] - x[b, i]]))
    got = conv(x, e)
    assert torch.allclose(got, want, rtol=0, atol=1e-12)
    # a node without an incoming edge gets zero
    e2 = torch.tensor([[0, 1], [1, 1]])
    assert torch.equal(conv(x, e2)[:, 0], torch.zeros(3, 4, dtype=torch.float64))


@pytest.mark.parametrize("name", ["pbn7", "hub"])
def test_per_env_forward_equals_a_loop_of_single_forwards(name):
    spec = gc.named_spec(name)
    q = gc.make_q(spec.n, 5, 11, bn="random")
    e = edge_index(spec)
    words, target = gc.random_inputs(spec, 32, 4)
    x = gc.observation(spec, words, target)
    before = copy.deepcopy(q.state_dict())
    got = q(x, e, per_env=True)
    assert all(torch.equal(v, before[k]) for k, v in q.state_dict().items())    # running statistics untouched
    want = torch.cat([q(x[b:b + 1], e) for b in range(32)])                     # BatchNorm1d itself, B = 1
    assert torch.allclose(got, want, rtol=0, atol=2e-6)
    assert int(q.bn1.num_batches_tracked) == 32
    # and the literal per-edge forward from the definitions
    lit = gc.literal_front(q, x, e, torch.float32)
    assert torch.allclose(q.front(x, e, per_env=True), lit, rtol=0, atol=2e-5)


def test_front_supported_and_capture():
    assert all(front_supported(n) for n in (1, 7, 28, 33, 70, 128)) and not front_supported(129) and not front_supported(0)


# ------------------------------------------------------------------------------------ the update
def _batch(spec, B, K, seed, reward_scale):
    rng = np.random.default_rng(seed)
    N = spec.n
    f = lambda: torch.from_numpy(rng.integers(0, 2, size=(B, N)).astype(np.float32))  # noqa: E731
    return {"states": f(), "targets": f(), "next_states": f(),
            "actions": torch.from_numpy(rng.integers(0, N + 1, size=(B, K, 1))),
            "rewards": torch.from_numpy((rng.standard_normal((B, 1)) * reward_scale).astype(np.float32)),
            "masks": torch.from_numpy(rng.integers(0, 2, size=(B, 1)).astype(np.float32))}


def test_gbdq_update_equals_the_longhand_arithmetic():
    spec = gc.named_spec("pbn7")
    e = edge_index(spec)
    q = gc.make_q(7, 5, 21, bn="random")
    target = gc.make_q(7, 5, 22, bn="random")
    q2, target2 = copy.deepcopy(q), copy.deepcopy(target)
    batch = _batch(spec, 24, 5, 9, reward_scale=3000.0)     # large TD errors: gradients beyond +-10
    opt = torch.optim.Adam(q.parameters(), lr=1e-4)
    opt2 = torch.optim.Adam(q2.parameters(), lr=1e-4)
    loss = gbdq_update(q, target, opt, batch, e, gamma=1.8)

    # update_policy, gbdq_model/__init__.py:111-131, longhand
    qvals = q2(torch.stack((batch["states"], batch["targets"]), dim=2), e)
    cur = qvals.gather(2, batch["actions"]).squeeze(-1)
    with torch.no_grad():
        nxt = torch.stack((batch["next_states"], batch["targets"]), dim=2)
        am = torch.argmax(q2(nxt, e), dim=2)
        mx = target2(nxt, e).gather(2, am.unsqueeze(2)).squeeze(-1)
    exp = batch["rewards"] + mx * 1.8 * batch["masks"]
    loss2 = ((exp - cur) ** 2).mean()
    grads = torch.autograd.grad(loss2, list(q2.parameters()))
    raw = torch.cat([g.reshape(-1) for g in grads])
    assert float(raw.max()) > 10.0 and float(raw.min()) < -10.0          # both sides of the clamp occur
    assert (raw.abs() < 10.0).any()
    for p, g in zip(q2.parameters(), grads):
        p.grad = g.clamp(-10.0, 10.0)
    opt2.step()
    assert torch.equal(loss, loss2.detach())
    for (k, a), (_, b) in zip(q.state_dict().items(), q2.state_dict().items()):
        assert torch.equal(a, b), k
    for (k, a), (_, b) in zip(target.state_dict().items(), target2.state_dict().items()):
        assert torch.equal(a, b), k                                      # (the target's running statistics too)
    assert int(q.bn1.num_batches_tracked) == 2 and int(target.bn1.num_batches_tracked) == 1


@pytest.mark.parametrize("mode", ["reference", "copy"])
def test_target_update_modes(mode):
    spec = gc.named_spec("pbn7", horizon=6)
    env = gc.CpuVectorEnv(spec, 32, seed=3)
    env.reset()
    lr = GBDQLearner(env, gc.make_q(7, 5, 5), batch_size=4, learning_starts=0, capacity=64, target_update=mode,
                     target_net_update_freq=2, seed=1)
    t0 = copy.deepcopy(lr.target.state_dict())
    for _ in range(8):
        lr.frame()
    assert lr.updates == 3 and lr.update_counter == 1
    same_as_start = all(torch.equal(v, t0[k]) for k, v in lr.target.state_dict().items() if "running" not in k
                        and "num_batches" not in k)
    assert same_as_start == (mode == "reference")
    if mode == "copy":
        assert not all(torch.equal(v, lr.q.state_dict()[k]) for k, v in lr.target.state_dict().items())  # one update on
    with pytest.raises(NotImplementedError):
        lr.capture()
    with pytest.raises(ValueError):
        GBDQLearner(env, target_update="soft")


# ------------------------------------------------------------------------------------ the split replay
@pytest.mark.parametrize("words,cap", [(1, 64), (3, 40)])
def test_split_replay_cpu_partition_equals_numpy(words, cap):
    rng = np.random.default_rng(words)
    n, K = 32, 5
    rp = SplitDeviceReplay(cap, words, K, "cpu")
    rings = {k: {"state": np.zeros((words, cap), np.int32), "next_state": np.zeros((words, cap), np.int32),
                 "target": np.zeros(cap, np.uint8), "action": np.zeros((cap, K), np.int32),
                 "reward": np.zeros(cap, np.float32), "done": np.zeros(cap, np.uint8)} for k in "pn"}
    pos, size, capd = {"p": 0, "n": 0}, {"p": 0, "n": 0}, {"p": cap, "n": cap}
    for frame in range(5):          # the negative ring wraps (cap 40) or fills (cap 64)
        flags = rng.choice(np.array([0, 1, 2, 3, 4, 17, 18], dtype=np.uint8), size=n)
        if frame == 1:
            flags[:] = 1            # all terminated
        if frame == 2:
            flags[:] = 2            # none
        if frame == 3:
            flags[:] = 0
            flags[n - 1] = 1        # one, the last env
        fields = {"state": rng.integers(-2 ** 31, 2 ** 31, size=(words, n)).astype(np.int32),
                  "next_state": rng.integers(-2 ** 31, 2 ** 31, size=(words, n)).astype(np.int32),
                  "target": rng.integers(0, 255, size=n).astype(np.uint8),
                  "action": rng.integers(0, 8, size=(n, K)).astype(np.int32),
                  "reward": rng.standard_normal(n).astype(np.float32)}
        t = {k: torch.from_numpy(v) for k, v in fields.items()}
        rp.store(t["state"], t["target"], t["action"], t["reward"], t["next_state"], torch.from_numpy(flags))
        cp, cn = gc.expected_rings(rings, pos, size, capd, fields, flags)
        assert rp.counts.tolist() == [cp, cn]
        for key, ring in (("p", rp.positive), ("n", rp.negative)):
            assert (ring.pos, ring.size) == (pos[key], size[key])
            for f, want in rings[key].items():
                assert np.array_equal(getattr(ring, f).numpy(), want), (frame, key, f)
    ip, in_ = rp.sample(1000, torch.Generator().manual_seed(0))
    assert ip.numel() == rp.positive.size and in_.numel() == rp.negative.size    # min(bs, len) of each
    sd = rp.state_dict()
    rp2 = SplitDeviceReplay(cap, words, K, "cpu")
    rp2.load_state_dict(sd)
    assert all(torch.equal(v, rp2.state_dict()[k]) if isinstance(v, torch.Tensor) else v == rp2.state_dict()[k]
               for k, v in sd.items())


def test_split_replay_gather_puts_positive_rows_first():
    spec = gc.named_spec("pbn7")
    rp = SplitDeviceReplay(32, 1, 5, "cpu")
    n = 32
    flags = torch.zeros(n, dtype=torch.uint8)
    flags[[3, 9]] = 1
    state = torch.arange(n, dtype=torch.int32).reshape(1, n)
    rp.store(state, torch.full((n,), 255, dtype=torch.uint8), torch.zeros(n, 5, dtype=torch.int32),
             torch.arange(n, dtype=torch.float32), state + 1, flags)
    b = rp.gather(torch.tensor([1, 0]), torch.tensor([0, 2]), spec=spec)
    assert b["rewards"].reshape(-1).tolist() == [9.0, 3.0, 0.0, 2.0]
    assert b["masks"].reshape(-1).tolist() == [1.0, 1.0, 0.0, 0.0]
    assert torch.equal(b["targets"], torch.zeros(4, 7))             # id 255: zeros
    assert b["states"][0].tolist() == [1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]     # 9
    assert b["actions"].shape == (4, 5, 1) and b["actions"].dtype == torch.int64


# ------------------------------------------------------------------------------------ acting on the CPU
def test_cpu_act_follows_the_explore_law():
    from oracle import agent_oracle
    spec = gc.named_spec("pbn7")
    env = gc.CpuVectorEnv(spec, 32, seed=77)
    env.reset()
    agent = BatchedGBDQ(env, gc.make_q(7, 5, 2), branches=5)
    heads = agent.heads()
    qv = torch.from_numpy(agent_oracle.heads_q(heads.numpy()))
    for eps in (0.0, 0.4, 1.0):
        agent.act(eps)
        flip, actions = agent_oracle.q_to_flipmask(spec, qv.numpy(), env.seed, env.step_index, 0, eps)
        assert np.array_equal(agent.actions.numpy(), actions), eps
        assert np.array_equal(env.flipmask.numpy().view(np.uint32), flip), eps


def test_act_gap_budget_of_the_gpu_test():
    """The GPU acting test leaves out (env, branch) pairs whose top-two Q gap in float64 is at most
    1e-4, at most 1 % of them: its network and inputs stay under that cap, and on the pairs kept the
    fp32 CPU forward picks the float64 forward's actions."""
    for name, K in (("pbn7", 1), ("pbn28", 5)):
        spec = gc.named_spec(name)
        q = gc.make_q(spec.n, K, gc.ACT_SEED, adv_scale=gc.ACT_ADV_SCALE)
        words, target = gc.act_inputs(spec)
        keep, greedy64 = gc.act_reference(spec, q, words, target)
        assert float((~keep).float().mean()) <= 0.01
        q32 = q(gc.observation(spec, words, target), edge_index(spec), per_env=True)
        assert torch.equal(torch.argmax(q32, 2)[keep], greedy64[keep])


# ------------------------------------------------------------------------------------ resume
def _learner(seed=4, **kw):
    spec = gc.named_spec("pbn7", horizon=5)
    env = gc.CpuVectorEnv(spec, 32, seed=seed)
    env.reset()
    return GBDQLearner(env, gc.make_q(7, 5, 8), batch_size=8, learning_starts=0, capacity=96, epsilon_start=0.5,
                       epsilon_final=0.1, epsilon_decay=10, target_update="copy", target_net_update_freq=3, seed=seed,
                       **kw)


def _snapshot(lr):
    sd = lr.state_dict()
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in sd.items()}


def test_learner_resume_is_bit_equal(tmp_path):
    k = 14
    a = _learner()
    for _ in range(k):
        a.frame()
    assert a.updates == k - 9 and a.replay.positive.size > 0 and a.replay.negative.size > 0
    path = str(tmp_path / "ckpt.npz")
    a.save(path)
    for _ in range(k):
        a.frame()
    b = _learner()
    b.load(path)
    assert b.frames == k and b.epsilon == pytest.approx(0.5 - 0.04 * (k - 8))    # learning_starts = max(0, 8)
    for _ in range(k):
        b.frame()
    want, got = _snapshot(a), _snapshot(b)
    assert want.keys() == got.keys()
    for key, v in want.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, got[key]), key
        else:
            assert v == got[key], key
    assert a.updates == 2 * k - 9
    c = _learner(seed=5)
    with pytest.raises(ValueError, match="seed"):
        c.load(path)
