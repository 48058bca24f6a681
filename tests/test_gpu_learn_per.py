"""The fused BDQ update on a prioritised batch (pbn_bdq_learn_per, csrc/pbn_learn.hip
learn_bwd_kernel<true>; FusedBDQUpdate.update(weights=, priorities_out=)) against the PyTorch
prioritised update it replaces (bdq_update(weights=, priorities_out=) + torch.optim.Adam), against
the unweighted fused update at unit weights, and as BDQLearner(fused=True, prioritised=True), eager
and captured.

Tolerances (test_gpu_learn.py's and test_gpu_per.py's for the same comparisons): the loss and the
priorities to rtol 1e-5; the clamped gradient to rtol 1e-3 / atol 1e-6; the Adam step to rtol 1e-5 /
atol 1e-7 against torch.optim.Adam's formula applied to the kernel's own gradient; the online image
bit-exact against pbn_bdq_pack of the new weights.  Unit weights: everything the gradient path
writes is bit-equal to pbn_bdq_learn's (g * 1.0f is exact); the losses are two associations of the
same sum (rtol 1e-5).  The learners: the update has no GEMM library in it and every kernel reduces
in a fixed order, so eager and captured agree as bits."""
import copy

import numpy as np
import pytest
import torch

from pbn_rl_amd.agent import BranchingQNetwork
from pbn_rl_amd.attractors import load_attractors
from pbn_rl_amd.network import load_network
from pbn_rl_amd.replay import BDQLearner, FusedBDQUpdate, PrioritisedDeviceReplay, bdq_update
from pbn_rl_amd.spec import EnvSpec
from pbn_rl_amd.vector_env import VectorPBNEnv

from .test_gpu_learn import _check_image, _filled_replay, _nets

pytestmark = pytest.mark.gpu

RC = 1e-5
# (network, B, K): one tile on pbn7; three tiles and one branch; the benched shape; bb33's Apad = 48
# (the A > 32 loop of the second head layers)
SHAPES = [("pbn7", 16, 3), ("pbn28", 48, 1), ("pbn28", 256, 3), ("bb33", 32, 3)]
ZERO_AT = 5     # the batch position whose weight is 0


def _inputs(net, B, K):
    spec = EnvSpec(load_network(net), load_attractors(net))
    env = VectorPBNEnv(spec, 64)
    R = _filled_replay(spec, K, 1024, seed=B + K)
    idx = R.sample_indices(B, torch.Generator(device="cuda").manual_seed(B))
    idx[3] = idx[7] = idx[1]                    # one ring row three times, each with its own weight
    w = torch.rand(B, device="cuda", generator=torch.Generator(device="cuda").manual_seed(K)) + 0.05
    w[ZERO_AT] = 0.0
    return spec, env, R, idx, w


def _gathered(R, idx, net):
    """The batch of rows idx as bdq_update takes it (pbn_replay_batch gathers multiples of 32 rows:
    pad, then keep the first B)."""
    B = idx.shape[0]
    pad = torch.cat([idx, idx[: (-B) % 32]]) if B % 32 else idx
    g = R.gather(pad, net)
    return {"obs": g["obs"][:, :B].contiguous(), "next_obs": g["next_obs"][:, :B].contiguous(),
            "actions": g["actions"][:B], "rewards": g["rewards"][:B], "masks": g["masks"][:B]}


@pytest.mark.parametrize("net,B,K", SHAPES)
def test_fused_prioritised_update_matches_pytorch(net, B, K):
    spec, env, R, idx, w = _inputs(net, B, K)
    N = spec.n
    assert N == {"pbn7": 7, "pbn28": 28, "bb33": 33}[net]
    q, tgt = _nets(N, K, seed=7)
    q_ref, tgt_ref = copy.deepcopy(q), copy.deepcopy(tgt)
    lr, gamma = 1e-3, 0.9
    fused = FusedBDQUpdate(q, tgt, env.net, K, batch_size=B, learning_rate=lr, gamma=gamma, keep_grad=True)
    p0 = [p.detach().clone() for p in q.parameters()]
    prio = torch.full((B,), -1.0, device="cuda")
    loss = float(fused.update(R, idx, weights=w, priorities_out=prio, replay_constant=RC))
    torch.cuda.synchronize()
    opt = torch.optim.Adam(q_ref.parameters(), lr=lr)
    prio_ref = torch.full((B,), -1.0, device="cuda")
    loss_ref = float(bdq_update(q_ref, tgt_ref, opt, _gathered(R, idx, env.net), gamma, weights=w,
                                priorities_out=prio_ref, replay_constant=RC))
    print(f"{net} B={B} K={K}: loss {loss!r} ref {loss_ref!r}; "
          f"priorities max rel {((prio - prio_ref).abs() / prio_ref).max().item():.3g}")
    assert abs(loss - loss_ref) <= 1e-5 * abs(loss_ref), (loss, loss_ref)
    assert torch.allclose(prio, prio_ref, rtol=1e-5, atol=0), ((prio - prio_ref).abs() / prio_ref).max().item()
    assert prio[ZERO_AT].item() == torch.tensor(RC, dtype=torch.float32).item()      # |0 * l| + rc, exactly
    assert (prio > 0).all() and not torch.equal(prio[1], prio[3])                    # one row, two weights
    names = [n for n, _ in q.named_parameters()]
    for name, g, p in zip(names, fused.grads(), q_ref.parameters()):
        assert torch.allclose(g, p.grad, rtol=1e-3, atol=1e-6), (name, (g - p.grad).abs().max().item())
    # Adam's first step from the kernel's own gradient (torch.optim.Adam's arithmetic)
    b1, b2, eps = 0.9, 0.999, 1e-8
    for name, g, a, b in zip(names, fused.grads(), p0, q.parameters()):
        m, v = (1 - b1) * g, (1 - b2) * g * g
        want = a - (lr / (1 - b1)) * m / (v.sqrt() / (1 - b2) ** 0.5 + eps)
        assert torch.allclose(b, want, rtol=1e-5, atol=1e-7), (name, (b - want).abs().max().item())
    assert float(fused.step) == 1.0
    # the online image written by the update = pbn_bdq_pack of the new weights, bit for bit, and
    # the table equal to the PyTorch contraction to rounding
    t_upd = fused.q_image.clone()
    fused.pack("online")
    assert torch.equal(t_upd, fused.q_image)
    _check_image(fused, q, N, K)
    targets = torch.tensor([list(a[0]) for a in spec.attractors], dtype=torch.float32, device="cuda")
    T = q.model[0].target_table(targets)
    assert torch.allclose(fused.q_table.transpose(2, 3).reshape(T.shape), T, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("net,B,K", SHAPES)
def test_unit_weights_are_todays_update(net, B, K):
    spec, env, R, idx, _ = _inputs(net, B, K)
    q1, t1 = _nets(spec.n, K, seed=7)
    q2, t2 = copy.deepcopy(q1), copy.deepcopy(t1)
    kw = dict(batch_size=B, learning_rate=1e-3, gamma=0.9, keep_grad=True)
    f1 = FusedBDQUpdate(q1, t1, env.net, K, **kw)
    f2 = FusedBDQUpdate(q2, t2, env.net, K, **kw)
    ones = torch.ones(B, device="cuda")
    prio = torch.full((B,), -1.0, device="cuda")
    for u in range(2):
        l1 = f1.update(R, idx).clone()
        l2 = f2.update(R, idx, weights=ones, priorities_out=prio, replay_constant=RC).clone()
        torch.cuda.synchronize()
        for name in ("q_flat", "m", "v", "step", "q_image", "grad"):
            assert torch.equal(getattr(f1, name), getattr(f2, name)), (u, name)
        print(f"{net} B={B} K={K} update {u}: loss {l1.item()!r} weighted {l2.item()!r} "
              f"mean priority - rc {(prio.mean() - RC).item()!r}")
        assert torch.allclose(l1, l2, rtol=1e-5, atol=0), (u, l1.item(), l2.item())
        assert torch.allclose(prio.mean() - RC, l1, rtol=1e-4, atol=0), (u, prio.mean().item(), l1.item())
    assert float(f1.step) == float(f2.step) == 2.0


def _learner(n, seed, updates_per_frame=1):
    spec = EnvSpec(load_network("pbn28"), load_attractors("pbn28"), perturbation=0.01)
    env = VectorPBNEnv(spec, n, seed=seed)
    torch.manual_seed(4)
    lr = BDQLearner(env, BranchingQNetwork((28, 28), 29, 3), capacity=8 * n, learning_starts=2 * n, batch_size=256,
                    target_update=4, epsilon_start=1.0, epsilon_final=1.0, seed=11, graphable=True, fused=True,
                    prioritised=True, per_beta=0.4, per_beta_steps=20, updates_per_frame=updates_per_frame)
    env.reset()
    return env, lr


def _tree_invariant(rp):
    T = rp.tree_size
    s, m = rp.sum_tree.cpu().numpy(), rp.min_tree.cpu().numpy()
    assert np.array_equal(s[1:T], s[2:2 * T:2] + s[3:2 * T:2])
    assert np.array_equal(m[1:T], np.minimum(m[2:2 * T:2], m[3:2 * T:2]))


def test_fused_prioritised_learner_eager_and_captured():
    """pbn28, 1,024 envs, batch 256, twelve frames at epsilon = 1, target_update 4: the eager and the
    captured fused prioritised learner agree as bits on rewards, dones and env state every frame,
    and at the end on the ring, the counters, beta, the weights, Adam's moments, both trees and
    max_priority."""
    n = 1024
    env_e, eager = _learner(n, 21)
    env_g, graph = _learner(n, 21)
    for lr in (eager, graph):
        assert isinstance(lr.replay, PrioritisedDeviceReplay) and lr.fused is not None and lr.opt is None
    graph.capture()
    assert graph.updates == 3 and graph.frames == 4
    for _ in range(graph.frames):
        eager.frame()
    for k in range(8):
        re, de = eager.frame()
        rg, dg = graph.frame()
        torch.cuda.synchronize()
        assert torch.equal(re, rg) and torch.equal(de, dg), k
        assert torch.equal(env_e.state, env_g.state), k
        assert torch.equal(eager.last_loss, graph.last_loss), k
    assert graph.frames == eager.frames == 12 and graph.updates == eager.updates == 11
    R, S = eager.replay, graph.replay
    assert R.pos == S.pos == int(graph._pos_t.item()) and R.size == S.size == int(graph._size_t.item())
    for f in ("state", "next_state", "target", "action", "reward", "done"):
        assert torch.equal(getattr(R, f), getattr(S, f)), f
    assert R.beta == S.beta == float(R.beta_t) == float(S.beta_t) and R.beta > 0.4
    assert int(R.counter_t) == int(S.counter_t) == 11
    fe, fg = eager.fused, graph.fused
    for name in ("q_flat", "t_flat", "m", "v", "q_image", "t_image"):
        assert torch.equal(getattr(fe, name), getattr(fg, name)), name
    assert float(fe.step) == float(fg.step) == 11.0
    assert torch.equal(R.sum_tree, S.sum_tree) and torch.equal(R.min_tree, S.min_tree)
    assert torch.equal(R.max_priority, S.max_priority) and float(R.max_priority) >= 1.0
    _tree_invariant(R)
    _tree_invariant(S)
    assert torch.isfinite(graph.last_loss) and torch.isfinite(eager.last_loss)


def test_captured_fused_prioritised_two_updates_per_frame():
    """updates_per_frame = 2, four replayed frames: the draw counter advances by 2 per frame, beta
    is mirrored twice per frame, and the trees keep their invariant."""
    env, lr = _learner(1024, 22, updates_per_frame=2)
    lr.capture()
    rp = lr.replay
    u0, c0, b0 = lr.updates, int(rp.counter_t), rp.beta
    assert c0 == u0 and b0 == float(rp.beta_t)
    for k in range(4):
        lr.frame()
        torch.cuda.synchronize()
        assert int(rp.counter_t) == c0 + 2 * (k + 1) == lr.updates
        assert rp.beta == float(rp.beta_t)
    want = b0
    for _ in range(8):
        want = min(rp.max_beta, want + rp.beta_step)
    assert rp.beta == want and rp.beta > b0
    assert rp.size == int(lr._size_t.item()) and rp.pos == int(lr._pos_t.item())
    _tree_invariant(rp)
    assert float(lr.fused.step) == lr.updates and torch.isfinite(lr.last_loss)
