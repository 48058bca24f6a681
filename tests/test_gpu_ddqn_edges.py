"""The DDQN kernels (csrc/pbn_ddqn.hip, dqn_forward.h) and the policy rollout (step_wave.h) at
the action-tile and state-word edges of tests/edge_shapes.py, with hidden widths that differ
(H0T != H1T), fill a 16-tile exactly and sit one past it: [(1, 1)], [(16, 17)], [(17, 64)] and
[(64, 16)], each at W = 1 and at W = 4.

Acting and the update repeat test_gpu_ddqn.py's checks with the module evaluated in float64 as
the reference, at that file's tolerances (Q rtol 1e-5 / atol 1e-5; loss, norm and priorities rtol
1e-5; clipped gradients rtol 1e-3 / atol 1e-6; the Adam step from the kernel's own gradient rtol
1e-5 / atol 1e-7; the image bit-equal to a fresh pack; edge_shapes.FLOAT_BOUNDS lists any shape that
needs another bound and why).  The update's input conditions are asserted on the float64 reference:
no argmax tie in Q(s') within 1e-4, |delta| on both sides of 1; SEEDS holds ring seeds for which
they hold.  The policy rollout is compared bit for bit with act_q + pbn_step and with the CPU
oracle (test_gpu_policy_rollout.py's run_pair and steps_are_the_oracles)."""
import copy

import numpy as np
import pytest
import torch

from pbn_rl_amd import _lib
from pbn_rl_amd.ddqn import BatchedDDQN, FusedDDQNUpdate, ddqn_update
from pbn_rl_amd.vector_env import VectorPBNEnv
from tests.edge_shapes import ENVS, FLOAT_BOUNDS, NO_TARGET, check_close, edge_spec, u32
from tests.edge_updates import batch64_of, ddqn_conditions, ddqn_inputs
from tests.edge_updates import make_dqn_nets as make_nets
from tests.test_gpu_ddqn import RC, ZERO_AT, _batch
from tests.test_gpu_policy_rollout import run_pair, steps_are_the_oracles

pytestmark = pytest.mark.gpu

# EDGE_N and 3, the archs spread over them: every arch at W = 1 (N <= 32) and at W = 4 (N >= 97)
CASES = [(3, (1, 1)), (15, (16, 17)), (16, (17, 64)), (31, (64, 16)), (32, (16, 17)), (33, (17, 64)),
         (64, (64, 16)), (65, (1, 1)), (95, (16, 17)), (96, (17, 64)), (97, (64, 16)), (97, (1, 1)),
         (127, (17, 64)), (127, (16, 17))]
IDS = [f"N{N}-{a}x{b}" for N, (a, b) in CASES]
# ring seed of a case (N, arch) (default 100 + N): one for which the float64 reference meets the conditions
SEEDS = {}


def batch_size(N):
    return 16 if N % 2 else 48


# ---- acting ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,arch", CASES, ids=IDS)
def test_acting_launch_matches_the_module_and_the_explore_law(N, arch):
    spec = edge_spec(N)
    n, seed = ENVS[CASES.index((N, arch)) % 2], 17
    env = VectorPBNEnv(spec, n, seed=seed)
    env.reset()
    for e in NO_TARGET:                              # envs without a target
        env.target[e] = 255
    q = make_nets(N, arch, seed=3)[0].cuda()
    agent = BatchedDDQN(env, q)
    assert agent.kernel and env.n_alloc == n
    qk = agent.q_values().clone()
    assert qk.shape == (n, N + 1)
    s, g = BatchedDDQN(env, q, kernel=False).observe()   # pbn_obs_unpack's observation
    assert float(g[5].abs().sum()) == 0.0
    with torch.no_grad():
        want = copy.deepcopy(q).double()(s.double(), g.double())
        mod = q(s, g)
    check_close(f"Q N={N} arch={arch}", qk, want, mod, 1e-5, 1e-5, ("dqn_q", N, arch))
    L = _lib.load()
    flip_ref = torch.zeros_like(env.flipmask)
    act_ref = torch.zeros(n, dtype=torch.int32, device="cuda")
    step_t = torch.full((1,), env.step_index, dtype=torch.int64, device="cuda")
    for eps in (0.0, 0.3, 1.0):
        agent.act_q(eps)
        acts, flip = agent.actions.clone(), env.flipmask.clone()
        _lib.check(L.pbn_q_to_flipmask(env.net.handle, env.seed, env.step_index, env.env_offset, n, 1, N + 1,
                                       qk.data_ptr(), eps, flip_ref.data_ptr(), act_ref.data_ptr(), None),
                   "pbn_q_to_flipmask")
        torch.cuda.synchronize()
        assert torch.equal(acts, act_ref), eps
        assert torch.equal(flip, flip_ref), eps
        if eps == 0.0:
            assert torch.equal(acts.long(), qk.argmax(1))
        agent.actions.zero_()
        agent.act_q(0.9, step_t=step_t, epsilon_t=torch.full((1,), eps, device="cuda"))   # the device's values win
        assert torch.equal(agent.actions, act_ref) and torch.equal(env.flipmask, flip_ref), eps
    assert 0 < int((act_ref != qk.argmax(1)).sum())      # eps = 1 explored
    # the flip mask is the action's node bit
    a = act_ref.cpu().numpy()
    fm = u32(flip_ref)
    for e in range(n):
        want_w = np.zeros(spec.words, np.uint32)
        if a[e] > 0:
            want_w[(a[e] - 1) >> 5] = np.uint32(1) << np.uint32((a[e] - 1) & 31)
        assert np.array_equal(fm[:, e], want_w), e
    env.close()


# ---- the update against PyTorch in float64 --------------------------------------------------------
def update_inputs(N, arch):
    """test_gpu_ddqn.py's _inputs on an edge spec, the weights drawn on the host."""
    return ddqn_inputs(N, batch_size(N), SEEDS.get((N, arch), 100 + N))


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("N,arch", CASES, ids=IDS)
def test_fused_update_matches_pytorch_in_float64(N, arch, clip):
    spec, B, R, a, idx, w_np = update_inputs(N, arch)
    env = VectorPBNEnv(spec, 32)
    w = torch.from_numpy(w_np).cuda()
    q_cpu, tgt_cpu = make_nets(N, arch, seed=7)
    q, tgt = copy.deepcopy(q_cpu).cuda(), copy.deepcopy(tgt_cpu).cuda()
    q64, tgt64 = copy.deepcopy(q).double(), copy.deepcopy(tgt).double()
    q32, tgt32 = copy.deepcopy(q), copy.deepcopy(tgt)
    lr, gamma = 1e-3, 0.95
    batch = _batch(spec, a, idx)
    batch64 = batch64_of(batch)
    # the reference's input conditions: no argmax tie in Q(s'), |delta| on both sides of 1
    gap, delta = ddqn_conditions(q64, tgt64, batch64, gamma)
    assert gap > 1e-4
    assert bool((delta < 1).any()) and bool((delta > 1).any())
    # the gradient norm of this batch decides what clips: half of it, or far above it
    probe = copy.deepcopy(q64)
    _, norm0 = ddqn_update(probe, tgt64, torch.optim.SGD(probe.parameters(), lr=0.0), batch64, gamma, 1e30,
                           weights=w.double())
    norm0 = float(norm0)
    assert norm0 > 1e-6, norm0
    max_norm = 0.5 * norm0 if clip else 10.0 * max(norm0, 1.0)
    fused = FusedDDQNUpdate(q, tgt, env.net, batch_size=B, learning_rate=lr, gamma=gamma, max_grad_norm=max_norm,
                            keep_grad=True)
    p0 = [p.detach().clone() for p in q.parameters()]
    versions = [p._version for p in q.parameters()]
    prio = torch.full((B,), -1.0, device="cuda")
    loss = float(fused.update(R, torch.from_numpy(idx).cuda(), weights=w, priorities_out=prio, replay_constant=RC))
    torch.cuda.synchronize()
    assert q.input.weight.data_ptr() == fused.q_flat.data_ptr()
    assert all(p._version > v for p, v in zip(q.parameters(), versions))
    prio_ref = torch.full((B,), -1.0, device="cuda", dtype=torch.float64)
    loss_ref, norm_ref = ddqn_update(q64, tgt64, torch.optim.Adam(q64.parameters(), lr=lr), batch64, gamma, max_norm,
                                     weights=w.double(), priorities_out=prio_ref, replay_constant=RC)
    prio32 = torch.full((B,), -1.0, device="cuda")
    loss32, norm32 = ddqn_update(q32, tgt32, torch.optim.Adam(q32.parameters(), lr=lr), batch, gamma, max_norm,
                                 weights=w, priorities_out=prio32, replay_constant=RC)
    loss_ref, norm_ref = float(loss_ref), float(norm_ref)
    assert (norm_ref > max_norm) == clip, norm_ref
    norm = float(fused.grad_norm)
    print(f"N={N} {arch} B={B} clip={clip}: loss {loss!r} ref {loss_ref!r} fp32 {float(loss32)!r}; norm {norm!r} ref "
          f"{norm_ref!r} fp32 {float(norm32)!r}; priorities max rel "
          f"{((prio.double() - prio_ref).abs() / prio_ref).max().item():.3g} fp32 "
          f"{((prio32.double() - prio_ref).abs() / prio_ref).max().item():.3g}")
    assert abs(loss - loss_ref) <= 1e-5 * abs(loss_ref), (loss, loss_ref)
    assert abs(norm - norm_ref) <= 1e-5 * norm_ref, (norm, norm_ref)
    prio_rel = ((prio.double() - prio_ref).abs() / prio_ref).max().item()
    assert prio_rel <= FLOAT_BOUNDS.get(("ddqn_priorities", N, arch), (None, 1e-5))[1], prio_rel
    assert prio[ZERO_AT].item() == torch.tensor(RC, dtype=torch.float32).item()      # |0 * h| + rc, exactly
    assert (prio > 0).all() and not torch.equal(prio[1], prio[3])                    # one row, two weights
    names = [n for n, _ in q.named_parameters()]
    for name, g, p, p32 in zip(names, fused.grads(), q64.parameters(), q32.parameters()):
        err = (g.double() - p.grad).abs()
        over = (err - (1e-6 + 1e-3 * p.grad.abs())).max().item()
        assert over <= 0.0, (name, err.max().item(), (p32.grad.double() - p.grad).abs().max().item())
    b1, b2, eps = 0.9, 0.999, 1e-8
    for name, g, before, after in zip(names, fused.grads(), p0, q.parameters()):
        m, v = (1 - b1) * g, (1 - b2) * g * g
        want = before - (lr / (1 - b1)) * m / (v.sqrt() / (1 - b2) ** 0.5 + eps)
        assert torch.allclose(after, want, rtol=1e-5, atol=1e-7), (name, (after - want).abs().max().item())
    assert float(fused.step) == 1.0
    upd = fused.q_image.clone()
    fused.pack("online")
    torch.cuda.synchronize()
    assert torch.equal(upd, fused.q_image)
    env.close()


# ---- the policy rollout -----------------------------------------------------------------------------
# W = 4 with unequal widths, neither a multiple of 16; W = 4 at A = 128 with H0T = 4, H1T = 1;
# W = 1 at A = 33 with H0T = 2, H1T = 4
ROLLOUTS = [(97, (20, 40)), (127, (64, 16)), (32, (17, 64))]


@pytest.mark.parametrize("n", ENVS)
@pytest.mark.parametrize("N,arch", ROLLOUTS, ids=[f"N{N}-{a}x{b}" for N, (a, b) in ROLLOUTS])
def test_fused_rollout_equals_act_then_step(N, arch, n):
    run_pair(edge_spec(N, horizon=3), [arch], n)


def test_fused_rollout_equals_act_then_step_under_the_settle_law():
    run_pair(edge_spec(32, horizon=3, settle=6), [(17, 64)], 96, check_updates=True)


def test_fused_rollout_steps_are_the_oracles():
    steps_are_the_oracles(edge_spec(97, horizon=3), [(20, 40)])
