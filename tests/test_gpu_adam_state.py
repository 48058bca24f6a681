"""Adam past its first step in both fused updates: pbn_bdq_learn / pbn_bdq_learn_per
(learn_apply_kernel, csrc/pbn_learn.hip) and pbn_ddqn_learn (ddqn_adam_kernel, csrc/pbn_ddqn.hip)
against torch.optim.Adam in float64 (tests/adam_reference.py), from moments and step counts that are
not zero.  The edge sweeps check the first step only, where b1 m, b2 v and the loads of the old
moments contribute nothing and both bias corrections are 1 - b.

a. One update from a seeded state: m and v filled per element through the parameter-shaped views
   (independent draws: a moment read from a neighbouring element, the wrong j-tile or across a
   segment's padding moves the result), the count set to 1, 6 or 999 (and once per agent to
   2^24 - 1), on one N per bilinear j-tile count NT = 1 .. 8 and 1 .. 4 state words (BDQ) and on the
   DDQN widths with the most segment padding and on both sides of a 16-tile.
b. Four updates from zero state on other ring rows each, the float64 modules reloaded with the
   kernel's weights before every update, the target moved after the second (soft_update /
   sync_target), lr 1e-3 and 1e-4, one DDQN trajectory clipping at every step.
c. The BDQ element clamp set to the median |g|, so that half the gradient reaches it.

Every update's Adam step is checked with check_adam_step from the snapshot before it and the
kernel's own stored gradient (clamped for BDQ, clipped for DDQN), which tests the optimiser's
arithmetic apart from the gradient's fp32 noise; the count is asserted exactly; the layout's padding
stays zero in the parameters and both moments.  Loss, norm, priorities and gradients do not depend
on the moments and are held to the float64 module at the edge sweeps' tolerances (loss, norm and
priorities rtol 1e-5; gradients rtol 1e-3 / atol 1e-6), the online image to a fresh pack, bit for
bit.  Input condition, asserted at every update: the float64 module's top-2 gap of Q(s') exceeds
1e-4 on every row."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pbn_rl_amd.ddqn import FusedDDQNUpdate, ddqn_update
from pbn_rl_amd.replay import FusedBDQUpdate
from pbn_rl_amd.vector_env import VectorPBNEnv
from tests.adam_reference import LAST_T0, SEEDED_T0, STEPS, check_adam_step, seed_moments
from tests.edge_shapes import FLOAT_BOUNDS, edge_spec
from tests.edge_updates import (DDQN_CAP, batch64_of, batch_of, bdq_reference_update, bdq_ring, bdq_top2_gap,
                                ddqn_conditions, ddqn_inputs, ddqn_trajectory_rows, make_dqn_nets, make_nets, pick_rows)
from tests.test_gpu_ddqn import RC, ZERO_AT, _batch, _ring
from tests.test_gpu_learn import _check_image

pytestmark = pytest.mark.gpu

LR = 1e-3
BDQ_GAMMA, DDQN_GAMMA = 0.9, 0.95                  # the edge sweeps'
# (N, B, K): NT = 1 .. 8 (Apad = 16 .. 128) over 1 .. 4 state words; one head; the most heads the LDS takes
BDQ_SHAPES = [(N, 16, 3) for N in (15, 31, 33, 64, 65, 96, 97, 127)] + [(33, 16, 1), (95, 16, 7)]
BDQ_CASES = [(N, B, K, False) for N, B, K in BDQ_SHAPES] + [(33, 16, 3, True)]       # the last: pbn_bdq_learn_per
BDQ_IDS = [f"N{N}-B{B}-K{K}" + ("-per" if w else "") for N, B, K, w in BDQ_CASES]
# (N, arch), B = 16: the most segment padding, widths on both sides of a 16-tile, W = 1 .. 4
DDQN_B = 16
DDQN_SHAPES = [(3, (1, 1)), (16, (17, 64)), (33, (17, 64)), (65, (1, 1)), (97, (64, 16)), (127, (16, 17))]
DDQN_CASES = [(N, arch, False) for N, arch in DDQN_SHAPES] + [(33, (17, 64), True)]  # the last: weights, priorities
DDQN_IDS = [f"N{N}-{a}x{b}" + ("-per" if w else "") for N, (a, b), w in DDQN_CASES]
# trajectories: BDQ (N, B, K, lr); DDQN (N, arch, lr, clip at half the first norm)
BDQ_TRAJ = [(33, 16, 3, 1e-3), (97, 16, 3, 1e-3), (127, 16, 3, 1e-3), (33, 16, 3, 1e-4)]
DDQN_TRAJ = [(33, (17, 64), 1e-3, False), (127, (16, 17), 1e-3, False), (33, (17, 64), 1e-4, False),
             (127, (16, 17), 1e-3, True)]
# (ring seed, row seed) of a trajectory, chosen on the CPU from a pure float64 PyTorch trajectory
# (edge_updates.bdq_trajectory_gaps / ddqn_trajectory_gaps) on which the top-2 gap of Q(s') stays
# above 1e-3 at all four updates (test_adam_state_seeds_host.py holds them to that), so that the
# kernel's own trajectory, an fp32 one, keeps it above the 1e-4 asserted here
SEEDS = {
    ("bdq", 33, 16, 3, 1e-3): (21, 71), ("bdq", 97, 16, 3, 1e-3): (20, 71), ("bdq", 127, 16, 3, 1e-3): (19, 51),
    ("bdq", 33, 16, 3, 1e-4): (20, 109),
    ("ddqn", 33, (17, 64), 1e-3, False): (133, 42), ("ddqn", 127, (16, 17), 1e-3, False): (227, 40),
    ("ddqn", 33, (17, 64), 1e-4, False): (133, 40), ("ddqn", 127, (16, 17), 1e-3, True): (227, 40),
}


# ---- the optimiser's state ---------------------------------------------------------------------------
def param_mask(fused):
    """True at the flat layout's parameter elements, False in its padding."""
    mask = torch.zeros(fused.q_flat.numel(), dtype=torch.bool)
    for p, at in fused._params(fused.q):
        assert not mask[at:at + p.numel()].any()
        mask[at:at + p.numel()] = True
    return mask.cuda()


def seed_state(fused, t0, seed):
    """Fill m and v through the parameter-shaped views (adam_reference.seed_moments) and set the
    count to t0: non-zero at every parameter element, zero in the padding."""
    gen = torch.Generator().manual_seed(seed)
    for p, at in fused._params(fused.q):
        m, v = seed_moments(p.shape, gen)
        fused.m[at:at + p.numel()].view(p.shape).copy_(m)
        fused.v[at:at + p.numel()].view(p.shape).copy_(v)
    fused.step.fill_(float(t0))
    assert float(fused.step) == t0
    mask = param_mask(fused)
    assert (fused.m[mask] != 0).all() and (fused.v[mask] > 0).all()
    assert not fused.m[~mask].any() and not fused.v[~mask].any() and not fused.q_flat[~mask].any()


def snapshot(fused):
    return tuple(x.clone() for x in (fused.q_flat, fused.m, fused.v))


def check_state(tag, fused, snap, t):
    """The update that ``snap`` precedes took Adam's step number t from it, on the kernel's own
    stored gradient, tensor by tensor; the padding is still zero."""
    torch.cuda.synchronize()
    assert float(fused.step) == float(t), (float(fused.step), t)
    hyper = (fused.lr, *fused.betas, fused.eps)
    before = [x.cpu() for x in snap]
    after = [x.detach().cpu() for x in (fused.q_flat, fused.m, fused.v)]
    grad = fused.grad.cpu()
    names = {id(p): n for n, p in fused.q.named_parameters()}
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    for p, at in fused._params(fused.q):
        sl = slice(at, at + p.numel())
        got = check_adam_step(f"{tag} {names[id(p)]}", [x[sl] for x in before], [x[sl] for x in after], t, grad[sl],
                              hyper)
        worst = {k: max(worst[k], got[k]) for k in worst}
    print(f"ADAM-MAX {tag} t={int(t)}: m {worst['m']:.3e} v {worst['v']:.3e} step {worst['p']:.3f} of its bound")
    pad = ~param_mask(fused).cpu()
    for name, x in zip(("q_flat", "m", "v"), after):
        assert not x[pad].any(), (tag, name, "padding written")


def check_image(fused):
    upd = fused.q_image.clone()
    fused.pack("online")
    torch.cuda.synchronize()
    assert torch.equal(upd, fused.q_image)


def check_gradients(tag, fused, grads64):
    worst = (-float("inf"), "")
    for (name, _), g, ref in zip(fused.q.named_parameters(), fused.grads(), grads64):
        err = (g.detach().cpu().double() - ref).abs()
        over = (err - (1e-6 + 1e-3 * ref.abs())).max().item()
        worst = max(worst, (over, f"{name}: kernel err {err.max().item():.2e}"))
        assert over <= 0.0, (tag, name, err.max().item())
    print(f"{tag}: gradient closest to rtol 1e-3 / atol 1e-6: {worst[1]}")


def close(tag, what, got, ref, rtol=1e-5):
    print(f"{tag}: {what} {got!r} float64 {ref!r} (rel {abs(got - ref) / abs(ref):.2e})")
    assert abs(got - ref) <= rtol * abs(ref), (tag, what, got, ref)


def zero_step_optimiser(module):
    """Gradients without a step: the float64 module keeps the weights it was given."""
    return torch.optim.SGD(module.parameters(), lr=0.0)


# ---- BDQ ---------------------------------------------------------------------------------------------
_BDQ = {}


def bdq_case(N, B, K, weighted=False, grad_clamp=1.0, device="cuda"):
    """The inputs of one update at the edge sweeps' seeds, and the float64 reference at the initial
    weights (loss, clamped gradients, priorities), computed once per shape."""
    key = (N, B, K, weighted, grad_clamp, device)
    if key in _BDQ:
        return _BDQ[key]
    spec, seed = edge_spec(N), B + K
    R = bdq_ring(spec, K, seed, device=device)
    idx = pick_rows(R, B, seed)
    kw, w, prio = {}, None, None
    if weighted:                                   # test_gpu_learn_per.py's weights
        idx[3] = idx[7] = idx[1]                   # one ring row three times, each with its own weight
        w = torch.from_numpy((np.random.default_rng(K).random(B) + 0.05).astype(np.float32))
        w[ZERO_AT] = 0.0
        prio = torch.full((B,), -1.0)
        kw = dict(weights=w, priorities_out=prio, replay_constant=RC)
    q_cpu, tgt_cpu = make_nets(N, K, seed=7)
    q64, tgt64 = copy.deepcopy(q_cpu).double(), copy.deepcopy(tgt_cpu).double()
    b64 = batch_of(spec, R, idx, "cpu", torch.float64)
    gap = bdq_top2_gap(q64, b64)
    print(f"N={N} B={B} K={K}: smallest top-2 gap of Q(s') {gap:.3e}")
    assert gap > 1e-4, gap
    loss = bdq_reference_update(q64, tgt64, b64, LR, BDQ_GAMMA, opt=zero_step_optimiser(q64), grad_clamp=grad_clamp,
                                **kw)
    _BDQ[key] = SimpleNamespace(spec=spec, R=R, idx=idx, w=w, q_cpu=q_cpu, tgt_cpu=tgt_cpu, loss=loss, prio=prio,
                                grads=[p.grad.clone() for p in q64.parameters()], grad_clamp=grad_clamp)
    return _BDQ[key]


def run_bdq_update(N, B, K, weighted, t0, grad_clamp=1.0):
    c = bdq_case(N, B, K, weighted, grad_clamp)
    tag = f"bdq N={N} B={B} K={K}" + (" per" if weighted else "") + f" t0={t0}"
    env = VectorPBNEnv(c.spec, 32)
    q, tgt = copy.deepcopy(c.q_cpu).cuda(), copy.deepcopy(c.tgt_cpu).cuda()
    fused = FusedBDQUpdate(q, tgt, env.net, K, batch_size=B, learning_rate=LR, gamma=BDQ_GAMMA, grad_clamp=grad_clamp,
                           keep_grad=True)
    if t0:
        seed_state(fused, t0, seed=t0 % 1000)
    snap = snapshot(fused)
    kw, prio = {}, None
    if weighted:
        prio = torch.full((B,), -1.0, device="cuda")
        kw = dict(weights=c.w.cuda(), priorities_out=prio, replay_constant=RC)
    loss = float(fused.update(c.R, torch.from_numpy(c.idx).cuda(), **kw))
    check_state(tag, fused, snap, t0 + 1)
    close(tag, "loss", loss, c.loss)
    if weighted:
        rel = ((prio.cpu().double() - c.prio.double()).abs() / c.prio.double()).max().item()
        print(f"{tag}: priorities max rel {rel:.3g}")
        assert rel <= 1e-5, rel
        assert prio[ZERO_AT].item() == torch.tensor(RC, dtype=torch.float32).item()      # |0 * l| + rc, exactly
    check_gradients(tag, fused, c.grads)
    check_image(fused)
    _check_image(fused, q, N, K)
    env.close()
    return fused


@pytest.mark.parametrize("t0", SEEDED_T0)
@pytest.mark.parametrize("N,B,K,weighted", BDQ_CASES, ids=BDQ_IDS)
def test_bdq_update_from_a_seeded_state(N, B, K, weighted, t0):
    run_bdq_update(N, B, K, weighted, t0)


def test_bdq_update_to_the_count_two_to_the_24():
    fused = run_bdq_update(33, 16, 3, False, LAST_T0)
    assert float(fused.step) == 2.0 ** 24


@pytest.mark.parametrize("N,B,K,lr", BDQ_TRAJ, ids=[f"N{N}-B{B}-K{K}-lr{lr:g}" for N, B, K, lr in BDQ_TRAJ])
def test_bdq_trajectory_from_zero_state(N, B, K, lr):
    ring_seed, row_seed = SEEDS[("bdq", N, B, K, lr)]
    spec = edge_spec(N)
    env = VectorPBNEnv(spec, 32)
    R = bdq_ring(spec, K, ring_seed)
    q_cpu, tgt_cpu = make_nets(N, K, seed=7)
    q, tgt = copy.deepcopy(q_cpu).cuda(), copy.deepcopy(tgt_cpu).cuda()
    q64, tgt64 = copy.deepcopy(q_cpu).double(), copy.deepcopy(tgt_cpu).double()
    fused = FusedBDQUpdate(q, tgt, env.net, K, batch_size=B, learning_rate=lr, gamma=BDQ_GAMMA, keep_grad=True)
    for k in range(STEPS):
        tag = f"bdq N={N} B={B} K={K} lr={lr:g} update {k + 1}"
        idx = pick_rows(R, B, row_seed + k)
        # the float64 modules at the kernel's current weights
        q64.load_state_dict(q.state_dict())
        tgt64.load_state_dict(tgt.state_dict())
        b64 = batch_of(spec, R, idx, "cpu", torch.float64)
        gap = bdq_top2_gap(q64, b64)
        print(f"{tag}: smallest top-2 gap of Q(s') {gap:.3e}")
        assert gap > 1e-4, (k, gap)
        loss_ref = bdq_reference_update(q64, tgt64, b64, lr, BDQ_GAMMA, opt=zero_step_optimiser(q64))
        snap = snapshot(fused)
        loss = float(fused.update(R, torch.from_numpy(idx).cuda()))
        check_state(tag, fused, snap, k + 1)
        close(tag, "loss", loss, loss_ref)
        check_gradients(tag, fused, [p.grad for p in q64.parameters()])
        check_image(fused)
        if k == 1:      # the soft target update; updates 3 and 4 run against the moved target
            t_prev = fused.t_flat.clone()
            fused.soft_update()
            torch.cuda.synchronize()
            assert torch.equal(fused.t_flat, t_prev.div(2).add(fused.q_flat / 2))
            assert not torch.equal(fused.t_flat, t_prev)
            t_image = fused.t_image.clone()
            fused.pack("target")
            torch.cuda.synchronize()
            assert torch.equal(t_image, fused.t_image)
    env.close()


@pytest.mark.parametrize("t0", [0, 6])
def test_bdq_element_clamp_active(t0):
    """grad_clamp at the median non-zero |g| of the float64 reference gradient: between a quarter and
    three quarters of its non-zero entries exceed it, the kernel's stored gradient is the clamped
    reference (run_bdq_update's gradient check, against bdq_update at that clamp), and Adam steps
    from it, from zero state and from a seeded one."""
    N, B, K = 33, 16, 3
    free = bdq_case(N, B, K, grad_clamp=1e30)
    mag = torch.cat([g.abs().reshape(-1) for g in free.grads])
    mag = mag[mag > 0]
    clampv = float(mag.median())
    over = float((mag > clampv).double().mean())
    print(f"grad_clamp {clampv:.3e}: {over:.3f} of {mag.numel()} non-zero reference entries exceed it "
          f"(max {float(mag.max()):.3e})")
    assert 0.25 <= over <= 0.75, over
    c = bdq_case(N, B, K, grad_clamp=clampv)
    for g, g_free in zip(c.grads, free.grads):
        assert torch.equal(g, g_free.clamp(-clampv, clampv))
    fused = run_bdq_update(N, B, K, False, t0, grad_clamp=clampv)
    at = fused.grad.abs() == np.float32(clampv)                 # the ABI's float
    print(f"{int(at.sum())} stored gradient entries sit at the clamp")
    assert 0.2 * mag.numel() <= int(at.sum()) <= 0.8 * mag.numel()
    assert float(fused.grad.abs().max()) == float(np.float32(clampv))


# ---- DDQN --------------------------------------------------------------------------------------------
_DDQN = {}


def ddqn_case(N, arch, weighted, device="cuda"):
    """The inputs of one update (the edge sweeps' ring and rows at B = 16) and the float64 reference
    at the initial weights, computed once per shape."""
    key = (N, arch, weighted, device)
    if key in _DDQN:
        return _DDQN[key]
    spec, B, R, a, idx, w = ddqn_inputs(N, DDQN_B, 100 + N, device=device)
    q_cpu, tgt_cpu = make_dqn_nets(N, arch, seed=7)
    q64, tgt64 = copy.deepcopy(q_cpu).double(), copy.deepcopy(tgt_cpu).double()
    batch64 = batch64_of(_batch(spec, a, idx, device="cpu"))
    gap = ddqn_conditions(q64, tgt64, batch64, DDQN_GAMMA)[0]
    print(f"N={N} {arch}: smallest top-2 gap of Q(s') {gap:.3e}")
    assert gap > 1e-4, gap
    w64 = torch.from_numpy(w).double() if weighted else None
    probe = copy.deepcopy(q64)
    norm0 = float(ddqn_update(probe, tgt64, zero_step_optimiser(probe), batch64, DDQN_GAMMA, 1e30, weights=w64)[1])
    assert norm0 > 1e-6, norm0
    max_norm = 10.0 * max(norm0, 1.0)              # nothing clips (the edge sweeps' "noclip")
    prio = torch.full((B,), -1.0, dtype=torch.float64) if weighted else None
    loss, norm = ddqn_update(q64, tgt64, zero_step_optimiser(q64), batch64, DDQN_GAMMA, max_norm, weights=w64,
                             priorities_out=prio, replay_constant=RC)
    _DDQN[key] = SimpleNamespace(spec=spec, R=R, idx=idx, w=w, q_cpu=q_cpu, tgt_cpu=tgt_cpu, loss=float(loss),
                                 norm=float(norm), prio=prio, max_norm=max_norm,
                                 grads=[p.grad.clone() for p in q64.parameters()])
    return _DDQN[key]


def run_ddqn_update(N, arch, weighted, t0):
    c = ddqn_case(N, arch, weighted)
    tag = f"ddqn N={N} {arch}" + (" per" if weighted else "") + f" t0={t0}"
    env = VectorPBNEnv(c.spec, 32)
    q, tgt = copy.deepcopy(c.q_cpu).cuda(), copy.deepcopy(c.tgt_cpu).cuda()
    fused = FusedDDQNUpdate(q, tgt, env.net, batch_size=DDQN_B, learning_rate=LR, gamma=DDQN_GAMMA,
                            max_grad_norm=c.max_norm, keep_grad=True)
    seed_state(fused, t0, seed=t0 % 1000)
    snap = snapshot(fused)
    kw, prio = {}, None
    if weighted:
        prio = torch.full((DDQN_B,), -1.0, device="cuda")
        kw = dict(weights=torch.from_numpy(c.w).cuda(), priorities_out=prio, replay_constant=RC)
    loss = float(fused.update(c.R, torch.from_numpy(c.idx).cuda(), **kw))
    check_state(tag, fused, snap, t0 + 1)
    close(tag, "loss", loss, c.loss)
    close(tag, "norm", float(fused.grad_norm), c.norm)
    if weighted:
        rel = ((prio.cpu().double() - c.prio).abs() / c.prio).max().item()
        print(f"{tag}: priorities max rel {rel:.3g}")
        assert rel <= FLOAT_BOUNDS.get(("ddqn_priorities", N, arch), (None, 1e-5))[1], rel
        assert prio[ZERO_AT].item() == torch.tensor(RC, dtype=torch.float32).item()      # |0 * h| + rc, exactly
    check_gradients(tag, fused, c.grads)
    check_image(fused)
    env.close()
    return fused


@pytest.mark.parametrize("t0", SEEDED_T0)
@pytest.mark.parametrize("N,arch,weighted", DDQN_CASES, ids=DDQN_IDS)
def test_ddqn_update_from_a_seeded_state(N, arch, weighted, t0):
    run_ddqn_update(N, arch, weighted, t0)


def test_ddqn_update_to_the_count_two_to_the_24():
    fused = run_ddqn_update(33, (17, 64), False, LAST_T0)
    assert float(fused.step) == 2.0 ** 24


@pytest.mark.parametrize("N,arch,lr,clip", DDQN_TRAJ,
                         ids=[f"N{N}-{a}x{b}-lr{lr:g}" + ("-clip" if c else "") for N, (a, b), lr, c in DDQN_TRAJ])
def test_ddqn_trajectory_from_zero_state(N, arch, lr, clip):
    ring_seed, row_seed = SEEDS[("ddqn", N, arch, lr, clip)]
    spec, B = edge_spec(N), DDQN_B
    env = VectorPBNEnv(spec, 32)
    R, a = _ring(spec, DDQN_CAP, seed=ring_seed)
    q_cpu, tgt_cpu = make_dqn_nets(N, arch, seed=7)
    q, tgt = copy.deepcopy(q_cpu).cuda(), copy.deepcopy(tgt_cpu).cuda()
    q64, tgt64 = copy.deepcopy(q_cpu).double(), copy.deepcopy(tgt_cpu).double()
    # the first update's float64 norm decides what clips: half of it (every update clips), or far above it
    b0 = batch64_of(_batch(spec, a, ddqn_trajectory_rows(B, row_seed, 0), device="cpu"))
    probe = copy.deepcopy(q64)
    norm0 = float(ddqn_update(probe, tgt64, zero_step_optimiser(probe), b0, DDQN_GAMMA, 1e30)[1])
    max_norm = 0.5 * norm0 if clip else 10.0 * max(norm0, 1.0)
    fused = FusedDDQNUpdate(q, tgt, env.net, batch_size=B, learning_rate=lr, gamma=DDQN_GAMMA, max_grad_norm=max_norm,
                            keep_grad=True)
    for k in range(STEPS):
        tag = f"ddqn N={N} {arch} lr={lr:g}" + (" clip" if clip else "") + f" update {k + 1}"
        idx = ddqn_trajectory_rows(B, row_seed, k)
        q64.load_state_dict(q.state_dict())
        tgt64.load_state_dict(tgt.state_dict())
        batch64 = batch64_of(_batch(spec, a, idx, device="cpu"))
        gap = ddqn_conditions(q64, tgt64, batch64, DDQN_GAMMA)[0]
        print(f"{tag}: smallest top-2 gap of Q(s') {gap:.3e}")
        assert gap > 1e-4, (k, gap)
        loss_ref, norm_ref = (float(x) for x in ddqn_update(q64, tgt64, zero_step_optimiser(q64), batch64, DDQN_GAMMA,
                                                            max_norm))
        assert (norm_ref > max_norm) == clip, (k, norm_ref, max_norm)
        snap = snapshot(fused)
        loss = float(fused.update(R, torch.from_numpy(idx).cuda()))
        check_state(tag, fused, snap, k + 1)
        close(tag, "loss", loss, loss_ref)
        close(tag, "norm", float(fused.grad_norm), norm_ref)
        check_gradients(tag, fused, [p.grad for p in q64.parameters()])
        check_image(fused)
        if k == 1:      # the hard target copy; updates 3 and 4 run against the moved target
            t_prev = fused.t_flat.clone()
            fused.sync_target()
            torch.cuda.synchronize()
            assert torch.equal(fused.t_flat, fused.q_flat) and torch.equal(fused.t_image, fused.q_image)
            assert not torch.equal(fused.t_flat, t_prev)
    env.close()
