"""NaN and infinite values fed into the fused updates (DESIGN.md "Non-finite values"): one update from
zero Adam state, B = 16: FusedDDQNUpdate clipped and unclipped, FusedBDQUpdate, each uniform and
weighted, against ddqn_update / bdq_update + torch.optim.Adam on the CPU (tests/nonfinite_cases.py):
in fp32 for the pattern of NaN, +inf and -inf of the loss, the norm, the priorities and every parameter, m and v; in float64 for
whatever is finite, at test_gpu_ddqn_edges.py's tolerances (loss, norm and priorities rtol 1e-5;
clipped gradients rtol 1e-3 / atol 1e-6; the Adam step from the kernel's own gradient rtol 1e-5 /
atol 1e-7).  A diverged update must look diverged: a NaN TD error makes the loss, the norm and every
parameter NaN, as it does in PyTorch."""
import copy

import pytest
import torch

from pbn_rl_amd.ddqn import FusedDDQNUpdate
from pbn_rl_amd.replay import FusedBDQUpdate
from pbn_rl_amd.vector_env import VectorPBNEnv
from tests import nonfinite_cases as C

pytestmark = pytest.mark.gpu

_INPUTS = {}


def the_inputs(shape, arch):
    """One ring on the device per shape, with its host arrays, rows, weights, networks and env."""
    if (shape, arch) not in _INPUTS:
        spec, R, a, idx, w, q, tgt = C.ddqn_update_inputs(shape, arch, device="cuda")
        _INPUTS[(shape, arch)] = (spec, R, a, idx, w, q, tgt, VectorPBNEnv(spec, 32))
    return _INPUTS[(shape, arch)]


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("name,weighted", C.DDQN_UPD_RUNS, ids=C.DDQN_UPD_RUN_IDS)
@pytest.mark.parametrize("shape,arch", C.DDQN_UPD_SHAPES, ids=C.DDQN_UPD_IDS)
def test_ddqn_update_is_pytorchs(shape, arch, name, weighted, clip):
    spec, R, a0, idx, w0, q0, tgt0, env = the_inputs(shape, arch)
    B = C.B
    max_norm = C.max_norm_of(spec, a0, idx, w0, q0, tgt0, weighted, clip)
    a, w, q_cpu, tgt_cpu, row = C.ddqn_case(name, spec, a0, idx, w0, q0, tgt0)
    r32, r64 = C.ddqn_refs(name, spec, a, idx, w, q_cpu, tgt_cpu, max_norm, weighted)
    expect = C.DDQN_UPD_CASES[name]
    q, tgt = copy.deepcopy(q_cpu).cuda(), copy.deepcopy(tgt_cpu).cuda()
    fused = FusedDDQNUpdate(q, tgt, env.net, batch_size=B, learning_rate=C.LR, gamma=C.GAMMA, max_grad_norm=max_norm,
                            keep_grad=True)
    p0 = [p.detach().clone() for p in q.parameters()]
    clean_reward = float(R.reward[row]) if row is not None else None
    if row is not None:
        R.reward[row] = C.REWARDS[name]
    try:
        wt = torch.from_numpy(w).cuda() if weighted else None
        prio = torch.full((B,), -1.0, device="cuda") if weighted else None
        loss = fused.update(R, torch.from_numpy(idx).cuda(), weights=wt, priorities_out=prio, replay_constant=C.RC)
        torch.cuda.synchronize()
    finally:
        if row is not None:
            R.reward[row] = clean_reward
    loss, norm = loss.reshape(1).cpu(), fused.grad_norm.cpu()
    print(f"{shape} {arch} {name} weighted={weighted} clip={clip}: loss {float(loss)!r} ref {float(r64['loss'])!r}; "
          f"norm {float(norm)!r} ref {float(r64['norm'])!r}")
    C.assert_same_pattern(loss, r32["loss"], "loss")
    C.assert_same_pattern(norm, r32["norm"], "norm")
    C.check_finite(loss, r64["loss"], 1e-5, 0.0, "loss")
    C.check_finite(norm, r64["norm"], 1e-5, 0.0, "norm")
    assert float(fused.step) == 1.0
    if weighted:
        C.assert_same_pattern(prio, r32["prio"], "priorities")
        C.check_finite(prio, r64["prio"], 1e-5, 0.0, "priorities")
        if row is not None:
            # the injected row's priority alone is not finite; the others are the clean run's
            clean = C.ddqn_reference(spec, a0, idx, w0, q0, tgt0, max_norm, True, torch.float64)["prio"]
            bad = ~torch.isfinite(prio.cpu())
            assert bad.nonzero().flatten().tolist() == [C.ROW]
            assert bool(torch.isnan(prio[C.ROW])) if expect == "nan" else bool(torch.isposinf(prio[C.ROW]))
            assert torch.allclose(prio.cpu().double()[~bad], clean[~bad], rtol=1e-5, atol=0)
        if name == "target_out_bias_nan":
            bad = torch.isnan(prio.cpu())
            assert 0 < int(bad.sum()) < B and torch.equal(bad, torch.isnan(r32["prio"]))
    names = [n for n, _ in q.named_parameters()]
    seg = {id(p): at for p, at in fused._params(q)}
    for n, p, g, before in zip(names, q.parameters(), fused.grads(), p0):
        at = seg[id(p)]
        m, v = (buf[at:at + p.numel()].view(p.shape) for buf in (fused.m, fused.v))
        for key, got in (("grad", g), ("p", p.detach()), ("m", m), ("v", v)):
            C.assert_same_pattern(got, r32[n][key], f"{n} {key}")
        if expect == "nan":
            assert all(bool(torch.isnan(t).all()) for t in (g, p.detach(), m, v)), n
        else:
            err = (g.cpu().double() - r64[n]["grad"]).abs()
            assert (err - (1e-6 + 1e-3 * r64[n]["grad"].abs())).max().item() <= 0.0, (n, err.max().item())
            b1, b2, eps = 0.9, 0.999, 1e-8
            m1, v1 = (1 - b1) * g, (1 - b2) * g * g
            want = before - (C.LR / (1 - b1)) * m1 / (v1.sqrt() / (1 - b2) ** 0.5 + eps)
            assert torch.allclose(p.detach(), want, rtol=1e-5, atol=1e-7), (n, (p.detach() - want).abs().max().item())
    if expect == "finite":
        assert (float(r64["norm"]) > max_norm) == clip
        if not clip:
            # the infinite row's TD error is clamped: its gradient is -+ w / B where the clean row's is
            # clamp(delta) w / B, and no other row's changed (unclipped: every coefficient is 1)
            clean = C.ddqn_reference(spec, a0, idx, w0, q0, tgt0, max_norm, weighted, torch.float64)
            assert float(clean["norm"]) <= max_norm
            act = int(a["act"][row, 0])
            d = float(C.clean_deltas(spec, a0, idx, q0, tgt0)[C.ROW].clamp(-1, 1))
            sign = -1.0 if name == "reward_pinf" else 1.0
            want = (sign - d) * (float(w[C.ROW]) if weighted else 1.0) / B
            got = float(fused.grads()[names.index("output.bias")][act]) - float(clean["output.bias"]["grad"][act])
            assert abs(got - want) <= 2e-6 + 1e-3 * abs(want), (got, want)
    # the padding of the flat buffers stays zero, whatever the segments hold
    real = torch.zeros_like(fused.q_flat, dtype=torch.bool)
    for p, at in fused._params(q):
        real[at:at + p.numel()] = True
    for buf in (fused.q_flat, fused.m, fused.v, fused.grad):
        assert not bool(buf[~real].any())
    upd = fused.q_image.clone()
    fused.pack("online")
    torch.cuda.synchronize()
    assert torch.equal(upd.view(torch.int32), fused.q_image.view(torch.int32))


# ---- BDQ --------------------------------------------------------------------------------------------
_BDQ_INPUTS = {}


def the_bdq_inputs(shape, K):
    if (shape, K) not in _BDQ_INPUTS:
        spec, R, idx, pos, w, q, tgt = C.bdq_update_inputs(shape, K, device="cuda")
        _BDQ_INPUTS[(shape, K)] = (spec, R, idx, pos, w, q, tgt, VectorPBNEnv(spec, 32))
    return _BDQ_INPUTS[(shape, K)]


@pytest.mark.parametrize("name,weighted", C.BDQ_UPD_RUNS, ids=C.BDQ_UPD_RUN_IDS)
@pytest.mark.parametrize("shape,K", C.BDQ_SHAPES, ids=C.BDQ_IDS)
def test_bdq_update_is_pytorchs(shape, K, name, weighted):
    """FusedBDQUpdate (pbn_bdq_learn, and pbn_bdq_learn_per with weights) with one sampled row's reward
    NaN, +inf or -inf, and with weight 0 on the NaN row: the loss, the priorities and the pattern of
    every segment's clamped gradient, parameter, m and v are the fp32 reference's; what is finite
    equals the float64 reference at test_gpu_learn_edges.py's tolerances.  The bilinear weight's
    gradient is accumulated from the set (state, target) bits, where PyTorch's dense product puts a
    row's NaN into every element: for that segment only 'holds a NaN' is compared."""
    spec, R, idx, pos, w0, q_cpu, tgt_cpu, env = the_bdq_inputs(shape, K)
    B, row = C.B, int(idx[pos])
    w = w0.copy()
    if name == "weight0_nan":
        w[pos] = 0.0
    clean_reward = float(R.reward[row])
    R.reward[row] = C.REWARDS[name]
    try:
        r32, r64 = C.bdq_refs(spec, R, idx, w, q_cpu, tgt_cpu, weighted)
        q, tgt = copy.deepcopy(q_cpu).cuda(), copy.deepcopy(tgt_cpu).cuda()
        fused = FusedBDQUpdate(q, tgt, env.net, K, batch_size=B, learning_rate=C.LR, gamma=C.BDQ_GAMMA, keep_grad=True)
        p0 = [p.detach().clone() for p in q.parameters()]
        wt = torch.from_numpy(w).cuda() if weighted else None
        prio = torch.full((B,), -1.0, device="cuda") if weighted else None
        loss = fused.update(R, torch.from_numpy(idx).cuda(), weights=wt, priorities_out=prio, replay_constant=C.RC)
        torch.cuda.synchronize()
    finally:
        R.reward[row] = clean_reward
    loss = loss.reshape(1).cpu()
    print(f"{shape} K={K} {name} weighted={weighted}: loss {float(loss)!r} ref {float(r64['loss'])!r}")
    C.assert_same_pattern(loss, r32["loss"], "loss")
    C.check_finite(loss, r64["loss"], 1e-5, 0.0, "loss")
    assert float(fused.step) == 1.0
    if weighted:
        C.assert_same_pattern(prio, r32["prio"], "priorities")
        C.check_finite(prio, r64["prio"], 1e-5, 0.0, "priorities")
        assert (~torch.isfinite(prio.cpu())).nonzero().flatten().tolist() == [pos]
    names = [n for n, _ in q.named_parameters()]
    seg = {id(p): at for p, at in fused._params(q)}
    b1, b2, eps = 0.9, 0.999, 1e-8
    for n, p, g, before in zip(names, q.parameters(), fused.grads(), p0):
        at = seg[id(p)]
        m, v = (buf[at:at + p.numel()].view(p.shape) for buf in (fused.m, fused.v))
        for key, got in (("grad", g), ("p", p.detach()), ("m", m), ("v", v)):
            if n == C.BDQ_BILINEAR_WEIGHT:
                assert bool(torch.isnan(got).any()) == bool(torch.isnan(r32[n][key]).any()), (n, key)
            else:
                C.assert_same_pattern(got, r32[n][key], f"{n} {key}")
        if n != C.BDQ_BILINEAR_WEIGHT:
            fin = torch.isfinite(r64[n]["grad"])
            err = (g.cpu().double() - r64[n]["grad"]).abs()[fin]
            assert fin.sum() == 0 or (err - (1e-6 + 1e-3 * r64[n]["grad"][fin].abs())).max().item() <= 0.0, (n, err.max())
        # Adam's first step from the kernel's own gradient, wherever that is finite
        m1, v1 = (1 - b1) * g, (1 - b2) * g * g
        want = before - (C.LR / (1 - b1)) * m1 / (v1.sqrt() / (1 - b2) ** 0.5 + eps)
        ok = torch.isfinite(want)
        assert torch.allclose(p.detach()[ok], want[ok], rtol=1e-5, atol=1e-7), n
        assert torch.equal(torch.isnan(p.detach()), torch.isnan(g)), n     # a NaN gradient, and only that, a NaN weight
