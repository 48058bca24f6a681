"""The fused BDQ update (pbn_bdq_learn, csrc/pbn_learn.hip) at every action-tile and state-word
edge (tests/edge_shapes.py): N = 15 .. 127 runs every bilinear j-tile count NT = 1 .. 8 of
learn_apply_kernel, Apad on both sides of 16, 32, 64, 96 and 128, and 1 .. 4 state words, where the
bundled networks run NT = 1, 2 and 5 and W <= 3.

Reference: bdq_update (replay.py) on float64 copies of both networks and of the batch, as PyTorch
expressions on the CPU.  Tolerances are test_gpu_learn.py's for the same quantities, against that
float64 reference: loss rtol 1e-5; clamped gradients rtol 1e-3 / atol 1e-6; the Adam step from the
kernel's own gradient rtol 1e-5 / atol 1e-7; the image after the update bit-equal to a fresh pack
(edge_shapes.FLOAT_BOUNDS lists any shape that needs another bound and why).  The reference's
input condition is asserted: no online Q(s') row has its two largest entries within 1e-4 (the
double-DQN argmax is then the same in float32 and float64)."""
import copy
import ctypes

import pytest
import torch

from pbn_rl_amd import _lib
from pbn_rl_amd.replay import FusedBDQUpdate, bdq_update, fused_update_supported
from pbn_rl_amd.vector_env import VectorPBNEnv
from tests.edge_shapes import EDGE_N, edge_spec, u32
from tests.edge_updates import batch_of, bdq_reference_update, bdq_ring, bdq_top2_gap, make_nets, pick_rows
from tests.test_gpu_learn import _check_image

pytestmark = pytest.mark.gpu

SHAPES = ([(N, B, 3) for N in EDGE_N for B in (16, 48)]
          + [(33, 16, 1), (33, 48, 7), (95, 48, 1), (95, 16, 7)])
# the ring / index seed of a shape is B + K (test_gpu_learn.py's); these shapes take another one,
# for which the float64 reference meets the no-tie condition
SEEDS = {(65, 48, 3): 1013, (96, 48, 3): 1000}


def run_update(N, B, K):
    spec = edge_spec(N)
    seed = SEEDS.get((N, B, K), B + K)
    env = VectorPBNEnv(spec, 32)
    R = bdq_ring(spec, K, seed)
    idx = pick_rows(R, B, seed)
    st = u32(R.state[:, torch.from_numpy(idx).cuda()])
    assert not st[:, 0].any() and sum(bin(int(x)).count("1") for x in st[:, 1]) == N
    q_cpu, tgt_cpu = make_nets(N, K, seed=7)
    q, tgt = copy.deepcopy(q_cpu).cuda(), copy.deepcopy(tgt_cpu).cuda()
    q64, tgt64 = copy.deepcopy(q_cpu).double(), copy.deepcopy(tgt_cpu).double()
    q32, tgt32 = copy.deepcopy(q), copy.deepcopy(tgt)
    lr, gamma = 1e-3, 0.9
    # the float64 reference and its input condition
    b64 = batch_of(spec, R, idx, "cpu", torch.float64)
    gap = bdq_top2_gap(q64, b64)
    print(f"N={N} B={B} K={K}: smallest top-2 gap of Q(s') {gap:.3e}")
    assert gap > 1e-4, gap
    loss_ref = bdq_reference_update(q64, tgt64, b64, lr, gamma)
    # the PyTorch fp32 update on the same batch (printed beside the kernel's errors)
    opt32 = torch.optim.Adam(q32.parameters(), lr=lr)
    loss32 = float(bdq_update(q32, tgt32, opt32, batch_of(spec, R, idx, "cuda", torch.float32), gamma))
    fused = FusedBDQUpdate(q, tgt, env.net, K, batch_size=B, learning_rate=lr, gamma=gamma, keep_grad=True)
    p0 = [p.detach().clone() for p in q.parameters()]
    loss = float(fused.update(R, torch.from_numpy(idx).cuda()))
    torch.cuda.synchronize()
    print(f"  loss {loss!r} float64 {loss_ref!r} (rel {abs(loss - loss_ref) / abs(loss_ref):.2e}); "
          f"PyTorch fp32 {loss32!r} (rel {abs(loss32 - loss_ref) / abs(loss_ref):.2e})")
    assert abs(loss - loss_ref) <= 1e-5 * abs(loss_ref), (loss, loss_ref)
    names = [n for n, _ in q.named_parameters()]
    worst = (-float("inf"), "")
    for name, g, p, p32 in zip(names, fused.grads(), q64.parameters(), q32.parameters()):
        ref = p.grad.cuda()
        over = ((g.double() - ref).abs() - (1e-6 + 1e-3 * ref.abs())).max().item()
        e32 = (p32.grad.double() - ref).abs().max().item()
        worst = max(worst, (over, f"{name}: kernel err {(g.double() - ref).abs().max().item():.2e}, fp32 {e32:.2e}"))
        assert over <= 0.0, (name, (g.double() - ref).abs().max().item(), e32)
    print("  gradient closest to its bound:", worst[1])
    # Adam's first step from the kernel's own gradient (torch.optim.Adam's arithmetic)
    b1, b2, eps = 0.9, 0.999, 1e-8
    for name, g, a, b in zip(names, fused.grads(), p0, q.parameters()):
        m, v = (1 - b1) * g, (1 - b2) * g * g
        want = a - (lr / (1 - b1)) * m / (v.sqrt() / (1 - b2) ** 0.5 + eps)
        assert torch.allclose(b, want, rtol=1e-5, atol=1e-7), (name, (b - want).abs().max().item())
    assert float(fused.step) == 1.0
    # the value head's padding (outputs past 0) stays zero in the flat buffer
    o, A = fused.off, N + 1
    assert not fused.q_flat[o[10] + 64:o[10] + A * 64].any() and not fused.q_flat[o[11] + 1:o[11] + A].any()
    # the online image written by the update = pbn_bdq_pack of the new weights, bit for bit
    t_upd = fused.q_image.clone()
    fused.pack("online")
    assert torch.equal(t_upd, fused.q_image)
    _check_image(fused, q, N, K)
    targets = torch.tensor([list(a[0]) for a in spec.attractors], dtype=torch.float64, device="cuda")
    T = copy.deepcopy(q).double().model[0].target_table(targets)
    got = fused.q_table.transpose(2, 3).reshape(T.shape).double()
    assert torch.allclose(got, T, rtol=1e-5, atol=1e-6), (got - T).abs().max().item()
    env.close()


@pytest.mark.parametrize("N,B,K", SHAPES)
def test_fused_update_matches_pytorch_in_float64(N, B, K):
    run_update(N, B, K)


def test_lds_limit_refusal_boundary():
    """The backward's LDS (learn_bwd_lds) bounds (K + 1) x Apad: K = 7 fits at N = 95 (Apad = 96;
    the update there is the (95, 16, 7) case above) and is refused from N = 96 (Apad = 112), by the
    workspace query and by FusedBDQUpdate, which launches nothing."""
    L = _lib.load()
    nb = ctypes.c_int64(-1)
    assert L.pbn_bdq_learn_workspace(95, 7, 16, ctypes.byref(nb)) == 0 and nb.value > 0
    assert fused_update_supported(95, 7, 16)
    nb = ctypes.c_int64(-1)
    assert L.pbn_bdq_learn_workspace(96, 7, 16, ctypes.byref(nb)) == -22
    assert "too large for one block's LDS" in L.pbn_last_error().decode()
    assert nb.value == -1 and not fused_update_supported(96, 7, 16)
    assert L.pbn_bdq_learn_workspace(96, 6, 16, ctypes.byref(nb)) == 0      # one head fewer fits
    spec = edge_spec(96)
    env = VectorPBNEnv(spec, 32)
    q, tgt = make_nets(96, 7, seed=7)
    q, tgt = q.cuda(), tgt.cuda()
    before = [p.detach().clone() for p in q.parameters()]
    with pytest.raises(_lib.PbnError, match="too large for one block's LDS"):
        FusedBDQUpdate(q, tgt, env.net, 7, batch_size=16)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, q.parameters()))
    FusedBDQUpdate(*[m.cuda() for m in make_nets(96, 6, seed=7)], env.net, 6, batch_size=16)
    env.close()
