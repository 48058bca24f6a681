"""Adam past its first step: the float64 reference the fused updates' optimiser is held to
(learn_apply_kernel, csrc/learn_apply.h; ddqn_adam_kernel, csrc/pbn_ddqn.hip), its bounds, and the
seeded moments the tests start from (test_adam_reference_host.py, test_gpu_adam_state.py).

The kernels take lr, beta1, beta2 and eps as ``float``, so their contract is torch.optim.Adam at
those four values rounded to fp32; ``t`` is the step count after the increment.

Bounds of check_adam_step, for a correct fp32 evaluation of the kernels' expression:
  m   |m_k - m_ref| <= 2^-22 (|b1 m| + |(1 - b1) g|): three fp32 roundings of a two-term sum.
  v   |v_k - v_ref| <= 2^-21 v_ref: all terms positive, four roundings.
  p   on the step D = after - before, |D_k - D_ref| <= 1e-4 |D_ref| + 1e-5 lr + ulp(before):
      1 - b2^t cancels in fp32 (at most two ulps of powf over 1 - b2 ~ 1e-3, halved by the square
      root); m' cancels when m and g oppose (at most about 2^-23 |m| / sqrt(v) <= 2^-23 / sqrt(1 - b2)
      of lr); and p itself is rounded.
test_adam_reference_host.py shows that adam_step32_restated meets them at every (lr, start count)
the GPU tests use, and that three wrong restatements do not."""
import numpy as np
import torch

BETAS, EPS = (0.9, 0.999), 1e-8
LRS = (1e-3, 1e-4)
SEEDED_T0 = (1, 6, 999)         # start counts of the seeded-state cases: the counts asserted are 2, 7, 1000
LAST_T0 = 2 ** 24 - 1           # the count becomes exactly 2^24 and both bias corrections are 1
STEPS = 4                       # a trajectory's updates, from zero state

M_BOUND, V_BOUND = 2.0 ** -22, 2.0 ** -21
P_REL, P_LR = 1e-4, 1e-5


def fp32_hyper(lr, b1=BETAS[0], b2=BETAS[1], eps=EPS):
    """The four hyperparameters as the ABI passes them: rounded to fp32 (returned as Python floats)."""
    return tuple(float(np.float32(x)) for x in (lr, b1, b2, eps))


def adam_step64(p, m, v, t, g, lr, b1, b2, eps):
    """One torch.optim.Adam step in float64 on fp32 (or float64) tensors; the hyperparameters are
    rounded to fp32 first.  Returns (p', m', v') as float64."""
    lr, b1, b2, eps = fp32_hyper(lr, b1, b2, eps)
    p, m, v, g = (x.detach().double() for x in (p, m, v, g))
    t = float(t)
    m1 = b1 * m + (1 - b1) * g
    v1 = b2 * v + (1 - b2) * g * g
    p1 = p - lr / (1 - b1 ** t) * m1 / (v1.sqrt() / (1 - b2 ** t) ** 0.5 + eps)
    return p1, m1, v1


def adam_step32_restated(p, m, v, t, g, lr, b1, b2, eps):
    """The kernels' own expression (adam_apply, learn_apply.h; ddqn_adam_kernel), in their order, in
    fp32 numpy on the CPU.  Only ever used to show that a correct fp32 evaluation meets the bounds,
    never as what a kernel is compared with.  Returns (p', m', v') as fp32 tensors."""
    f = np.float32
    lr, b1, b2, eps, one, tc = f(lr), f(b1), f(b2), f(eps), f(1), f(t)
    p, m, v, g = (x.detach().cpu().numpy().astype(f) for x in (p, m, v, g))
    bc1 = one - np.power(b1, tc)
    bc2s = np.sqrt(one - np.power(b2, tc))
    m1 = b1 * m + (one - b1) * g
    v1 = b2 * v + (one - b2) * g * g
    denom = np.sqrt(v1) / bc2s + eps
    p1 = p - (lr / bc1) * m1 / denom
    assert p1.dtype == m1.dtype == v1.dtype == f
    return torch.from_numpy(p1), torch.from_numpy(m1), torch.from_numpy(v1)


def seed_moments(shape, gen):
    """Non-zero moments for a parameter of ``shape``, drawn per element from the CPU generator
    ``gen``: m = 1e-2 randn, v = (|m| U(0.5, 2))^2 + 1e-12.  Independent draws, so a moment loaded
    from a neighbouring element moves the result."""
    m = 1e-2 * torch.randn(shape, generator=gen)
    m = torch.where(m == 0, torch.full_like(m, 1e-2), m)
    u = 0.5 + 1.5 * torch.rand(shape, generator=gen)
    v = (m.abs() * u) ** 2 + 1e-12
    return m.float(), v.float()


def _ulp(x):
    """The spacing of fp32 at |x| (fp32 tensor), as float64."""
    a = x.detach().float().abs()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def adam_errors(before, after, t, g, hyper):
    """The three quantities' errors over their bounds, elementwise: (m, v, p) float64 tensors of
    error / bound (<= 1 passes), then the parameter step's plain relative error (for the record)."""
    lr = fp32_hyper(*hyper)[0]
    p0, m0, v0 = (x.detach().cpu() for x in before)
    p1, m1, v1 = (x.detach().cpu() for x in after)
    g = g.detach().cpu()
    for x in (p0, m0, v0, p1, m1, v1, g):
        assert x.dtype == torch.float32, x.dtype
    p_ref, m_ref, v_ref = adam_step64(p0, m0, v0, t, g, *hyper)
    b1 = fp32_hyper(*hyper)[1]
    m_scale = (b1 * m0.double()).abs() + ((1 - b1) * g.double()).abs()
    tiny = torch.finfo(torch.float64).tiny
    em = (m1.double() - m_ref).abs() / (M_BOUND * m_scale).clamp_min(tiny)
    ev = (v1.double() - v_ref).abs() / (V_BOUND * v_ref).clamp_min(tiny)
    d_k, d_ref = p1.double() - p0.double(), p_ref - p0.double()
    ep = (d_k - d_ref).abs() / (P_REL * d_ref.abs() + P_LR * lr + _ulp(p0))
    rel = (d_k - d_ref).abs() / d_ref.abs().clamp_min(tiny)
    return em, ev, ep, rel


def check_adam_step(name, before, after, t, g, hyper):
    """One Adam step of a kernel against adam_step64.  ``before`` / ``after``: (p, m, v) fp32
    tensors of one shape, ``t`` the count after the increment, ``g`` the gradient the step used
    (fp32), ``hyper`` = (lr, b1, b2, eps).  Prints each quantity's measured maximum beside its
    bound, as edge_shapes.check_close does, then asserts the three bounds.  Returns the maxima (m
    and v in units of their scale, the parameter step as error over its bound)."""
    em, ev, ep, rel = adam_errors(before, after, t, g, hyper)
    mm, vm, pm = (float(e.max()) if e.numel() else 0.0 for e in (em, ev, ep))
    got = {"m": mm * M_BOUND, "v": vm * V_BOUND, "p": pm}
    rel_max = float(rel.max()) if rel.numel() else 0.0
    print(f"{name} t={int(t)}: m err {got['m']:.3e} of |b1 m| + |(1-b1) g| (bound {M_BOUND:.3e}); "
          f"v err {got['v']:.3e} of v (bound {V_BOUND:.3e}); step err {pm:.3f} of its bound "
          f"{P_REL:g}|D| + {P_LR:g} lr + ulp(p) (max rel err of the step alone {rel_max:.3e})")
    for what, e in (("m", em), ("v", ev), ("p", ep)):
        assert torch.isfinite(e).all(), (name, what, "not finite")
        assert float(e.max()) <= 1.0 if e.numel() else True, (
            name, what, int(t), f"{int((e > 1).sum())} of {e.numel()} elements over the bound, "
            f"worst x{float(e.max()):.3g} at flat index {int(e.argmax())}")
    return got
