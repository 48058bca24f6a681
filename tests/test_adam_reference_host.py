"""tests/adam_reference.py on the CPU: the float64 reference is torch.optim.Adam, a correct fp32
evaluation of the kernels' expression meets check_adam_step's bounds at every (lr, start count)
test_gpu_adam_state.py uses, and three wrong evaluations do not."""
import numpy as np
import pytest
import torch

from tests.adam_reference import (BETAS, EPS, LAST_T0, LRS, SEEDED_T0, STEPS, adam_errors, adam_step32_restated,
                                  adam_step64, check_adam_step, fp32_hyper, seed_moments)

N_EL = 20000


def _gradient(gen, n=N_EL):
    """Magnitudes log-uniform in 1e-6 .. 1e-1 with random signs; one element in sixteen exactly 0
    (an action no row of the batch took)."""
    g = 10.0 ** (-6 + 5 * torch.rand(n, generator=gen)) * (2.0 * (torch.rand(n, generator=gen) < 0.5) - 1)
    g[::16] = 0.0
    return g.float()


def _seeded(seed, n=N_EL):
    gen = torch.Generator().manual_seed(seed)
    p = (0.2 * torch.randn(n, generator=gen)).float()
    m, v = seed_moments((n,), gen)
    return p, m, v, _gradient(gen, n)


def test_reference_is_torch_adam():
    """adam_step64 chained over 6 steps from zero state = torch.optim.Adam on float64 parameters
    with the same fp32-rounded hyperparameters, to 1e-12 relative."""
    gen = torch.Generator().manual_seed(0)
    lr, b1, b2, eps = fp32_hyper(1e-3)
    p = (0.2 * torch.randn(1000, generator=gen)).float()
    w = torch.nn.Parameter(p.double().clone())
    opt = torch.optim.Adam([w], lr=lr, betas=(b1, b2), eps=eps)
    q, m, v = p.double(), torch.zeros(1000, dtype=torch.float64), torch.zeros(1000, dtype=torch.float64)
    for t in range(1, 7):
        g = _gradient(gen, 1000)
        w.grad = g.double().clone()
        opt.step()
        q, m, v = adam_step64(q, m, v, t, g, 1e-3, *BETAS, EPS)
        assert torch.allclose(q, w.detach(), rtol=1e-12, atol=0), (t, (q - w.detach()).abs().max().item())
        st = opt.state[w]
        assert torch.allclose(m, st["exp_avg"], rtol=1e-12, atol=0)
        assert torch.allclose(v, st["exp_avg_sq"], rtol=1e-12, atol=0)
    assert float((q - p.double()).abs()[1::16].min()) > 0      # (every element with a gradient moved)


@pytest.mark.parametrize("lr", LRS)
@pytest.mark.parametrize("t0", SEEDED_T0 + (LAST_T0,))
def test_restatement_meets_the_bounds_from_a_seeded_state(lr, t0):
    p, m, v, g = _seeded(t0 % 1000)
    hyper = (lr, *BETAS, EPS)
    t = float(np.float32(t0) + np.float32(1))
    assert t == t0 + 1
    check_adam_step(f"restated lr={lr:g}", (p, m, v), adam_step32_restated(p, m, v, t, g, *hyper), t, g, hyper)


@pytest.mark.parametrize("lr", LRS)
def test_restatement_meets_the_bounds_on_a_trajectory_from_zero_state(lr):
    gen = torch.Generator().manual_seed(5)
    p = (0.2 * torch.randn(N_EL, generator=gen)).float()
    m, v = torch.zeros(N_EL), torch.zeros(N_EL)
    hyper = (lr, *BETAS, EPS)
    for t in range(1, STEPS + 1):
        g = _gradient(gen)
        after = adam_step32_restated(p, m, v, t, g, *hyper)
        check_adam_step(f"restated lr={lr:g}", (p, m, v), after, t, g, hyper)
        p, m, v = after


def _fails(what, before, after, t, g, hyper):
    with pytest.raises(AssertionError):
        check_adam_step(what, before, after, t, g, hyper)


@pytest.mark.parametrize("t0", SEEDED_T0)
def test_wrong_restatements_fail(t0):
    """The check has teeth at the GPU file's seeded-state cases (lr 1e-3): bias corrections at
    t - 1, m and v rolled by one element, and the b1 m term dropped each fail check_adam_step.

    Bias corrections at t - 1 must fail at start counts 1 and 6 and are asserted there only.  At 999
    they also fail: 1 - b1^t is 1 on both sides, sqrt(1 - b2^1000) / sqrt(1 - b2^999) - 1 = 2.9e-4 of
    the step against the bound's 1e-4 |D| + 1e-5 lr + ulp(p), so no element can be over it by
    more than 2.9 x -- measured here: 19,665 of 20,000 elements over, the worst 2.8 x its bound
    (printed, not asserted: a margin below 3 is no basis for a test)."""
    p, m, v, g = _seeded(t0)
    hyper = (1e-3, *BETAS, EPS)
    t = t0 + 1
    good = adam_step32_restated(p, m, v, t, g, *hyper)
    check_adam_step("correct", (p, m, v), good, t, g, hyper)
    # a step count read before its increment: the moments are right, the parameters are not
    late = adam_step32_restated(p, m, v, t - 1, g, *hyper)
    ep = adam_errors((p, m, v), late, t, g, hyper)[2]
    print(f"t0={t0}: bias corrections at t - 1: {int((ep > 1).sum())} of {ep.numel()} over the bound, "
          f"worst x{float(ep.max()):.3g}")
    if t0 != 999:
        assert float(ep.max()) > 10.0
        _fails("t - 1", (p, m, v), late, t, g, hyper)
    # the moments of the neighbouring element
    _fails("rolled", (p, m, v), adam_step32_restated(p, m.roll(1), v.roll(1), t, g, *hyper), t, g, hyper)
    _fails("rolled m", (p, m, v), adam_step32_restated(p, m.roll(1), v, t, g, *hyper), t, g, hyper)
    _fails("rolled v", (p, m, v), adam_step32_restated(p, m, v.roll(1), t, g, *hyper), t, g, hyper)
    # m' = (1 - b1) g
    _fails("no b1 m", (p, m, v), adam_step32_restated(p, torch.zeros_like(m), v, t, g, *hyper), t, g, hyper)
