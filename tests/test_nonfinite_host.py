"""csrc/dqn_scalar.h, the DDQN kernels' scalar laws, on the host against PyTorch on the CPU, and the
preconditions of tests/nonfinite_cases.py without a GPU.

tests/dqn_scalar_check.cpp (compiled with hipcc, host side only, as test_curriculum_host.py compiles
its program) calls the functions dqn_forward.h and pbn_ddqn.hip call, on a grid that holds NaN, both
infinities, both zeros, +-1, their fp32 neighbours on either side and FLT_MAX.  The ReLU, the Huber
loss, its derivative, the clip coefficient and Adam's first step from zero state are compared bit for
bit (a NaN with a NaN) with F.relu, F.huber_loss under autograd, clip_grad_norm_ and
torch.optim.Adam.  Adam's second step, from non-zero m and v, differs from torch's in the last bits
(torch evaluates m as a lerp and v as mul_ + addcmul_) and is held to adam_reference.py's bounds."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import nonfinite_cases as C
from tests.adam_reference import BETAS, EPS, check_adam_step, fp32_hyper

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "pbn_rl_amd", "csrc")
f32 = np.float32
FLT_MAX = float(np.finfo(f32).max)


def _grid():
    one = f32(1)
    near = [np.nextafter(one, f32(0)), np.nextafter(one, f32(2)), f32(0.5), f32(2), f32(1e-3), f32(1e-30), f32(3.25)]
    vals = [f32(0), one, f32(FLT_MAX), f32(np.inf)] + near
    return np.array([f32(np.nan)] + vals + [-v for v in vals], dtype=f32)


GRID = _grid()


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.fail("hipcc not found: dqn_scalar.h needs the HIP headers")
    exe = tmp_path_factory.mktemp("dqn_scalar") / "dqn_scalar_check"
    subprocess.run(["hipcc", "-x", "hip", "--offload-host-only", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC,
                    "-o", str(exe), os.path.join(HERE, "dqn_scalar_check.cpp")], check=True)
    return str(exe)


def bits(x):
    return np.asarray(x, dtype=f32).reshape(-1).view(np.uint32)


def run(exe, cmd, *columns):
    """One command per row of the float columns -> the results as float32 (rows, fields)."""
    cols = [bits(c) for c in columns]
    lines = [cmd + " " + " ".join(str(int(c[i])) for c in cols) for i in range(len(cols[0]))]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    rows = [ln.split() for ln in out.split("\n") if ln.strip()]
    assert len(rows) == len(lines) and all(r[0] == cmd for r in rows)
    return np.array([[int(v) for v in r[1:]] for r in rows], dtype=np.uint32).view(f32)


def same_bits(got, want, what):
    """Bit-equal, a NaN matching any NaN."""
    got, want = np.asarray(got, dtype=f32).reshape(-1), np.asarray(want, dtype=f32).reshape(-1)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)), \
        (what, got[~nan][got[~nan].view(np.uint32) != want[~nan].view(np.uint32)][:4])


def test_the_grid_holds_the_edges():
    assert np.isnan(GRID).sum() == 1 and np.isposinf(GRID).any() and np.isneginf(GRID).any()
    assert (np.signbit(GRID) & (GRID == 0)).any() and (~np.signbit(GRID) & (GRID == 0)).any()
    for v in (1.0, -1.0, FLT_MAX, -FLT_MAX):
        assert (GRID == f32(v)).any()
    assert ((np.abs(GRID) < 1) & (np.abs(GRID) > 0.9999)).sum() == 2 and ((np.abs(GRID) > 1) & (np.abs(GRID) < 1.0001)).sum() == 2


def test_relu_is_torchs(check_exe):
    want = F.relu(torch.from_numpy(GRID)).numpy()
    assert np.isnan(want[np.isnan(GRID)]).all()                      # F.relu keeps a NaN
    assert np.signbit(want[(GRID == 0) & np.signbit(GRID)]).all()    # and -0.0
    same_bits(run(check_exe, "relu", GRID)[:, 0], want, "relu")


def test_huber_and_its_derivative_are_torchs(check_exe):
    x = torch.from_numpy(GRID).clone().requires_grad_(True)
    h = F.huber_loss(x, torch.zeros_like(x), reduction="none")
    h.sum().backward()
    got = run(check_exe, "hub", GRID)
    same_bits(got[:, 0], h.detach().numpy(), "huber")
    same_bits(got[:, 1], x.grad.numpy(), "huber derivative")
    nan = np.isnan(GRID)
    assert np.isnan(got[nan]).all()                                  # a NaN TD error: NaN loss, NaN gradient
    assert np.array_equal(got[np.isposinf(GRID)][0], [f32(np.inf), f32(1)])
    assert np.array_equal(got[np.isneginf(GRID)][0], [f32(np.inf), f32(-1)])


def _torch_clip(first, max_norm):
    """clip_grad_norm_ on the gradient (first, 1): (total norm, the second element afterwards = the
    clamped coefficient itself)."""
    p = torch.nn.Parameter(torch.zeros(2))
    p.grad = torch.tensor([float(first), 1.0])
    norm = torch.nn.utils.clip_grad_norm_([p], float(max_norm))
    return f32(norm.item()), f32(p.grad[1].item())


def test_clip_coefficient_is_clip_grad_norms(check_exe):
    cases = []
    for t in GRID:
        for max_norm in (0.5, 10.0, 1e30):
            cases.append((t, f32(max_norm)))
    # around coef = 1: the gradient (3, 1), max_norm at its norm + 1e-6 and that value's neighbours
    n31 = f32(torch.tensor([3.0, 1.0]).norm().item())
    edge = f32(n31 + f32(1e-6))
    cases += [(f32(3), m) for m in (edge, np.nextafter(edge, f32(0)), np.nextafter(edge, f32(10)), n31)]
    res = [_torch_clip(t, m) for t, m in cases]
    totals = np.array([r[0] for r in res], dtype=f32)
    want = np.array([r[1] for r in res], dtype=f32)
    got = run(check_exe, "clip", totals, np.array([m for _, m in cases], dtype=f32))[:, 0]
    same_bits(got, want, "clip coefficient")
    assert np.isnan(totals).any() and np.isnan(got[np.isnan(totals)]).all()    # a NaN norm: every gradient NaN
    assert (got[np.isposinf(totals)] == 0).all() and (got == 1).any() and ((got < 1) & (got > 0.99)).any()


def _adam_gradients(seed, grid):
    """``grid`` and 2,000 gradients with magnitudes log-uniform in 1e-6 .. 1 and random signs."""
    rng = np.random.default_rng(seed)
    return np.concatenate([grid, (10.0 ** rng.uniform(-6, 0, 2000) * rng.choice([-1.0, 1.0], 2000)).astype(f32)])


def _torch_adam_state(w, opt):
    return [x.detach().numpy().copy() for x in (w, opt.state[w]["exp_avg"], opt.state[w]["exp_avg_sq"])]


def test_adam_element_is_torch_adams_first_step(check_exe):
    """From zero state at t = 1: p', m' and v' bit for bit."""
    lr, b1, b2, eps = fp32_hyper(1e-3, *BETAS, EPS)
    g = _adam_gradients(0, GRID)
    p0 = np.linspace(-0.5, 0.5, g.size).astype(f32)
    w = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([w], lr=lr, betas=(b1, b2), eps=eps)
    w.grad = torch.from_numpy(g.copy())
    opt.step()
    want = _torch_adam_state(w, opt)
    z = np.zeros_like(g)
    full = lambda v: np.full_like(g, v)  # noqa: E731
    got = run(check_exe, "adam", p0, z, z, g, full(lr), full(b1), full(b2), full(eps), full(1.0))
    for k, name in enumerate(("p", "m", "v")):
        same_bits(got[:, k], want[k], "adam " + name)
    assert np.isnan(got[np.isnan(g)]).all()                          # a NaN gradient: p, m and v NaN
    assert np.isnan(got[np.isinf(g), 0]).all()                       # an infinite one: inf / inf in the step
    assert np.isfinite(got[g == f32(FLT_MAX), 0]).all() and np.isposinf(got[g == f32(FLT_MAX), 2]).all()


def test_adam_element_follows_torch_adams_second_step(check_exe):
    """The step at t = 2 from torch.optim.Adam's own state after its first: b1 m, b2 v and both bias
    corrections at a count other than 1.  Here the bits do differ (measured: about a fifth of the
    finite elements in each of p, m and v): torch evaluates m as a lerp, m + (1 - b1)(g - m), and v as
    mul_ then addcmul_, the same sums in another order.  So the pattern of non-finite values is held
    to torch.optim.Adam's, and the finite values to check_adam_step's bounds (adam_reference.py:
    float64 torch.optim.Adam, test_adam_reference_host.py; roundings of a two- and a three-term sum).
    The first gradients hold no infinity: the update's clip turns an infinite gradient into NaN
    (coefficient 0 times inf) before Adam sees it, and with m = inf torch's lerp gives inf - inf."""
    hyper = fp32_hyper(1e-3, *BETAS, EPS)
    lr, b1, b2, eps = hyper
    grid = GRID[~np.isinf(GRID)]
    g1, g2 = _adam_gradients(1, grid), _adam_gradients(2, np.roll(grid, 3))
    p0 = np.linspace(-0.5, 0.5, g1.size).astype(f32)
    w = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([w], lr=lr, betas=(b1, b2), eps=eps)
    w.grad = torch.from_numpy(g1.copy())
    opt.step()
    before = _torch_adam_state(w, opt)
    assert (before[1][np.isfinite(g1)] != 0).sum() > 2000 and (before[2][np.isfinite(g1)] != 0).sum() > 2000
    w.grad = torch.from_numpy(g2.copy())
    opt.step()
    want = _torch_adam_state(w, opt)
    full = lambda v: np.full_like(g1, v)  # noqa: E731
    got = run(check_exe, "adam", *before, g2, full(lr), full(b1), full(b2), full(eps), full(2.0))
    for k, name in enumerate(("p", "m", "v")):
        C.assert_same_pattern(torch.from_numpy(got[:, k].copy()), torch.from_numpy(want[k]), "adam " + name)
    assert np.isnan(got[np.isnan(g1) | np.isnan(g2)]).all()          # a NaN state or gradient: p, m and v NaN
    fin = np.isfinite(got).all(1) & np.all([np.isfinite(x) for x in before], 0) & np.isfinite(g2)
    for g in (g1, g2):                 # 1e-30 squares below fp32's range: v underflows (subnormals are out of scope)
        fin &= (g == 0) | ~(np.abs(g) < 1e-15)
    assert fin.sum() > 2000
    sub = lambda xs: tuple(torch.from_numpy(np.ascontiguousarray(x[fin])) for x in xs)  # noqa: E731
    check_adam_step("dqn_scalar.h", sub(before), sub(got.T), 2, sub([g2])[0], hyper)
    check_adam_step("torch.optim.Adam fp32", sub(before), sub(want), 2, sub([g2])[0], hyper)


# ---- the preconditions of nonfinite_cases.py ----------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.DDQN_INJECTIONS))
@pytest.mark.parametrize("shape,arch", C.DDQN_ACT_SHAPES, ids=C.DDQN_ACT_IDS)
def test_ddqn_acting_references_share_their_pattern(shape, arch, name):
    spec = C.the_spec(shape)
    s, g = C.observation(spec)
    assert float(g[C.NO_TARGET[0]].abs().sum()) == 0.0
    q32, q64 = C.dqn_refs(C.inject(C.dqn_net(spec.n, arch), *C.DDQN_INJECTIONS[name]), s, g)
    C.finite_row_filter(q32, q64)
    nan, pinf, ninf = C.pattern(q32)
    A = spec.n + 1
    if name == "nan_out_bias":
        assert bool(nan[:, A - 1].all()) and int(nan.sum()) == C.N_ENVS and bool((q32.argmax(1) == A - 1).all())
    if name == "pinf_out_bias":
        assert bool(pinf[:, A - 1].all()) and int(pinf.sum()) == C.N_ENVS and bool((q32.argmax(1) == A - 1).all())
    if name == "ninf_out_bias":
        assert bool(ninf[:, A - 1].all()) and not bool((q32.argmax(1) == A - 1).any())
    if name == "ninf_input_bias":
        assert bool(torch.isfinite(q32).all())                       # relu(-inf) = 0
    if name in ("nan_input_bias", "nan_l1_bias"):
        assert bool(nan.all()) and bool((q32.argmax(1) == 0).all())  # an all-NaN row: action 0
    if name == "pinf_input_bias":
        assert bool(nan.any()) and not bool(torch.isfinite(q32).any())
    if name == "pinf_l1_bias":
        assert bool(pinf.any() and ninf.any()) and not bool(nan.any()) and not bool(torch.isfinite(q32).any())


@pytest.mark.parametrize("shape,arch", C.DDQN_ACT_SHAPES, ids=C.DDQN_ACT_IDS)
def test_sparse_bilinear_restatement(shape, arch):
    """Without a NaN the sparse restatement is the module's first layer; with one in a bilinear weight
    it makes NaN exactly the rows that select it, where nn.Bilinear makes every row NaN."""
    spec = C.the_spec(shape)
    s, g = C.observation(spec)
    q = C.dqn_net(spec.n, arch)
    with torch.no_grad():
        dense = torch.relu(q.double().input(s.double(), g.double()))
    assert torch.allclose(C.sparse_bilinear_features(q, s, g), dense, rtol=1e-12, atol=1e-12)
    i, j = C.bilinear_nan_pair(s, g)
    qn = C.inject(q, "input.weight", (-1, i, j), C.NAN)
    feat = C.sparse_bilinear_features(qn, s, g)
    hit = (s[:, i] > 0) & (g[:, j] > 0)
    assert 0 < int(hit.sum()) < s.shape[0]
    assert torch.equal(torch.isnan(feat[:, -1]), hit) and not bool(torch.isnan(feat[:, :-1]).any())
    with torch.no_grad():
        assert bool(torch.isnan(qn.input(s.double(), g.double())[:, -1]).all())


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("name,weighted", C.DDQN_UPD_RUNS, ids=C.DDQN_UPD_RUN_IDS)
@pytest.mark.parametrize("shape,arch", C.DDQN_UPD_SHAPES, ids=C.DDQN_UPD_IDS)
def test_ddqn_update_references_share_their_pattern(shape, arch, name, clip, weighted):
    spec, _, a, idx, w, q, tgt = C.ddqn_update_inputs(shape, arch)
    max_norm = C.max_norm_of(spec, a, idx, w, q, tgt, weighted, clip)
    a2, w2, q2, t2, _ = C.ddqn_case(name, spec, a, idx, w, q, tgt)
    r32, _ = C.ddqn_refs(name, spec, a2, idx, w2, q2, t2, max_norm, weighted)
    if C.DDQN_UPD_CASES[name] == "finite":
        assert (float(r32["norm"]) > max_norm) == clip


@pytest.mark.parametrize("name", sorted(C.BDQ_INJECTIONS))
@pytest.mark.parametrize("shape,K", C.BDQ_SHAPES, ids=C.BDQ_IDS)
def test_bdq_acting_references_share_their_pattern(shape, K, name):
    spec = C.the_spec(shape)
    s, g = C.observation(spec)
    q = C.inject(C.bdq_net(spec.n, K), *C.bdq_injection(name, K))
    obs = torch.stack([s, g])
    with torch.no_grad():
        q32, q64 = q(obs), q.double()(obs.double())
    C.assert_same_pattern(q32, q64)
    A = spec.n + 1
    C.finite_row_filter(q32.reshape(-1, A), q64.reshape(-1, A))
    if name.endswith("_adv_bias"):        # one advantage entry reaches its branch's whole row, and no other branch
        assert not bool(torch.isfinite(q32[:, K - 1]).any()) and bool(torch.isfinite(q32[:, :K - 1]).all())
        assert bool(torch.isnan(q32[:, K - 1, A - 1]).all())


@pytest.mark.parametrize("name,weighted", C.BDQ_UPD_RUNS, ids=C.BDQ_UPD_RUN_IDS)
@pytest.mark.parametrize("shape,K", C.BDQ_SHAPES, ids=C.BDQ_IDS)
def test_bdq_update_references_share_their_pattern(shape, K, name, weighted):
    spec, R, idx, pos, w, q, tgt = C.bdq_update_inputs(shape, K)
    if name == "weight0_nan":
        w[pos] = 0.0
    R.reward[int(idx[pos])] = C.REWARDS[name]
    r32, _ = C.bdq_refs(spec, R, idx, w, q, tgt, weighted)
    assert not bool(torch.isfinite(r32["loss"]).any())
    assert bool(torch.isnan(r32[C.BDQ_BILINEAR_WEIGHT]["grad"]).all())     # PyTorch's dense product
    if weighted:
        assert (~torch.isfinite(r32["prio"])).nonzero().flatten().tolist() == [pos]
