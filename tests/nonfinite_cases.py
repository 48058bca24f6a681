"""NaN and infinite values fed through the agent kernels' forwards and into their updates: the named
injections, the PyTorch references and the comparison helpers shared by test_gpu_nonfinite_acting.py,
test_gpu_nonfinite_updates.py and test_nonfinite_host.py (DESIGN.md "Non-finite values").

Everything but the injected value is the O(1) data of the edge sweeps (edge_updates.py's seeded
networks and rings).  Every reference is the PyTorch module on the CPU: in fp32 for the
pattern of non-finite values (where the NaNs, +infs and -infs are), in float64 for the finite values,
at the tolerances of edge_shapes.py's docstring.  The precondition of every case is that the two
references have the same pattern (``*_refs`` assert it before anything is compared with a kernel, and
test_nonfinite_host.py asserts it without a GPU): a pattern is then a property of the operation, not
of a rounding.  Nothing here needs a GPU to import."""
import copy

import numpy as np
import torch

from oracle import oracle
from pbn_rl_amd.attractors import load_attractors
from pbn_rl_amd.ddqn import ddqn_update
from pbn_rl_amd.network import load_network
from pbn_rl_amd.replay import bdq_update
from pbn_rl_amd.spec import EnvSpec
from tests.edge_shapes import edge_spec
from tests.edge_updates import (DDQN_CAP, _batch, _ring, batch64_of, batch_of, bdq_ring, make_dqn_nets, make_nets,
                                pick_rows)

NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")
N_ENVS, NO_TARGET, ENV_SEED = 96, (5, 64), 17


# ---- helpers ----------------------------------------------------------------------------------------
def pattern(x):
    """(isnan, isposinf, isneginf) of a tensor, on the CPU."""
    x = x.detach().cpu()
    return torch.isnan(x), torch.isposinf(x), torch.isneginf(x)


def assert_same_pattern(got, ref32, what=""):
    """``got`` has its NaNs, +infs and -infs exactly where ``ref32`` has them."""
    for name, g, r in zip(("NaN", "+inf", "-inf"), pattern(got), pattern(ref32)):
        assert g.shape == r.shape, (what, g.shape, r.shape)
        assert torch.equal(g, r), (what, name, int(g.sum()), int(r.sum()), (g != r).nonzero()[:8].tolist())


def check_finite(got, ref64, rtol, atol, what=""):
    """The entries that are finite in the float64 reference: ``got`` equals them at rtol / atol."""
    got, ref64 = got.detach().cpu().double(), ref64.detach().cpu().double()
    fin = torch.isfinite(ref64)
    err = (got[fin] - ref64[fin]).abs()
    over = err - (atol + rtol * ref64[fin].abs())
    assert bool(torch.isfinite(got[fin]).all()), what
    assert fin.sum() == 0 or over.max().item() <= 0.0, (what, err.max().item())
    return int(fin.sum())


_SPECS = {}


def the_spec(shape, **kw):
    """A bundled network's spec by name, or edge_shapes.edge_spec(N) (cached)."""
    if not isinstance(shape, str):
        return edge_spec(shape, **kw)
    key = (shape, tuple(sorted(kw.items())))
    if key not in _SPECS:
        _SPECS[key] = EnvSpec(load_network(shape), load_attractors(shape), **kw)
    return _SPECS[key]


def first_states(spec):
    """(256, N) float32: row t = the first state of attractor t, zeros past them (target id 255)."""
    tab = torch.zeros(256, spec.n)
    for t, a in enumerate(spec.attractors):
        tab[t] = torch.tensor(list(a[0]), dtype=torch.float32)
    return tab


def observation(spec, n=N_ENVS, seed=ENV_SEED):
    """(state, target) float32 (n, N) of ``n`` envs after VectorPBNEnv(spec, n, seed).reset(), with
    the envs NO_TARGET set to no target: the CPU oracle's reset, which the env's equals bit for bit."""
    st, tg, _ = oracle.reset(spec, seed, 0, 0, n)
    tg = tg.copy()
    for e in NO_TARGET:
        tg[e] = 255
    w = st.T[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]
    s = (w & 1).reshape(n, -1)[:, :spec.n].astype(np.float32)
    return torch.from_numpy(s), first_states(spec)[torch.from_numpy(tg.astype(np.int64))]


def inject(module, param, index, value):
    """A copy of ``module`` with one element of the named parameter set to ``value``; a negative index
    counts from the end, so (-1, ...) is the last real element of the segment."""
    m = copy.deepcopy(module)
    with torch.no_grad():
        dict(m.named_parameters())[param][index] = value
    return m


def special_rows(q32):
    """Rows whose argmax is decided by a non-finite value: a NaN, or exactly one +inf."""
    nan, pinf, _ = pattern(q32)
    return nan.any(1) | (~nan.any(1) & (pinf.sum(1) == 1))


# ---- DDQN acting ------------------------------------------------------------------------------------
# (spec, net_arch): widths 17, 20 and 40 leave padded lanes in a 16-tile; with h1 = 17 the last tile's
# real feature shares its lane's four with three padded ones (40 and 8 pad whole lanes)
DDQN_ACT_SHAPES = [("pbn7", (8, 8)), (33, (17, 64)), (97, (20, 40)), (15, (16, 17))]
DDQN_ACT_IDS = ["pbn7-8x8", "N33-17x64", "N97-20x40", "N15-16x17"]
# name -> (parameter, index, value), always the last real element
DDQN_INJECTIONS = {
    "nan_input_bias": ("input.bias", (-1,), NAN),
    "nan_l1_bias": ("linears.0.bias", (-1,), NAN),
    "nan_l1_weight": ("linears.0.weight", (-1, -1), NAN),
    "nan_out_bias": ("output.bias", (-1,), NAN),
    "pinf_out_bias": ("output.bias", (-1,), PINF),
    "ninf_out_bias": ("output.bias", (-1,), NINF),
    "pinf_out_weight": ("output.weight", (-1, -1), PINF),
    "pinf_input_bias": ("input.bias", (-1,), PINF),
    "pinf_l1_bias": ("linears.0.bias", (-1,), PINF),
    "ninf_input_bias": ("input.bias", (-1,), NINF),
}
ROLLOUT_INJECTIONS = ("nan_l1_bias", "pinf_input_bias")


def dqn_net(N, arch, seed=3):
    return make_dqn_nets(N, arch, seed)[0]


def dqn_refs(q, s, g):
    """(Q in fp32, Q in float64) of the module on the CPU; asserts the precondition."""
    with torch.no_grad():
        q32 = q(s, g)
        q64 = copy.deepcopy(q).double()(s.double(), g.double())
    assert_same_pattern(q32, q64, "precondition: the fp32 and float64 modules")
    return q32, q64


def finite_row_filter(q32, q64, gap=1e-4):
    """Of the finite rows (no NaN and no +inf: a -inf never wins), those whose float64 top-2 gap
    exceeds ``gap``; asserts that they are at least half of them.  Returns (rows compared, finite
    rows).  A row with several +inf and no NaN is a tie, which neither this nor special_rows takes."""
    nan, pinf, _ = pattern(q32)
    plain = ~nan.any(1) & ~pinf.any(1)
    top2 = torch.where(torch.isnan(q64), torch.full_like(q64, NINF), q64).topk(2, dim=1)[0]
    clear = plain & ((top2[:, 0] - top2[:, 1]) > gap)
    assert 2 * int(clear.sum()) >= int(plain.sum()), (int(clear.sum()), int(plain.sum()))
    return clear, plain


def sparse_bilinear_features(q, s, g):
    """The first layer as the kernels evaluate it, restated plainly in float64: relu(bias + the sum
    over a row's set state bits i of T[i], T[i][o] = the sum over the target's set bits j of
    W[o][i][j]).  An unset bit selects nothing, so a NaN weight reaches a row only through a set
    (i, j) pair; nn.Bilinear's dense product makes every row NaN (0 * NaN)."""
    W = q.input.weight.detach().double()
    b = q.input.bias.detach().double()
    out = torch.empty(s.shape[0], W.shape[0], dtype=torch.float64)
    for r in range(s.shape[0]):
        ii = torch.nonzero(s[r] > 0).flatten()
        jj = torch.nonzero(g[r] > 0).flatten()
        out[r] = b + W[:, ii][:, :, jj].sum(dim=(1, 2))
    return torch.relu(out)


def bilinear_nan_pair(s, g):
    """A bilinear weight's (i, j) that some rows select (state bit i and target bit j set) and some do
    not, as evenly as the observation allows."""
    n = s.shape[0]
    c = (s > 0).double().t() @ (g > 0).double()
    k = int(torch.minimum(c, n - c).argmax())
    i, j = divmod(k, c.shape[1])
    assert 0 < int(c[i, j]) < n
    return i, j


# ---- BDQ acting -------------------------------------------------------------------------------------
# (spec, branches): A = 34 crosses the 32-action tile
BDQ_SHAPES = [("pbn7", 3), (33, 1)]
BDQ_IDS = ["pbn7-K3", "N33-K1"]
# name -> (parameter, index, value); {last} is the last branch, -1 the last real element
BDQ_INJECTIONS = {
    "nan_bilinear_bias": ("model.0.bilinear.bias", (-1,), NAN),
    "pinf_bilinear_bias": ("model.0.bilinear.bias", (-1,), PINF),
    "nan_trunk_bias": ("model.2.bias", (-1,), NAN),
    "nan_value_bias": ("value_head.2.bias", (-1,), NAN),
    "nan_adv_bias": ("adv_heads.{last}.2.bias", (-1,), NAN),
    "pinf_adv_bias": ("adv_heads.{last}.2.bias", (-1,), PINF),
    "ninf_adv_bias": ("adv_heads.{last}.2.bias", (-1,), NINF),
}


def bdq_net(N, K, seed=7):
    return make_nets(N, K, seed)[0]


def bdq_injection(name, K):
    param, index, value = BDQ_INJECTIONS[name]
    return param.format(last=K - 1), index, value


# ---- DDQN updates -----------------------------------------------------------------------------------
DDQN_UPD_SHAPES = [("pbn7", (8, 8)), (33, (17, 64))]
DDQN_UPD_IDS = ["pbn7-8x8", "N33-17x64"]
B, ROW = 16, 2                    # the batch, and the batch position of the injected ring row
LR, GAMMA, RC = 1e-3, 0.95, 1e-5
# name -> what the reference must give: "nan" (loss, norm, every parameter and moment NaN) or
# "finite" (loss infinite, everything else finite)
DDQN_UPD_CASES = {"reward_nan": "nan", "reward_pinf": "finite", "reward_ninf": "finite", "weight0_nan": "nan",
                  "online_l1_bias_nan": "nan", "target_out_bias_nan": "nan"}
# (case, weighted): weight0_nan is a weight
DDQN_UPD_RUNS = [(n, wt) for n in sorted(DDQN_UPD_CASES) for wt in (False, True) if wt or n != "weight0_nan"]
DDQN_UPD_RUN_IDS = [f"{n}-{'weighted' if wt else 'uniform'}" for n, wt in DDQN_UPD_RUNS]
REWARDS = {"reward_nan": NAN, "reward_pinf": PINF, "reward_ninf": NINF, "weight0_nan": NAN}


def ddqn_update_inputs(shape, arch, device="cpu"):
    """The ring (edge_updates.py's _ring), B distinct sampled rows, weights in (0.05, 1] and the seeded
    online and target networks of one shape."""
    spec = the_spec(shape)
    R, a = _ring(spec, DDQN_CAP, seed=100 + spec.n, device=device)
    rng = np.random.default_rng(B + spec.n)
    idx = rng.choice(DDQN_CAP, size=B, replace=False).astype(np.int64)
    w = (0.05 + 0.95 * rng.random(B)).astype(np.float32)
    q, tgt = make_dqn_nets(spec.n, arch, seed=7)
    return spec, R, a, idx, w, q, tgt


def ddqn_case(name, spec, a, idx, w, q, tgt):
    """The inputs of one case: (ring arrays, weights, online, target) with the injection applied, and
    the ring row whose reward changed (or None).  For target_out_bias_nan the action is the one the
    most rows' a' takes in the clean float64 reference without taking all of them."""
    a = {k: v.copy() for k, v in a.items()}
    w = w.copy()
    row = None
    if name in REWARDS:
        row = int(idx[ROW])
        a["rew"][row] = REWARDS[name]
        if name == "weight0_nan":
            w[ROW] = 0.0
    elif name == "online_l1_bias_nan":
        q = inject(q, "linears.0.bias", (-1,), NAN)
    elif name == "target_out_bias_nan":
        b64 = batch64_of(_batch(spec, a, idx, device="cpu"))
        with torch.no_grad():
            ap = copy.deepcopy(q).double()(b64["next_state"], b64["target"]).argmax(1)
        counts = torch.bincount(ap, minlength=spec.n + 1)
        counts[counts == B] = 0
        act = int(counts.argmax())
        assert 0 < int(counts[act]) < B          # some rows take it and some do not
        tgt = inject(tgt, "output.bias", (act,), NAN)
    else:
        raise KeyError(name)
    return a, w, q, tgt, row


def ddqn_reference(spec, a, idx, w, q, tgt, max_norm, weighted, dtype):
    """ddqn_update + torch.optim.Adam from zero state on CPU copies in ``dtype``: a dict of loss, norm,
    priorities (None when not weighted), and per parameter name the clipped gradient, the parameter,
    m and v after the step."""
    q, tgt = copy.deepcopy(q).to(dtype), copy.deepcopy(tgt).to(dtype)
    batch = _batch(spec, a, idx, device="cpu")
    if dtype == torch.float64:
        batch = batch64_of(batch)
    opt = torch.optim.Adam(q.parameters(), lr=LR)
    wt = torch.from_numpy(w).to(dtype) if weighted else None
    prio = torch.full((B,), -1.0, dtype=dtype) if weighted else None
    loss, norm = ddqn_update(q, tgt, opt, batch, GAMMA, max_norm, weights=wt, priorities_out=prio, replay_constant=RC)
    out = {"loss": loss.reshape(1), "norm": norm.reshape(1), "prio": prio}
    for name, p in q.named_parameters():
        st = opt.state[p]
        out[name] = {"grad": p.grad.detach(), "p": p.detach(), "m": st["exp_avg"], "v": st["exp_avg_sq"]}
    return out


def clean_norm(spec, a, idx, w, q, tgt, weighted):
    """The clean batch's gradient norm in float64 (no step taken): what decides the clip."""
    q64 = copy.deepcopy(q).double()
    batch = batch64_of(_batch(spec, a, idx, device="cpu"))
    wt = torch.from_numpy(w).double() if weighted else None
    prio = torch.empty(B, dtype=torch.float64) if weighted else None
    _, norm = ddqn_update(q64, copy.deepcopy(tgt).double(), torch.optim.SGD(q64.parameters(), lr=0.0), batch, GAMMA,
                          1e30, weights=wt, priorities_out=prio, replay_constant=RC)
    return float(norm)


def clean_deltas(spec, a, idx, q, tgt):
    """The batch's TD errors q_b - y_b in float64 (B,)."""
    b = batch64_of(_batch(spec, a, idx, device="cpu"))
    q64, t64 = copy.deepcopy(q).double(), copy.deepcopy(tgt).double()
    with torch.no_grad():
        ap = q64(b["next_state"], b["target"]).argmax(1, keepdim=True)
        y = b["reward"] + (1 - b["done"]) * GAMMA * t64(b["next_state"], b["target"]).gather(1, ap)
        return (q64(b["state"], b["target"]).gather(1, b["action"]) - y).squeeze(1)


def max_norm_of(spec, a, idx, w, q, tgt, weighted, clip):
    """Half the clean batch's norm (clips), or far above it."""
    norm0 = clean_norm(spec, a, idx, w, q, tgt, weighted)
    assert norm0 > 1e-6
    return 0.5 * norm0 if clip else 10.0 * max(norm0, 1.0)


def ddqn_refs(name, spec, a, idx, w, q, tgt, max_norm, weighted):
    """(fp32 reference, float64 reference) of one case; asserts the precondition on every quantity and
    what DDQN_UPD_CASES says the reference gives."""
    r32 = ddqn_reference(spec, a, idx, w, q, tgt, max_norm, weighted, torch.float32)
    r64 = ddqn_reference(spec, a, idx, w, q, tgt, max_norm, weighted, torch.float64)
    names = [k for k in r32 if k not in ("loss", "norm", "prio")]
    for key in ("loss", "norm") + (("prio",) if weighted else ()):
        assert_same_pattern(r32[key], r64[key], f"precondition: {key}")
    for n in names:
        for k in ("grad", "p", "m", "v"):
            assert_same_pattern(r32[n][k], r64[n][k], f"precondition: {n} {k}")
    if DDQN_UPD_CASES[name] == "nan":
        assert bool(torch.isnan(r32["loss"]).all() and torch.isnan(r32["norm"]).all())
        assert all(bool(torch.isnan(r32[n][k]).all()) for n in names for k in ("p", "m", "v"))
    else:
        assert bool(torch.isposinf(r32["loss"]).all() and torch.isfinite(r32["norm"]).all())
        assert all(bool(torch.isfinite(r32[n][k]).all()) for n in names for k in ("grad", "p", "m", "v"))
    return r32, r64


# ---- BDQ updates ------------------------------------------------------------------------------------
BDQ_GAMMA = 0.9
BDQ_UPD_CASES = ("reward_nan", "reward_ninf", "reward_pinf", "weight0_nan")
BDQ_UPD_RUNS = [(n, wt) for n in BDQ_UPD_CASES for wt in (False, True) if wt or n != "weight0_nan"]
BDQ_UPD_RUN_IDS = [f"{n}-{'weighted' if wt else 'uniform'}" for n, wt in BDQ_UPD_RUNS]
BDQ_BILINEAR_WEIGHT = "model.0.bilinear.weight"


def bdq_update_inputs(shape, K, device="cpu"):
    """edge_updates.py's ring and rows (the all-zeros and all-ones states, a row without a target),
    weights in (0.05, 1], the seeded networks, and the batch position of a row sampled once."""
    spec = the_spec(shape)
    R = bdq_ring(spec, K, B + K, device=device)
    idx = pick_rows(R, B, B + K)
    pos = next(b for b in range(3, B) if int((idx == idx[b]).sum()) == 1)
    w = (0.05 + 0.95 * np.random.default_rng(K + spec.n).random(B)).astype(np.float32)
    q, tgt = make_nets(spec.n, K, seed=7)
    return spec, R, idx, pos, w, q, tgt


def bdq_reference(spec, R, idx, w, q, tgt, weighted, dtype):
    """bdq_update (its PyTorch expressions) + torch.optim.Adam from zero state on CPU copies in
    ``dtype``, on the ring's rows as they are: loss, priorities (fp32, None when not weighted) and per
    parameter name the clamped gradient, the parameter, m and v after the step."""
    q, tgt = copy.deepcopy(q).to(dtype), copy.deepcopy(tgt).to(dtype)
    batch = batch_of(spec, R, idx, "cpu", dtype)
    opt = torch.optim.Adam(q.parameters(), lr=LR)
    wt = torch.from_numpy(w) if weighted else None
    prio = torch.full((B,), -1.0) if weighted else None
    loss = bdq_update(q, tgt, opt, batch, BDQ_GAMMA, weights=wt, priorities_out=prio, replay_constant=RC)
    out = {"loss": loss.reshape(1), "prio": prio}
    for name, p in q.named_parameters():
        st = opt.state[p]
        out[name] = {"grad": p.grad.detach(), "p": p.detach(), "m": st["exp_avg"], "v": st["exp_avg_sq"]}
    return out


def bdq_refs(spec, R, idx, w, q, tgt, weighted):
    """(fp32 reference, float64 reference); asserts the precondition on every quantity."""
    r32 = bdq_reference(spec, R, idx, w, q, tgt, weighted, torch.float32)
    r64 = bdq_reference(spec, R, idx, w, q, tgt, weighted, torch.float64)
    for key in ("loss",) + (("prio",) if weighted else ()):
        assert_same_pattern(r32[key], r64[key], f"precondition: {key}")
    for n in r32:
        if n not in ("loss", "prio"):
            for k in ("grad", "p", "m", "v"):
                assert_same_pattern(r32[n][k], r64[n][k], f"precondition: {n} {k}")
    return r32, r64
