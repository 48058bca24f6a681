"""The conditions on the inputs of the replay-path edge sweeps (tests/replay_edge_cases.py), checked
on the CPU from the oracle and the float64 references alone.  Each one is a cap that keeps a GPU
test from passing a wrong kernel: an argmax that fp32 may legitimately move, a prefix whose
association does not matter, a batch that never leaves one half of the tree, a ring that never sets
the last bit."""
import numpy as np
import pytest
import torch

from oracle import agent_oracle
from tests import replay_edge_cases as C


# ---- TD loss ---------------------------------------------------------------------------------

def test_td_cases_cover_the_kernels_paths():
    """Partial and single blocks, K = 1 and 7, A = 1 and 128, and the LDS request on both sides of
    64 KB up to the largest accepted shape (98,752 B)."""
    Bs = {B for B, _, _ in C.TD_CASES}
    assert {1, 7, 8, 9, 33} <= Bs and any(B % C.TD_ROWS for B in Bs) and any(B < C.TD_ROWS for B in Bs)
    assert {K for _, K, _ in C.TD_CASES} >= {1, 7} and {A for _, _, A in C.TD_CASES} >= {1, 2, 16, 71, 128}
    assert C.td_lds_bytes(4, 128) == 61696 < 64 * 1024 < C.td_lds_bytes(5, 128) == 74048
    assert C.td_lds_bytes(7, 128) == 98752 == max(C.td_lds_bytes(K, A) for _, K, A in C.TD_CASES)
    assert (9, 4, 128) in C.TD_CASES and (9, 5, 128) in C.TD_CASES and (9, 7, 128) in C.TD_CASES


@pytest.mark.parametrize("B,K,A", C.TD_CASES)
def test_td_argmax_cannot_legitimately_differ(B, K, A):
    """Every (row, branch): the float64 top-two gap of the next-state Q is >= 1e-3 (unit-scale
    heads: fp32 rounding moves a Q by ~1e-6), so the fp32 module's a* is the float64 one; the
    double-DQN term is live in one row at least; and the reference's a* is argmax_torch's."""
    inp = C.td_inputs(B, K, A)
    assert C.top_two_gap(inp) >= C.MIN_GAP
    assert float(inp["online"].abs().max()) < 8.0 and float(inp["masks"][0]) == 1.0
    assert int(inp["actions"].min()) >= 0 and int(inp["actions"].max()) < A
    _, _, _, am64 = C.td_reference(inp)
    _, _, _, am32 = C.td_reference(inp, torch.float32)
    assert torch.equal(am64, am32)
    assert np.array_equal(am64.numpy(), agent_oracle.argmax_torch(C.next_q64(inp).numpy()))


def test_td_tie_rows_tie_exactly():
    """The tie case: the fp32 dueling of every next-state row equals the float64 one bit for bit,
    its maximum stands at exactly j1 < j2, the reference takes j1, and taking j2 instead moves the
    target Q by 0.5 in a row whose mask is 1."""
    inp = C.td_tie_inputs()
    B, K, A = C.TIE_SHAPE
    q64 = C.next_q64(inp)                                               # (K, B, A)
    assert torch.equal(C.dueling(inp["online"][:, B:]).double(), q64)
    top = q64 == q64.max(2, keepdim=True).values
    assert bool((top.sum(2) == 2).all())
    j1, j2 = inp["j1"].t(), inp["j2"].t()                               # (K, B)
    assert bool((j1 < j2).all()) and (int(j1[0, 0]), int(j2[0, 0])) == (0, A - 1)
    assert bool(top.gather(2, j1.unsqueeze(2)).all()) and bool(top.gather(2, j2.unsqueeze(2)).all())
    _, _, _, am = C.td_reference(inp)
    assert torch.equal(am, j1)
    assert np.array_equal(am.numpy(), agent_oracle.argmax_torch(q64.numpy()))
    tq = C.dueling(inp["target"].double())
    d = tq.gather(2, j2.unsqueeze(2)) - tq.gather(2, j1.unsqueeze(2))
    assert bool(((d - 0.5).abs() < 1e-6).all()) and bool((inp["masks"] == 1).all())


def test_td_inf_rows_have_one_nan():
    """The +inf case: each marked row's Q is NaN at j and -inf elsewhere, torch.argmax and
    argmax_torch pick j, and the float64 loss and gradient stay finite."""
    inp = C.td_inf_inputs()
    q = C.next_q64(inp)
    for b, k, j in C.INF_AT:
        assert j > 0 and bool(torch.isnan(q[k, b, j])) and int(torch.isnan(q[k, b]).sum()) == 1
        assert bool((q[k, b][torch.arange(q.shape[2]) != j] == float("-inf")).all())
        assert float(inp["masks"][b]) == 1.0
    assert int(torch.isnan(q).sum()) == len(C.INF_AT)
    for weighted in (False, True):
        loss, prio, grad, am = C.td_reference(inp, weighted=weighted)
        assert all(int(am[k, b]) == j for b, k, j in C.INF_AT)
        assert np.array_equal(am.numpy(), agent_oracle.argmax_torch(q.numpy()))
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
        assert prio is None or bool(torch.isfinite(prio).all())


def test_td_reference_gradient_is_the_comments_formula():
    """The autograd gradient of the reference equals the closed form of the kernel's comment
    (g (j == a) - g / A, the value head's output 0 = sum_k g, everything else exactly 0)."""
    B, K, A = 9, 3, 16
    inp = C.td_inputs(B, K, A)
    for weighted in (False, True):
        _, _, grad, am = C.td_reference(inp, weighted=weighted)
        on, tg = inp["online"].double(), inp["target"].double()
        a = inp["actions"].t().unsqueeze(2)
        cur = C.dueling(on[:, :B]).gather(2, a).squeeze(2)
        exp = inp["rewards"].double() + C.dueling(tg).gather(2, am.unsqueeze(2)).squeeze(2) * C.GAMMA32 * inp["masks"].double()
        g = 2 * (cur - exp) / (B * K) * (inp["weights"].double() if weighted else 1.0)     # (K, B)
        want = torch.zeros_like(on)
        want[1:, :B] = -g.unsqueeze(2) / A
        want[1:, :B].scatter_add_(2, a, g.unsqueeze(2))
        want[0, :B, 0] = g.sum(0)
        assert torch.allclose(grad, want, rtol=1e-12, atol=1e-15)
        assert not grad[:, B:].any() and not grad[0, :, 1:].any()


# ---- priority trees --------------------------------------------------------------------------

def test_per_sample_cases_cover_the_walks_exits():
    cases = {(cap, size) for cap, size, _, _, _ in C.PER_SAMPLE_CASES}
    assert {(2, 2), (200, 2), (512, 512), (1024, 1024)} <= cases                 # size 2; size = capacity = T
    for cap, size in cases:
        assert 2 <= size <= cap
    T = lambda cap: C.PerOracle(cap).T  # noqa: E731
    assert sum(size == T(cap) // 2 + 1 for cap, size in cases) >= 3               # rem == w at node 2
    assert any(size == cap - 1 for cap, size in cases)
    assert {B for _, _, _, bs, _ in C.PER_SAMPLE_CASES for B in bs} == {1, 63, 64, 65, 1024}
    assert any(kw.get("beta") == kw.get("max_beta") for *_, kw in C.PER_SAMPLE_CASES if kw)


@pytest.mark.parametrize("cap,size,seed,batches,kw", C.PER_SAMPLE_CASES)
def test_per_sample_case_conditions(cap, size, seed, batches, kw):
    """Strictly positive priorities over more than five decades; p_total differs from the
    left-to-right sum of the same leaves, and, where it has three terms or more, from the
    left-to-right sum of its own terms; a size-2 case draws row 0 only, every batch of 63 rows or
    more draws two distinct rows at least and one from each half of the live range."""
    o = C.per_sample_oracle(cap, size, seed)
    leaves = o.sum_leaves()[:size]
    assert o.size == size and bool((leaves > 0).all())
    t = o.prefix_terms()
    if size == 2:
        assert len(t) == 1 and o.p_total() == leaves[0]
    else:
        assert leaves.max() / leaves.min() > 10.0 ** (5 * C.ALPHA)
        assert o.p_total() != C.sequential_prefix(o)
        if size == o.T // 2 + 1:
            assert t == [float(o.sum[2])]
        if size == o.T:
            assert len(t) == o.T.bit_length() - 1
        if len(t) >= 3:
            s = t[0]
            for x in t[1:]:
                s = s + x
            assert s != o.p_total()
    for B, rows in zip(batches, C.per_sample_rows(o, batches, kw.get("beta", 0.4))):
        assert rows.min() >= 0 and rows.max() < size
        if size == 2:
            assert not rows.any()
        elif B >= 63:
            assert len(np.unique(rows)) >= 2
            assert bool((rows < size // 2).any()) and bool((rows >= size // 2).any())


def test_association_tree_turns_the_association_into_a_row():
    """The constructed tree: three prefix terms whose two associations differ by one ulp, and a
    batch-1 draw whose row is 2 under the reference's association and 1 under left-to-right."""
    ctr, o = C.association_oracle()
    u = C.replay_uniforms(C.PER_SEED, ctr, 1)
    assert 0.5 < u[0] < 1.0 and bool((o.sum_leaves() > 0).all())
    assert o.prefix_terms() == [1.0, 2.0 ** -53, 2.0 ** -53]
    assert o.p_total() == 1.0 + 2.0 ** -52 and (1.0 + 2.0 ** -53) + 2.0 ** -53 == 1.0
    assert float(o.sum[4]) == u[0] + 2.0 ** -53 and float(o.sum[2]) == 1.0
    rows, _ = o.sample(1, 0.4, u)
    assert rows.tolist() == [2]
    o.p_total = lambda: 1.0                                  # the left-to-right prefix
    rows, _ = o.sample(1, 0.4, u)
    assert rows.tolist() == [1]


def test_per_update_batches_cover_every_row_once():
    for size in (2, 3, 200, 1500):
        b = C.varied_updates(size, 3)
        rows = np.concatenate([r for r, _ in b])
        assert np.array_equal(np.sort(rows), np.arange(size)) and all(len(r) <= 1024 for r, _ in b)
        p = np.concatenate([p for _, p in b])
        assert p.dtype == np.float32 and p.min() >= 1e-3 * (1 - 1e-6) and p.max() <= 1e3 * (1 + 1e-6)
    assert len(C.varied_updates(1500, 3)[0][0]) == 1024            # B = 1024, all distinct


# ---- batch gather ----------------------------------------------------------------------------

@pytest.mark.parametrize("N", C.GATHER_N)
def test_gather_rings_reach_the_last_bit_and_the_zero_plane(N):
    """Bit N - 1 set in one ring row and clear in another, in both state fields, and no bit above
    it; a gathered row whose target (< n_attr) has bit N - 1 set in its first state; gathered rows
    with target ids n_attr and 255 whose expected plane 1 is zero while attractor 0's first state
    is not; rows 0 and capacity - 1 and a duplicate in every batch above one row."""
    for K in (1, 7):
        spec, ring = C.gather_ring(N, K)
        W, n_attr, cap = spec.words, len(spec.attractors), C.GATHER_CAP
        assert W == (N + 31) // 32 and ring["action"].shape == (cap, K)
        w, sh = (N - 1) >> 5, (N - 1) & 31
        for f in ("state", "next_state"):
            bit = (ring[f][w] >> np.uint32(sh)) & 1
            assert bit.any() and not bit.all()
            if N % 32:
                assert not (ring[f][W - 1] >> np.uint32(N % 32)).any()
        if N > 64:   # a word index that wraps at two words reads another word
            assert (ring["state"][2] != ring["state"][0]).any()
        tg = ring["target"]
        assert tg[0] < n_attr and spec.attractors[tg[0]][0][N - 1] == 1
        assert any(spec.attractors[0][0]) and tg[7] == 255 and tg[9] == n_attr
        for B in C.GATHER_B:
            idx = C.gather_idx(B)
            assert idx[0] == 0 and idx.min() >= 0 and idx.max() < cap
            x, act, rew, msk = C.gather_expected(spec, ring, idx)
            assert x.shape == (2, 2 * B, N) and act.shape == (B, K) and act.dtype == np.int64
            assert x[1, 0, N - 1] == 1.0 and x[0, 0, N - 1] == 0.0 and x[0, B, N - 1] == 1.0
            assert np.array_equal(x[1, :B], x[1, B:])
            if B > 1:
                assert idx[1] == cap - 1 and len(np.unique(idx)) < B
                assert {7, 9} <= set(idx.tolist())
                for b in np.flatnonzero(tg[idx] >= n_attr):
                    assert not x[1, b].any() and not x[1, B + b].any()
