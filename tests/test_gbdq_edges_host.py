"""The GBDQ edge sweep's cases, checked without a GPU (tests/gbdq_cases.py; DESIGN.md "GBDQ", "Non-finite
values"): every size spec builds at an edge of csrc/gbdq_front.h's layout; the fp32 literal forward's
own error e_ref is positive wherever test_gpu_gbdq_edges.py uses 8 e_ref as a bound; the custom edge
lists are what they say; every planted NaN or infinity gives one pattern in fp32 and float64, so the
GPU comparison is decided by the reference alone; and the numpy partition with two capacities and
arbitrary masks against the law stated row by row and against the CPU SplitDeviceReplay."""
import numpy as np
import pytest
import torch

from pbn_rl_amd.gbdq import SplitDeviceReplay, edge_csr, edge_index, front_supported
from tests import gbdq_cases as gc

NONFINITE_NETS = ["pbn7", "size65", "hub"]


# ------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("N", gc.SIZE_N)
def test_size_spec_builds_at_its_layout_edge(N):
    spec = gc.size_spec(N)
    assert spec.n == N and spec.words == (N + 31) // 32 and front_supported(N)
    assert 1 <= len(spec.attractors) <= 5 and all(len(a) == 1 for a in spec.attractors)
    e = edge_index(spec)
    start, src = edge_csr(e, N)
    deg = (start[1:] - start[:-1]).tolist()
    assert min(deg) >= 1 and int(start[-1]) == e.shape[1] == src.numel()       # every node has its self pair
    Kp = (N + 3) & ~3
    NS = Kp + (4 - Kp % 32 + 32) % 32
    assert (NS == Kp) == (N in (1, 4, 36, 65, 100))                             # act without padding columns
    assert (N >= 97) == (spec.words == 4)


def test_smallest_and_largest_node_count():
    """1 is the smallest N a pbn_net accepts and 128 the largest (csrc/net_image.h: n_nodes 1..128)."""
    assert gc.SIZE_N[0] == 1 and gc.SIZE_N[-1] == 128 and not front_supported(0) and not front_supported(129)


SWEEP_BOUNDS = ([(f"size{N}", None) for N in gc.SIZE_N] + [("pbn7", None)]
                + [(f"size{N}", kind) for N in (17, 65) for kind in ("isolated", "dense")])


@pytest.mark.parametrize("name,kind", SWEEP_BOUNDS)
def test_e_ref_is_a_bound(name, kind):
    """8 e_ref bounds something only where e_ref > 0.  At N = 1 a row has one feature and zero deviation
    in any precision: both literal forwards give relu(beta) exactly, e_ref is 0, and the rule asks the
    kernel for the exact value."""
    spec, q, edges, words, target, f32, f64, e_ref = gc.sweep_case(name, kind)
    assert torch.isfinite(f32).all() and torch.isfinite(f64).all()
    if spec.n == 1:
        assert e_ref == 0.0 and torch.equal(f32, torch.relu(q.bn3.bias.detach()).expand(32, 1))
    else:
        assert 1e-8 < e_ref < 1e-4


@pytest.mark.parametrize("name", ["pbn7", "size65"])
def test_block_reuse_inputs(name):
    """32 distinct inputs (reuse_case asserts it) with the three target ids that matter, a positive
    e_ref, and a second env per block whose input differs from the block's first."""
    spec, q, edges, words, target, f32, f64, e_ref, env_input = gc.reuse_case(name)
    n_attr = len(spec.attractors)
    assert {n_attr - 1, n_attr, 255} <= set(target.tolist()) and 1e-8 < e_ref < 1e-4
    assert len(env_input) == 2048 + 32 and sorted(set(env_input.tolist())) == list(range(32))
    assert all(env_input[b] != env_input[2048 + b] for b in range(32))
    x = gc.observation(spec, words, target)
    assert torch.equal(x[4, :, 1], torch.zeros(spec.n)) and torch.equal(x[5, :, 1], torch.zeros(spec.n))     # no such attractor


# ------------------------------------------------------------------------------------ edge lists
@pytest.mark.parametrize("N", [17, 65])
def test_custom_edges_are_what_they_say(N):
    iso, dense, empty = (gc.custom_edges(N, k) for k in gc.EDGE_KINDS)
    assert iso.dtype == torch.long and iso.shape[0] == 2 and empty.shape == (2, 0)
    assert not set(iso[1].tolist()) & {0, N - 1} and {0, N - 1} <= set(iso[0].tolist())     # receive nothing, still send
    assert set(iso[1].tolist()) == set(range(1, N - 1))
    start, src = edge_csr(iso, N)
    assert start[1] == 0 and start[N] == start[N - 1] == iso.shape[1]
    start, src = edge_csr(dense, N)
    assert int(start[1]) == 2 * N and src[: 2 * N].tolist() == list(range(N)) * 2          # in-degree 2 N
    assert (start[2:] - start[1:-1]).tolist() == [1] * (N - 1) and src[2 * N:].tolist() == list(range(1, N))
    start, src = edge_csr(empty, N)
    assert start.tolist() == [0] * (N + 1) and src.numel() == 0 and src.dtype == torch.int32


@pytest.mark.parametrize("N", [17, 65])
def test_a_node_without_messages_gives_relu_beta(N):
    """The all-zero row: zero mean, zero variance, so relu(bn3.bias[i]) exactly in either precision."""
    for kind, rows in (("isolated", [0, N - 1]), ("empty", list(range(N)))):
        spec, q, edges, words, target, f32, f64, e_ref = gc.sweep_case(f"size{N}", kind)
        want = torch.relu(q.bn3.bias.detach())[None, :, None].expand(32, N, N)
        assert torch.equal(f32.reshape(32, N, N)[:, rows], want[:, rows])
        assert torch.equal(f64.reshape(32, N, N)[:, rows], want[:, rows].double())
        assert torch.equal(q.front(gc.observation(spec, words, target), edges, per_env=True).detach().reshape(32, N, N)[:, rows],
                           want[:, rows])


# ------------------------------------------------------------------------------------ non-finite values
@pytest.mark.parametrize("case", gc.NONFINITE_NAMES)
@pytest.mark.parametrize("name", NONFINITE_NETS)
def test_nonfinite_case_has_one_pattern(name, case):
    """fp32 and float64 literal forwards: the same NaN / +inf / -inf entries, and the reach
    gbdq_cases.nonfinite_front_cases states ("all": every entry; "rows": whole rows, some of them;
    "none": -inf in bn1.bias goes to 0 at the ReLU).  q.front has the same pattern, except where a NaN
    row enters a layer whose other rows are finite: its 0/1-matrix gathers spread that NaN to every
    node (ONEHOT_SPREADS), and there its non-finite entries contain the literal forward's."""
    assert [c for c, _ in gc.nonfinite_front_cases(7)] == gc.NONFINITE_NAMES
    spec, q, edges, words, target, f32, f64, e_ref = gc.sweep_case(name, None, case)
    N = spec.n
    assert gc.same_pattern(f32, f64)
    bad = ~torch.isfinite(f32).reshape(32, N, N)
    reach = gc.NONFINITE_REACH[case]
    if reach == "all":
        assert bool(torch.isnan(f32).all())
    elif reach == "none":
        assert not bool(bad.any()) and e_ref > 0
    else:
        assert bool(bad.any()) and bool((~bad).any())                         # some entries non-finite, some finite
        assert torch.equal(bad.any(2), bad.all(2))                            # whole rows
        assert bool(bad[:, gc.NF_I].all())
        assert e_ref > 0
    assert not bool(torch.isneginf(f32).any())                               # behind a ReLU
    with torch.no_grad():
        front = q.front(gc.observation(spec, words, target), edges, per_env=True)
    if case in gc.ONEHOT_SPREADS:
        assert bool((~torch.isfinite(front))[~torch.isfinite(f32)].all()) and bool(torch.isnan(front).all())
    else:
        assert gc.same_pattern(front, f32)


def test_m1_statement_keeps_a_nan():
    """The numpy statement of the M1 table with F.relu's law: a NaN first-Linear weight that meets a
    zero input still makes the hidden unit NaN (0 * NaN), so every entry of the table is NaN; a NaN
    second-Linear bias makes exactly its column NaN."""
    cases = dict(gc.nonfinite_front_cases(7))
    q = gc.make_q(7, 5, 47, bn="random")
    assert np.isfinite(gc.m1_table_numpy(q)).all()
    cases["nan conv1.0.weight"](q)
    assert np.isnan(gc.m1_table_numpy(q)).all()
    q = gc.make_q(7, 5, 47, bn="random")
    cases["nan conv1.2.bias"](q)
    nan = np.isnan(gc.m1_table_numpy(q))
    assert nan[:, gc.NF_O].all() and nan.sum() == 16


# ------------------------------------------------------------------------------------ the split store
@pytest.mark.parametrize("n,words,term_mask,done_mask", [(1, 2, 1, 3), (65, 4, 1, 3), (257, 2, 4, 0x30), (255, 4, 0x80, 0x01)])
def test_numpy_partition_equals_the_law_row_by_row(n, words, term_mask, done_mask):
    """Two capacities (n and 3 n + 1), masks other than 1 / 3, flags from all 256 byte values."""
    rng = np.random.default_rng(n)
    a = gc.canary_rings(n, 3 * n + 1, words, 1)
    b = gc.canary_rings(n, 3 * n + 1, words, 1)
    all_bytes = np.arange(256, dtype=np.uint8)
    for kind in gc.SPLIT_FRAMES:
        fields, flags = gc.split_frame(rng, n, words, 1, kind, all_bytes, term_value=term_mask, other_value=done_mask & ~term_mask)
        ca = gc.expected_rings(a[0], a[1], a[2], a[3], fields, flags, term_mask, done_mask)
        cb = gc.expected_rings_rowwise(b[0], b[1], b[2], b[3], fields, flags, term_mask, done_mask)
        assert ca == cb and a[1] == b[1] and a[2] == b[2], kind
        for key in "pn":
            for f in a[0][key]:
                assert np.array_equal(a[0][key][f].view(np.uint8), b[0][key][f].view(np.uint8)), (kind, key, f)
    assert a[2]["p"] == n and a[2]["n"] <= 3 * n + 1 and a[1]["p"] < n


@pytest.mark.parametrize("n,words", [(1, 2), (63, 4), (65, 2), (257, 4)])
def test_numpy_partition_equals_the_cpu_split_replay(n, words):
    """Where the CPU path can say it (one capacity for both rings, the env's own masks): the GPU sweep's
    frame kinds, "only env 0 terminated" among them, at its partly filled waves and blocks."""
    rng = np.random.default_rng(100 + n)
    cap = 3 * n + 1
    rp = SplitDeviceReplay(cap, words, 1, "cpu")
    rings, pos, size, capd = gc.canary_rings(cap, cap, words, 1)
    for key, ring in (("p", rp.positive), ("n", rp.negative)):
        for f, v in gc.RING_CANARY.items():
            getattr(ring, f).fill_(v)
    for kind in gc.SPLIT_FRAMES:
        fields, flags = gc.split_frame(rng, n, words, 1, kind)
        t = {k: torch.from_numpy(v) for k, v in fields.items()}
        rp.store(t["state"], t["target"], t["action"], t["reward"], t["next_state"], torch.from_numpy(flags))
        cp, cn = gc.expected_rings(rings, pos, size, capd, fields, flags)
        assert rp.counts.tolist() == [cp, cn] and rp._ctr.tolist() == [pos["p"], size["p"], pos["n"], size["n"]], kind
        for key, ring in (("p", rp.positive), ("n", rp.negative)):
            for f, want in rings[key].items():
                assert np.array_equal(getattr(ring, f).numpy(), want), (kind, key, f)
    assert size["n"] == cap or n == 1
