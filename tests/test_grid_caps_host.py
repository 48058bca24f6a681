"""tests/grid_caps.py against the sources (no GPU): every stated cap is the literal that stands in the
launch line of pbn_rl_amd/csrc, every case of test_gpu_grid_caps.py is past its cap, and every numpy
reference of that file is evaluated once on a small input whose answer is known by construction."""
import os
import re

import numpy as np
import pytest

from oracle import agent_oracle
from tests import grid_caps as G
from tests import replay_edge_cases as C
from tests.edge_shapes import edge_spec
from tests.test_gpu_evaluate import reduce_np
from tests.test_gpu_state_table import unique_counts

CUS = [1, 64, 256, 304]      # pbn_copy_async's cap is per compute unit: the cases hold at any count


def source(name):
    with open(os.path.join(G.CSRC, name)) as f:
        return f.read()


# ---- the caps are the sources' ----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(G.CAPS))
def test_cap_literal_stands_in_the_launch_line(name):
    """The grid expression is in the source verbatim, exactly once, it ends in the stated literal, the
    literal resolves (itself, or through the stated constexpr lines) to the stated value, and the next
    launch after it is the stated kernel's."""
    cap = G.CAPS[name]
    text = source(cap.source)
    assert text.count(cap.line) == 1, (name, "the launch line changed: restate the cap and its cases")
    m = re.fullmatch(r"std::min<int64_t>\((.*), (?:\(int64_t\)n_cus \* )?(\w+)\)", cap.line)
    assert m and m.group(2) == cap.literal
    for d in cap.defs:
        assert text.count(d) == 1, (name, d)
    consts = {x.group(1): int(x.group(2)) for x in (re.fullmatch(r"constexpr \w+ (\w+) = (\d+);", d) for d in cap.defs)
              if x}
    value_of = lambda s: int(s) if s.isdigit() else consts[s]  # noqa: E731
    assert value_of(cap.literal) == cap.blocks
    div = re.search(r"\) / (\w+)$", m.group(1))      # the elements are divided by the block size the launch uses
    if div:
        assert value_of(div.group(1)) == cap.threads
    after = text[text.index(cap.line):]
    launch = re.search(r"hipLaunchKernelGGL\(([^,]+(?:\([^)]*\))?),", after)
    assert launch and launch.group(1) == G.KERNELS[name], (name, launch and launch.group(1))


def test_every_capped_launch_is_stated():
    """Every std::min-clamped grid of csrc is one of CAPS or one of the three the suite crosses
    elsewhere: a new capped launch needs a row and a case."""
    known = {c.line for c in G.CAPS.values()}
    elsewhere = {
        # tests/test_gpu_replay_edges.py::test_replay_batch_grid_stride
        "std::min<int64_t>((total + kObsThreads - 1) / kObsThreads, 4096)",
        # tests/test_gpu_gbdq_edges.py: 2,080 envs against 2,048 blocks
        "std::min<int64_t>(n_envs, 2048)",
        # the DDQN update's Adam pass: tests/test_gpu_ddqn_edges.py at N = 97, arch (64, 16) (below)
        "std::min<int64_t>((a.d.off[TOTAL] + kGradThreads - 1) / kGradThreads, 1024)",
    }
    found = set()
    for name in sorted(os.listdir(G.CSRC)):
        text = source(name)
        for m in re.finditer(r"std::min<int64_t>\(", text):
            depth, end = 1, m.end()
            while depth:
                depth += {"(": 1, ")": -1}.get(text[end], 0)
                end += 1
            found.add(text[m.start():end])
    assert found == known | elsewhere, found ^ (known | elsewhere)


def test_adam_grid_is_crossed_by_the_edge_sweep():
    """The DDQN update's Adam pass (1024 x 256 parameters a trip) takes three trips at N = 97, arch
    (64, 16), a case of test_gpu_ddqn_edges.py that holds every parameter to the Adam step."""
    al16 = lambda x: (x + 15) // 16 * 16  # noqa: E731
    N, (h0, h1) = 97, (64, 16)
    total = sum(al16(s) for s in (h0 * N * N, h0, h1 * h0, h1, (N + 1) * h1, N + 1))
    assert 2 * 1024 * 256 < total


# ---- every case is past its cap ---------------------------------------------------------------------
def test_histogram_cases_are_past_the_cap():
    for rows, stride, cols in G.HIST_SHAPES:
        assert G.past("hist", rows * cols) and stride >= cols
    one = G.CAPS["hist"].elements()
    assert G.HIST_SHAPES[0][0] * G.HIST_SHAPES[0][2] == one + 1
    over = 33 * 32_771 - one
    assert 0 < over < one and over % 64 != 0                                # a ragged last wave, on the second trip
    assert 3 * 699_071 > 2 * one                                            # a third trip
    assert max(G.HIST_BITS) <= 20 and 1 in G.HIST_BITS


@pytest.mark.parametrize("n_cus", CUS)
def test_copy_cases_are_past_the_cap(n_cus):
    S, sizes = G.copy_sizes(n_cus)
    one = G.CAPS["copy"].elements(n_cus)
    assert one == 4 * S == 1024 * 8 * n_cus
    assert all(G.past("copy", n, n_cus) for n in sizes[-5:]) and not G.past("copy", sizes[1], n_cus)
    # what the sizes reach, from the kernel's two loops restated
    assert G.copy_trips(sizes[0], S, S - 1) == (0, 3) and G.copy_trips(sizes[0], S, 0) == (1, 0)
    assert G.copy_trips(sizes[1], S, S - 1) == (1, 0)
    assert G.copy_trips(sizes[2], S, 0) == (1, 1) and G.copy_trips(sizes[2], S, 1) == (1, 0)
    assert G.copy_trips(sizes[3], S, 6) == (1, 2) and G.copy_trips(sizes[3], S, 7) == (1, 1)
    assert G.copy_trips(sizes[4], S, 254) == (2, 0) and G.copy_trips(sizes[4], S, 255) == (1, 3)      # in one wave
    assert G.copy_trips(sizes[5], S, S - 1) == (2, 0)
    assert G.copy_trips(sizes[6], S, 0) == (2, 1)
    # test_copy_async_entry_point's 4 MiB: one unrolled trip at most, never a trip and a tail
    n16 = ((1 << 22) - 16 * 7) // 16
    S4 = G.copy_stride(n16, n_cus)
    if n_cus >= 128:
        assert {G.copy_trips(n16, S4, i) for i in (0, S4 - 8, S4 - 7, S4 - 1)} <= {(1, 0), (0, 3)}


def test_reduce_cases_are_past_the_cap():
    for shape in G.REDUCE_SHAPES:
        n_pairs, _ = shape
        if shape == G.REDUCE_AT_CAP:
            assert n_pairs == G.CAPS["eval_reduce"].elements()             # the last one-trip size
        else:
            assert G.past("eval_reduce", n_pairs)
    assert sum(G.past("eval_reduce", p) for p, _ in G.REDUCE_SHAPES) == len(G.REDUCE_SHAPES) - 1
    assert 254 * 254 == 64_516 and G.REDUCE_CLAMPED in G.REDUCE_SHAPES
    assert max(G.REDUCE_MAX_STEPS) == 254


def test_obs_store_table_cases_are_past_the_cap():
    for N, n in G.OBS_CASES:
        assert G.past("obs_unpack", n * N) and n % 32 == 0 and N % 4 != 0 and n * N < 2 ** 31
        assert n * N - G.CAPS["obs_unpack"].elements() < 4 * N * 32          # just past it
    assert G.past("replay_store", G.STORE_N) and G.STORE_CAPACITY == G.STORE_N + 13
    wrap = G.STORE_CAPACITY - G.STORE_POS                                     # the first row written to slot 0
    assert G.CAPS["replay_store"].elements() <= wrap < G.STORE_N
    rows, stride, cols = G.TABLE_SHAPE
    assert G.past("table_insert", rows * cols) and stride > cols
    assert 2 * rows * cols <= G.TABLE_CAPACITY


def test_dqn_case_is_past_both_caps():
    N, A = 70, 254
    h0, h1 = G.DQN_ARCH
    iT, t_floats, itotal = G.dqn_image_layout(N, A, h0, h1)
    assert t_floats == 254 * 70 * 64 == 1_137_920
    assert G.past("dqn_pack", itotal)
    n_flat = sum((s + 15) // 16 * 16 for s in (h0 * N * N, h0, h1 * h0, h1, (N + 1) * h1, N + 1))
    assert G.past("ddqn_schedule", n_flat + itotal)
    one = G.CAPS["dqn_pack"].elements()
    assert [t for t in range(A) if iT + G.dqn_t_row(N, h0, t) >= one][0] == 235
    assert {234, 235, 253} <= set(G.DQN_TARGETS)


# ---- the references, once, on inputs whose answer is known -------------------------------------------
def test_histogram_reference_and_mixes():
    shape = (3, 200, 150)
    for n_bits in G.HIST_BITS:
        empty = G.hist_empty_bin(shape, n_bits)
        for mix in G.HIST_MIXES:
            st = G.hist_input(shape, n_bits, mix)
            want = G.hist_expected(st, 150, n_bits)
            assert int(want.sum()) == 450 and want[empty] == 0
            assert ((st[:, 150:] & np.uint32((1 << n_bits) - 1)) == empty).all()
            assert (st >> np.uint32(n_bits)).max() > 0 or n_bits == 32      # the mask matters
            if mix == "equal":
                assert (want != 0).sum() == 1
            if mix == "distinct" and n_bits >= 7:
                assert G.distinct_per_wave(st, 150, n_bits) == 64             # far above the four merge rounds
            if mix == "hot" and n_bits >= 7:
                assert np.sort(want)[-5:].sum() > 0.6 * 450
    # a hand count
    st = np.array([[1, 2, 9], [3, 3, 9]], np.uint32)
    assert G.hist_expected(st, 2, 2).tolist() == [0, 1, 1, 2]
    # without uncounted columns both bins of n_bits = 1 are in use
    assert G.hist_empty_bin(G.HIST_SHAPES[0], 1) is None
    st = G.hist_input((1, 640, 640), 1, "distinct")
    assert G.hist_expected(st, 640, 1).tolist() == [320, 320]


def test_reduce_reference_and_plants():
    for n_pairs, runs in [(2048, 3), (2049, 1), (4097, 65)]:
        given, clamped, planted = G.reduce_counts(n_pairs, runs, 5)
        s, f, h = reduce_np(clamped, 5)
        assert s[planted["fail_first"]] == 6 * runs and f[planted["fail_first"]] == runs
        assert s[planted["zero_first"]] == 0 and f[planted["zero_first"]] == 0
        assert ("fail_second" in planted) == (n_pairs > 2048)
        if "fail_second" in planted:
            assert planted["fail_second"] >= 2048 and f[planted["fail_second"]] == runs
        if "zero_second" in planted:
            assert planted["zero_second"] >= 2048 and s[planted["zero_second"]] == 0
        assert int(h.sum()) == n_pairs * runs and len(h) == 7
        assert np.array_equal(given, clamped) == ((n_pairs, runs) != G.REDUCE_CLAMPED)
    given, clamped, _ = G.reduce_counts(*G.REDUCE_CLAMPED, 5)
    assert given.min() == -3 and given.max() == 14 and clamped.min() == 0 and clamped.max() == 6
    assert np.array_equal(clamped, np.clip(given, 0, 6))
    assert reduce_np(np.array([[0, 6], [2, 3]], np.int32), 5)[2].tolist() == [1, 0, 1, 1, 0, 0, 1]


def test_obs_reference_on_a_small_input():
    spec = edge_spec(33)
    st, tg = G.obs_input(spec, 64)
    A = len(spec.attractors)
    assert set(range(A)) <= set(tg.tolist()) and 255 in tg and A in tg
    want = agent_oracle.obs_unpack(spec, st, tg)
    assert want.shape == (2, 64, 33)
    e = 7
    assert want[0, e].tolist() == [float((int(st[i >> 5, e]) >> (i & 31)) & 1) for i in range(33)]
    assert want[1, e].tolist() == ([float(b) for b in spec.attractors[tg[e]][0]] if tg[e] < A else [0.0] * 33)
    assert not want[1][tg >= A].any()


def test_store_reference_on_a_small_input():
    t = C.store_transitions(5, 2, 3, seed=1)
    ring, done01 = C.store_expected(7, 2, 3, 4, t, done_mask=5)
    assert done01.tolist() == [int(bool(d & 5)) for d in t["done"]]
    for e, j in enumerate((4, 5, 6, 0, 1)):
        assert ring["state"][:, j].tolist() == t["state"][:, e].tolist()
        assert ring["action"][j].tolist() == t["action"][e].tolist() and ring["done"][j] == done01[e]
    assert (ring["target"][2:4] == 0xEE).all() and (ring["state"][:, 2:4] == 0xF9F9F9F9).all()
    assert (ring["action"][2:4] == -7).all() and (ring["reward"][2:4] == -7.0).all()
    assert C.store_expected(7, 2, 3, 4, t)[1].tolist() == [int(d != 0) for d in t["done"]]


def test_table_reference_on_a_small_input():
    st = np.array([[[5, 9, 5, 7]], [[9, 9, 1, 7]]], np.uint32)                # (T = 2, W = 1, stride 4), 3 counted
    words, counts = unique_counts(st, 3, 32)
    assert words.ravel().tolist() == [1, 5, 9] and counts.tolist() == [1, 2, 3]
    words, counts = unique_counts(st, 3, 32, np.array([2, 0, 1, 0, 4, 0], np.uint64))
    assert words.ravel().tolist() == [5, 9] and counts.tolist() == [3, 4]
