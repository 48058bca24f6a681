"""csrc/curriculum_law.h, the device statement of the curriculum reset law, on the host against
tests/curriculum_reference.py.

tests/curriculum_law_check.cpp (compiled with hipcc, host side only, as tests/test_step_law_host.py
compiles its program) calls the table build and the draw that pbn_curriculum.hip's kernels call.
Also here, on the reference alone: that the integer rule is the facade's float rule to within its
quantisation, and that the draw has the table's distribution.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import pyoracle
from tests import curriculum_reference as C

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "pbn_rl_amd", "csrc")
M32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.fail("hipcc not found: curriculum_law.h needs the HIP headers")
    exe = tmp_path_factory.mktemp("curriculum_law") / "curriculum_law_check"
    subprocess.run(["hipcc", "-x", "hip", "--offload-host-only", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC,
                    "-o", str(exe), os.path.join(HERE, "curriculum_law_check.cpp")], check=True)
    return str(exe)


def run(exe, lines):
    """One command per line -> the result lines' fields (without the command word)."""
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    rows = [ln.split() for ln in out.split("\n") if ln.strip()]
    assert len(rows) == len(lines) and all(r[0] == ln.split()[0] for r, ln in zip(rows, lines))
    return [[int(v) for v in r[1:]] for r in rows]


def tab_line(A, H, entries):
    return "tab %d %d %d %s" % (A, H, len(entries), " ".join("%d %d %d %d" % e for e in entries))


def att_start_of(sizes):
    return [0] + [int(x) for x in np.cumsum(sizes)]


def edge_words(table, rng):
    """The 64-bit draws the issue names, as (x0, x1): X = 0 and 2^64 - 1, the last value of a row and
    the first of the next for the first, a middle and the last row, the same around the diagonal
    entry inside those rows, and seeded ones."""
    rowcdf, cdf, total = [int(x) for x in table["rowcdf"]], table["cdf"], table["total"]
    A = len(rowcdf)
    vs = {0, total - 1}
    for s in sorted({0, A // 2, A - 1}):
        base = rowcdf[s - 1] if s else 0
        vs |= {rowcdf[s] - 1, min(rowcdf[s], total - 1), base}
        left = int(cdf[s][s - 1]) if s else 0              # the prefix sum the diagonal entry repeats
        vs |= {base + max(left - 1, 0), min(base + left, rowcdf[s] - 1)}
    words = [(0, 0), (M32, M32)] + [C.x_for(v, total) for v in sorted(vs)]
    words += [(int(a), int(b)) for a, b in rng.integers(0, 1 << 32, size=(200, 2), dtype=np.uint64)]
    return words


def sizes_for(name, A):
    """The attractors' sizes of a case's draws: one state each, or mixed with a 1,000-state one."""
    if name == "a5_skewed":
        return list(C.SKEWED_SIZES)
    if name.endswith("_seeded"):
        return [(1000, 1, 3, 7)[a % 4] for a in range(A)]
    return [1] * A


@pytest.mark.parametrize("name", sorted(C.PAIR_CASES))
def test_table_and_draws(check_exe, name):
    A, H, entries = C.PAIR_CASES[name]
    table = C.build_table(C.dense_pairs(A, entries), H)
    att_start = att_start_of(sizes_for(name, A))
    rng = np.random.default_rng(500 + A)
    draws = [(x0, x1, int(x2), int(x3)) for (x0, x1), (x2, x3) in
             zip(edge_words(table, rng), rng.integers(0, 1 << 32, size=(400, 2), dtype=np.uint64))]
    draws[0] = draws[0][:2] + (0, 0)                       # the first and the last state of the attractor
    draws[1] = draws[1][:2] + (M32, M32)
    res = run(check_exe, [tab_line(A, H, entries), "first " + " ".join(map(str, att_start))] +
              ["draw %d %d %d %d" % d for d in draws])
    total, size = res[0][:2]
    assert total == table["total"] == int(table["rowcdf"][-1]) and size == 8 * A + (4 * A * A + 7) // 8 * 8 + 16
    assert res[0][2:2 + A] == [int(x) for x in table["rowcdf"]]
    assert res[0][2 + A:] == [int(x) for x in table["cdf"].ravel()]
    assert res[1] == [A + 1]
    seen_s, seen_t = set(), set()
    for d, r in zip(draws, res[2:]):
        s, t, row = C.draw_from_words(table, d, att_start)
        assert r == [s, t, row], (name, d)
        assert s != t and att_start[s] <= row < att_start[s + 1]
        seen_s.add(s)
        seen_t.add((s, t))
    assert {0, A // 2, A - 1} <= seen_s
    # around the diagonal: the last target left of it and the first right of it, in a middle row
    m = A // 2
    assert A == 2 or {(m, m - 1), (m, m + 1 if m + 1 < A else m - 1)} <= seen_t
    # the weights: all equal without statistics, and never below 2^8 off the diagonal
    w = table["w"]
    off = ~np.eye(A, dtype=bool)
    assert (w[off] >= 256).all() and (np.diag(w) == 0).all()
    if not entries:
        assert (w[off] == H << 8).all()


def test_cap_and_large_sums():
    A, H, entries = C.PAIR_CASES["a3_cap"]
    w = C.build_table(C.dense_pairs(A, entries), H)["w"]
    assert w[0, 1] == C.CAP and w[2, 0] == ((H + 65515) << 8) < C.CAP and w[1, 1] == 0
    A, H, entries = C.PAIR_CASES["a3_huge"]
    w = C.build_table(C.dense_pairs(A, entries), H)["w"]
    assert w[1, 2] == C.CAP and w[0, 2] == ((H + 9) << 8) // 4
    A, H, entries = C.PAIR_CASES["a254_all_cap"]
    t = C.build_table(C.dense_pairs(A, entries), H)
    assert t["total"] == 254 * 253 * C.CAP < 1 << 40 and int(t["cdf"][:, -1].max()) == 253 * C.CAP < 1 << 32


def test_philox_call(check_exe):
    """Stream 8, call 0, the env's global id and the step's index as pyoracle.draw packs them."""
    cases = [(0, 0, 0), (0xC3A5C85C97CB3127, (1 << 33) + 64 + 5, 12), (977, 69, (3 << 32) | 7)]
    res = run(check_exe, ["phx %d %d %d" % c for c in cases])
    for c, r in zip(cases, res):
        assert tuple(r) == pyoracle.draw(*c, C.CURRICULUM, 0)
    assert C.CURRICULUM == 8 and tuple(res[0]) != pyoracle.draw(0, 0, 0, 7, 0)


@pytest.mark.parametrize("name", ["a3_seeded", "a14_seeded", "a254_seeded", "a3_cap", "a3_huge", "a5_skewed"])
def test_the_rule_is_the_facades(name):
    """weights() against EpisodeStats.pair_weights' float formula on the same pairs.  An integer weight
    is floor(2^8 f) for the float rule's f = (H + L) / (1 + E), so w / 2^8 lies in (f - 2^-8, f]: a
    relative error of at most d = 2^-8 / f_min, where f_min is the smallest f of the matrix (f >= 1: H
    >= 1 and every episode has a step).  The normalising sum has the same one-sided error, so a
    normalised weight is off by a factor in [1 - d, 1 / (1 - d)].  A weight at the cap is compared
    with the capped formula."""
    A, H, entries = C.PAIR_CASES[name]
    pairs = C.dense_pairs(A, entries)
    got = C.weights(C.build_table(pairs, H))
    want = C.float_rule(pairs, H, capped=True)
    f = (H + pairs[..., 2].astype(np.float64)) / (1.0 + pairs[..., 0])
    off = ~np.eye(A, dtype=bool)
    f_min = min(f[off].min(), C.CAP / 256.0)
    assert f_min >= 1.0
    d = 2.0 ** -8 / f_min
    ratio = got[off] / want[off]
    assert (ratio >= 1 - d - 1e-12).all() and (ratio <= 1 / (1 - d) + 1e-12).all(), (ratio.min(), ratio.max(), d)
    assert abs(got.sum() - 1.0) < 1e-12 and (np.diag(got) == 0).all()
    if name not in ("a3_cap", "a3_huge"):                  # nothing capped: the plain formula
        assert np.array_equal(want, C.float_rule(pairs, H))


DIST_SEED, DIST_DRAWS = 20261021, 200_000


def test_distribution():
    """200,000 reference draws on the skewed table: chi-square over the 20 pairs against w / total,
    and over the 7 states of attractor 1 among the draws that start there."""
    A, H, entries = C.PAIR_CASES["a5_skewed"]
    table = C.build_table(C.dense_pairs(A, entries), H)
    att_start = att_start_of(C.SKEWED_SIZES)
    rowcdf, cdf, total = table["rowcdf"].astype(np.uint64), table["cdf"], table["total"]
    counts = np.zeros((A, A), dtype=np.int64)
    states = np.zeros(7, dtype=np.int64)
    words = np.array([pyoracle.draw(DIST_SEED, e, 3, C.CURRICULUM, 0) for e in range(DIST_DRAWS)], dtype=object)
    for x in words[:2000]:                                  # the vectorised form below is the law's
        s, t, row = C.draw_from_words(table, x, att_start)
        counts[s, t] += 1
        if s == 1:
            states[row - att_start[1]] += 1
    first = counts.copy(), states.copy()
    counts[:], states[:] = 0, 0
    v = np.array([(((int(x[1]) << 32) | int(x[0])) * total) >> 64 for x in words], dtype=np.uint64)
    s = np.searchsorted(rowcdf, v, side="right")
    vs = v - np.where(s > 0, rowcdf[np.maximum(s, 1) - 1], np.uint64(0))
    for a in range(A):
        sel = s == a
        t = np.searchsorted(cdf[a], vs[sel].astype(np.uint32), side="right")
        np.add.at(counts[a], t, 1)
        if a == 1:
            idx = [(((int(x[3]) << 32) | int(x[2])) * 7) >> 64 for x in words[sel]]
            np.add.at(states, idx, 1)
        if a == 0:
            assert t.min() >= 1
    chk, chk_states = np.zeros_like(counts), np.zeros_like(states)
    sub = np.searchsorted(rowcdf, v[:2000], side="right")
    for a in range(A):
        np.add.at(chk[a], np.searchsorted(cdf[a], vs[:2000][sub == a].astype(np.uint32), side="right"), 1)
    assert np.array_equal(chk, first[0])
    assert counts.sum() == DIST_DRAWS and (np.diag(counts) == 0).all()
    off = ~np.eye(A, dtype=bool)
    expect = C.weights(table)[off] * DIST_DRAWS
    assert expect.min() >= 5                                # the chi-square approximation's usual floor
    chi = float((((counts[off] - expect) ** 2) / expect).sum())
    p_pairs = C.chi2_sf(chi, A * (A - 1) - 1)
    n1 = int(states.sum())
    chi_s = float((((states - n1 / 7.0) ** 2) / (n1 / 7.0)).sum())
    p_states = C.chi2_sf(chi_s, 6)
    print(f"pairs: chi2 {chi:.3f} p {p_pairs:.4f}; states of attractor 1: n {n1} chi2 {chi_s:.3f} p {p_states:.4f}")
    assert n1 > 0.5 * DIST_DRAWS
    assert p_pairs >= 1e-3 and p_states >= 1e-3
    # it is skewed: (1, 3) takes most draws
    assert counts[1, 3] > 0.5 * DIST_DRAWS


def test_chi2_sf_known_values():
    """The survival function at tabulated points (chi-square tables, three decimals)."""
    for x, df, p in [(30.144, 19, 0.05), (43.820, 19, 0.001), (12.592, 6, 0.05), (22.458, 6, 0.001), (18.338, 19, 0.5)]:
        assert abs(C.chi2_sf(x, df) - p) < 2e-4 * max(1.0, p / 0.05), (x, df, C.chi2_sf(x, df))
