"""csrc/state_table.h on the host, and the numpy side of the sparse steady-state distribution.

tests/state_table_check.cpp (compiled with hipcc, host side only) runs the hash, the masked key
load, the key compare and the probe loop the insert kernel runs, with a single thread's atomics;
this test compares the drained table with np.unique and measures the hash on structured keys.
"""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from pbn_rl_amd.attractors import load_attractors
from pbn_rl_amd.network import load_network
from pbn_rl_amd.spec import EnvSpec
from pbn_rl_amd.ssd import compute_ssd_hist
from pbn_rl_amd.state_table import SparseSSD, _capacity_for, sort_states

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "pbn_rl_amd", "csrc")
WORDS = [1, 2, 3, 4]


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.fail("hipcc not found: state_table.h needs the HIP headers")
    exe = tmp_path_factory.mktemp("state_table") / "state_table_check"
    subprocess.run(["hipcc", "-x", "hip", "--offload-host-only", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC,
                    "-o", str(exe), os.path.join(HERE, "state_table_check.cpp")], check=True)
    return str(exe)


def run(exe, lines):
    """One command per line -> the result lines' fields (without the command word), as ints."""
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    rows = [ln.split() for ln in out.split("\n") if ln.strip()]
    assert len(rows) == len(lines) and all(r[0] == ln.split()[0] for r, ln in zip(rows, lines))
    return [[int(x) for x in r[1:]] for r in rows]


def insert_line(epoch, rows, counts=None, pad=0):
    """rows (R, W) uint32 as one launch of T = 1 (stride R + pad; the padding columns hold junk)."""
    R, W = rows.shape
    st = np.full((W, R + pad), 0xDEADBEEF, dtype=np.uint32)
    st[:, :R] = rows.T
    tail = "" if counts is None else " " + " ".join(str(int(c)) for c in counts)
    return "insert %d 1 %d %d %d %s%s" % (epoch, R, R + pad, counts is not None, " ".join(map(str, st.ravel())), tail)


def drained(fields, W):
    """a drain line -> (words (S, W), counts (S,)) ascending by state value"""
    S = fields[0]
    body = np.array(fields[1:], dtype=np.uint64).reshape(S, W + 1)
    words, counts = body[:, :W].astype(np.uint32), body[:, W]
    order = sort_states(words)
    return words[order], counts[order]


def unique_counts(rows, n_bits, counts=None):
    """np.unique of the rows masked to n_bits, ascending by state value, with summed counts"""
    W = rows.shape[1]
    rows = rows.copy()
    top = n_bits - 32 * (W - 1)
    rows[:, W - 1] &= np.uint32((1 << top) - 1)
    uniq, inv = np.unique(rows, axis=0, return_inverse=True)
    cnt = np.bincount(inv.ravel(), weights=None if counts is None else counts.astype(np.float64),
                      minlength=len(uniq)).astype(np.uint64)
    keep = cnt > 0
    uniq, cnt = uniq[keep], cnt[keep]
    order = sort_states(uniq)
    return uniq[order], cnt[order]


def hot_rows(rng, W, n_rows, hot_share=0.7, n_hot=5, n_pool=1500):
    """n_rows keys of W words: hot_share of them drawn from n_hot hot keys, the rest from a pool of
    n_pool random keys (so cold keys repeat too, within and across launches)"""
    pool = rng.integers(0, 1 << 32, size=(n_pool, W), dtype=np.uint64).astype(np.uint32)
    rows = pool[rng.integers(0, n_pool, size=n_rows)]
    hot = rng.integers(0, 1 << 32, size=(n_hot, W), dtype=np.uint64).astype(np.uint32)
    pick = rng.random(n_rows) < hot_share
    rows[pick] = hot[rng.integers(0, n_hot, size=int(pick.sum()))]
    return rows


@pytest.mark.parametrize("W", WORDS)
def test_two_launches_equal_np_unique(check_exe, W):
    """4,000 rows, 70 % from 5 hot keys, as two launches (epochs 1 and 2; the second holds keys of
    the first -- compared with `keys` -- and new ones -- compared with the input)."""
    rng = np.random.default_rng(10 + W)
    n_bits = 32 * W - 3
    rows = hot_rows(rng, W, 4000)
    first, second = rows[:1800], rows[1800:]
    allrows = rows
    res = run(check_exe, ["table %d %d %d" % (W, n_bits, _capacity_for(len(allrows))),
                          insert_line(1, first, pad=3), insert_line(2, second, pad=5), "drain"])
    words, counts = drained(res[3], W)
    want_w, want_c = unique_counts(allrows, n_bits)
    assert res[2] == [len(want_w), 0]          # used, lost
    assert np.array_equal(words, want_w) and np.array_equal(counts, want_c)
    assert int(counts.sum()) == len(allrows) == 4000 and len(want_w) > 500
    # the second launch held keys of the first (beyond the hot ones) and keys of its own
    old = {tuple(r) for r in unique_counts(first, n_bits)[0].tolist()}
    seen2 = {tuple(r) for r in unique_counts(second, n_bits)[0].tolist()}
    assert len(seen2 & old) > 50 and len(seen2 - old) > 50


@pytest.mark.parametrize("W", WORDS)
def test_rehash_from_capacity_64_gives_the_same_table(check_exe, W):
    """The same rows in launches of 500 into a table that starts at 64 slots and is rehashed (a
    launch over its own keys with its counts) whenever the next launch might pass load 1/2."""
    rng = np.random.default_rng(10 + W)
    n_bits = 32 * W - 3
    rows = hot_rows(rng, W, 4000)
    lines, cap, used_ub, epoch, n_rehash = ["table %d %d 64" % (W, n_bits)], 64, 0, 1, 0
    for lo in range(0, len(rows), 500):
        part = rows[lo:lo + 500]
        if used_ub + len(part) > cap // 2:
            cap = _capacity_for(used_ub + len(part))
            lines.append("rehash %d" % cap)
            epoch, n_rehash = 2, n_rehash + 1
        lines.append(insert_line(epoch, part))
        epoch += 1
        used_ub += len(part)
    res = run(check_exe, lines + ["drain"])
    words, counts = drained(res[-1], W)
    want_w, want_c = unique_counts(rows, n_bits)
    assert n_rehash >= 3 and all(r[1] == 0 for r in res[1:-1])      # nothing lost in any launch
    assert np.array_equal(words, want_w) and np.array_equal(counts, want_c)


def test_keys_that_differ_in_high_words_only_and_above_n_bits(check_exe):
    """Keys equal in their low 64 bits that differ only in word 2 or word 3 stay apart; keys that
    differ only above n_bits merge."""
    base = np.array([0x12345678, 0x9ABCDEF0, 7, 1], dtype=np.uint32)
    rows = np.stack([base, base, base ^ np.uint32([0, 0, 1 << 31, 0]), base ^ np.uint32([0, 0, 0, 2]),
                     base ^ np.uint32([0, 0, 0, 1 << 20]),       # bit 116: above n_bits = 110
                     base ^ np.uint32([0, 0, 0, 1 << 31])]).astype(np.uint32)
    res = run(check_exe, ["table 4 110 64", insert_line(1, rows[:3]), insert_line(2, rows[3:]), "drain"])
    words, counts = drained(res[3], 4)
    want_w, want_c = unique_counts(rows, 110)
    assert len(want_w) == 3 and sorted(want_c.tolist()) == [1, 1, 4]
    assert np.array_equal(words, want_w) and np.array_equal(counts, want_c)
    # W = 3: word 2 alone tells the keys apart; bits above n_bits = 70 are no part of the key
    rows3 = np.array([[5, 6, 1], [5, 6, 2], [5, 6, 1 | (1 << 6)], [5, 6, 2 | (1 << 30)]], dtype=np.uint32)
    res = run(check_exe, ["table 3 70 64", insert_line(1, rows3), "drain"])
    words, counts = drained(res[2], 3)
    assert words.tolist() == [[5, 6, 1], [5, 6, 2]] and counts.tolist() == [2, 2]


def test_row_counts_and_skipped_rows(check_exe):
    rng = np.random.default_rng(5)
    rows = hot_rows(rng, 2, 600)
    mult = rng.integers(0, 4, size=600).astype(np.uint64)
    mult[:5] = [0, 1 << 40, 0, 3, 0]          # zeros skip; counts are 64-bit
    res = run(check_exe, ["table 2 64 2048", insert_line(1, rows, counts=mult), "drain"])
    words, counts = drained(res[2], 2)
    want_w, want_c = unique_counts(rows[mult > 0], 64, mult[mult > 0])
    assert np.array_equal(words, want_w)
    assert int(counts.sum()) == int(mult.sum()) and np.array_equal(counts, want_c)


def structured_sets(W):
    ints = np.arange(1 << 15, dtype=np.uint32)
    low = np.zeros((len(ints), W), dtype=np.uint32)
    low[:, 0] = ints
    top = np.zeros((len(ints), W), dtype=np.uint32)
    top[:, W - 1] = ints
    nb = 32 * W
    keys = [1 << a for a in range(nb)] + [(1 << a) | (1 << b) for a, b in itertools.combinations(range(nb), 2)]
    sparse = np.array([[(k >> (32 * w)) & 0xFFFFFFFF for w in range(W)] for k in keys], dtype=np.uint32)
    return {"ints_in_word0": low, "ints_in_top_word": top, "one_and_two_bit_keys": sparse}


@pytest.mark.parametrize("W", WORDS)
def test_hash_quality_on_structured_keys(check_exe, W):
    """Mean probe displacement at load <= 1/2 (the largest load the table allows).  Linear probing
    with a uniform hash gives 0.5 at load 1/2 (Knuth: (1 / (1 - a) - 1) / 2 probes past the home
    slot); the bound is twice that.  A weak mix (e.g. the low key bits as the slot) would put
    0..2^15-1 in the top word all on one slot."""
    for name, keys in structured_sets(W).items():
        cap = _capacity_for(len(keys))
        res = run(check_exe, ["table %d %d %d" % (W, 32 * W, cap), insert_line(1, keys), "disp"])
        assert res[1] == [len(keys), 0]
        total, n = res[2]
        mean = total / n
        print(f"W={W} {name}: {n} keys in {cap} slots, mean displacement {mean:.3f}")
        assert n == len(keys) and mean <= 1.0, (name, mean)


def test_sparse_ssd_on_a_hand_made_table():
    # N = 5: states 3 (nodes 0, 1), 9 (nodes 0, 3), 16 (node 4), 30 (nodes 1..4)
    ssd = SparseSSD(np.array([[3], [9], [16], [30]], dtype=np.uint32), np.array([5, 1, 10, 4], dtype=np.uint64), 5)
    assert ssd.total == 20 and len(ssd) == 4 and ssd.n_nodes == 5
    assert np.array_equal(ssd.probs, np.array([5, 1, 10, 4]) / 20) and ssd.probs.dtype == np.float64
    assert ssd.bits.dtype == np.uint8
    assert ssd.bits.tolist() == [[1, 1, 0, 0, 0], [1, 0, 0, 1, 0], [0, 0, 0, 0, 1], [0, 1, 1, 1, 1]]
    bits, probs = ssd.top(2)
    assert bits.tolist() == [[0, 0, 0, 0, 1], [1, 1, 0, 0, 0]] and probs.tolist() == [0.5, 0.25]
    assert len(ssd.top(10)[1]) == 4
    assert np.allclose(ssd.marginals(), np.array([6, 9, 4, 5, 14]) / 20, rtol=0, atol=1e-15)
    dense = ssd.to_dense()
    want = np.zeros(32)
    want[[3, 9, 16, 30]] = np.array([5, 1, 10, 4]) / 20
    assert dense.shape == (32,) and np.array_equal(dense, want)
    # round trip: the non-zero bins of the dense array are the table
    nz = np.nonzero(dense)[0]
    assert np.array_equal(nz.astype(np.uint32), ssd.words[:, 0]) and np.array_equal(dense[nz], ssd.probs)


def test_sparse_ssd_of_a_wide_network_and_an_empty_one():
    words = np.array([[1, 0, 1 << 5], [0xFFFFFFFF, 2, 0]], dtype=np.uint32)
    ssd = SparseSSD(words, np.array([3, 1], dtype=np.uint64), 70)
    assert ssd.bits.shape == (2, 70) and ssd.bits[0, 69] == 1 and ssd.bits[1, :32].all() and ssd.bits[1, 33] == 1
    assert ssd.marginals()[69] == 0.75 and ssd.marginals()[0] == 1.0
    with pytest.raises(ValueError, match="at most 32 nodes"):
        ssd.to_dense()
    empty = SparseSSD(np.zeros((0, 1), dtype=np.uint32), np.zeros(0, dtype=np.uint64), 7)
    assert empty.total == 0 and empty.probs.shape == (0,) and empty.marginals().tolist() == [0.0] * 7
    assert not empty.to_dense().any()


def test_dense_call_still_stops_at_32_nodes_before_any_device_call():
    spec = EnvSpec(load_network("pbn70"), load_attractors("pbn70"))
    with pytest.raises(ValueError, match="at most 32 nodes") as e:
        compute_ssd_hist(spec, resets=32, iters=1, sparse=False)
    assert "sparse=True" in str(e.value)
