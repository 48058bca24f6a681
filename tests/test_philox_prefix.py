"""philox_prefix / philox_tail (csrc/philox.h: the part of Philox4x32-R's first three rounds that
does not depend on counter word 1, built once, and the rest of the call from it) against philox,
the C oracle and the known answers, on the host.

The rollout kernel's RNG waves build one prefix per call site in front of their step loops, where
only the step's low word (counter word 1) moves, and call philox_tail every step; it has to be
the function philox is, for every counter and key, with and without the output xor XM.  The
selection wave also relies on two of the prefix's five words (B, D) being the same for calls that
differ in counter word 2 alone.  philox.h has no host binding, so a small program of its own is
compiled with hipcc, host side only (as tests/test_philox_round_keys.py does)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "pbn_rl_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden", "philox_kat.json")
SEEDS = [977, 2 ** 64 - 1, 0xC3A5C85C97CB3127]
XM = 0x80008000   # philox_prefix_check.cpp's kXM
# Random123 kat_vectors, philox4x32 R = 7, on the inputs of the golden file's cases 0..2
# (tests/test_philox.py pins the same words on the oracles)
R123_KAT7 = [[0x5F6FB709, 0x0D893F64, 0x4F121F81, 0x4F730A48],
             [0x5207DDC2, 0x45165E59, 0x4D8EE751, 0x8C52F662],
             [0x4DFCCABA, 0x190A87F0, 0xC47362BA, 0xB6B5242A]]


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.fail("hipcc not found: philox.h needs the HIP headers")
    exe = tmp_path_factory.mktemp("philox_prefix") / "philox_prefix_check"
    subprocess.run(["hipcc", "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                    "-o", str(exe), os.path.join(HERE, "philox_prefix_check.cpp")], check=True)
    return str(exe)


def run(exe, rows):
    """rows of (c0, c1, c2, c3, k0, k1) -> {(R, xm): (tail, ref)}, each [len(rows)][4], and the
    prefixes {R: [len(rows)][5]} (A, B, D, E, d3)."""
    text = "".join(" ".join("%x" % int(x) for x in r) + "\n" for r in rows)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    words = np.array([[int(w, 16) for w in ln.split()] for ln in out if ln.strip()], dtype=np.uint32)
    assert words.shape == (len(rows), 42)
    calls = {}
    for i, key in enumerate([(7, 0), (7, XM), (10, 0), (10, XM)]):
        calls[key] = (words[:, 8 * i:8 * i + 4], words[:, 8 * i + 4:8 * i + 8])
    return calls, {7: words[:, 32:37], 10: words[:, 37:42]}


def assert_all_equal(calls):
    for (R, xm), (tail, ref) in calls.items():
        assert np.array_equal(tail, ref), (R, hex(xm))
    for R in (7, 10):   # XM lands on output words 0 and 2 and nowhere else
        x = np.array([XM, 0, XM, 0], dtype=np.uint32)
        assert np.array_equal(calls[(R, XM)][1], calls[(R, 0)][1] ^ x)


def test_philox_tail_equals_philox_on_random_counters(check_exe):
    rng = np.random.default_rng(20240911)
    n = 1200
    ctr = rng.integers(0, 2 ** 32, size=(n, 4), dtype=np.uint64)
    # counter word 1 (the one the tail takes) at its corners, on random other words
    ctr[0:40, 1] = 0
    ctr[40:80, 1] = 1
    ctr[80:120, 1] = 0xFFFFFFFF
    # the rollout's counter map around the step's wraps, and the all-ones counter
    ctr[120] = [0xFFFFFFFF] * 4
    ctr[121] = [0xFFFFFFE0, 0xFFFFFFFF, 1 << 28, 0xFFFF0000]
    ctr[122] = [0x0000001F, 0x00000000, 2 << 28, 0x00010001]
    rows = [(*c, s & 0xFFFFFFFF, s >> 32) for s in SEEDS for c in ctr]
    rows += [(*c, *k) for c, k in zip(rng.integers(0, 2 ** 32, size=(n, 4), dtype=np.uint64),
                                      rng.integers(0, 2 ** 32, size=(n, 2), dtype=np.uint64))]
    rows.append((0, 0, 0, 0, 0, 0))   # the zero counter and key
    for c1 in (0, 1, 0xFFFFFFFF):
        rows.append((0, c1, 0, 0, 0, 0))
    calls, _ = run(check_exe, rows)
    assert_all_equal(calls)
    for i in range(0, len(rows), 97):   # and the C oracle's Philox, an implementation of its own
        c, k = rows[i][:4], rows[i][4:]
        assert list(oracle.philox(c, k, 7)) == list(calls[(7, 0)][0][i])
        assert list(oracle.philox(c, k, 10)) == list(calls[(10, 0)][0][i])


def test_philox_tail_known_answers(check_exe):
    with open(GOLDEN) as f:
        cases = json.load(f)["cases"]
    calls, _ = run(check_exe, [(*c["ctr"], *c["key"]) for c in cases])
    assert_all_equal(calls)
    for i, c in enumerate(cases):   # rocRAND's philox4x32_10 and Random123's 10-round vectors
        assert list(calls[(10, 0)][0][i]) == c["out"]
    for i, want in enumerate(R123_KAT7):
        assert list(calls[(7, 0)][0][i]) == want


def test_prefixes_differing_in_c2_share_b_and_d(check_exe):
    """The selection wave holds one (B, D) per lane for its four calls (counter word 2 =
    SEL << 28 | 4 * node + c, c = 0..3) and one (A, E, d3) per call."""
    rng = np.random.default_rng(5)
    rows, groups = [], 200
    for g in range(groups):
        c0, c1, c3, k0, k1 = (int(x) for x in rng.integers(0, 2 ** 32, size=5, dtype=np.uint64))
        base = 4 * (g % 32) if g % 2 == 0 else int(rng.integers(0, 2 ** 32 - 4))
        rows += [(c0, c1, base + c, c3, k0, k1) for c in range(4)]
    calls, pre = run(check_exe, rows)
    assert_all_equal(calls)
    for R in (7, 10):
        p = pre[R].reshape(groups, 4, 5)
        assert np.array_equal(p[:, :, 1], np.repeat(p[:, :1, 1], 4, axis=1)), "B"
        assert np.array_equal(p[:, :, 2], np.repeat(p[:, :1, 2], 4, axis=1)), "D"
        # (and the per-call words do differ: the check above is not vacuous)
        assert (p[:, 0, 0] != p[:, 1, 0]).any() and (p[:, 0, 3] != p[:, 1, 3]).any()
