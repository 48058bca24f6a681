"""philox_rk (csrc/philox.h: Philox4x32-R with the round keys given, built once by
philox_round_keys) against philox, the C oracle and the known answers, on the host.

The rollout kernel's RNG waves build the key schedule once per launch and call philox_rk every
step; it has to be the function philox is, for every seed: the round keys are k + r * Weyl
constant modulo 2^32, and the three seeds here (small halves, all-ones halves, two large halves)
wrap at different rounds.  philox.h has
no host binding (the oracle has its own Philox), so a small program of its own is compiled with
hipcc, host side only."""
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
# Random123 kat_vectors, philox4x32 R = 7, on the inputs of the golden file's cases 0..2
# (tests/test_philox.py pins the same words on the oracles)
R123_KAT7 = [[0x5F6FB709, 0x0D893F64, 0x4F121F81, 0x4F730A48],
             [0x5207DDC2, 0x45165E59, 0x4D8EE751, 0x8C52F662],
             [0x4DFCCABA, 0x190A87F0, 0xC47362BA, 0xB6B5242A]]


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.fail("hipcc not found: philox.h needs the HIP headers")
    exe = tmp_path_factory.mktemp("philox_rk") / "philox_rk_check"
    subprocess.run(["hipcc", "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                    "-o", str(exe), os.path.join(HERE, "philox_rk_check.cpp")], check=True)
    return str(exe)


def run(exe, rows):
    """rows of (c0, c1, c2, c3, k0, k1) -> (rk7, ref7, rk10, ref10), each [len(rows)][4]."""
    text = "".join(" ".join("%x" % int(x) for x in r) + "\n" for r in rows)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    words = np.array([[int(w, 16) for w in ln.split()] for ln in out if ln.strip()], dtype=np.uint32)
    assert words.shape == (len(rows), 16)
    return words[:, 0:4], words[:, 4:8], words[:, 8:12], words[:, 12:16]


def test_philox_rk_equals_philox_on_random_counters(check_exe):
    rng = np.random.default_rng(20240607)
    ctr = rng.integers(0, 2 ** 32, size=(64, 4), dtype=np.uint64)
    # the corners of the rollout's counter map beside the random ones: step words around their
    # wraps, all-ones and zero counters
    ctr[0] = [0, 0, 0, 0]
    ctr[1] = [0xFFFFFFFF] * 4
    ctr[2] = [0xFFFFFFE0, 0xFFFFFFFF, 1 << 28, 0xFFFF0000]
    ctr[3] = [0x0000001F, 0x00000000, 2 << 28, 0x00010001]
    rows = [(*c, s & 0xFFFFFFFF, s >> 32) for s in SEEDS for c in ctr]
    rk7, ref7, rk10, ref10 = run(check_exe, rows)
    assert np.array_equal(rk7, ref7)
    assert np.array_equal(rk10, ref10)
    for i in range(0, len(rows), 7):   # and the C oracle's Philox, an implementation of its own
        c, k = rows[i][:4], rows[i][4:]
        assert list(oracle.philox(c, k, 7)) == list(rk7[i])
        assert list(oracle.philox(c, k, 10)) == list(rk10[i])


def test_philox_rk_known_answers(check_exe):
    with open(GOLDEN) as f:
        cases = json.load(f)["cases"]
    rk7, ref7, rk10, ref10 = run(check_exe, [(*c["ctr"], *c["key"]) for c in cases])
    for i, c in enumerate(cases):   # rocRAND's philox4x32_10 and Random123's 10-round vectors
        assert list(rk10[i]) == c["out"]
        assert list(ref10[i]) == c["out"]
    for i, want in enumerate(R123_KAT7):
        assert list(rk7[i]) == want
        assert list(ref7[i]) == want
