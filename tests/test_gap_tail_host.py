"""The rare fourth-flip tail of the env-draw wave's fast loop on the host, under the address and
undefined-behaviour sanitizers.

tests/gap_tail_check.cpp (compiled with hipcc, host side only, -fsanitize=address,undefined, and
run as a program of its own) checks:
  - the PERT call's prefix (csrc/philox.h philox_prefix_sibling: A, E, d3 of its own, B and D of
    the ENV prefix) with philox_tail against the whole philox call for 20,000 seeded (c0, c3, key),
    the edge values of c0 and c3 among them, each at c1 = 0, 0xFFFFFFFF and two seeded words;
  - csrc/step_law.h gap_tail_split (the fourth gap in line, the rest behind a second branch;
    without its early no-flip test and with one) against pbn::gap_tail from every start position
    p2 in -1..N-1 at N = 7, 10, 28, 31, with word streams in which 0, 1, 4, 5 and 9 further gaps
    land and 50 seeded mixed ones per position: the same mask, nothing past the network, and the
    same PERT calls in the same order (calls 1 and 2 among them).
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "pbn_rl_amd", "csrc")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.fail("hipcc not found: step_law.h needs the HIP headers")
    exe = tmp_path_factory.mktemp("gap_tail") / "gap_tail_check"
    subprocess.run(["hipcc", "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                    "-o", str(exe), os.path.join(HERE, "gap_tail_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    return {row[0]: [int(x) for x in row[1:]] for row in (ln.split() for ln in r.stdout.splitlines() if ln.strip())}


def test_pert_prefix_equals_the_whole_call(lines):
    n, bad = lines["pert_prefix"]
    assert n == 20000 * 4 and bad == 0


def test_split_equals_gap_tail_from_every_position(lines):
    n, bad = lines["split"]
    assert n == sum((N + 1) * (5 + 50) for N in (7, 10, 28, 31))
    assert bad == 0


def test_split_cases_land_nine_gaps_and_cross_calls_1_and_2(lines):
    assert lines["split_landed_max"][0] >= 9
    assert lines["split_calls_1_and_2"][0] == 1
