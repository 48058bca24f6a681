"""The bounded draws of csrc/step_law.h on the host: two divisions for the three action digits,
and gap 2's uniform taken from the running X.

tests/bounded_draws_check.cpp (compiled with hipcc, host side only) calls the helpers with the
magics net_image.h gives the kernels and compares them with the three-division forms they
replaced, restated in the program, and with integer division:
  - actions_mask31 for every n1 in 2..32 and every c < n1^3;
  - actions_from_draw<W> for W = 2, 3, 4 (and 1 at N = 32) at N = 32, 33, 64, 96, 128, every c;
  - pair_start / pair_target / pair_draw for A = 2, 3, 255 and every c < A(A-1);
  - the running X's top word after the two draws against hi32(X * x_mult) for five edge values and
    10^4 seeded ones at (n1, A) = (2, 2), (29, 14), (32, 255).
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
    exe = tmp_path_factory.mktemp("bounded_draws") / "bounded_draws_check"
    subprocess.run(["hipcc", "-x", "hip", "--offload-host-only", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC,
                    "-o", str(exe), os.path.join(HERE, "bounded_draws_check.cpp")], check=True)
    out = subprocess.run([str(exe), "1"], capture_output=True, text=True, check=True).stdout   # stride 1: every c
    return {r[0]: [int(x) for x in r[1:]] for r in (ln.split() for ln in out.splitlines() if ln.strip())}


def test_actions_mask31_equals_the_three_division_form(lines):
    n, bad = lines["mask31"]
    assert n == sum(n1 ** 3 for n1 in range(2, 33))
    assert bad == 0


def test_actions_from_draw_every_word_count(lines):
    n, bad = lines["from_draw"]
    words = {32: (1, 2, 3, 4), 33: (2, 3, 4), 64: (2, 3, 4), 96: (3, 4), 128: (4,)}
    assert n == sum(len(ws) * ((N + 1) ** 3 + N + 1) for N, ws in words.items())   # every c, the last n1 twice
    assert bad == 0


def test_pair_halves_and_the_no_divide_arm(lines):
    n, bad = lines["pairs"]
    assert n == sum(A * (A - 1) for A in (2, 3, 255))
    assert bad == 0


def test_gap2_uniform_is_the_running_x(lines):
    n, bad = lines["u2"]
    assert n == 3 * 10005 and bad == 0
