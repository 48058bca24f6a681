"""csrc/step_law.h, the device statement of the per-env law, on the host against the Python oracle.

tests/step_law_check.cpp (compiled with hipcc, host side only) calls the helpers the step kernels
call -- the magic divides, the autoreset pair and start state, the random reset state, the
perturbation mask with its tail under both stream mappings, the step's outcome -- and this test
compares its lines with oracle/pyoracle.py (ext64, PyPBN.reset_draw, PyPBN.gap, PyPBN.step) and with
the flag definitions of include/pbn_env.h.  The magics are net_image.h's, as the kernels get them.
"""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import pyoracle
from pbn_rl_amd.attractors import load_attractors
from pbn_rl_amd.network import load_network
from pbn_rl_amd.spec import NO_TARGET, EnvSpec

from .synthetic import multi_state_spec

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "pbn_rl_amd", "csrc")
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.fail("hipcc not found: step_law.h needs the HIP headers")
    exe = tmp_path_factory.mktemp("step_law") / "step_law_check"
    subprocess.run(["hipcc", "-x", "hip", "--offload-host-only", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC,
                    "-o", str(exe), os.path.join(HERE, "step_law_check.cpp")], check=True)
    return str(exe)


def run(exe, lines):
    """One command per line -> the result lines' fields (without the command word)."""
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    rows = [ln.split() for ln in out.split("\n") if ln.strip()]
    assert len(rows) == len(lines) and all(r[0] == ln.split()[0] for r, ln in zip(rows, lines))
    return [r[1:] for r in rows]


def net_lines(spec):
    """The commands that describe spec's net to the program: sizes, attractor starts, CDF."""
    starts = [int(x) for x in spec.arrays["attractor_start"]] if spec.attractors else []
    return ["net %d %d %s" % (spec.n, len(spec.attractors), " ".join(map(str, starts))),
            "cdf " + " ".join(str(int(c)) for c in spec.arrays["perturb_cdf"])]


def specs():
    out = {name: EnvSpec(load_network(name), load_attractors(name)) for name in ("pbn7", "pbn28", "pbn70")}
    out["one_attractor"] = EnvSpec(load_network("pbn28"), load_attractors("pbn28")[:1])
    out["no_attractors"] = EnvSpec(load_network("pbn28"), None)
    out["multi_state"] = multi_state_spec()
    return out


def test_magic_divides_exhaustively(check_exe):
    """Every c < A(A-1) for A in 2..255 splits as integer division does; every c < (N+1)^3 gives
    divmod's three actions for eight N; actions_mask31 equals actions_from_draw<1> for N <= 31."""
    (n_pair, bad_pair, n_act, bad_act, n_m31, bad_m31), = [[int(x) for x in r] for r in run(check_exe, ["div"])]
    assert n_pair == sum(A * (A - 1) for A in range(2, 256)) and bad_pair == 0
    assert n_act == sum((N + 1) ** 3 for N in (1, 7, 28, 31, 32, 70, 127, 128)) and bad_act == 0
    assert n_m31 == sum((N + 1) ** 3 for N in (1, 7, 28, 31)) and bad_m31 == 0


@pytest.mark.parametrize("name", ["pbn7", "pbn28", "pbn70", "one_attractor", "no_attractors", "multi_state"])
def test_pair_draw_start_pick_and_u2(check_exe, name):
    spec = specs()[name]
    py = pyoracle.PyPBN(spec)
    A, n1 = len(spec.attractors), spec.n + 1
    rng = np.random.default_rng(1000 + spec.n + A)
    xs = [int(x) for x in rng.integers(0, 1 << 64, size=1000, dtype=np.uint64)]
    xs[:3] = [0, M64, 1 << 63]
    res = run(check_exe, net_lines(spec) + ["draw %d %d" % (x >> 32, x & 0xFFFFFFFF) for x in xs])
    n1_magic, am1_magic, x_mult, att_single = (int(v) for v in res[0])
    # net_image.h's magics: ceil(2^32 / d), and the product of the draws' ranges
    assert n1_magic == -(-(1 << 32) // n1)
    assert am1_magic == (-(-(1 << 32) // (A - 1)) if A >= 3 else 0)
    assert x_mult == n1 ** 3 * (A * (A - 1) if A >= 2 else 1)
    assert att_single == int(A >= 1 and all(len(a) == 1 for a in spec.attractors))
    flat = [s for att in spec.attractors for s in att]
    for x, r in zip(xs, res[2:]):
        c_act, a_s, rt, row, top, xr_top = (int(v) for v in r)
        c, rest = pyoracle.ext64(x, n1 ** 3)
        assert c_act == c
        size = 1
        if A:
            if A >= 2:
                pair, _ = pyoracle.ext64(rest, A * (A - 1))
                assert a_s == pair // (A - 1)
            else:
                assert a_s == 0
            state, tgt, rest = py.reset_draw(rest)
            assert rt == tgt and list(flat[row]) == state and tuple(state) in spec.attractors[a_s]
            size = len(spec.attractors[a_s])
        # what the draws leave of X, two ways: down the chain, and as the one product the fast
        # paths take off it
        assert top == rest >> 32 == xr_top == ((x * x_mult * size) & M64) >> 32


def test_random_reset_state(check_exe):
    for name in ("pbn7", "pbn70"):
        spec = EnvSpec(load_network(name), None)
        py = pyoracle.PyPBN(spec)
        seed, e, step = 0xC3A5C85C97CB3127, (5 << 32) | 77, (3 << 32) | 12
        c3 = ((e >> 32) & 0xFFFF) | (((step >> 32) & 0xFFFF) << 16)
        res = run(check_exe, net_lines(spec)[:1] + ["rst %d %d %d %d %d" % (e & 0xFFFFFFFF, step & 0xFFFFFFFF, c3,
                                                                           seed & 0xFFFFFFFF, seed >> 32)])
        state, tgt = py.random_state(seed, e, step)
        assert [int(w, 16) for w in res[1][:4]] == (spec.network.pack(state) + [0] * 4)[:4]
        assert int(res[1][4]) == tgt == NO_TARGET


class GapLog(pyoracle.PyPBN):
    """PyPBN that records the gaps its step draws, in order."""

    def __init__(self, spec):
        super().__init__(spec)
        self.gaps = []

    def gap(self, u):
        g = super().gap(u)
        self.gaps.append(g)
        return g


def masks_from_gaps(gaps, n):
    """The gap sequence of one PyPBN.step, split into its updates' flip masks (packed words,
    gap counts): an update's gaps end with the first position at or past the last node."""
    out, pos, mask, cnt = [], -1, 0, 0
    for g in gaps:
        pos += g
        cnt += 1
        if pos < n:
            mask |= 1 << pos
        if pos >= n - 1:
            out.append(([(mask >> (32 * w)) & 0xFFFFFFFF for w in range(4)], cnt))
            pos, mask, cnt = -1, 0, 0
    assert cnt == 0
    return out


@pytest.mark.parametrize("name,p,attractors", [("pbn28", 0.3, False), ("pbn70", 0.12, False), ("pbn28", 0.3, True),
                                               ("pbn7", 0.6, True)])
def test_perturbation_mask_with_tail(check_exe, name, p, attractors):
    """The mask of the three first gaps and the tail equals the mask PyPBN.step applies: update 0
    under the PERT mapping, updates 1 and 2 under the SETTLE_ENV mapping (a net without
    attractors never settles, so the settle law runs all three)."""
    net = load_network(name)
    spec = EnvSpec(net, load_attractors(name) if attractors else None, perturbation=p,
                   settle=0 if attractors else 3)
    seed = 977
    cases = [(e, step) for e in ((1 << 33) + 5, 64, 65) for step in range(8)]
    lines, want = net_lines(spec), []
    for e, step in cases:
        py = GapLog(spec)
        py.step(seed, step, e, [0] * spec.n, [0] * spec.n, 0, 0, 0)
        per_update = masks_from_gaps(py.gaps, spec.n)
        assert len(per_update) == (1 if attractors else 3)
        c3 = ((e >> 32) & 0xFFFF) | (((step >> 32) & 0xFFFF) << 16)
        for k, w in enumerate(per_update):
            lines.append("pert %d %d %d %d %d %d" % (k, e & 0xFFFFFFFF, step & 0xFFFFFFFF, c3, seed & 0xFFFFFFFF,
                                                     seed >> 32))
            want.append((k,) + w)
    res = run(check_exe, lines)[2:]
    second_call = {0: 0, 1: 0}   # cases whose tail went on to a second Philox call, by mapping
    more_than_three = 0
    for (k, mask, n_gaps), r in zip(want, res):
        assert [int(w, 16) for w in r[:4]] == mask, (k, r)
        assert int(r[4]) == max(n_gaps, 3)      # (the kernels always compute the three first gaps)
        assert r[6] == "1" and r[7] == "1"      # the one-word form; settle_updates' whole-update tail
        n_calls = int(r[5])
        # PERT: the tail's words 0-3 are call 0's, word 4 (gap 7) call 1's; SETTLE_ENV: the tail
        # starts at word 3 of the update's first call, word 4 (gap 4) is call 1's
        assert n_calls == (0 if n_gaps <= 3 else (-(-(n_gaps - 3) // 4) if k == 0 else (n_gaps - 1) // 4))
        more_than_three += n_gaps > 4              # a fourth flip, or the gap that ends after three
        second_call[min(k, 1)] += n_calls >= (2 if k == 0 else 1) and n_gaps >= (8 if k == 0 else 5)
    assert more_than_three >= len(want) // 3      # the tail is common at these p, not a rare arm
    if name != "pbn7":   # (seven nodes: at most eight gaps)
        assert second_call[0] > 0
    if not attractors:
        assert second_call[1] > 0


def test_step_outcome_table(check_exe):
    """Every combination of the outcome's inputs against the flag bits of include/pbn_env.h:
    TERMINATED 1, TRUNCATED 2, IN_ATTRACTOR 4, PERTURBED 8, RESET 16, UNSETTLED 32; t saturates
    at 255 and is 0 after an autoreset; the reward row is {none, wrong, term}."""
    target, other = 3, 5
    combos = []
    for horizon in (0, 20):
        ts = sorted({0, max(horizon - 2, 0), max(horizon - 1, 0), 254, 255})
        combos += list(itertools.product((-1, target, other), ts, (horizon,), (0, 1), (0, 1), (0, 1)))
    res = run(check_exe, ["out %d %d %d %d %d %d %d" % (att, target, t, h, ar, pt, op)
                          for att, t, h, ar, pt, op in combos])
    for (att, t, h, ar, pt, op), r in zip(combos, res):
        flags, t_new, term, wrong, trunc, reset, pick = (int(v) for v in r)
        w_term, w_in = att == target, att >= 0
        w_t = min(t + 1, 255)
        w_trunc = h > 0 and w_t >= h
        w_reset = bool(ar) and (w_term or w_trunc)
        assert flags == (1 * w_term | 2 * w_trunc | 4 * w_in | 8 * pt | 16 * w_reset | 32 * op), (att, t, h, ar)
        assert t_new == (0 if w_reset else w_t)
        assert (term, wrong, trunc, reset) == (w_term, w_in and not w_term, w_trunc, w_reset)
        assert pick == (2 if w_term else (1 if w_in else 0))
