"""The curriculum reset law (DESIGN.md "Curriculum resets", csrc/curriculum_law.h) restated with Python
ints and numpy.  TEST INFRASTRUCTURE ONLY.

``build_table`` is the table of a ``pairs`` array, ``draw_from_words`` one restart from a Philox call's
four words, ``redraw`` one frame's restarts of a batch, and ``Trajectory`` the whole loop -- redraw,
episode statistics (tests/episode_stats_reference.py), refresh -- over per-frame flags and rewards.
The Philox call is oracle/pyoracle.py's ``draw``.
"""
import math

import numpy as np

from oracle import pyoracle
from tests import episode_stats_reference as E

CURRICULUM = 8                 # the Philox stream
CAP = 2 ** 24 - 1
SHIFT = 8
RESET = 16                     # PBN_FLAG_RESET
M64 = (1 << 64) - 1


def horizon_of(spec) -> int:
    return int(spec.horizon or 20)


def int_weights(pairs, H: int):
    """w[s][t] as Python ints (lists): 0 on the diagonal, else min(((H + L) << 8) // (1 + E), CAP)."""
    A = len(pairs)
    return [[0 if s == t else min(((H + int(pairs[s][t][2])) << SHIFT) // (1 + int(pairs[s][t][0])), CAP)
             for t in range(A)] for s in range(A)]


def build_table(pairs, H: int, refreshes: int = 0) -> dict:
    """rowcdf uint64 [A], cdf uint32 [A][A], total, refreshes, and w (int64 [A][A]) of ``pairs``
    ([A][A][4]: episodes, missed, len_sum, ret_sum; ints of any size)."""
    w = int_weights(pairs, H)
    A = len(w)
    cdf, rowcdf, total = [], [], 0
    for s in range(A):
        acc, row = 0, []
        for t in range(A):
            acc += w[s][t]
            row.append(acc)
        assert acc < 1 << 32
        cdf.append(row)
        total += acc
        rowcdf.append(total)
    assert total < 1 << 40
    return {"rowcdf": np.array(rowcdf, dtype=np.uint64), "cdf": np.array(cdf, dtype=np.uint32), "total": total,
            "refreshes": refreshes, "w": np.array(w, dtype=np.int64)}


def weights(table) -> np.ndarray:
    """(A, A) float64: w / total."""
    return table["w"].astype(np.float64) / float(table["total"])


def float_rule(pairs, H: int, capped: bool = False) -> np.ndarray:
    """EpisodeStats.pair_weights' float formula on ``pairs`` (``capped``: a weight above the table's
    cap, CAP / 2^8, takes the cap)."""
    p = np.asarray(pairs)
    w = (float(H) + p[..., 2].astype(np.float64)) / (1.0 + p[..., 0])
    if capped:
        w = np.minimum(w, CAP / 2.0 ** SHIFT)
    np.fill_diagonal(w, 0.0)
    return w / w.sum()


def draw_from_words(table, x, att_start):
    """(s, t, row) of the restart drawn from the four words ``x``."""
    rowcdf, cdf, total = table["rowcdf"], table["cdf"], table["total"]
    A = len(rowcdf)
    v = ((((x[1] << 32) | x[0]) * total) >> 64)
    s = next(i for i in range(A) if int(rowcdf[i]) > v)
    v -= int(rowcdf[s - 1]) if s else 0
    t = next(j for j in range(A) if int(cdf[s][j]) > v)
    assert t != s
    size = int(att_start[s + 1]) - int(att_start[s])
    return s, t, int(att_start[s]) + ((((x[3] << 32) | x[2]) * size) >> 64)


def x_for(v: int, total: int):
    """The smallest 64-bit X with floor(X total / 2^64) == v, as (x0, x1)."""
    X = -(-(v << 64) // total)
    assert X <= M64 and (X * total) >> 64 == v
    return X & 0xFFFFFFFF, X >> 32


def redraw(table, spec, seed: int, env_offset: int, step: int, flags, state, target):
    """One frame's restarts: copies of ``state`` (uint32 [W][n]) and ``target`` (uint8 [n]) with the
    envs whose flag has RESET overwritten, and the list of (env, s, t, row)."""
    W = spec.words
    att_start = [int(a) for a in spec.arrays["attractor_start"]]
    rows = np.asarray(spec.arrays["attractor_states"], dtype=np.uint32).reshape(-1, W)
    state, target, picks = np.array(state, dtype=np.uint32), np.array(target, dtype=np.uint8), []
    for i in np.nonzero(np.asarray(flags) & RESET)[0]:
        i = int(i)
        s, t, row = draw_from_words(table, pyoracle.draw(seed, env_offset + i, step, CURRICULUM, 0), att_start)
        state[:, i] = rows[row]
        target[i] = t
        picks.append((i, s, t, row))
    return state, target, picks


class Trajectory:
    """The reference of a learner's frames with the curriculum on: ``frame(step, reward, flags,
    state_after)`` is one frame -- ``state_after`` is what the step left (the restarts it drew itself are
    overwritten here) -- and ``state``, ``target``, ``stats`` (episode_stats_reference's dict) and
    ``table`` then hold what the device must hold."""

    def __init__(self, spec, seed, env_offset, state0, target0, refresh_every, log_every=0, series_rows=1024):
        self.spec, self.seed, self.env_offset = spec, seed, env_offset
        self.H, self.A = horizon_of(spec), len(spec.attractors)
        self.refresh_every, self.log_every, self.series_rows = refresh_every, log_every, series_rows
        self.state0, self.target0 = np.array(state0, dtype=np.uint32), np.array(target0, dtype=np.uint8)
        self.state, self.target = self.state0.copy(), self.target0.copy()
        self.frames, self.picks = [], []
        self.lookup = E.spec_attractor_id(spec)
        self.table = build_table(np.zeros((self.A, self.A, 4), dtype=np.int64), self.H, 1)   # the constructor's
        self.stats = None

    def frame(self, step, reward, flags, state_after):
        flags = np.asarray(flags)
        keep = (flags & RESET) == 0
        target_after = self.target.copy()             # a step changes the target of the envs it resets only
        self.state, self.target, picks = redraw(self.table, self.spec, self.seed, self.env_offset, step, flags,
                                                state_after, target_after)
        assert np.array_equal(self.state[:, keep], np.asarray(state_after, dtype=np.uint32)[:, keep])
        self.picks.append(picks)
        self.frames.append((np.asarray(reward, dtype=np.float32).copy(), flags.copy(), self.state.copy(),
                            self.target.copy()))
        self.stats = E.episode_stats(self.frames, self.state0, self.target0, self.lookup, self.A,
                                     log_every=self.log_every, series_rows=self.series_rows)
        if self.refresh_every > 0 and len(self.frames) % self.refresh_every == 0:
            self.table = build_table(self.stats["pairs"], self.H, self.table["refreshes"] + 1)


# ---------------------------------------------------------------- the pair matrices the host and GPU tests share
def dense_pairs(A: int, entries) -> np.ndarray:
    """int64 [A][A][4] that is zero but for ``entries``: (s, t, episodes, len_sum)."""
    pairs = np.zeros((A, A, 4), dtype=np.int64)
    for s, t, e, length in entries:
        pairs[s, t, 0], pairs[s, t, 2] = e, length
    return pairs


def _seeded_entries(A: int, count: int, seed: int):
    """``count`` distinct seeded entries, the diagonal included (its statistics must not count):
    1..60 episodes of mean length 1..40."""
    rng = np.random.default_rng(seed)
    cells = rng.choice(A * A, size=count, replace=False)
    out = []
    for c in cells:
        e = int(rng.integers(1, 61))
        out.append((int(c) // A, int(c) % A, e, e + int(rng.integers(0, 39 * e + 1))))
    return out


# name -> (A, H, entries)
PAIR_CASES = {
    "a2_zero": (2, 20, []),
    "a3_zero": (3, 5, []),
    "a14_zero": (14, 20, []),
    "a254_zero": (254, 20, []),
    "a2_seeded": (2, 4, _seeded_entries(2, 4, 41)),
    "a3_seeded": (3, 20, _seeded_entries(3, 7, 42)),
    "a14_seeded": (14, 20, _seeded_entries(14, 150, 43)),
    "a254_seeded": (254, 3, _seeded_entries(254, 9000, 44)),
    # no episode yet and a length sum that reaches the cap: ((20 + 65516) << 8) == 2^24
    "a3_cap": (3, 20, [(0, 1, 0, 65516), (2, 0, 0, 65515), (1, 1, 0, 99999)]),
    "a3_huge": (3, 20, [(1, 2, 5, 2 ** 55), (0, 2, 3, 9)]),
    "a254_all_cap": (254, 20, [(s, t, 0, 2 ** 55) for s in range(254) for t in range(254)]),
    # nearly all the weight on (1, 3), whose source is a 7-state attractor (sizes below)
    "a5_skewed": (5, 20, [(1, 3, 0, 60000), (0, 4, 2, 300), (2, 3, 9, 12), (4, 0, 1, 77), (3, 2, 3, 40)]),
}
SKEWED_SIZES = (1, 7, 2, 1, 3)      # a5_skewed's attractors, for the draws within an attractor


def chi2_sf(x: float, df: int) -> float:
    """P(chi-square with df degrees of freedom > x): the regularised upper incomplete gamma
    Q(df / 2, x / 2) by its finite sum (integer and half-integer first arguments)."""
    y = x / 2.0
    if df % 2 == 0:
        return math.exp(-y) * sum(y ** j / math.factorial(j) for j in range(df // 2))
    return math.erfc(math.sqrt(y)) + math.exp(-y) * sum(y ** (j - 0.5) / math.gamma(j + 0.5)
                                                        for j in range(1, (df - 1) // 2 + 1))
