"""Numpy restatement of the prioritised replay law (DESIGN.md "Prioritised replay"; the reference's
PrioritisedER, bdq_model/memory.py:73-186, over bdq_model/data_structures.py's segment trees).

TEST INFRASTRUCTURE ONLY.  Two trees over T leaves (T the smallest power of two >= capacity) as
float64 arrays of 2T nodes: node 1 is the root, leaf i is node T + i, a sum node is left + right, a
min node is min(left, right); empty leaves are 0.0 / +inf.  Every ancestor equals the operation of
its two children, so ``rebuild`` recomputes the trees from their leaves level by level (vectorised
slices) and the order of leaf writes never matters.  The uniforms of a sample are passed in: the
golden traces carry the reference's ``random.random()`` values, the GPU tests the REPLAY Philox
stream's (``replay_uniforms``).

Scalar powers are Python's ``**`` (the reference's ``max_priority ** alpha`` and ``priority **
alpha`` are Python floats); the sample's numerator is numpy's array power and its denominator a
Python one, as memory.py:159-161 has them.
"""
from __future__ import annotations

import numpy as np

from oracle import pyoracle

REPLAY = 7   # csrc/philox.h kStreamReplay


def replay_uniforms(seed: int, counter: int, batch: int) -> np.ndarray:
    """u_i = ((x << 21) | (y >> 11)) * 2^-53 from the REPLAY Philox words (x, y) of (seed, id = i,
    step = counter): what pbn_per_sample draws."""
    out = np.empty(batch, dtype=np.float64)
    for i in range(batch):
        x, y, _, _ = pyoracle.draw(seed, i, counter, REPLAY, 0)
        out[i] = float((x << 21) | (y >> 11)) * 2.0 ** -53
    return out


class PerOracle:
    def __init__(self, capacity: int, alpha: float = 0.6):
        self.capacity = int(capacity)
        self.alpha = float(alpha)
        T = 1
        while T < capacity:
            T *= 2
        self.T = T
        self.clear()

    def clear(self) -> None:
        self.sum = np.zeros(2 * self.T, dtype=np.float64)
        self.min = np.full(2 * self.T, np.inf, dtype=np.float64)
        self.max_priority = 1.0
        self.pos = 0
        self.size = 0

    # ---- trees
    def rebuild(self) -> None:
        w = self.T // 2
        while w >= 1:
            self.sum[w:2 * w] = self.sum[2 * w:4 * w:2] + self.sum[2 * w + 1:4 * w:2]
            self.min[w:2 * w] = np.minimum(self.min[2 * w:4 * w:2], self.min[2 * w + 1:4 * w:2])
            w //= 2

    def sum_leaves(self) -> np.ndarray:
        return self.sum[self.T:]

    def min_leaves(self) -> np.ndarray:
        return self.min[self.T:]

    def adopt_leaves(self, sum_leaves, min_leaves) -> None:
        """Take over leaves computed elsewhere (the device's ``p ** alpha``, equal to this
        restatement's to a few ulp) and rebuild: the internal nodes of both sides can then be
        compared bit for bit."""
        self.sum[self.T:] = np.asarray(sum_leaves, dtype=np.float64)
        self.min[self.T:] = np.asarray(min_leaves, dtype=np.float64)
        self.rebuild()

    # ---- the three operations
    def store(self, n: int) -> np.ndarray:
        """n transitions at ring position pos: max_priority ** alpha at the slot AFTER each stored
        row (memory.py:114).  Returns the written leaves."""
        v = self.max_priority ** self.alpha
        leaves = (self.pos + 1 + np.arange(n, dtype=np.int64)) % self.capacity
        self.sum[self.T + leaves] = v
        self.min[self.T + leaves] = v
        self.pos = (self.pos + n) % self.capacity
        self.size = min(self.size + n, self.capacity)
        self.rebuild()
        return leaves

    def prefix_terms(self) -> list:
        """The subtree totals whose sum is p_total, top down (t_1 .. t_m; [] below two rows)."""
        rem, w, node, t = self.size - 1, self.T, 1, []
        if rem < 1:
            return t
        while True:
            if rem == w:
                t.append(float(self.sum[node]))
                break
            w //= 2
            if rem <= w:
                node = 2 * node
            else:
                t.append(float(self.sum[2 * node]))
                node = 2 * node + 1
                rem -= w
        return t

    def p_total(self) -> float:
        """sum(0, size - 1) of memory.py:123: leaves [0, size - 2] (reduce's end -= 1), in the
        association of _reduce (data_structures.py:33-60): the left-sibling totals collected top
        down, added as t_1 + (t_2 + (... + t_m))."""
        t = self.prefix_terms()
        if not t:
            return 0.0
        p = t[-1]
        for x in reversed(t[:-1]):
            p = x + p
        return p

    def sample(self, batch: int, beta: float, uniforms):
        """(indices int64 [batch], weights float32 [batch])."""
        N = self.size
        u = np.asarray(uniforms, dtype=np.float64)
        r = self.p_total() / batch
        mass = u * r + np.arange(batch, dtype=np.float64) * r      # two rounded products, one sum
        node = np.ones(batch, dtype=np.int64)
        w = 1
        while w < self.T:                                           # find_prefixsum_index
            left = self.sum[2 * node]
            go_left = left > mass
            mass = np.where(go_left, mass, mass - left)
            node = np.where(go_left, 2 * node, 2 * node + 1)
            w *= 2
        idx = np.clip(node - self.T, 0, max(N - 1, 0))
        S = float(self.sum[1])
        prob = self.sum[self.T + idx] / S
        max_weight = (N * (float(self.min[1]) / S)) ** (-beta)
        weights = ((N * prob) ** (-beta)) / max_weight
        return idx, weights.astype(np.float32)

    def update(self, idx, priorities) -> np.ndarray:
        """The pairs in order (of equal indices the last wins); pairs with an index outside
        [0, size) are skipped.  Returns the mask of applied pairs."""
        idx = np.asarray(idx, dtype=np.int64)
        p = np.asarray(priorities, dtype=np.float32)
        ok = (idx >= 0) & (idx < self.size)
        for i, x in zip(idx[ok].tolist(), p[ok].tolist()):         # fp32 widened to Python floats
            leaf = x ** self.alpha
            self.sum[self.T + i] = leaf
            self.min[self.T + i] = leaf
            self.max_priority = max(self.max_priority, x)
        self.rebuild()
        return ok


def ulp_distance(a, b) -> np.ndarray:
    """Distance in units of the last place between finite float64 (or float32) arrays of equal sign."""
    a, b = np.asarray(a), np.asarray(b)
    it = np.int64 if a.dtype == np.float64 else np.int32
    return np.abs(a.view(it).astype(np.int64) - b.view(it).astype(np.int64))
