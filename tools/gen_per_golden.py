"""Generate tests/golden/per_trace.npz: the reference's own ``PrioritisedER``
(bdq_model/memory.py:73-186 over bdq_model/data_structures.py) driven through recorded traces of
store, sample and update_priorities -- the pin of DESIGN.md "Prioritised replay".

  python tools/gen_per_golden.py       (build container only: reads /root/reference)

The reference package cannot be imported (its __init__ imports the absent gym), so memory.py and
data_structures.py are loaded by path under a stand-in package (as tools/gen_update_golden.py
loads network.py).  ``random.random`` is wrapped inside the loaded module: every uniform a sample
draws is recorded, so a restatement can be fed the same ones.

A trace of shape (capacity, n, B) is ``rounds`` rounds of: n single stores; sample(B, beta); then
update_priorities on the sampled indices with positions 3 and 7 forced to the index of position 1
(duplicates: the last pair wins) and random float32 priorities in (0, 4), passed as the reference's
caller passes them (``.tolist()`` of a float32 tensor: widened Python floats).  beta starts at 0.4
and moves by min(1, beta + 0.05) per round.  Shapes: (1000, 40, 32) over 30 rounds, (1024, 64, 256)
over 20 and (100, 70, 32) over 6; every ring wraps.

Stored per trace <t>: <t>.meta = (capacity, n, B, rounds, snap_every), <t>.alpha, <t>.betas
[rounds], <t>.u [rounds][B] (the uniforms), <t>.idx [rounds][B], <t>.w float32 [rounds][B],
<t>.upd_idx [rounds][B], <t>.upd_p float32 [rounds][B]; after each of a round's three operations
<t>.roots [rounds][3][2] (sum root, min root) and <t>.maxp [rounds][3]; and after every
snap_every-th round both trees' leaves, <t>.sum_leaves / <t>.min_leaves [snaps][T].
"""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "per_trace.npz")
ALPHA = 0.6
TRACES = {"c1000": (1000, 40, 32, 30, 5), "c1024": (1024, 64, 256, 20, 4), "c100": (100, 70, 32, 6, 1)}


def ref_memory_module():
    pkg = types.ModuleType("ref_bdq_model")
    pkg.__path__ = [os.path.join(REF, "bdq_model")]      # a stand-in package: no __init__ runs
    sys.modules["ref_bdq_model"] = pkg
    return importlib.import_module("ref_bdq_model.memory")


class RecordingRandom:
    """Stands in for the ``random`` module inside the reference's memory.py."""

    def __init__(self, seed):
        import random
        self._r = random.Random(seed)
        self.drawn = []

    def random(self):
        u = self._r.random()
        self.drawn.append(u)
        return u

    def sample(self, population, k):
        return self._r.sample(population, k)


def trace(mem, name, capacity, n, B, rounds, snap_every, out):
    rec = RecordingRandom(capacity)
    mem.random = rec
    rng = np.random.default_rng(capacity + 7)
    per = mem.PrioritisedER(capacity, ALPHA)
    T = per.sum_helper_buffer.size
    beta = 0.4
    keep = {k: [] for k in ("betas", "u", "idx", "w", "upd_idx", "upd_p", "roots", "maxp", "sum_leaves", "min_leaves")}
    stored = 0

    def state():
        return ([per.sum_helper_buffer.data[1], per.weight_helper_buffer.data[1]], per.max_priority)

    for r in range(rounds):
        roots, maxp = [], []
        for _ in range(n):
            per.store(mem.Transition(stored, 0, 0, 0.0, stored, False))
            stored += 1
        s = state()
        roots.append(s[0]); maxp.append(s[1])
        rec.drawn = []
        _, indices, weights = per.sample(B, beta)
        assert weights.dtype == np.float32 and len(rec.drawn) == B
        s = state()
        roots.append(s[0]); maxp.append(s[1])
        upd_idx = np.array(indices, dtype=np.int64)
        upd_idx[3] = upd_idx[7] = upd_idx[1]
        upd_p = (rng.random(B) * 4 + 1e-3).astype(np.float32)
        if r == 2:
            upd_p[5] = np.float32(9.5)      # max_priority grows past the priorities' range
            upd_p[3] = np.float32(12.25)    # ... through a duplicate that loses, too
        per.update_priorities([int(i) for i in upd_idx], upd_p.tolist())
        s = state()
        roots.append(s[0]); maxp.append(s[1])
        keep["betas"].append(beta)
        keep["u"].append(list(rec.drawn))
        keep["idx"].append(list(indices))
        keep["w"].append(weights)
        keep["upd_idx"].append(upd_idx)
        keep["upd_p"].append(upd_p)
        keep["roots"].append(roots)
        keep["maxp"].append(maxp)
        if (r + 1) % snap_every == 0:
            keep["sum_leaves"].append(per.sum_helper_buffer.data[T:])
            keep["min_leaves"].append(per.weight_helper_buffer.data[T:])
        beta = min(1.0, beta + 0.05)
    out[name + ".meta"] = np.array([capacity, n, B, rounds, snap_every], dtype=np.int64)
    out[name + ".alpha"] = np.float64(ALPHA)
    for k, v in keep.items():
        dt = {"idx": np.int64, "upd_idx": np.int64, "w": np.float32, "upd_p": np.float32}.get(k, np.float64)
        out[f"{name}.{k}"] = np.array(v, dtype=dt)


def main():
    mem = ref_memory_module()
    out = {}
    for name, shape in TRACES.items():
        trace(mem, name, *shape, out)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
