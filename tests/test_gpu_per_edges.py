"""The priority-tree kernels (csrc/pbn_per.hip) at the tree sizes, ring wraps, fill levels and batch
sizes where they change path, by test_gpu_per.py's comparison method (its helpers, not copies): the
leaves within 16 fp64 ulp of the oracle's ``p ** alpha``, the oracle then adopting the device's
leaves, every internal node of both trees and max_priority bit for bit, sampled rows exact, weights
within 1 fp32 ulp, beta and the draw counter advanced.

  capacity  tree_size
         2          2   one level; the chunk is the two leaves
         3          4   the smallest tree with an empty leaf
       200        256   the chunk is the whole tree, below kChunk = 512: one block
       300        512   one chunk, no launch above the chunk roots, capacity < tree_size
       512        512   the same with capacity == tree_size
       513       1024   two chunk roots; chunk 1 holds one live leaf
      1500       2048   four chunk roots

Every store and sample runs on trees whose rows were all updated with strictly positive priorities
spread over six decades (a store writes max_priority ** alpha: on a varied tree a leaf it misses or
writes in excess differs from the oracle's).  tests/test_replay_edges_host.py checks the conditions
on the sample cases (tests/replay_edge_cases.py) from the oracle alone.

The seeded sample cases do not pin the association of p_total, although it differs from the
left-to-right sum in each of them: a p_total one ulp off moves a row only if a search mass lies
within an ulp of a node boundary, and a left-to-right prefix passed all of them.  One constructed
tree (replay_edge_cases.association_tree, written into the device trees) turns the association into
a sampled row."""
import numpy as np
import pytest
import torch

from tests import replay_edge_cases as C
from tests.test_gpu_per import check_trees, dev_sample, dev_store, dev_update, make

pytestmark = pytest.mark.gpu


def vary(rp, o, seed, what):
    """Every live row gets a new priority (batches of at most 1024 distinct rows)."""
    for idx, prio in C.varied_updates(o.size, seed):
        assert dev_update(rp, o, idx, prio).all()
    return check_trees(rp, o, what)


def edge_stores(cap):
    """(pos, n): one leaf with no wrap (leaf 0), the wrap of two leaves (capacity - 1 and 0: inside
    one chunk up to capacity 512; at 513 segment A is chunk 1 and segment B chunk 0), the whole ring
    from a mid-ring position (1500 from 699: segment B ends in segment A's first chunk), and at
    1500 a wrap both of whose segments end inside a chunk."""
    out = [(cap - 1, 1), (cap - 2, 2), (699 if cap == 1500 else cap // 2, cap)]
    if cap == 1500:
        out.append((1199, 600))
    return out


@pytest.mark.parametrize("cap", list(C.PER_CAPACITIES))
def test_store_at_every_tree_shape(cap):
    rp, o = make(cap)
    assert rp.tree_size == o.T == C.PER_CAPACITIES[cap]
    dev_store(rp, o, cap)
    assert check_trees(rp, o, f"{cap}: fill") == 0
    for k, (pos, n) in enumerate(edge_stores(cap)):
        d = vary(rp, o, 10 * cap + k, f"{cap}: update before store {k}")
        rp.pos = o.pos = pos
        before = rp.sum_tree.clone()
        dev_store(rp, o, n)
        d = max(d, check_trees(rp, o, f"{cap}: store n={n} at pos={pos}"))
        print(f"store cap={cap} pos={pos} n={n}: largest leaf distance {d} ulp")
        leaves = (pos + 1 + np.arange(n)) % cap
        hit = np.zeros(o.T, dtype=bool)
        hit[leaves] = True
        s = rp.sum_tree.cpu().numpy()[o.T:]
        assert len(np.unique(s[hit])) == 1                                 # one value, n leaves
        assert np.array_equal(s[~hit], before.cpu().numpy()[o.T:][~hit])   # no other leaf moved


@pytest.mark.parametrize("cap,size,seed,batches,kw", C.PER_SAMPLE_CASES)
def test_sample_at_every_fill_level(cap, size, seed, batches, kw):
    """The walk's exits (a leaf; an internal node where rem == w; no term at all below two rows)
    and batches of 1, 63, 64, 65 and 1024 rows; a partial fill passes the fill level as a device
    tensor, as a captured frame does."""
    rp, o = make(cap, **kw)
    dev_store(rp, o, size)
    vary(rp, o, seed, f"{cap}/{size}: update")
    size_t = torch.tensor([size], dtype=torch.int64, device=rp.device) if size < cap else None
    for B in batches:
        idx, _ = dev_sample(rp, o, B, size_t)
        if size == 2:
            assert not idx.any()
    assert int(rp.counter_t) == len(batches)
    if kw:
        assert float(rp.beta_t) == kw["max_beta"]


def test_sample_adds_the_prefix_in_the_references_association():
    """replay_edge_cases.association_tree written into the device trees: the row is 2 only if
    p_total is t_1 + (t_2 + t_3).  (The seeded cases above pin everything but this: their rows do
    not move when p_total is one ulp off.)"""
    ctr, ref = C.association_oracle()
    rp, o = make(8)
    o.size, o.sum, o.min = ref.size, ref.sum, ref.min
    rp.size = 8
    rp.sum_tree.copy_(torch.from_numpy(o.sum))
    rp.min_tree.copy_(torch.from_numpy(o.min))
    rp.counter_t.fill_(ctr)
    check_trees(rp, o, "association tree")
    idx, _ = dev_sample(rp, o, 1)
    assert idx.tolist() == [2] and int(rp.counter_t) == ctr + 1


def test_update_one_pair():
    rp, o = make(300)
    dev_store(rp, o, 300)
    vary(rp, o, 1, "300: update")
    for row, p in ((0, 2.5e-3), (299, 7.0e3), (150, 1.0)):
        ok = dev_update(rp, o, np.array([row], dtype=np.int64), np.array([p], dtype=np.float32))
        assert ok.all()
        check_trees(rp, o, f"B = 1, row {row}")
    assert o.max_priority == float(np.float32(7.0e3))


def test_update_1024_pairs_of_one_row():
    """All 1024 pairs name the same row: position 1023 wins the leaf, and max_priority sees the
    largest of all 1024 priorities (which stands elsewhere)."""
    rp, o = make(1500)
    dev_store(rp, o, 1500)
    vary(rp, o, 2, "1500: update")              # (its first batch: 1024 distinct rows)
    rng = np.random.default_rng(4)
    prio = C.six_decades(rng, 1024)
    prio[517] = np.float32(4321.0)
    prio[1023] = np.float32(0.037)
    dev_update(rp, o, np.full(1024, 777, dtype=np.int64), prio)
    check_trees(rp, o, "B = 1024, one row")
    assert o.max_priority == 4321.0 == float(rp.max_priority)
    want = float(np.float32(0.037)) ** C.ALPHA
    assert abs(float(rp.sum_tree[o.T + 777]) / want - 1) < 1e-14


def test_update_around_the_fill_level():
    """size < capacity: row size - 1 is applied; rows size and -1 are skipped, leaf and
    max_priority alike."""
    rp, o = make(513)
    dev_store(rp, o, 400)
    vary(rp, o, 3, "513/400: update")
    top = o.max_priority
    idx = np.array([399, 400, -1, 0], dtype=np.int64)
    prio = np.array([0.5, 1e6, 1e6, 0.25], dtype=np.float32)
    ok = dev_update(rp, o, idx, prio)
    assert ok.tolist() == [True, False, False, True]
    check_trees(rp, o, "rows size - 1, size, -1")
    assert o.max_priority == top < 1e6
    assert float(rp.sum_tree[o.T + 400]) == 1.0          # (the store's leaf after the last row)


def test_update_64_pairs_on_a_one_level_tree():
    rp, o = make(2)
    dev_store(rp, o, 2)
    rng = np.random.default_rng(6)
    for r in range(3):
        idx = rng.integers(0, 2, size=64).astype(np.int64)
        dev_update(rp, o, idx, C.six_decades(rng, 64))
        check_trees(rp, o, f"capacity 2, round {r}")
    dev_update(rp, o, np.zeros(64, dtype=np.int64), C.six_decades(rng, 64))
    check_trees(rp, o, "capacity 2, row 0 only")
