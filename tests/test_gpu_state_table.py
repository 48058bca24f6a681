"""StateTable / pbn_table_insert on the GPU == np.unique, for keys of 1..4 words."""
import numpy as np
import pytest
import torch

from pbn_rl_amd._lib import PbnError
from pbn_rl_amd.state_table import StateTable, sort_states

pytestmark = pytest.mark.gpu

WORDS = [1, 2, 3, 4]
ROWS, STRIDE, COLS = 37, 2080, 2050


def make_input(W, seed, rows=ROWS, stride=STRIDE, hot_share=0.7, n_pool=3000, hot=None, pool=None):
    """(rows, W, stride) uint32: hot_share of the entries from 5 hot keys, the rest from a pool of
    n_pool keys (random in all 32 W bits: the bits above n_bits must be masked off)."""
    rng = np.random.default_rng(seed)
    hot = rng.integers(0, 1 << 32, size=(5, W), dtype=np.uint64).astype(np.uint32) if hot is None else hot
    pool = rng.integers(0, 1 << 32, size=(n_pool, W), dtype=np.uint64).astype(np.uint32) if pool is None else pool
    keys = pool[rng.integers(0, len(pool), size=rows * stride)]
    pick = rng.random(rows * stride) < hot_share
    keys[pick] = hot[rng.integers(0, 5, size=int(pick.sum()))]
    return np.ascontiguousarray(keys.reshape(rows, stride, W).transpose(0, 2, 1)), hot, pool


def unique_counts(st, n_cols, n_bits, counts=None):
    """np.unique over the counted columns of st (T, W, stride), keys masked to n_bits, ascending by
    state value; counts (T * n_cols,) are multiplicities (0 drops the row)."""
    W = st.shape[1]
    rows = st[:, :, :n_cols].transpose(0, 2, 1).reshape(-1, W).copy()
    rows[:, W - 1] &= np.uint32((1 << (n_bits - 32 * (W - 1))) - 1)
    if counts is not None:
        rows, counts = rows[counts > 0], counts[counts > 0]
    uniq, inv = np.unique(rows, axis=0, return_inverse=True)
    cnt = np.zeros(len(uniq), dtype=np.uint64)
    np.add.at(cnt, inv.ravel(), np.uint64(1) if counts is None else counts.astype(np.uint64))
    order = sort_states(uniq)
    return uniq[order], cnt[order]


def merged(*pairs):
    """the union of (words, counts) results, counts of equal keys summed"""
    words = np.concatenate([p[0] for p in pairs])
    uniq, inv = np.unique(words, axis=0, return_inverse=True)
    cnt = np.zeros(len(uniq), dtype=np.uint64)
    np.add.at(cnt, inv.ravel(), np.concatenate([p[1] for p in pairs]))
    order = sort_states(uniq)
    return uniq[order], cnt[order]


def dev(a):
    return torch.from_numpy(a.view(np.int32)).cuda()


def assert_items(table, want):
    words, counts = table.items()
    assert table.n_lost == 0
    assert words.dtype == np.uint32 and counts.dtype == np.uint64
    assert np.array_equal(words, want[0]) and np.array_equal(counts, want[1])
    assert len(table) == len(want[0]) and table.total == int(want[1].sum())
    assert 2 * len(table) <= table.capacity


@pytest.mark.parametrize("W", WORDS)
def test_insert_equals_np_unique_while_the_table_grows(W):
    n_bits = 32 * W - 3
    st, _, _ = make_input(W, 100 + W)
    table = StateTable(n_bits, "cuda", capacity=64)
    # in slices, so that the table grows several times and later launches meet earlier keys
    for lo, hi in ((0, 1), (1, 2), (2, 5), (5, 17), (17, ROWS)):
        table.add(dev(st[lo:hi]), COLS)
    want = unique_counts(st, COLS, n_bits)
    assert len(want[0]) > 2500 and int(want[1].sum()) == ROWS * COLS
    assert_items(table, want)
    assert table.n_growths >= 3 and table.capacity >= 8192


@pytest.mark.parametrize("W", WORDS)
def test_one_launch_into_a_sized_table(W):
    """All 37 x 2,050 rows in one launch (297 blocks): every new key is claimed and met again
    within the launch, so equal keys are compared through the claiming input row."""
    n_bits = 32 * W - 3
    st, _, _ = make_input(W, 200 + W)
    table = StateTable(n_bits, "cuda", capacity=1 << 18, grow=False)
    table.add(dev(st), COLS)
    assert_items(table, unique_counts(st, COLS, n_bits))
    assert table.n_growths == 0


@pytest.mark.parametrize("W", WORDS)
def test_two_adds_mix_old_and_new_keys(W):
    n_bits = 32 * W - 3
    a, hot, pool = make_input(W, 300 + W, rows=5)
    extra = np.random.default_rng(W).integers(0, 1 << 32, size=(1500, W), dtype=np.uint64).astype(np.uint32)
    b, _, _ = make_input(W, 400 + W, rows=5, hot=hot, pool=np.concatenate([pool[:1500], extra]))
    table = StateTable(n_bits, "cuda", capacity=1 << 16, grow=False)
    table.add(dev(a), COLS)
    first = table.items()
    assert_items(table, unique_counts(a, COLS, n_bits))
    table.add(dev(b), COLS)
    want = unique_counts(np.concatenate([a, b]), COLS, n_bits)
    assert_items(table, want)
    second = unique_counts(b, COLS, n_bits)
    old = {tuple(r) for r in first[0].tolist()}
    new = {tuple(r) for r in second[0].tolist()}
    assert len(new & old) > 500 and len(new - old) > 500


@pytest.mark.parametrize("W", [1, 3])
def test_merge_equals_the_table_of_the_concatenated_inputs(W):
    n_bits = 32 * W - 3
    a, hot, pool = make_input(W, 500 + W, rows=4)
    b, _, _ = make_input(W, 600 + W, rows=3, hot=hot, pool=np.concatenate([pool[:1000], pool[:2000] ^ np.uint32(1)]))
    ta, tb = StateTable(n_bits, "cuda", capacity=64), StateTable(n_bits, "cuda", capacity=1 << 15)
    ta.add(dev(a), COLS)
    tb.add(dev(b), COLS)
    before_b = tb.items()
    ta.merge(tb)
    assert_items(ta, unique_counts(np.concatenate([a, b]), COLS, n_bits))
    assert_items(tb, before_b)            # the merged-in table is only read
    with pytest.raises(ValueError):
        ta.merge(StateTable(n_bits + 1, "cuda"))


@pytest.mark.parametrize("W", [2, 4])
def test_row_counts_with_zeros_that_skip_rows(W):
    n_bits = 32 * W - 3
    st, _, _ = make_input(W, 700 + W, rows=3)
    rng = np.random.default_rng(W)
    mult = rng.integers(0, 4, size=3 * COLS).astype(np.uint64)
    mult[:4] = [0, 1 << 40, 0, (1 << 33) + 1]      # 64-bit multiplicities
    table = StateTable(n_bits, "cuda", capacity=64)
    table.add(dev(st), COLS, row_counts=torch.from_numpy(mult.view(np.int64)).cuda())
    want = unique_counts(st, COLS, n_bits, mult)
    assert int((mult == 0).sum()) > 1000 and int(want[1].sum()) == int(mult.sum())
    assert_items(table, want)


def test_grow_false_raises_before_launching_and_keeps_the_table():
    W, n_bits = 2, 61
    rng = np.random.default_rng(800)
    keys = np.unique(rng.integers(0, 1 << 29, size=(400, W), dtype=np.uint64).astype(np.uint32), axis=0)
    keys = keys[rng.permutation(len(keys))[:192]]
    st, more = (np.ascontiguousarray(k.T[None]) for k in (keys[:96], keys[96:]))      # (1, W, 96) each, all distinct
    table = StateTable(n_bits, "cuda", capacity=256, grow=False)
    table.add(dev(st), 90)
    want = unique_counts(st, 90, n_bits)
    assert len(want[0]) == 90
    assert_items(table, want)
    epoch, owner = table._epoch, table.owner.clone()
    with pytest.raises(PbnError, match="grow=False"):
        table.add(dev(more), 39)            # 90 + 39 > 128: too many distinct rows for load 1/2
    assert table._epoch == epoch and torch.equal(table.owner, owner) and table.capacity == 256      # nothing ran
    assert table.n_used == 90
    assert_items(table, want)
    table.add(dev(more), 38)                # 90 + 38 = 128: fits
    both = np.concatenate([st[:, :, :90], more[:, :, :38]], axis=2)
    assert_items(table, unique_counts(both, 128, n_bits))
    assert len(table) == 128


@pytest.mark.parametrize("W", [1, 4])
def test_load_exactly_one_half_stays_exact(W):
    """cap = 2 x distinct keys, grow=False: 2,048 distinct rows (with multiplicities) fill a table of
    4,096 slots to load 1/2, in one launch and, for a second table, in two."""
    n_bits = 32 * W
    rng = np.random.default_rng(900 + W)
    keys = np.unique(rng.integers(0, 1 << 32, size=(4096, W), dtype=np.uint64).astype(np.uint32), axis=0)[:2048]
    assert len(keys) == 2048
    keys = keys[rng.permutation(2048)]
    st = np.ascontiguousarray(keys.T[None])                      # (1, W, 2048)
    mult = rng.integers(1, 1000, size=2048).astype(np.uint64)
    want = unique_counts(st, 2048, n_bits, mult)
    one = StateTable(n_bits, "cuda", capacity=4096, grow=False)
    one.add(dev(st), 2048, row_counts=torch.from_numpy(mult.view(np.int64)).cuda())
    assert_items(one, want)
    assert len(one) == 2048 and one.capacity == 4096
    two = StateTable(n_bits, "cuda", capacity=4096, grow=False)
    for lo, hi in ((0, 1000), (1000, 2048)):
        two.add(dev(np.ascontiguousarray(st[:, :, lo:hi])), hi - lo,
                row_counts=torch.from_numpy(mult[lo:hi].view(np.int64)).cuda())
    assert_items(two, want)
    with pytest.raises(PbnError):
        two.add(dev(st[:, :, :1].copy()), 1)


def test_items_do_not_depend_on_growth_history_and_an_epoch_rebuild_keeps_the_table():
    W, n_bits = 3, 70
    st, _, _ = make_input(W, 1000, rows=6)
    grown, sized = StateTable(n_bits, "cuda", capacity=64), StateTable(n_bits, "cuda", capacity=1 << 17)
    for r in range(6):
        grown.add(dev(st[r:r + 1]), COLS)
    sized.add(dev(st[::-1].copy()), COLS)
    a, b = grown.items(), sized.items()
    assert grown.capacity != sized.capacity
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # the launch after the last epoch: the table rebuilds itself (epochs restart) and stays exact
    sized._epoch = 0xFFFFFFFF
    sized.add(dev(st[:1]), COLS)
    assert sized._epoch == 1 << 32
    sized.add(dev(st[1:2]), COLS)
    assert sized._epoch == 3 and sized.n_growths == 0
    assert_items(sized, merged(b, unique_counts(st[:2], COLS, n_bits)))
