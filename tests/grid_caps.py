"""The launches of pbn_rl_amd/csrc that clamp their grid and walk the rest in a grid-stride loop, each
cap stated once, and the cases that run every one of them past it (test_gpu_grid_caps.py) with their
plain numpy references.  test_grid_caps_host.py reads the launch lines from the sources and holds them
to what is stated here, so an edited cap fails on the CPU instead of silently un-crossing a case.
Nothing here needs a GPU.

A Cap is (source file, the grid expression as it stands in the launch line, the literal that caps it,
threads per block, elements a thread takes per trip).  ``elements()`` is what one trip of the full
grid covers: a case is past the cap when its size exceeds that, i.e. when some thread takes a second
trip.  pbn_eval_reduce takes one pair per block and trip (``block_elements``); pbn_copy_async's cap
is per compute unit, so its capacity needs the device's CU count.
"""
import dataclasses
import os
from typing import Optional, Tuple

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pbn_rl_amd", "csrc")


@dataclasses.dataclass(frozen=True)
class Cap:
    source: str
    line: str                            # the grid expression of the launch, verbatim from the source
    literal: str                         # the cap inside it, as written
    blocks: int                          # its value (copy: per compute unit)
    threads: int
    per_thread: int
    defs: Tuple[str, ...] = ()           # the source lines that give the names in ``line`` their values
    block_elements: Optional[int] = None  # a block's elements per trip where that is not threads * per_thread
    per_cu: bool = False

    def elements(self, n_cus: Optional[int] = None) -> int:
        """What one trip of the capped grid covers."""
        blocks = self.blocks
        if self.per_cu:
            assert n_cus is not None and n_cus > 0, "this cap is per compute unit"
            blocks *= n_cus
        per_block = self.threads * self.per_thread if self.block_elements is None else self.block_elements
        return blocks * per_block


CAPS = {
    "hist": Cap("pbn_env.hip", "std::min<int64_t>((total + 255) / 256, 4096)", "4096", 4096, 256, 1),
    "copy": Cap("pbn_env.hip", "std::min<int64_t>(want, (int64_t)n_cus * kCopyBlocksPerCu)", "kCopyBlocksPerCu", 8,
                256, 4, defs=("constexpr int64_t kCopyBlocksPerCu = 8;",
                              "const int64_t want = (n16 + 4 * 256 - 1) / (4 * 256);"), per_cu=True),
    "eval_reduce": Cap("pbn_eval.hip", "std::min<int64_t>(n_pairs, 2048)", "2048", 2048, 256, 1,
                       defs=("constexpr int kThreads = 256;",), block_elements=1),
    "obs_unpack": Cap("pbn_agent.hip", "std::min<int64_t>((total4 + kObsThreads - 1) / kObsThreads, 8192)", "8192",
                      8192, 256, 4, defs=("constexpr int kObsThreads = 256;",)),
    "replay_store": Cap("pbn_agent.hip", "std::min<int64_t>((n + kObsThreads - 1) / kObsThreads, 4096)", "4096", 4096,
                        256, 1, defs=("constexpr int kObsThreads = 256;",)),
    "table_insert": Cap("pbn_table.hip", "std::min<int64_t>((total + kThreads - 1) / kThreads, kMaxBlocks)",
                        "kMaxBlocks", 4096, 256, 1,
                        defs=("constexpr int kThreads = 256;", "constexpr int kMaxBlocks = 4096;")),
    "dqn_pack": Cap("pbn_ddqn.hip", "std::min<int64_t>((d.itotal + 255) / 256, 4096)", "4096", 4096, 256, 1),
    "ddqn_schedule": Cap("pbn_ddqn.hip", "std::min<int64_t>((a.n_flat + a.n_img + 255) / 256, 1024)", "1024", 1024, 256,
                         4),
}

# the kernel each capped grid launches: the launch that follows the grid expression in the source
KERNELS = {"hist": "pbn_hist_kernel", "copy": "pbn_copy_kernel", "eval_reduce": "eval_reduce_kernel",
           "obs_unpack": "obs_unpack_kernel", "replay_store": "replay_store_kernel", "table_insert": "pick_insert(n_words)",
           "dqn_pack": "dqn_pack_kernel", "ddqn_schedule": "ddqn_schedule_kernel"}


def past(name: str, size: int, n_cus: Optional[int] = None) -> bool:
    return size > CAPS[name].elements(n_cus)


# ---- a. histogram ---------------------------------------------------------------------------------
# (rows, row_stride, cols): one element past the cap; a ragged last wave on the second trip
# (33 * 32,771 = 1,081,443 = 1,048,576 + 32,867, and 32,867 mod 64 = 35); a third trip
HIST_SHAPES = [(1, 1_048_577, 1_048_577), (33, 32_800, 32_771), (3, 700_000, 699_071)]
HIST_BITS = [1, 7, 20]
HIST_MIXES = ["equal", "hot", "distinct"]


def hist_empty_bin(shape, n_bits):
    """The bin only the uncounted columns [cols, row_stride) hold; None without such columns."""
    _, stride, cols = shape
    return ((1 << n_bits) - 1) // 3 * 2 + 1 if stride > cols else None      # 1, 85, 699,051


def hist_input(shape, n_bits, mix, seed=0):
    """(rows, row_stride) uint32 words, random above bit n_bits.  The counted columns draw their low
    n_bits from every bin but hist_empty_bin: ``equal`` one bin for all; ``hot`` 70 % from five hot
    bins, the rest uniform; ``distinct`` the 64 consecutive elements a wave takes in one trip all
    differ (as far as the bins allow: at n_bits = 1 they alternate, or are equal where one of the two
    bins is the empty one).  The uncounted columns hold the empty bin."""
    rows, stride, cols = shape
    total, bins = rows * cols, 1 << n_bits
    rng = np.random.default_rng(seed + 1000 * n_bits + rows)
    empty = hist_empty_bin(shape, n_bits)
    usable = np.arange(bins, dtype=np.uint32)
    if empty is not None:
        usable = np.delete(usable, empty)
    if mix == "equal":
        low = np.full(total, usable[len(usable) // 2], np.uint32)
    elif mix == "hot":
        hot = rng.choice(usable, size=min(5, len(usable)), replace=False)
        low = usable[rng.integers(0, len(usable), size=total)]
        pick = rng.random(total) < 0.7
        low[pick] = hot[rng.integers(0, len(hot), size=int(pick.sum()))]
    elif mix == "distinct":
        i = np.arange(total, dtype=np.int64)
        low = usable[((i >> 6) * 7 + (i & 63)) % len(usable)]
    else:
        raise KeyError(mix)
    high = lambda n: (rng.integers(0, 1 << (32 - n_bits), size=n, dtype=np.uint64) << np.uint64(n_bits)).astype(np.uint32)  # noqa: E731
    st = np.empty((rows, stride), np.uint32)
    st[:, :cols] = (low | high(total)).reshape(rows, cols)
    if empty is not None:
        st[:, cols:] = (np.uint32(empty) | high(rows * (stride - cols))).reshape(rows, stride - cols)
    return st


def hist_expected(st, cols, n_bits):
    """np.bincount of the masked counted words, as uint32 [2^n_bits]."""
    mask = np.uint32((1 << n_bits) - 1)
    return np.bincount((st[:, :cols] & mask).ravel(), minlength=1 << n_bits).astype(np.uint32)


def distinct_per_wave(st, cols, n_bits):
    """The smallest number of distinct masked values among the 64 consecutive elements of a full wave."""
    v = (st[:, :cols] & np.uint32((1 << n_bits) - 1)).ravel()
    v = np.sort(v[:len(v) // 64 * 64].reshape(-1, 64), axis=1)
    return int((1 + (np.diff(v, axis=1) != 0).sum(axis=1)).min())


# ---- b. copy --------------------------------------------------------------------------------------
def copy_stride(n16: int, n_cus: int) -> int:
    """pbn_copy_async's grid stride in 16-byte vectors: 256 threads x min(ceil(n16 / 1024), 8 x CUs) blocks."""
    c = CAPS["copy"]
    want = (n16 + c.threads * c.per_thread - 1) // (c.threads * c.per_thread)
    return c.threads * max(1, min(want, c.blocks * n_cus))


def copy_sizes(n_cus: int):
    """Sizes in vectors around the unrolled trip of the capped grid (stride S = 256 x 8 x CUs): 4S - 1
    (the last thread misses the unrolled trip and walks three single ones), 4S (exactly one unrolled
    trip each), 4S + 1 (one thread's single-vector tail after its unrolled trip), 5S + 7 (an unrolled
    trip, then two single ones for seven threads and one for the rest), 7S + 255 (lanes 0..254 of
    the first wave take a second unrolled trip, lane 255 and the rest three single ones), 8S (two
    unrolled trips), 8S + 1 (two and a tail).  Each size's own stride, computed as the kernel does,
    is S."""
    S = CAPS["copy"].threads * CAPS["copy"].blocks * n_cus
    sizes = [4 * S - 1, 4 * S, 4 * S + 1, 5 * S + 7, 7 * S + 255, 8 * S, 8 * S + 1]
    assert all(copy_stride(n, n_cus) == S for n in sizes)
    return S, sizes


def copy_trips(n16: int, S: int, i: int):
    """(unrolled trips, single trips) of the thread that starts at vector i: the kernel's two loops."""
    u = 0
    while i + 3 * S < n16:
        i += 4 * S
        u += 1
    s = 0
    while i < n16:
        i += S
        s += 1
    return u, s


# ---- c. pbn_eval_reduce ---------------------------------------------------------------------------
REDUCE_SHAPES = [(2048, 3), (2049, 1), (4097, 65), (64_516, 1), (2050, 257)]      # (n_pairs, runs)
REDUCE_MAX_STEPS = [1, 100, 254]
REDUCE_AT_CAP = (2048, 3)             # the last size with one trip: every other shape is past the cap
REDUCE_CLAMPED = (4097, 65)           # the shape that also holds counts outside 0..max_steps + 1


def reduce_counts(n_pairs, runs, max_steps, seed=0):
    """(counts (n_pairs, runs) int32 as given to the kernel, the same clamped to 0..max_steps + 1, the
    planted pairs {name: pair}).  Uniform in 0..max_steps + 1; pair 1 all failures and pair 2 all zeros
    (first trip); of the pairs a block reaches on its second trip (2048 and up) the last all failures
    and the first all zeros (with one such pair: all failures); REDUCE_CLAMPED has -3 and
    max_steps + 9 in four pairs, two of them on later trips."""
    blocks = CAPS["eval_reduce"].blocks
    rng = np.random.default_rng(seed + 7 * n_pairs + runs + 1000 * max_steps)
    c = rng.integers(0, max_steps + 2, size=(n_pairs, runs)).astype(np.int32)
    planted = {"fail_first": 1, "zero_first": 2}
    c[1], c[2] = max_steps + 1, 0
    if n_pairs > blocks:
        planted["fail_second"] = n_pairs - 1
        c[n_pairs - 1] = max_steps + 1
        if n_pairs - 1 > blocks:
            planted["zero_second"] = blocks
            c[blocks] = 0
    clamped = c.copy()
    if (n_pairs, runs) == REDUCE_CLAMPED:
        for p in (5, 6, blocks + 5, 2 * blocks - 1):
            c[p, 0::3], c[p, 1::3] = -3, max_steps + 9
            clamped[p, 0::3], clamped[p, 1::3] = 0, max_steps + 1
    return c, clamped, planted


# ---- d. pbn_obs_unpack ----------------------------------------------------------------------------
# (N, envs): N mod 4 != 0, so a float4 straddles two envs; envs * N just past 8192 * 256 * 4
OBS_CASES = [(127, 66_080), (33, 254_240)]


def obs_input(spec, n, seed=0):
    """Random state words (W, n) masked to N bits and targets that cover every attractor id, the
    first id past them, and 255."""
    N, W, A = spec.n, spec.words, len(spec.attractors)
    rng = np.random.default_rng(seed + N)
    st = rng.integers(0, 2 ** 32, size=(W, n), dtype=np.uint64).astype(np.uint32)
    if N % 32:
        st[W - 1] &= np.uint32((1 << (N % 32)) - 1)
    tg = rng.integers(0, A, size=n).astype(np.uint8)
    tg[3::17] = 255
    tg[4::29] = A
    tg[n - A:] = np.arange(A)            # every id in the last envs: the second trip
    tg[:A] = np.arange(A)[::-1]
    return st, tg


# ---- e. pbn_replay_store --------------------------------------------------------------------------
STORE_N = 1_048_833                   # 4096 * 256 + 257
STORE_CAPACITY = STORE_N + 13
STORE_POS = STORE_CAPACITY - (4096 * 256 + 100)     # slot 0 is written by row 1,048,676: a second trip
STORE_WK = [(1, 1), (4, 7)]
# (done_mask, done_out given, state_dst / target_dst given)
STORE_VARIANTS = {"plain": (0, False, False), "out": (0, True, False), "mask_copies": (5, False, True),
                  "mask_out_copies": (36, True, True)}


# ---- f. pbn_table_insert --------------------------------------------------------------------------
TABLE_SHAPE = (33, 32_800, 32_771)    # (rows, col_stride, cols)
TABLE_POOL = 3000
TABLE_CAPACITY = 1 << 22              # grow=False: 2 * 33 * 32,771 rows must fit


def table_input(W, seed=0):
    """(states (rows, W, col_stride) uint32, row_counts (rows * cols,) uint64).  Keys from TABLE_POOL
    distinct random states, 70 % of the entries from five of them: equal keys in every wave.  The
    uncounted columns hold one key no counted column holds.  A quarter of the row counts are 0."""
    rows, stride, cols = TABLE_SHAPE
    rng = np.random.default_rng(seed + W)
    pool = np.unique(rng.integers(0, 2 ** 32, size=(TABLE_POOL + 64, W), dtype=np.uint64).astype(np.uint32), axis=0)
    pool = pool[rng.permutation(len(pool))[:TABLE_POOL + 1]]
    outside, pool = pool[TABLE_POOL], pool[:TABLE_POOL]
    keys = pool[rng.integers(0, TABLE_POOL, size=rows * stride)]
    pick = rng.random(rows * stride) < 0.7
    keys[pick] = pool[rng.integers(0, 5, size=int(pick.sum()))]
    st = np.ascontiguousarray(keys.reshape(rows, stride, W).transpose(0, 2, 1))
    st[:, :, cols:] = outside[None, :, None]
    mult = rng.integers(0, 4, size=rows * cols).astype(np.uint64)
    mult[:4] = [0, 1 << 40, 0, (1 << 33) + 1]
    mult[-3:] = [(1 << 35) + 5, 0, 3]
    return st, mult


# ---- g. DQN pack and target sync ------------------------------------------------------------------
DQN_SPEC, DQN_ARCH, DQN_ENVS = "hold70_a254", (64, 16), 160
DQN_TARGETS = [0, 1, 233, 234, 235, 236, 253]       # and 255 on two envs
DQN_NO_TARGET = (5, 64)


def dqn_image_layout(N, n_attr, h0, h1):
    """(iT, floats of the T section, image floats) of csrc/dqn_forward.h's make_dims."""
    p16 = lambda x: 16 * ((x + 15) // 16)  # noqa: E731
    H0p, H1p, Ap = p16(h0), p16(h1), p16(N + 1)
    t_floats = n_attr * N * H0p
    return 0, t_floats, t_floats + H0p + H1p + Ap + 2 * H1p * H0p + Ap * H1p


def dqn_t_row(N, h0, t):
    """The image offset of target t's rows: iT + t * N * H0p."""
    return t * N * 16 * ((h0 + 15) // 16)
