"""A count of visited states on the device, keyed by the full state of any width the env runs.

``StateTable`` owns the arrays of an open-addressing hash table (csrc/state_table.h) and fills
them with ``pbn_table_insert`` (csrc/pbn_table.hip): the sparse counterpart of the dense
``pbn_state_histogram`` bins, for networks above 32 nodes and for long runs that visit a small
part of 2^N.  ``SparseSSD`` is the drained table as plain numpy.

The capacity rule is a condition of the kernel, not a tuning knob: the load never exceeds 1/2, so
a probe always meets an empty slot.  The table keeps a host-side upper bound of the claimed
slots (every ``add`` can claim at most its number of rows), reads the true number only when the
bound says the next launch might not fit, and grows -- or raises -- before anything is launched.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

from . import _lib
from ._lib import PbnError

__all__ = ["StateTable", "SparseSSD", "sort_states"]

MIN_CAPACITY = 64
EPOCH_LAST = 0xFFFFFFFF      # the largest epoch a launch can carry
ROW_LIMIT = 0xFFFFFFFF       # rows of one launch: a slot's owner names its row in 32 bits


def sort_states(words: np.ndarray) -> np.ndarray:
    """The order of the (S, W) uint32 rows ascending by the state's integer value (word W-1 is the
    most significant)."""
    words = np.asarray(words, dtype=np.uint32)
    return np.lexsort(tuple(words[:, w] for w in range(words.shape[1])))


class SparseSSD:
    """The visited states of a steady-state run and their counts, ascending by state value.

    ``words`` (S, W) uint32 packed states (bit i of word i // 32 = node i), ``counts`` (S,) uint64,
    ``n_nodes``, ``total`` (the counted steps, a Python int)."""

    def __init__(self, words: np.ndarray, counts: np.ndarray, n_nodes: int):
        self.n_nodes = int(n_nodes)
        self.counts = np.ascontiguousarray(counts, dtype=np.uint64)
        self.words = np.ascontiguousarray(words, dtype=np.uint32)
        if self.words.shape != (len(self.counts), (self.n_nodes + 31) // 32):
            raise ValueError("words must be (len(counts), ceil(n_nodes / 32))")
        self.total = int(self.counts.sum(dtype=np.uint64))

    def __len__(self) -> int:
        return len(self.counts)

    @property
    def probs(self) -> np.ndarray:
        """counts / total (float64): the fraction of counted steps spent in each visited state"""
        out = np.zeros(len(self.counts), dtype=np.float64)
        if self.total > 0:
            np.divide(self.counts, self.total, out=out)
        return out

    @property
    def bits(self) -> np.ndarray:
        """(S, N) uint8: node i of each visited state"""
        shifts = np.arange(32, dtype=np.uint32)
        return ((self.words[:, :, None] >> shifts) & 1).reshape(len(self.words), -1)[:, :self.n_nodes].astype(np.uint8)

    def top(self, k: int) -> Tuple[np.ndarray, np.ndarray]:
        """The k most visited states, most visited first (ties: the smaller state first):
        (bits (k, N) uint8, probs (k,))."""
        order = np.argsort(-self.counts.astype(np.int64), kind="stable")[:max(int(k), 0)]
        return self.bits[order], self.probs[order]

    def marginals(self) -> np.ndarray:
        """(N,) float64: P(node i = 1)"""
        return self.probs @ self.bits.astype(np.float64) if len(self.counts) else np.zeros(self.n_nodes)

    def to_dense(self) -> np.ndarray:
        """The 2^N array the dense ``compute_ssd_hist`` returns (N <= 32)."""
        if self.n_nodes > 32:
            raise ValueError("to_dense has 2^N entries: networks with at most 32 nodes")
        counts = np.zeros(1 << self.n_nodes, dtype=np.uint64)
        counts[self.words[:, 0]] = self.counts
        ssd = np.zeros(counts.shape, dtype=np.float64)
        if self.total > 0:
            np.divide(counts, self.total, out=ssd)
        return ssd


def _capacity_for(slots: int) -> int:
    """the smallest power of two (at least MIN_CAPACITY) with slots <= capacity / 2"""
    cap = MIN_CAPACITY
    while 2 * slots > cap:
        cap *= 2
    return cap


class StateTable:
    """Counts of states of ``n_bits`` bits (1..128) on ``device``.

    ``capacity`` (a power of two >= 64) is the initial number of slots; with ``grow`` the table
    doubles as needed, without it an ``add`` that might push the load past 1/2 raises ``PbnError``
    before launching.  ``n_growths`` counts the rehashes into a larger table."""

    def __init__(self, n_bits: int, device, capacity: int = 1 << 16, grow: bool = True):
        import torch
        if not 1 <= n_bits <= 128:
            raise ValueError("n_bits must be 1..128")
        if capacity < MIN_CAPACITY or capacity & (capacity - 1):
            raise ValueError("capacity must be a power of two, at least 64")
        self.n_bits = int(n_bits)
        self.words = (self.n_bits + 31) // 32
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.grow = bool(grow)
        self.n_growths = 0
        self._alloc(int(capacity))

    def _alloc(self, capacity: int) -> None:
        import torch
        dev = self.device
        self.capacity = capacity
        self.owner = torch.zeros(capacity, dtype=torch.int64, device=dev)
        self.keys = torch.zeros(self.words, capacity, dtype=torch.int32, device=dev)
        self.counts = torch.zeros(capacity, dtype=torch.int64, device=dev)
        self._meta = torch.zeros(2, dtype=torch.int64, device=dev)      # n_used, n_lost
        self._epoch = 1          # of the next launch
        self._used_ub = 0        # host-side upper bound of n_used

    # ---- launches
    def _launch(self, states, n_rows: int, n_cols: int, col_stride: int, row_counts) -> None:
        import torch
        L = _lib.load()
        with torch.cuda.device(self.device):
            _lib.check(L.pbn_table_insert(states.data_ptr(), n_rows, n_cols, col_stride, self.words, self.n_bits,
                                          row_counts.data_ptr() if row_counts is not None else None, self.capacity,
                                          self.owner.data_ptr(), self.keys.data_ptr(), self.counts.data_ptr(),
                                          self._meta[0:].data_ptr(), self._meta[1:].data_ptr(), self._epoch,
                                          torch.cuda.current_stream(self.device).cuda_stream),
                       "pbn_table_insert")
        self._epoch += 1

    def _rehash(self, capacity: int) -> None:
        """this table's entries into fresh arrays of ``capacity`` slots (epochs restart at 1)"""
        keys, counts, cap = self.keys, self.counts, self.capacity
        self._alloc(capacity)
        self._launch(keys, 1, cap, cap, counts)

    def _reserve(self, rows: int) -> None:
        """Makes room for a launch that claims at most ``rows`` slots, or raises before it."""
        if rows >= ROW_LIMIT:
            raise PbnError(f"{rows} rows in one launch: at most 2^32 - 2 (split the input)")
        if self._used_ub + rows > self.capacity // 2:
            self._used_ub = self.n_used            # one synchronisation: the true number of claimed slots
            if self._used_ub + rows > self.capacity // 2:
                if not self.grow:
                    raise PbnError(f"state table full: {self._used_ub} of {self.capacity} slots used and {rows} "
                                   "more rows would pass load 1/2 (grow=False)")
                used = self._used_ub
                self._rehash(_capacity_for(used + rows))
                self._used_ub = used
                self.n_growths += 1
        if self._epoch > EPOCH_LAST:               # before the epoch could wrap: rebuild in place
            used = self._used_ub = self.n_used
            self._rehash(self.capacity)
            self._used_ub = used
        self._used_ub += rows

    def add(self, states, n_cols: int, row_counts=None) -> None:
        """Counts ``states[t, :, c]`` for every t and c < n_cols: an int32 / uint32 (T, W, stride)
        tensor on the table's device, the rollouts' ``obs`` / ``final_state``.  ``row_counts``
        (int64 / uint64 (T * n_cols,), row t * n_cols + c) gives each row's multiplicity; 0 skips it."""
        import torch
        if states.dim() != 3 or states.shape[1] != self.words or not states.is_contiguous():
            raise ValueError(f"states must be a contiguous (T, {self.words}, stride) tensor")
        if states.dtype not in (torch.int32, torch.uint32) or states.device != self.device:
            raise ValueError("states must be int32 / uint32 on the table's device")
        T, _, stride = states.shape
        if not 0 <= n_cols <= stride:
            raise ValueError("n_cols must be in 0..stride")
        rows = T * n_cols
        if row_counts is not None:
            if (row_counts.dtype not in (torch.int64, torch.uint64) or row_counts.device != self.device or
                    row_counts.numel() != rows or not row_counts.is_contiguous()):
                raise ValueError("row_counts must be a contiguous int64 / uint64 tensor of T * n_cols entries "
                                 "on the table's device")
        if rows == 0:
            return
        self._reserve(rows)
        self._launch(states, T, n_cols, stride, row_counts)

    def merge(self, other: "StateTable") -> None:
        """Adds every count of ``other`` (same n_bits and device) to this table."""
        if other.n_bits != self.n_bits or other.device != self.device:
            raise ValueError("merge needs a table of the same n_bits on the same device")
        if other is self:
            raise ValueError("a table cannot be merged into itself")
        self._reserve(other.n_used)
        self._launch(other.keys, 1, other.capacity, other.capacity, other.counts)

    # ---- reading (each synchronises)
    def _meta_host(self) -> np.ndarray:
        return self._meta.cpu().numpy().view(np.uint64)

    @property
    def n_used(self) -> int:
        return int(self._meta_host()[0])

    @property
    def n_lost(self) -> int:
        return int(self._meta_host()[1])

    def __len__(self) -> int:
        return self.n_used

    @property
    def total(self) -> int:
        """the sum of all counts"""
        return int(self.counts.sum().item())

    def items(self) -> Tuple[np.ndarray, np.ndarray]:
        """(words (S, W) uint32, counts (S,) uint64), ascending by the state's integer value."""
        import torch
        lost = self.n_lost
        if lost != 0:
            raise PbnError(f"state table lost {lost} rows: the load passed 1/2 (capacity {self.capacity})")
        slots = torch.nonzero(self.owner != 0).flatten()
        for w in range(self.words):      # stable sorts from the least significant word up, on the device
            word = self.keys[w, slots].to(torch.int64) & 0xFFFFFFFF
            slots = slots[torch.sort(word, stable=True)[1]]
        words = self.keys[:, slots].t().contiguous().cpu().numpy().view(np.uint32).reshape(-1, self.words)
        counts = self.counts[slots].cpu().numpy().view(np.uint64)
        return words, counts
