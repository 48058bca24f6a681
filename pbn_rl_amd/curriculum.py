"""Curriculum: weighted (source, target) restarts of a VectorPBNEnv, decided on the device.

The reference's BDQ loop calls ``env.rework_probas(ep_len)`` after every episode
(bdq_model/__init__.py:203): the next resets favour the (start attractor, target attractor) pairs
whose episodes run long.  The scalar facade states the rule (env.py ``PBNEnv.pair_weights``); here it
runs for a whole batch with no host round trip, as two launches of csrc/pbn_curriculum.hip that a
captured frame holds like any other (include/pbn_env.h states the contract, csrc/curriculum_law.h the
law):

* ``redraw()`` after the step and the ring store, before ``EpisodeStats.track()``: every env the step
  reset restarts from a draw over the table instead of the step law's uniform one;
* ``refresh()`` after ``track()``: every ``refresh_every`` frames the table is rebuilt from
  ``stats.pairs_t``.

The step kernels and their law are untouched: an env's uniform restart is simply overwritten.  The
multi-step rollouts (``VectorPBNEnv.rollout``) keep the uniform autoreset.  Under data parallelism
every rank builds its table from its own ``pairs``.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from .episode_stats import EpisodeStats

__all__ = ["Curriculum", "table_layout", "read_table"]


def table_layout(A: int) -> Dict[str, int]:
    """Byte offsets of the table's parts and its size (include/pbn_env.h)."""
    cdf = 8 * A
    total = cdf + (4 * A * A + 7) // 8 * 8
    return {"rowcdf": 0, "cdf": cdf, "total": total, "refreshes": total + 8, "bytes": total + 16}


def read_table(table_t: torch.Tensor, A: int) -> dict:
    """The parts of a table buffer (int64 words on any device) as numpy arrays and ints."""
    lay = table_layout(A)
    raw = table_t.cpu().numpy().view(np.uint8)
    cdf = raw[lay["cdf"]:lay["cdf"] + 4 * A * A].view(np.uint32).reshape(A, A).copy()
    u64 = raw.view(np.uint64)
    return {"rowcdf": u64[:A].copy(), "cdf": cdf, "total": int(u64[lay["total"] // 8]),
            "refreshes": int(u64[lay["refreshes"] // 8])}


class Curriculum:
    """The curriculum of ``venv``'s envs from ``stats`` (an EpisodeStats of the same env).  The
    constructor builds the table from ``stats``' current pair matrix (all zero: uniform weights).
    ``refresh_every`` frames between rebuilds; 0: only ``refresh(force=True)`` rebuilds."""

    def __init__(self, venv, stats: EpisodeStats, refresh_every: int = 1000):
        A = len(venv.spec.attractors)
        if A < 2:
            raise ValueError(f"a curriculum needs at least two attractors, the env's spec has {A}")
        if stats.venv is not venv or stats.n_attractors != A:
            raise ValueError(f"the statistics were built for another env or spec ({stats.n_attractors} attractors, "
                             f"the env's spec has {A})")
        if refresh_every < 0:
            raise ValueError("refresh_every must be >= 0")
        self.venv, self.stats, self.refresh_every = venv, stats, int(refresh_every)
        self.n_attractors = A
        self.horizon = int(venv.spec.horizon or 20)
        self.layout = table_layout(A)
        with torch.cuda.device(venv.device):
            size = _lib.load().pbn_curriculum_table_bytes(A)
        if size < 0:
            _lib.check(size, "pbn_curriculum_table_bytes")
        if size != self.layout["bytes"]:
            raise _lib.PbnError(f"the library's table has {size} bytes, table_layout({A}) {self.layout['bytes']}")
        self.table_t = torch.zeros(size // 8, dtype=torch.int64, device=venv.device)
        self.refresh(force=True)

    def _check_spec(self) -> None:
        A = len(self.venv.spec.attractors)
        if A != self.n_attractors or self.stats.n_attractors != A:
            raise ValueError(f"the env's spec has {A} attractors, this curriculum was built for "
                             f"{self.n_attractors}: construct a new Curriculum after set_spec")

    def redraw(self, step: Optional[int] = None, step_t: Optional[torch.Tensor] = None,
               target_copy: Optional[torch.Tensor] = None) -> None:
        """Restarts the envs whose last step reset them (``flags & RESET``) from the table, on the
        env's current stream.  The Philox step coordinate is the index that step ran at: ``step_t``
        (a one-element int64 device tensor read when the kernel runs: a captured frame's, before it
        advances) or ``step`` (default: ``venv.step_index - 1``, right after ``step_flipmask``).
        ``target_copy``: a second uint8 [n_alloc] buffer that receives the new targets too."""
        self._check_spec()
        v = self.venv
        if step_t is not None and (step_t.dtype != torch.int64 or step_t.device != v.device or step_t.numel() != 1):
            raise ValueError("step_t must be a one-element int64 tensor on the env's device")
        if target_copy is not None and (target_copy.dtype != torch.uint8 or target_copy.numel() != v.n_alloc
                                        or target_copy.device != v.device):
            raise ValueError("target_copy must be a uint8 tensor of n_alloc elements on the env's device")
        if step is None:
            step = v.step_index - 1
        with torch.cuda.device(v.device):
            _lib.check(_lib.load().pbn_curriculum_redraw(
                v.net.handle, v.seed, int(step) & 0xFFFFFFFFFFFFFFFF, step_t.data_ptr() if step_t is not None else None,
                v.env_offset, v.n_alloc, v.num_envs, v.flags.data_ptr(), v.state.data_ptr(), v.target.data_ptr(),
                target_copy.data_ptr() if target_copy is not None else None, self.table_t.data_ptr(), v._stream()),
                "pbn_curriculum_redraw")

    def refresh(self, force: bool = False) -> None:
        """One launch after ``stats.track()``: rebuilds the table when ``stats``' frame count is a
        multiple of ``refresh_every`` (decided on the device), or now with ``force``."""
        self._check_spec()
        v, st = self.venv, self.stats
        with torch.cuda.device(v.device):
            _lib.check(_lib.load().pbn_curriculum_refresh(
                st.totals_t.data_ptr(), st.pairs_t.data_ptr(), self.n_attractors, self.horizon,
                -1 if force else self.refresh_every, self.table_t.data_ptr(), v._stream()), "pbn_curriculum_refresh")

    # ------------------------------------------------------------ checkpoints
    def state_dict(self) -> dict:
        return {"table_t": self.table_t.detach().to("cpu", copy=True)}

    def load_state_dict(self, sd: dict) -> None:
        self.table_t.copy_(sd["table_t"])

    # ------------------------------------------------------------ reading (each synchronises)
    def table(self) -> dict:
        """``rowcdf`` uint64 [A], ``cdf`` uint32 [A][A], ``total`` and ``refreshes`` (ints)."""
        return read_table(self.table_t, self.n_attractors)

    def weights(self) -> np.ndarray:
        """(A, A) float64: the probability of every (source, target) restart, ``w / total``."""
        t = self.table()
        w = np.diff(t["cdf"].astype(np.int64), axis=1, prepend=0)
        return w.astype(np.float64) / float(t["total"])
