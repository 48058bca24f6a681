"""EpisodeStats: episode statistics of a VectorPBNEnv kept on the device, one ``track()`` per frame.

What the reference logs on the host every frame -- ``RecordEpisodeStatistics``' ``rollout/ep_rew_mean``
and ``rollout/ep_len_mean`` (ddqn_per/__init__.py:67,357-377), the BDQ loop's ``ep_len``,
``ep_reward`` and ``missed[(state_attractor_id, target_attractor_id)]`` (bdq_model/__init__.py:179-236)
-- needs a device-to-host copy and a synchronisation per frame when it is rebuilt from
``(reward, done)``; inside a captured frame that is impossible.  Here the bookkeeping is two launches
of csrc/pbn_episode.hip (``pbn_episode_track``; include/pbn_env.h states the contract), which a
captured frame holds like any other, and the host reads the aggregates when it wants to print.

The aggregates are int64 and written by integer atomics only, so they do not depend on the order of
the adds.  A return is the plain float32 sum of its episode's rewards in frame order; it enters
``ret_sum`` once, at the close, in units of 2^-20 (``FIXED_ONE``).
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib

__all__ = ["EpisodeStats", "TOTALS", "PAIR_FIELDS", "FIXED_ONE", "HIST_BINS"]

TOTALS = ("frames", "episodes", "successes", "missed", "len_sum", "ret_sum", "last_reward_sum", "unpaired")
PAIR_FIELDS = ("episodes", "missed", "len_sum", "ret_sum")
FIXED_ONE = 1 << 20      # ret_sum and last_reward_sum count 2^-20
HIST_BINS = 256          # bin 255 holds every length >= 255
NO_TARGET = 0xFF


def _means(d: Dict[str, int]) -> Dict[str, float]:
    """The three means and the success rate of a set of totals (or of a difference of two)."""
    n = d["episodes"]
    nan = float("nan")
    return {"ep_len_mean": d["len_sum"] / n if n else nan,
            "ep_rew_mean": d["ret_sum"] / FIXED_ONE / n if n else nan,
            "ep_last_reward_mean": d["last_reward_sum"] / FIXED_ONE / n if n else nan,
            "success_rate": d["successes"] / n if n else nan}


class EpisodeStats:
    """Episode statistics of ``venv``'s ``num_envs`` envs (autoreset envs: without autoreset a
    finished env keeps producing done steps, each of which closes a one-step episode).

    The constructor opens an episode for every env from its current state and target (``begin()``);
    call ``begin()`` again after ``venv.reset()`` or ``set_state``.  ``track()`` is one frame, after the
    step.  ``log_every`` > 0 records the totals every ``log_every`` frames into a ring of
    ``series_rows`` rows on the device (``series()``), so that the windows that elapse inside
    back-to-back graph replays are kept.  An episode ends when ``flags & done_mask``."""

    def __init__(self, venv, *, log_every: int = 0, series_rows: int = 1024,
                 done_mask: int = _lib.FLAG_TERMINATED | _lib.FLAG_TRUNCATED):
        if log_every < 0:
            raise ValueError("log_every must be >= 0")
        if log_every > 0 and series_rows < 1:
            raise ValueError("series_rows must be >= 1")
        self.venv = venv
        self.log_every, self.series_rows, self.done_mask = int(log_every), int(series_rows), int(done_mask)
        self.n_attractors = A = len(venv.spec.attractors)
        dev, n = venv.device, venv.n_alloc
        self.ret = torch.zeros(n, dtype=torch.float32, device=dev)
        self.len = torch.zeros(n, dtype=torch.int32, device=dev)       # uint32 on the device
        self.src = torch.full((n,), NO_TARGET, dtype=torch.uint8, device=dev)
        self.tgt = torch.full((n,), NO_TARGET, dtype=torch.uint8, device=dev)
        z64 = lambda *s: torch.zeros(*s, dtype=torch.int64, device=dev)  # noqa: E731
        self.totals_t = z64(len(TOTALS))
        self.pairs_t = z64(A, A, len(PAIR_FIELDS)) if A else None
        self.hist_t = z64(HIST_BINS)
        self.series_t = z64(self.series_rows, len(TOTALS)) if self.log_every else None
        self._mark()
        self.begin()

    # ------------------------------------------------------------ the device calls
    def _check_spec(self) -> None:
        A = len(self.venv.spec.attractors)
        if A != self.n_attractors:
            raise ValueError(f"the env's spec has {A} attractors, these statistics were built for "
                             f"{self.n_attractors}: construct a new EpisodeStats after set_spec")

    def begin(self) -> None:
        """Opens an episode for every env from its current state and target."""
        self._check_spec()
        v = self.venv
        with torch.cuda.device(v.device):
            _lib.check(_lib.load().pbn_episode_begin(
                v.net.handle, v.n_alloc, v.num_envs, v.state.data_ptr(), v.target.data_ptr(), self.ret.data_ptr(),
                self.len.data_ptr(), self.src.data_ptr(), self.tgt.data_ptr(), v._stream()), "pbn_episode_begin")

    def track(self) -> None:
        """One frame's bookkeeping, on the env's current stream.  The env's pointers are taken at
        every call (``step_flipmask`` swaps its state buffers)."""
        self._check_spec()
        v = self.venv
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        with torch.cuda.device(v.device):
            _lib.check(_lib.load().pbn_episode_track(
                v.net.handle, v.n_alloc, v.num_envs, self.done_mask, v.reward.data_ptr(), v.flags.data_ptr(),
                v.state.data_ptr(), v.target.data_ptr(), self.ret.data_ptr(), self.len.data_ptr(),
                self.src.data_ptr(), self.tgt.data_ptr(), self.totals_t.data_ptr(), ptr(self.pairs_t),
                self.hist_t.data_ptr(), self.log_every, self.series_rows, ptr(self.series_t), v._stream()),
                "pbn_episode_track")

    def reset(self) -> None:
        """Zeroes the aggregates and opens the episodes anew."""
        for t in (self.totals_t, self.pairs_t, self.hist_t, self.series_t):
            if t is not None:
                t.zero_()
        self._mark()
        self.begin()

    # ------------------------------------------------------------ checkpoints
    _STATE_TENSORS = ("ret", "len", "src", "tgt", "totals_t", "pairs_t", "hist_t", "series_t")

    def state_dict(self) -> dict:
        """CPU copies of the per-env episode state and of the aggregates, and the baseline
        ``window()`` differences against (``last_totals`` in TOTALS' order, ``last_missed``)."""
        out = {k: getattr(self, k).detach().to("cpu", copy=True) for k in self._STATE_TENSORS
               if getattr(self, k) is not None}
        out["last_totals"] = [int(self._last_totals[k]) for k in TOTALS]
        out["last_missed"] = torch.from_numpy(np.array(self._last_missed, dtype=np.int64))
        return out

    def load_state_dict(self, sd: dict) -> None:
        """In place; ``window()`` then reports what happens after the checkpoint's last ``window()``."""
        for k in self._STATE_TENSORS:
            if getattr(self, k) is not None:
                getattr(self, k).copy_(sd[k])
        self._last_totals = dict(zip(TOTALS, (int(x) for x in sd["last_totals"])))
        self._last_missed = np.array(sd["last_missed"].numpy(), dtype=np.int64)

    # ------------------------------------------------------------ reading (each synchronises)
    def _raw_totals(self) -> Dict[str, int]:
        return dict(zip(TOTALS, (int(x) for x in self.totals_t.cpu().tolist())))

    def _raw_pairs(self) -> np.ndarray:
        A = self.n_attractors
        return self.pairs_t.cpu().numpy() if A else np.zeros((0, 0, len(PAIR_FIELDS)), dtype=np.int64)

    def totals(self) -> dict:
        """The eight totals as Python ints, the means over every closed episode, ``success_rate``
        and ``steps`` = frames * num_envs."""
        d = self._raw_totals()
        return {**d, **_means(d), "steps": d["frames"] * self.venv.num_envs}

    def pairs(self) -> Dict[str, np.ndarray]:
        """(A, A) arrays by (source, target) attractor: ``episodes``, ``missed``, ``mean_len``,
        ``mean_ret`` (nan where no episode closed)."""
        p = self._raw_pairs()
        eps = p[..., 0]
        with np.errstate(invalid="ignore", divide="ignore"):
            mean_len = np.where(eps > 0, p[..., 2] / eps, np.nan)
            mean_ret = np.where(eps > 0, p[..., 3] / FIXED_ONE / eps, np.nan)
        return {"episodes": eps.copy(), "missed": p[..., 1].copy(), "mean_len": mean_len, "mean_ret": mean_ret}

    def length_hist(self) -> np.ndarray:
        """int64 [256]: closed episodes by length; bin 255 holds every length >= 255."""
        return self.hist_t.cpu().numpy()

    def series(self) -> dict:
        """``{"windows": [...], "lost": n}``: one entry per recorded window still in the ring, oldest
        first.  An entry holds the totals at the window's end and, from the difference to the row
        before it, the window's own ``episodes``, ``missed``, means and ``success_rate`` (under
        ``"window"``; None for the oldest entry of a wrapped ring, whose predecessor is gone).
        ``lost``: the windows overwritten."""
        if not self.log_every:
            return {"windows": [], "lost": 0}
        rows = self.series_t.cpu().numpy()
        done = int(self.totals_t[0].item()) // self.log_every
        kept = min(done, self.series_rows)
        out: List[dict] = []
        prev: Optional[Dict[str, int]] = None if done > kept else dict.fromkeys(TOTALS, 0)
        for j in range(done - kept, done):              # window j ends at frame (j + 1) log_every
            cur = dict(zip(TOTALS, (int(x) for x in rows[j % self.series_rows])))
            entry = dict(cur)
            entry["window"] = None
            if prev is not None:
                diff = {k: cur[k] - prev[k] for k in TOTALS}
                entry["window"] = {"episodes": diff["episodes"], "missed": diff["missed"], **_means(diff)}
            out.append(entry)
            prev = cur
        return {"windows": out, "lost": done - kept}

    def _mark(self) -> None:
        self._last_totals = dict.fromkeys(TOTALS, 0)
        self._last_missed = np.zeros((self.n_attractors, self.n_attractors), dtype=np.int64)

    def window(self) -> dict:
        """What changed since the last ``window()`` (or ``reset()``, or construction): ``frames``,
        ``episodes``, the three means, ``success_rate``, ``missed`` and ``missed_pairs``, the number of
        (source, target) pairs whose ``missed`` grew -- the reference's "Average episode reward",
        "Avg len" and "Missed paths" every 1,000 frames."""
        cur = self._raw_totals()
        missed = self._raw_pairs()[..., 1].copy()
        diff = {k: cur[k] - self._last_totals[k] for k in TOTALS}
        out = {"frames": diff["frames"], "episodes": diff["episodes"], **_means(diff), "missed": diff["missed"],
               "missed_pairs": int((missed > self._last_missed).sum())}
        self._last_totals, self._last_missed = cur, missed
        return out

    def pair_weights(self) -> Optional[np.ndarray]:
        """The scalar facade's ``rework_probas`` rule (env.py PBNEnv.pair_weights) on the device's
        matrix: a pair's weight is (``horizon or 20`` + ``len_sum``) / (1 + ``episodes``), the diagonal
        is 0, the weights are normalised.  None with fewer than two attractors."""
        if self.n_attractors < 2:
            return None
        p = self._raw_pairs()
        w = (float(self.venv.spec.horizon or 20) + p[..., 2].astype(np.float64)) / (1.0 + p[..., 0])
        np.fill_diagonal(w, 0.0)
        return w / w.sum()
