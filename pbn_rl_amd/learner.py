"""The plumbing of a graph-captured learning frame, shared by BDQLearner (replay.py) and
DDQNLearner (ddqn.py).

A captured frame keeps the env's step index, epsilon, the ring position and fill level in
one-element device tensors that its launches advance, and the host mirrors them after every replay
with the eager frame's own arithmetic.  The learners differ here only in values (the done mask, a
done-out buffer, the action tensor, epsilon's floor and step, the seed), which they pass to
``_capture_counters`` and ``_capture_ring``.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch

from . import _lib
from .curriculum import Curriculum
from .episode_stats import EpisodeStats

__all__ = ["FrameLearner"]


class FrameLearner:
    """Reads the subclass's ``env``, ``replay``, ``prioritised``, ``epsilon`` and ``frame()``."""

    stats: Optional[EpisodeStats] = None
    curriculum: Optional[Curriculum] = None
    _tgt_prev: Optional[torch.Tensor] = None

    def _init_stats(self, episode_stats: bool, stats_log_every: int) -> None:
        """``episode_stats=True``: ``stats``, an EpisodeStats over the env's ``num_envs`` envs (those
        whose (reward, done) ``frame()`` returns), opened on the env's current state and tracked
        every frame; ``stats_log_every`` is its ``log_every``.  False: no launch is added."""
        self.stats = EpisodeStats(self.env, log_every=stats_log_every) if episode_stats else None

    def _init_curriculum(self, curriculum: bool, curriculum_refresh: int) -> None:
        """``curriculum=True`` (after ``_init_stats``; it needs ``episode_stats=True``): ``curriculum``,
        a Curriculum over ``stats``, whose redraw and refresh run every frame around ``_track_stats``;
        ``curriculum_refresh`` is its ``refresh_every``.  False: no launch is added."""
        if curriculum and self.stats is None:
            raise ValueError("curriculum=True needs episode_stats=True: the weights are the pair statistics'")
        self.curriculum = Curriculum(self.env, self.stats, refresh_every=curriculum_refresh) if curriculum else None

    def _redraw_resets(self) -> None:
        """Between the ring store and ``_track_stats``: the envs the step reset restart from the
        curriculum's draw, so the episode ``track`` opens, and ``pairs``, see the pair the env really
        starts from.  Eager: the step ran at ``env.step_index - 1``; captured: at ``*_step_t``, which
        advances later in the frame.  The settle law's captured frame carries the targets in
        ``_tgt_prev``, which pbn_replay_store has already moved on: it is rewritten too."""
        if self.curriculum is None:
            return
        if torch.cuda.is_current_stream_capturing():
            self.curriculum.redraw(step_t=self._step_t, target_copy=self._tgt_prev)
        else:
            self.curriculum.redraw()

    def _refresh_curriculum(self) -> None:
        """After ``_track_stats`` (which counted the frame): the table's rebuild, when due."""
        if self.curriculum is not None:
            self.curriculum.refresh()

    def _track_stats(self) -> None:
        """The frame's episode bookkeeping: after the step and the ring store, eager or captured
        (``env.state`` and ``env.target`` then hold what the step left, under either step law)."""
        if self.stats is not None:
            self.stats.track()

    def _warm_up(self, ready: Callable[[], bool]) -> None:
        """Eager frames on a side stream (as graph capture requires) until ``ready()``."""
        dev = torch.device(self.env.device)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            while not ready():
                self.frame()
        torch.cuda.current_stream(dev).wait_stream(side)

    def _capture_counters(self, eps_floor: float, eps_step: float, seed: int) -> None:
        """The device counters of a captured frame, from the host's values; ``eps_floor`` /
        ``eps_step``: epsilon's decay per frame; ``seed``: what pbn_replay_advance is given."""
        env, rp, dev = self.env, self.replay, torch.device(self.env.device)
        self._step_t = torch.full((1,), env.step_index, dtype=torch.int64, device=dev)
        self._eps64 = torch.full((1,), self.epsilon, dtype=torch.float64, device=dev)
        self._eps32 = self._eps64.float()     # (the eager frame's c_float of the same double: one rounding)
        self._pos_t = torch.full((1,), rp.pos, dtype=torch.int64, device=dev)
        self._size_t = torch.full((1,), rp.size, dtype=torch.int64, device=dev)
        self._eps_floor, self._eps_step, self._advance_seed = eps_floor, eps_step, seed

    def _capture_ring(self, done_mask: int, done_out: Optional[torch.Tensor], actions: torch.Tensor) -> None:
        """How the captured step stores: ``_ring`` under the one-update law (the step kernel writes
        the ring rows itself), else ``_tgt_prev``, the pre-step targets pbn_replay_store carries.
        A transition is done when ``flags & done_mask``; ``done_out`` (uint8 [n_alloc], optional)
        receives those values too; ``actions`` (int32 [n_alloc][K]) is what the agent writes."""
        env, rp = self.env, self.replay
        self._store_args = (int(done_mask), done_out, actions)
        self._ring = self._tgt_prev = None
        if env.spec.settle < 2:
            self._ring = _lib.RingStore(
                rp.capacity, self._pos_t.data_ptr(), rp.state.data_ptr(), rp.next_state.data_ptr(),
                rp.target.data_ptr(), rp.action.data_ptr(), rp.reward.data_ptr(), rp.done.data_ptr(),
                actions.data_ptr(), actions.shape[1], int(done_mask),
                done_out.data_ptr() if done_out is not None else None)
        else:
            self._tgt_prev = env.target.clone()

    def _step_and_store(self) -> None:
        """The captured frame's step and ring store (the position advances in ``_advance_counters``)."""
        env, rp = self.env, self.replay
        if self._ring is not None:
            # one launch: the step, in place, writing its transitions into the ring
            env.step_flipmask_dev_store(self._step_t, self._ring)
            if self.prioritised:   # (the new rows' priorities)
                rp.store_priorities(env.n_alloc, self._pos_t)
        else:
            env.step_flipmask_dev(self._step_t, copy_back=False)
            # the ring store reads the pre-step state (still in env.state) and target (carried in
            # _tgt_prev), derives done from the flags, and in the same pass moves the stepped state
            # into env.state and the new targets into _tgt_prev; PrioritisedDeviceReplay.store_at
            # stores the priorities first
            done_mask, done_out, actions = self._store_args
            rp.store_at(self._pos_t, self._size_t, env.state, self._tgt_prev, actions, env.reward, env.final_state,
                        env.flags, done_mask=done_mask, done_out=done_out, advance=False,
                        state_copy=(env.state, env._state_next), target_copy=(self._tgt_prev, env.target))

    def _advance_counters(self) -> None:
        """pbn_replay_advance: the step index, the ring position and fill level and epsilon move on
        by one frame, in one launch."""
        self.replay.advance(self.env.n_alloc, self._pos_t, self._size_t, self._step_t, self._eps64, self._eps32,
                            float(self._eps_floor), float(self._eps_step), self._advance_seed)

    def _mirror_frame(self) -> None:
        """The host's copies of the counters after one replayed frame."""
        env, rp = self.env, self.replay
        env.step_index += 1
        rp.pos = (rp.pos + env.n_alloc) % rp.capacity
        rp.size = min(rp.size + env.n_alloc, rp.capacity)
        self.epsilon = max(self._eps_floor, self.epsilon - self._eps_step)
