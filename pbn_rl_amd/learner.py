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

from . import _lib, checkpoint
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

    # ---- checkpoints (checkpoint.py; DESIGN.md "Checkpoint and resume") ----------------------
    agent_kind = ""

    def _parts(self) -> dict:
        """The stateful pieces by the prefix of their names in the learner's ``state_dict()``."""
        parts = {"env": self.env, "replay": self.replay}
        if self.fused is not None:
            parts["update"] = self.fused
        if self.stats is not None:
            parts["stats"] = self.stats
        if self.curriculum is not None:
            parts["curriculum"] = self.curriculum
        return parts

    def state_dict(self) -> dict:
        """The whole run, flat: ``<part>.<name>`` of every piece of ``_parts()``; without a fused
        update the networks (``q.*`` / ``target.*``) and torch.optim.Adam's state per parameter name
        (``adam.*``); the learner's generator (``gen``); and the learner's own counters
        (``learner.*``, among them ``captured``: whether a captured learner wrote them)."""
        out = {}
        for prefix, part in self._parts().items():
            for k, v in part.state_dict().items():
                out[f"{prefix}.{k}"] = v
        if self.fused is None:
            for prefix, net in (("q", self.q), ("target", self.target)):
                for k, v in net.state_dict().items():
                    out[f"{prefix}.{k}"] = checkpoint.cpu_copy(v)
            started = True
            for name, p in self.q.named_parameters():
                st = self.opt.state.get(p, {})
                started = started and len(st) > 0
                for k in ("exp_avg", "exp_avg_sq"):
                    out[f"adam.{k}.{name}"] = checkpoint.cpu_copy(st[k] if st else torch.zeros_like(p))
                step = st["step"] if st else torch.zeros(())
                out[f"adam.step.{name}"] = torch.as_tensor(step).detach().to("cpu", torch.float32, copy=True).reshape(1)
            out["adam.started"] = bool(started)
        out["gen"] = checkpoint.cpu_copy(self.gen.get_state())
        loss = self.last_loss
        out["learner.last_loss"] = (torch.zeros(1) if loss is None
                                    else loss.detach().to("cpu", torch.float32, copy=True).reshape(1))
        out["learner.has_loss"] = loss is not None
        out["learner.captured"] = self._graph is not None
        for k, v in self._own_state().items():
            out[f"learner.{k}"] = v
        return out

    def _check_loadable(self, host: dict) -> None:
        """The learner's own refusals, from the file's host values, before anything is written.  A
        captured frame holds the env's seed and offset as launch arguments, so a learner that is
        already captured takes only a checkpoint with the same ones."""
        if self._graph is not None:
            env = self.env
            for k in ("seed", "env_offset"):
                if int(host[f"env.{k}"]) != int(getattr(env, k)):
                    raise ValueError(f"checkpoint mismatch: env.{k} (file {host[f'env.{k}']}, learner {getattr(env, k)}): "
                                     "the captured frame holds it as a launch argument; load into a fresh learner "
                                     "and capture() after the load")
            self._check_loadable_captured(host)

    def _check_loadable_captured(self, host: dict) -> None:
        pass

    def load_state_dict(self, sd: dict) -> None:
        """In place, piece by piece; then the device counters are refilled from the host's values
        (``_load_counters``; ``capture()`` builds them from the same values)."""
        for prefix, part in self._parts().items():
            part.load_state_dict({k[len(prefix) + 1:]: v for k, v in sd.items() if k.startswith(prefix + ".")})
        if self.fused is None:
            with torch.no_grad():
                for prefix, net in (("q", self.q), ("target", self.target)):
                    for k, v in net.state_dict().items():
                        v.copy_(sd[f"{prefix}.{k}"])
                g = self.opt.param_groups[0]
                on_device = bool(g.get("capturable") or g.get("fused"))
                for name, p in self.q.named_parameters():
                    st = self.opt.state[p]
                    if not sd["adam.started"]:      # saved before the first update: Adam's state at step 0
                        for t in st.values():
                            t.zero_()
                        continue
                    if not st:      # as torch.optim.Adam creates it at its first step
                        st["step"] = (torch.zeros((), dtype=torch.float32, device=p.device) if on_device
                                      else torch.tensor(0.0, dtype=torch.float32))
                        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg"].copy_(sd[f"adam.exp_avg.{name}"])
                    st["exp_avg_sq"].copy_(sd[f"adam.exp_avg_sq.{name}"])
                    st["step"].copy_(sd[f"adam.step.{name}"].reshape(()))
        self.gen.set_state(sd["gen"])
        if not sd["learner.has_loss"]:
            self.last_loss = None
        elif self.fused is not None:
            self.last_loss = self.fused.loss[0]
        else:
            self.last_loss = sd["learner.last_loss"].to(self.env.device)[0]
        self._load_own_state({k[len("learner."):]: v for k, v in sd.items() if k.startswith("learner.")})
        self._load_counters()

    def _load_counters(self) -> None:
        """The host mirrors are authoritative: the device counters that exist are refilled from them
        (``_eps32`` as the ``.float()`` of the double, one rounding, as ``_capture_counters`` has it)."""
        env, rp = self.env, self.replay
        for name, v in (("_pos_t", rp.pos), ("_size_t", rp.size)):
            if getattr(self, name, None) is not None:
                getattr(self, name).fill_(v)
        if self._graph is not None:
            self._step_t.fill_(env.step_index)
            self._eps64.fill_(self.epsilon)
            self._eps32.copy_(self._eps64.float())
            if self._tgt_prev is not None:       # (the settle law's carried targets: the env's, at a frame boundary)
                self._tgt_prev.copy_(env.target)

    def save(self, path: str) -> None:
        """Write the run to ``path`` (checkpoint.py): one ``.npz``, moved into place when complete."""
        checkpoint.save(self, path)

    def load(self, path: str) -> dict:
        """Put back a run saved by a learner built with the same arguments; a ValueError naming what
        differs, before anything is written, otherwise.  Returns the file's header."""
        return checkpoint.load(self, path)

    def _mirror_frame(self) -> None:
        """The host's copies of the counters after one replayed frame."""
        env, rp = self.env, self.replay
        env.step_index += 1
        rp.pos = (rp.pos + env.n_alloc) % rp.capacity
        rp.size = min(rp.size + env.n_alloc, rp.capacity)
        self.epsilon = max(self._eps_floor, self.epsilon - self._eps_step)
