"""On-device replay and the BDQ learner update (rows A9, A10).

The reference keeps transitions as host ``Transition`` namedtuples in a Python list
(``ExperienceReplay``, bdq_model/memory.py:17-62), and every update ``np.stack``s 256 of them
and copies them to the GPU (``update_policy``, bdq_model/__init__.py:100-109).  Here the
replay is a ring of packed transitions in HBM, filled straight from the batched env:

    state, next_state   int32 [W][capacity]   packed words (bit i of word w = node 32w + i)
    target              uint8 [capacity]      target attractor id
    action              int32 [capacity][K]   the branch actions
    reward              float32 [capacity]
    done                uint8 [capacity]      terminated or truncated

Sampling gathers rows by index and unpacks them to the fp32 (2, B, N) network input with
``pbn_obs_unpack`` (the HIP kernel the acting frame uses), so nothing goes through the host.
Indices are drawn with replacement (torch's device generator); ``random.sample`` at
bdq_model/memory.py:62 draws without replacement, which only matters for batches comparable
to the ring size.

``bdq_update`` restates ``update_policy`` (bdq_model/__init__.py:100-139) on such a batch:
double-DQN targets ``r + gamma * mask * Q_target(s', argmax_a Q(s', a))`` with the
reference's ``mask = done`` (:109,122 -- it bootstraps only on done transitions; kept as is),
MSE loss, gradients clamped to [-1, 1] (:129-130), one Adam step, and every
``target_update`` updates the target network moves halfway to the online one (:133-139).

``PrioritisedDeviceReplay`` adds the other half of the reference's replay module,
``PrioritisedER`` (bdq_model/memory.py:73-186): proportional prioritised replay over a sum and a
min segment tree, held on the device (csrc/pbn_per.hip; DESIGN.md "Prioritised replay").

``FusedBDQUpdate`` is the update as HIP launches (its buffers and their bookkeeping: fused.py), and
``BDQLearner`` the training loop (the plumbing of its graph-captured frame: learner.py).
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

from . import _lib
from .agent import BatchedBDQ, BranchingQNetwork
from .checkpoint import cpu_copy
from .fused import FusedUpdate, bump
from .learner import FrameLearner
from .vector_env import VectorPBNEnv

__all__ = ["DeviceReplay", "PrioritisedDeviceReplay", "bdq_update", "soft_update", "BDQLearner", "FusedBDQUpdate",
           "bdq_layout", "fused_update_supported"]


class DeviceReplay:
    def __init__(self, capacity: int, words: int, branches: int, device):
        self.capacity = int(capacity)
        self.words = int(words)
        self.device = torch.device(device)
        dev = self.device
        self.state = torch.zeros(words, capacity, dtype=torch.int32, device=dev)
        self.next_state = torch.zeros(words, capacity, dtype=torch.int32, device=dev)
        self.target = torch.zeros(capacity, dtype=torch.uint8, device=dev)
        self.action = torch.zeros(capacity, branches, dtype=torch.int32, device=dev)
        self.reward = torch.zeros(capacity, dtype=torch.float32, device=dev)
        self.done = torch.zeros(capacity, dtype=torch.uint8, device=dev)
        self.pos = 0
        self.size = 0

    _STATE_TENSORS = ("state", "next_state", "target", "action", "reward", "done")

    def state_dict(self) -> dict:
        """CPU copies of the ring's arrays, and ``pos`` and ``size``."""
        out = {k: cpu_copy(getattr(self, k)) for k in self._STATE_TENSORS}
        out.update(pos=int(self.pos), size=int(self.size))
        return out

    def load_state_dict(self, sd: dict) -> None:
        """In place (a captured frame and ``_lib.RingStore`` hold the arrays' pointers)."""
        for k in self._STATE_TENSORS:
            getattr(self, k).copy_(sd[k])
        self.pos, self.size = int(sd["pos"]), int(sd["size"])

    def _slots(self, n: int) -> torch.Tensor:
        return (torch.arange(n, device=self.device, dtype=torch.int64) + self.pos) % self.capacity

    def store(self, state: torch.Tensor, target: torch.Tensor, action: torch.Tensor, reward: torch.Tensor,
              next_state: torch.Tensor, done: torch.Tensor) -> None:
        """Append n transitions: state / next_state (W, n) words, target (n,), action (n, K),
        reward (n,), done (n,) (any dtype castable to the ring's)."""
        n = target.shape[0]
        if n > self.capacity:
            raise ValueError("more transitions than the ring holds")
        idx = self._slots(n)
        self.state.index_copy_(1, idx, state)
        self.next_state.index_copy_(1, idx, next_state)
        self.target.index_copy_(0, idx, target.to(torch.uint8))
        self.action.index_copy_(0, idx, action.to(torch.int32))
        self.reward.index_copy_(0, idx, reward.to(torch.float32))
        self.done.index_copy_(0, idx, done.to(torch.uint8))
        self.pos = (self.pos + n) % self.capacity
        self.size = min(self.size + n, self.capacity)

    def store_at(self, pos_t: torch.Tensor, size_t: torch.Tensor, state, target, action, reward, next_state,
                 done, *, done_mask: int = 0, done_out: Optional[torch.Tensor] = None, advance: bool = True,
                 state_copy=None, target_copy=None) -> None:
        """``store`` with the ring position and fill level held in one-element int64 device
        tensors (advanced here, on the stream, unless ``advance`` is False) instead of host ints:
        graph-capturable.  The caller mirrors them in ``pos`` / ``size``.  ``done_mask`` != 0:
        ``done`` is the env's flags and a transition is done when ``flags & done_mask``;
        ``done_out`` (uint8 [n]) then receives those 0/1 values too.  ``state_copy`` / ``target_copy``:
        optional (dst, src) pairs copied element by element in the same pass, after the element of
        ``state`` / ``target`` is read (dst may be ``state`` / ``target`` itself; GPU path only)."""
        n = target.shape[0]
        if n > self.capacity:
            raise ValueError("more transitions than the ring holds")
        if (self.device.type == "cuda" and state.dtype == torch.int32 and next_state.dtype == torch.int32
                and target.dtype == torch.uint8 and action.dtype == torch.int32 and reward.dtype == torch.float32
                and done.dtype in (torch.bool, torch.uint8)):
            # the six field copies in one launch (pbn_replay_store)
            st, nst, act = state.contiguous(), next_state.contiguous(), action.contiguous()
            if done_out is not None and (done_out.dtype != torch.uint8 or done_out.numel() < n):
                raise ValueError("done_out must be uint8 with n elements")
            L = _lib.load()
            with torch.cuda.device(self.device):
                _lib.check(L.pbn_replay_store(n, pos_t.data_ptr(), self.capacity, self.words, self.action.shape[1],
                                              st.data_ptr(), nst.data_ptr(), target.contiguous().data_ptr(),
                                              act.data_ptr(), reward.contiguous().data_ptr(),
                                              done.contiguous().data_ptr(), int(done_mask),
                                              done_out.data_ptr() if done_out is not None else None,
                                              self.state.data_ptr(), self.next_state.data_ptr(), self.target.data_ptr(),
                                              self.action.data_ptr(), self.reward.data_ptr(), self.done.data_ptr(),
                                              *(t.data_ptr() if t is not None else None
                                                for t in (state_copy or (None, None)) + (target_copy or (None, None))),
                                              torch.cuda.current_stream(self.device).cuda_stream), "pbn_replay_store")
            if advance:
                pos_t.add_(n).remainder_(self.capacity)
                size_t.add_(n).clamp_(max=self.capacity)
            return
        if state_copy is not None or target_copy is not None:
            raise ValueError("state_copy / target_copy need the GPU path (int32 / uint8 / float32 fields)")
        if done_mask:
            done = (done & done_mask) != 0
            if done_out is not None:
                done_out[:n].copy_(done)
        idx = (torch.arange(n, device=self.device, dtype=torch.int64) + pos_t) % self.capacity
        self.state.index_copy_(1, idx, state)
        self.next_state.index_copy_(1, idx, next_state)
        self.target.index_copy_(0, idx, target.to(torch.uint8))
        self.action.index_copy_(0, idx, action.to(torch.int32))
        self.reward.index_copy_(0, idx, reward.to(torch.float32))
        self.done.index_copy_(0, idx, done.to(torch.uint8))
        if advance:
            pos_t.add_(n).remainder_(self.capacity)
            size_t.add_(n).clamp_(max=self.capacity)

    def sample_indices(self, batch: int, generator: Optional[torch.Generator] = None,
                       size_t: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``batch`` indices uniform over the filled part, with replacement: floor(u * size)
        for fp64 uniforms u.  ``size_t`` (a one-element int64 device tensor) replaces the host
        fill level in graph-captured frames; both forms draw the same indices."""
        if size_t is None:
            if self.size == 0:
                raise ValueError("empty replay")
            size_t = torch.full((1,), self.size, dtype=torch.int64, device=self.device)
        u = torch.rand(batch, dtype=torch.float64, device=self.device, generator=generator)
        idx = (u * size_t).long()
        return torch.minimum(idx, size_t - 1)

    def sample_rows(self, idx_out: torch.Tensor, seed: int, counter_t: torch.Tensor, size_t: torch.Tensor) -> torch.Tensor:
        """Fill ``idx_out`` (int64) with rows uniform over [0, size) with replacement, from the
        Philox REPLAY stream of (seed, row, *counter_t) (pbn_replay_advance; counter_t advances):
        one launch, graph-capturable, and the same rows eager or captured."""
        self.advance(0, None, size_t, None, None, None, 0.0, 0.0, seed, counter_t, idx_out)
        return idx_out

    def advance(self, n_store: int, pos_t, size_t, step_t, eps64, eps32, eps_floor: float, eps_step: float, seed: int,
                counter_t=None, idx_out=None) -> None:
        """pbn_replay_advance, one launch on one-element device tensors (None: left alone): the ring
        position and fill level move on by ``n_store`` rows, ``*step_t`` by one, epsilon (a double
        and its float copy) down by ``eps_step`` to ``eps_floor``; then ``idx_out``, if given, is
        filled as ``sample_rows`` describes, over the new fill level."""
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pbn_replay_advance(
                n_store, self.capacity, ptr(pos_t), ptr(size_t), ptr(step_t), ptr(eps64), ptr(eps32), eps_floor,
                eps_step, 0 if idx_out is None else idx_out.numel(), seed, ptr(counter_t), ptr(idx_out),
                torch.cuda.current_stream(self.device).cuda_stream), "pbn_replay_advance")

    def gather(self, idx: torch.Tensor, net_handle, stream=None) -> Dict[str, torch.Tensor]:
        """Rows ``idx`` (B a multiple of 32) as network inputs, in one launch (``pbn_replay_batch``):
        x fp32 (2, 2B, N) = obs and next_obs concatenated by rows (obs / next_obs are its halves:
        state or next state, and the target attractor's first state), actions (B, K, 1) int64,
        rewards (B, 1), masks (B, 1)."""
        B = idx.shape[0]
        if B % 32:
            raise ValueError("batch size must be a multiple of 32")
        N = net_handle.spec.n
        K = self.action.shape[1]
        dev = self.device
        x = torch.empty(2, 2 * B, N, dtype=torch.float32, device=dev)
        actions = torch.empty(B, K, dtype=torch.int64, device=dev)
        rewards = torch.empty(B, dtype=torch.float32, device=dev)
        masks = torch.empty(B, dtype=torch.float32, device=dev)
        idx = idx.to(torch.int64).contiguous()
        L = _lib.load()
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            _lib.check(L.pbn_replay_batch(net_handle.handle, B, idx.data_ptr(), self.capacity, self.state.data_ptr(),
                                          self.next_state.data_ptr(), self.target.data_ptr(), self.action.data_ptr(),
                                          K, self.reward.data_ptr(), self.done.data_ptr(), x.data_ptr(),
                                          actions.data_ptr(), rewards.data_ptr(), masks.data_ptr(), s),
                       "pbn_replay_batch")
        return {"x": x, "obs": x[:, :B], "next_obs": x[:, B:], "actions": actions.unsqueeze(-1),
                "rewards": rewards.reshape(-1, 1), "masks": masks.reshape(-1, 1)}


class PrioritisedDeviceReplay(DeviceReplay):
    """DeviceReplay with the reference's proportional priorities (PrioritisedER,
    bdq_model/memory.py:73-186) in two device segment trees of ``tree_size`` leaves (the smallest
    power of two >= capacity; double [2 * tree_size], node 1 the root, leaf i at tree_size + i):
    ``sum_tree`` and ``min_tree``, plus ``max_priority`` (a one-element double, 1.0 at first).  GPU
    only.  The law, quirks included (DESIGN.md "Prioritised replay"):

    * ``store`` / ``store_at`` give the n new transitions the priority ``max_priority ** alpha``,
      written at the slot AFTER each stored row (memory.py:114);
    * ``sample(batch)`` draws ``batch`` (<= 1024) rows proportional to priority, one per stratum of
      the total over leaves [0, size - 2], with the uniforms of the REPLAY Philox stream (seed, row,
      draw counter), and returns the rows and their float32 importance weights
      ``(N p_i) ** -beta / (N p_min) ** -beta``;
    * beta lives on the device (``beta_t``; ``beta`` is the host's mirror) and every sample moves
      it to ``min(max_beta, beta + beta_step)`` after reading it.  The reference's agent does this
      once per env step (increment_beta, ddqn_per/__init__.py:488-523); here it happens once per
      sample, so ``beta_step`` is per update;
    * ``update_priorities(idx, priorities)`` sets leaf idx[b] to ``priorities[b] ** alpha`` (of equal
      indices the highest b wins, as the reference's in-order loop has it), raises ``max_priority``
      to the largest priority seen, and skips indices outside [0, size).

    Every launch reads its counters from device memory, so all of it can be graph-captured."""

    def __init__(self, capacity: int, words: int, branches: int, device, *, alpha: float = 0.6, beta: float = 0.4,
                 max_beta: float = 1.0, beta_step: float = 0.0, seed: int = 0):
        if torch.device(device).type != "cuda":
            raise ValueError("PrioritisedDeviceReplay runs on the GPU")
        if capacity < 2:
            raise ValueError("capacity must be >= 2")
        if not beta > 0:
            raise ValueError("beta must be > 0")
        super().__init__(capacity, words, branches, device)
        dev = self.device
        self.alpha = float(alpha)
        self.tree_size = 1 << (self.capacity - 1).bit_length()
        self.sum_tree = torch.zeros(2 * self.tree_size, dtype=torch.float64, device=dev)
        self.min_tree = torch.full((2 * self.tree_size,), float("inf"), dtype=torch.float64, device=dev)
        self.max_priority = torch.ones(1, dtype=torch.float64, device=dev)
        self.beta, self.max_beta, self.beta_step = float(beta), float(max_beta), float(beta_step)
        self.beta_t = torch.full((1,), self.beta, dtype=torch.float64, device=dev)
        self.seed = int(seed)
        self.counter_t = torch.zeros(1, dtype=torch.int64, device=dev)

    _STATE_TENSORS = DeviceReplay._STATE_TENSORS + ("sum_tree", "min_tree", "max_priority", "counter_t")

    def state_dict(self) -> dict:
        """DeviceReplay's, the two trees whole (float64), ``max_priority``, the draw counter and the
        host's ``beta``.  ``beta_t`` is not saved: the learner sets it from its host beta by its mode."""
        out = super().state_dict()
        out["beta"] = float(self.beta)
        return out

    def load_state_dict(self, sd: dict) -> None:
        super().load_state_dict(sd)
        self.beta = float(sd["beta"])

    def _i64(self, v: int) -> torch.Tensor:
        return torch.full((1,), v, dtype=torch.int64, device=self.device)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def clear(self) -> None:
        """Empty the ring and the trees; max_priority back to 1 (PrioritisedER.clear)."""
        self.pos = self.size = 0
        self.sum_tree.zero_()
        self.min_tree.fill_(float("inf"))
        self.max_priority.fill_(1.0)

    def store_priorities(self, n: int, pos_t: torch.Tensor) -> None:
        """The priorities of n transitions stored at ring position ``*pos_t`` (the position before
        the store; a one-element int64 device tensor): pbn_per_store, two launches."""
        if not 1 <= n <= self.capacity:
            raise ValueError("n must be in 1..capacity")
        L = _lib.load()
        with torch.cuda.device(self.device):
            _lib.check(L.pbn_per_store(n, pos_t.data_ptr(), self.capacity, self.tree_size, self.alpha,
                                       self.max_priority.data_ptr(), self.sum_tree.data_ptr(),
                                       self.min_tree.data_ptr(), self._stream()), "pbn_per_store")

    def store(self, state, target, action, reward, next_state, done) -> None:
        self.store_priorities(target.shape[0], self._i64(self.pos))
        super().store(state, target, action, reward, next_state, done)

    def store_at(self, pos_t, size_t, state, target, *args, **kwargs) -> None:
        self.store_priorities(target.shape[0], pos_t)       # (reads the position before it advances)
        super().store_at(pos_t, size_t, state, target, *args, **kwargs)

    def mirror_beta(self) -> None:
        """The host's copy of beta after one sample (what a replayed graph's sample did)."""
        self.beta = min(self.max_beta, self.beta + self.beta_step)

    def sample(self, batch: int, size_t: Optional[torch.Tensor] = None):
        """(rows int64 [batch], importance weights float32 [batch]): pbn_per_sample, one launch.
        ``size_t`` (a one-element int64 device tensor) replaces the host fill level in
        graph-captured frames."""
        if not 1 <= batch <= 1024:
            raise ValueError("batch must be in 1..1024")
        if size_t is None:
            if self.size < 2:
                raise ValueError("prioritised sampling needs at least two stored transitions")
            size_t = self._i64(self.size)
        idx = torch.empty(batch, dtype=torch.int64, device=self.device)
        weights = torch.empty(batch, dtype=torch.float32, device=self.device)
        L = _lib.load()
        with torch.cuda.device(self.device):
            _lib.check(L.pbn_per_sample(batch, self.capacity, self.tree_size, size_t.data_ptr(),
                                        self.sum_tree.data_ptr(), self.min_tree.data_ptr(), self.beta_t.data_ptr(),
                                        self.max_beta, self.beta_step, self.seed, self.counter_t.data_ptr(),
                                        idx.data_ptr(), weights.data_ptr(), self._stream()), "pbn_per_sample")
        if not torch.cuda.is_current_stream_capturing():
            self.mirror_beta()
        return idx, weights

    def update_priorities(self, idx: torch.Tensor, priorities: torch.Tensor,
                          size_t: Optional[torch.Tensor] = None) -> None:
        """pbn_per_update on (idx int64 [B], priorities float32 [B]), B <= 1024: one launch."""
        if idx.dtype != torch.int64 or priorities.dtype != torch.float32 or idx.dim() != 1 or \
                idx.shape != priorities.shape or not 1 <= idx.shape[0] <= 1024:
            raise ValueError("idx int64 [B] and priorities float32 [B], B in 1..1024")
        if not idx.is_cuda or not priorities.is_cuda:
            raise ValueError("idx and priorities must be GPU tensors")
        if size_t is None:
            size_t = self._i64(self.size)
        idx, priorities = idx.contiguous(), priorities.contiguous()
        L = _lib.load()
        with torch.cuda.device(self.device):
            _lib.check(L.pbn_per_update(idx.shape[0], self.capacity, self.tree_size, self.alpha, size_t.data_ptr(),
                                        idx.data_ptr(), priorities.data_ptr(), self.max_priority.data_ptr(),
                                        self.sum_tree.data_ptr(), self.min_tree.data_ptr(), self._stream()),
                       "pbn_per_update")


@torch.no_grad()
def soft_update(target: torch.nn.Module, online: torch.nn.Module) -> None:
    """target <- target / 2 + online / 2, parameter by parameter (bdq_model/__init__.py:137-139)."""
    for (kt, t), (ko, o) in zip(target.state_dict().items(), online.state_dict().items()):
        t.div_(2).add_(o / 2)


class _TDLoss(torch.autograd.Function):
    """pbn_bdq_td_loss: the TD loss of bdq_update on raw head outputs and its gradient in one HIP
    launch (forward computes both; backward scales the stored gradient)."""

    @staticmethod
    def forward(ctx, online, target_heads, actions, rewards, masks, gamma):
        H, rows, A = online.shape
        B = rows // 2
        loss = torch.empty(1, dtype=torch.float32, device=online.device)
        grad = torch.empty_like(online)
        scratch = torch.empty((B + 7) // 8, dtype=torch.float32, device=online.device)
        L = _lib.load()
        with torch.cuda.device(online.device):
            _lib.check(L.pbn_bdq_td_loss(online.data_ptr(), target_heads.data_ptr(), actions.data_ptr(),
                                         rewards.data_ptr(), masks.data_ptr(), B, H - 1, A, float(gamma),
                                         loss.data_ptr(), grad.data_ptr(), scratch.data_ptr(),
                                         torch.cuda.current_stream(online.device).cuda_stream), "pbn_bdq_td_loss")
        ctx.save_for_backward(grad)
        return loss[0]

    @staticmethod
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        return grad * grad_out, None, None, None, None, None


class _TDLossPER(torch.autograd.Function):
    """pbn_bdq_td_loss_per: _TDLoss with per-row importance weights in and priorities out."""

    @staticmethod
    def forward(ctx, online, target_heads, actions, rewards, masks, weights, gamma, replay_constant, priorities_out):
        H, rows, A = online.shape
        B = rows // 2
        loss = torch.empty(1, dtype=torch.float32, device=online.device)
        grad = torch.empty_like(online)
        scratch = torch.empty((B + 7) // 8, dtype=torch.float32, device=online.device)
        L = _lib.load()
        with torch.cuda.device(online.device):
            _lib.check(L.pbn_bdq_td_loss_per(online.data_ptr(), target_heads.data_ptr(), actions.data_ptr(),
                                             rewards.data_ptr(), masks.data_ptr(), weights.data_ptr(), B, H - 1, A,
                                             float(gamma), float(replay_constant), loss.data_ptr(), grad.data_ptr(),
                                             priorities_out.data_ptr(), scratch.data_ptr(),
                                             torch.cuda.current_stream(online.device).cuda_stream),
                       "pbn_bdq_td_loss_per")
        ctx.save_for_backward(grad)
        return loss[0]

    @staticmethod
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        return (grad * grad_out,) + (None,) * 8


def bdq_update(q: torch.nn.Module, target: torch.nn.Module, opt: torch.optim.Optimizer, batch: Dict[str, torch.Tensor],
               gamma: float = 0.999, grad_clamp: float = 1.0, target_weights=None, weights: Optional[torch.Tensor] = None,
               priorities_out: Optional[torch.Tensor] = None, replay_constant: float = 1e-5) -> torch.Tensor:
    """One update_policy step (bdq_model/__init__.py:111-131) on a gathered batch; returns the loss.
    On the GPU the duelings, the double-DQN target, the MSE and their backward run as one HIP
    launch on the raw head outputs (``pbn_bdq_td_loss``); elsewhere (CPU tensors) as PyTorch
    expressions.  ``target_weights``: the target network's ``head_weights()`` computed beforehand
    (it changes only at soft updates).

    ``weights`` (float32 [B]; prioritised replay's importance weights): the update of
    DDQNPER._learn_step (ddqn_per/__init__.py:468-483) with this MSE: l_b = mean_k (y_bk - q_bk)^2,
    loss = mean_b w_b l_b, and ``priorities_out`` (float32 [B], optional) receives
    |w_b l_b| + ``replay_constant``.  On the GPU this is ``pbn_bdq_td_loss_per``."""
    if weights is None and priorities_out is not None:
        raise ValueError("priorities_out needs weights")
    if weights is not None:
        if weights.dtype != torch.float32 or weights.numel() != batch["obs"].shape[1]:
            raise ValueError("weights must be float32 [B]")
        if priorities_out is not None and (priorities_out.dtype != torch.float32 or priorities_out.shape != (weights.numel(),)
                                           or not priorities_out.is_contiguous()):
            raise ValueError("priorities_out must be a contiguous float32 [B]")
    # q(obs) and q(next_obs) as one forward over 2B rows (half the launches; only the first
    # half carries gradient)
    B = batch["obs"].shape[1]
    x = batch["x"] if "x" in batch else torch.cat([batch["obs"], batch["next_obs"]], 1)
    if x.is_cuda and isinstance(q, BranchingQNetwork) and isinstance(target, BranchingQNetwork):
        heads = q.forward_heads(q.model[0](x))                          # (K+1, 2B, A), raw
        with torch.no_grad():
            t_heads = target.forward_heads(target.model[0](batch["next_obs"]),
                                           weights=target_weights).contiguous()   # (K+1, B, A)
        if weights is None:
            loss = _TDLoss.apply(heads.contiguous(), t_heads, batch["actions"].reshape(B, -1).contiguous(),
                                 batch["rewards"].reshape(B).contiguous(), batch["masks"].reshape(B).contiguous(), gamma)
        else:
            if priorities_out is None:
                priorities_out = torch.empty(B, dtype=torch.float32, device=x.device)
            loss = _TDLossPER.apply(heads.contiguous(), t_heads, batch["actions"].reshape(B, -1).contiguous(),
                                    batch["rewards"].reshape(B).contiguous(), batch["masks"].reshape(B).contiguous(),
                                    weights.reshape(B).contiguous(), gamma, replay_constant, priorities_out)
    else:
        q_all = q(x)                                                    # (2B, K, A)
        current = q_all[:B].gather(2, batch["actions"]).squeeze(-1)     # (B, K)
        with torch.no_grad():
            argmax = torch.argmax(q_all[B:].detach(), dim=2)
            max_next = target(batch["next_obs"]).gather(2, argmax.unsqueeze(2)).squeeze(-1)
        expected = batch["rewards"] + max_next * gamma * batch["masks"]
        if weights is None:
            loss = F.mse_loss(expected, current)
        else:
            sq = (expected - current) ** 2                              # (B, K)
            loss = (weights.reshape(B, 1) * sq).mean()                  # = mean_b w_b l_b
            if priorities_out is not None:
                priorities_out.copy_((weights.reshape(B) * sq.detach().mean(1)).abs() + replay_constant)
    opt.zero_grad()
    loss.backward()
    grads = [p.grad for p in q.parameters() if p.grad is not None]
    torch._foreach_clamp_min_(grads, -grad_clamp)      # two multi-tensor launches, not one per tensor
    torch._foreach_clamp_max_(grads, grad_clamp)
    opt.step()
    return loss.detach()


def bdq_layout(n_nodes: int, n_branches: int) -> List[int]:
    """pbn_bdq_layout: the float offsets of the flat parameter buffer's 12 segments, then its size."""
    L = _lib.load()
    off = (ctypes.c_int64 * 13)()
    _lib.check(L.pbn_bdq_layout(n_nodes, n_branches, off), "pbn_bdq_layout")
    return list(off)


def fused_update_supported(n_nodes: int, n_branches: int, batch_size: int) -> bool:
    """Whether pbn_bdq_learn runs this shape (its workspace query accepts it): batch a multiple of
    16, n_nodes <= 127, n_branches 1..7, and the backward's LDS within one block."""
    L = _lib.load()
    nbytes = ctypes.c_int64()
    return L.pbn_bdq_learn_workspace(n_nodes, n_branches, batch_size, ctypes.byref(nbytes)) == 0


def _bdq_segments(q: BranchingQNetwork):
    """(parameter, segment, offset within the segment) in pbn_bdq_layout order."""
    m, A = q.model, q.ac_dim
    out = [(m[0].bilinear.weight, 0, 0), (m[0].bilinear.bias, 1, 0), (m[2].weight, 2, 0), (m[2].bias, 3, 0),
           (m[4].weight, 4, 0), (m[4].bias, 5, 0), (m[6].weight, 6, 0), (m[6].bias, 7, 0)]
    for h, hd in enumerate([q.value_head] + list(q.adv_heads)):
        out += [(hd[0].weight, 8, h * 64 * 32), (hd[0].bias, 9, h * 64), (hd[2].weight, 10, h * A * 64),
                (hd[2].bias, 11, h * A)]
    return out


class FusedBDQUpdate(FusedUpdate):
    """update_policy (bdq_model/__init__.py:100-139) as three HIP launches (``pbn_bdq_learn``,
    csrc/pbn_learn.hip) instead of ~100 PyTorch kernels: the online and target networks' forwards,
    the double-DQN TD loss, the backward, the gradient clamp and the Adam step.

    The buffers and their bookkeeping are FusedUpdate's (fused.py); the flat layout is
    ``pbn_bdq_layout``.  A network's image (pbn_bdq_pack) is its bilinear target table (``q_table``,
    the acting kernel's operand), then its dense weights as 16 x 16 tiles in the update kernels'
    MFMA-fragment orders.  The online image is rewritten by every update; ``pack()`` recomputes the
    images after weights change any other way (a loaded checkpoint), ``soft_update()`` moves the
    target network halfway (bdq_model/__init__.py:137-139) and repacks its image.  Adam is
    torch.optim.Adam's arithmetic, betas (0.9, 0.999), eps 1e-8."""

    def __init__(self, q: BranchingQNetwork, target: BranchingQNetwork, net, branches: int, *, batch_size: int,
                 learning_rate: float = 1e-4, gamma: float = 0.999, grad_clamp: float = 1.0,
                 betas=(0.9, 0.999), eps: float = 1e-8, keep_grad: bool = False):
        spec = net.spec
        N = spec.n
        self._require_gpu(q)
        for m in (q, target):
            if (not isinstance(m, BranchingQNetwork) or m.n != branches or m.ac_dim != N + 1
                    or m.model[0].input1_dim != N or m.model[0].input2_dim != N):
                raise ValueError("FusedBDQUpdate needs BranchingQNetwork((N, N), N + 1, branches) for both networks")
        self.K, self.grad_clamp = int(branches), float(grad_clamp)
        self.slope = float(q.model[1].negative_slope)
        self.off = bdq_layout(N, self.K)
        super().__init__(q, target, net, batch_size=batch_size, learning_rate=learning_rate, gamma=gamma, betas=betas,
                         eps=eps, keep_grad=keep_grad)
        # each image begins with the bilinear target table, which the acting kernel reads (a view)
        n_attr = len(spec.attractors)
        nt = n_attr * N * 256
        self.q_table = self.q_image[:nt].view(n_attr, N, 16, 16)
        self.t_table = self.t_image[:nt].view(n_attr, N, 16, 16)
        H, A = self.K + 1, N + 1
        o = self.off
        self._acting = (None, self.q_flat[o[1]:o[1] + 256],
                        (self.q_flat[o[8]:o[8] + H * 64 * 32].view(H * 64, 32), self.q_flat[o[9]:o[9] + H * 64],
                         self.q_flat[o[10]:o[10] + H * A * 64].view(H, A, 64),
                         self.q_flat[o[11]:o[11] + H * A].view(H, 1, A)),
                        self.q_table)

    def _sizes(self):
        L = _lib.load()
        nimg, nbytes = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(L.pbn_bdq_image_floats(self.net.handle, self.K, ctypes.byref(nimg)), "pbn_bdq_image_floats")
        _lib.check(L.pbn_bdq_learn_workspace(self.N, self.K, self.B, ctypes.byref(nbytes)), "pbn_bdq_learn_workspace")
        return self.off[12], nimg.value, nbytes.value

    def _params(self, q: BranchingQNetwork):
        return [(p, self.off[seg] + extra) for p, seg, extra in _bdq_segments(q)]

    def _pack(self, flat: torch.Tensor, image: torch.Tensor) -> None:
        _lib.check(_lib.load().pbn_bdq_pack(self.net.handle, self.K, flat.data_ptr(), image.data_ptr(), self._stream()),
                   "pbn_bdq_pack")

    def soft_update(self) -> None:
        """target <- target / 2 + online / 2 (soft_update's arithmetic, one pass over the buffer)."""
        with torch.no_grad():
            self.t_flat.div_(2).add_(self.q_flat / 2)
        self.mark_target_updated()
        self.pack("target")

    def acting_pack(self):
        """BatchedBDQ's weight-derived operands as views of the flat buffer (no assembly kernels)."""
        return self._acting

    def update(self, replay: "DeviceReplay", idx: torch.Tensor, advance=None, weights: Optional[torch.Tensor] = None,
               priorities_out: Optional[torch.Tensor] = None, replay_constant: float = 1e-5) -> torch.Tensor:
        """One update on ring rows ``idx`` (int64, ``batch_size`` of them); returns the loss buffer
        (overwritten by the next update).  ``advance``: an ``_lib.FrameAdvance`` whose counters
        the update's last launch advances (and the next frame's rows it draws; BDQLearner's
        captured frame).

        ``weights`` (float32 [B] on the device; prioritised replay's importance weights, by batch
        position): the weighted update of bdq_update, loss = mean_b w_b l_b, as the same three
        launches (``pbn_bdq_learn_per``); ``priorities_out`` (float32 [B], required with weights)
        receives |w_b l_b| + ``replay_constant`` from the backward's TD pass."""
        self._check_idx(idx)
        self.check_per_args(self.B, self.q_flat.device, weights, priorities_out)
        self.sync()
        L = _lib.load()
        b1, b2 = self.betas
        args = (self.net.handle, self.B, idx.contiguous().data_ptr(), replay.capacity,
                replay.state.data_ptr(), replay.next_state.data_ptr(), replay.target.data_ptr(),
                replay.action.data_ptr(), self.K, replay.reward.data_ptr(),
                replay.done.data_ptr(), self.q_flat.data_ptr(), self.q_image.data_ptr(),
                self.t_flat.data_ptr(), self.t_image.data_ptr(), self.m.data_ptr(),
                self.v.data_ptr(), self.step.data_ptr(), self.lr, b1, b2, self.eps, self.gamma,
                self.grad_clamp, self.slope, self.work.data_ptr(), self.work.numel() * 4,
                self.loss.data_ptr(), self.grad.data_ptr() if self.grad is not None else None)
        adv = ctypes.byref(advance) if advance is not None else None
        with torch.cuda.device(self.q_flat.device):
            if weights is None:
                _lib.check(L.pbn_bdq_learn(*args, adv, self._stream()), "pbn_bdq_learn")
            else:
                _lib.check(L.pbn_bdq_learn_per(*args, weights.data_ptr(), float(replay_constant),
                                               priorities_out.data_ptr(), adv, self._stream()), "pbn_bdq_learn_per")
        if not torch.cuda.is_current_stream_capturing():
            self.mark_updated()   # (a captured update is marked by each replay: BDQLearner._replay_frame)
        return self.loss[0]


class BDQLearner(FrameLearner):
    """BranchingDQN.learn (bdq_model/__init__.py:150-238) over a VectorPBNEnv: every frame acts
    for all envs (BatchedBDQ), appends their transitions to the device replay, and, once
    ``learning_starts`` transitions are stored, takes ``updates_per_frame`` update_policy steps.
    Exploration decays linearly from ``epsilon_start`` to ``epsilon_final`` over
    ``epsilon_decay`` frames after ``learning_starts`` (decrement_epsilon, :141-148).

    ``fused`` (default: whenever the network is the reference's BranchingQNetwork on the GPU and
    the batch is a multiple of 16) runs each update as FusedBDQUpdate's three HIP launches; the
    Adam state is then FusedBDQUpdate's and ``opt`` is None.  ``fused=False`` keeps the PyTorch
    update (bdq_update + torch.optim.Adam).

    ``prioritised=True`` (GPU only) trains from a PrioritisedDeviceReplay as DDQNPER does
    (ddqn_per/__init__.py:468-483): every update is sample -> importance-weighted update ->
    update_priorities with |w_b l_b| + ``replay_constant``.  By default (``fused=None``) the
    update is the PyTorch one (gather -> bdq_update); ``fused=True`` runs it as FusedBDQUpdate's
    three launches, the weights going into and the priorities coming out of the backward's TD
    pass (``pbn_bdq_learn_per``).  Either way every update samples for itself (a prioritised
    sample depends on the priorities the update before it wrote), so the fused prioritised
    learner does not pre-draw its rows as the fused uniform one does.  ``per_beta`` moves to
    ``per_max_beta`` in ``per_beta_steps`` equal steps, one per update; ``capture()`` works with
    it, the host mirroring beta as it mirrors epsilon.

    ``episode_stats=True`` keeps episode statistics on the device (``stats``, an EpisodeStats with
    ``log_every`` = ``stats_log_every``), tracked every frame, eager or captured.

    ``curriculum=True`` (needs ``episode_stats=True``) is the reference's ``env.rework_probas(ep_len)``
    (bdq_model/__init__.py:203): the envs a step reset restart from a (source, target) pair drawn by
    the per-pair statistics' weights (``curriculum``, a Curriculum; the table is rebuilt every
    ``curriculum_refresh`` frames), inside the frame, eager or captured."""

    def __init__(self, env: VectorPBNEnv, qnet: Optional[BranchingQNetwork] = None, *, capacity: int = 10 ** 4,
                 batch_size: int = 256, learning_rate: float = 1e-4, gamma: float = 0.999,
                 target_update: int = 10_000, learning_starts: int = 288, updates_per_frame: int = 1,
                 epsilon_start: float = 1.0, epsilon_final: float = 0.0, epsilon_decay: int = 10_000, seed: int = 0,
                 graphable: bool = False, blas: Optional[str] = "cublas", fused: Optional[bool] = None,
                 prioritised: bool = False, per_alpha: float = 0.6, per_beta: float = 0.4, per_max_beta: float = 1.0,
                 per_beta_steps: int = 10_000, replay_constant: float = 1e-5, episode_stats: bool = False,
                 stats_log_every: int = 0, curriculum: bool = False, curriculum_refresh: int = 1000):
        if prioritised:   # (arguments that cannot work: refused before the env is looked at)
            if batch_size > 1024:
                raise ValueError("prioritised replay samples at most 1024 rows per update")
            fused = bool(fused)   # (the default stays the PyTorch update)
        if fused and (not isinstance(env, VectorPBNEnv) or env.device.type != "cuda"):
            raise ValueError("fused update: needs a VectorPBNEnv on the GPU")
        if not env.keep_final_state:
            raise ValueError("BDQLearner needs the env's final_state (keep_final_state=True)")
        self.prioritised = bool(prioritised)
        self.replay_constant = float(replay_constant)
        self.env = env
        self.agent = BatchedBDQ(env, qnet)
        self.q = self.agent.q.train()
        self.target = BranchingQNetwork((env.n_nodes, env.n_nodes), env.n_nodes + 1, self.agent.branches).to(env.device)
        self.target.load_state_dict(self.q.state_dict())
        can_fuse = (env.device.type == "cuda" and self.agent.fused_tail and isinstance(self.q, BranchingQNetwork)
                    and fused_update_supported(env.n_nodes, self.agent.branches, batch_size))
        if fused and not can_fuse:
            raise ValueError("fused update: the reference BranchingQNetwork on a GPU env, batch a multiple of 16")
        self.fused: Optional[FusedBDQUpdate] = None
        self.opt = None
        if fused if fused is not None else can_fuse:
            self.fused = FusedBDQUpdate(self.q, self.target, env.net, self.agent.branches, batch_size=batch_size,
                                        learning_rate=learning_rate, gamma=gamma)
            self.agent.pack_provider = self.fused.acting_pack
        else:
            if blas:
                # the PyTorch update's GEMMs are small (batch 256-512, widths 28-256): rocBLAS
                # ("cublas" in torch's naming on ROCm) runs the weight-gradient products (K = batch)
                # 2.5-8x faster than hipBLASLt's picks (tools/learn_profile.py, profiles/r04_z*).
                # This sets the process-wide preference, so only this path sets it (the fused
                # update runs no GEMM); blas=None leaves it alone
                torch.backends.cuda.preferred_blas_library(blas)
            # one fused multi-tensor kernel per step instead of a handful per parameter tensor
            # capturable keeps Adam's step counts on the device (needed to replay it in a hipGraph)
            self.opt = torch.optim.Adam(self.q.parameters(), lr=learning_rate, fused=True, capturable=graphable)
        if prioritised:
            self.replay = PrioritisedDeviceReplay(
                max(capacity, env.n_alloc), env.words, self.agent.branches, env.device, alpha=per_alpha, beta=per_beta,
                max_beta=per_max_beta, beta_step=(per_max_beta - per_beta) / max(1, per_beta_steps), seed=seed)
            self._prio = torch.empty(batch_size, dtype=torch.float32, device=env.device)
        else:
            self.replay = DeviceReplay(max(capacity, env.n_alloc), env.words, self.agent.branches, env.device)
        self.batch_size, self.gamma, self.target_update = batch_size, gamma, target_update
        self.learning_starts = max(learning_starts, batch_size)
        self.updates_per_frame = updates_per_frame
        self.epsilon = epsilon_start
        self.epsilon_final = epsilon_final
        self.epsilon_step = (epsilon_start - epsilon_final) / max(1, epsilon_decay)
        self.frames = 0
        self.updates = 0
        self.gen = torch.Generator(device=env.device)
        self.gen.manual_seed(seed)
        self.seed = int(seed)
        if self.fused is not None and not self.prioritised:
            # the fused learner draws its rows from the REPLAY Philox stream (pbn_replay_advance):
            # all updates_per_frame batches of a frame in one draw, eager or captured.  (Not the
            # prioritised one: a prioritised sample depends on the priorities the update before
            # it wrote, so every update samples for itself)
            self._draw_t = torch.zeros(1, dtype=torch.int64, device=env.device)
            self._idx = torch.zeros(updates_per_frame * batch_size, dtype=torch.int64, device=env.device)
        # the host's mirror of the draw counter at a frame boundary: the draws completed frames have
        # consumed (a captured frame's last launch has already drawn the next frame's rows, so there
        # *_draw_t is one ahead of it)
        self.draws = 0
        self._loaded_at: Optional[int] = None    # ``updates`` when a checkpoint was loaded
        self.last_loss: Optional[torch.Tensor] = None
        self.graphable = graphable
        self._graph: Optional[torch.cuda.CUDAGraph] = None
        self._tw = None   # _target_weights()
        self._tw_key = None
        self._init_stats(episode_stats, stats_log_every)
        self._init_curriculum(curriculum, curriculum_refresh)

    def _target_weights(self):
        """The target network's stacked head weights (BranchingQNetwork.head_weights), held in
        fixed tensors (a captured frame reads these very tensors).  They are refreshed in place
        whenever the target's parameters changed since (soft updates, a load_state_dict: any
        in-place write bumps the parameters' versions)."""
        key = tuple(p._version for p in self.target.parameters())
        if self._tw is None:
            with torch.no_grad():
                self._tw = tuple(w.detach().clone() for w in self.target.head_weights())
        elif key != self._tw_key:
            self._refresh_target_weights()
        self._tw_key = key
        return self._tw

    def _refresh_target_weights(self) -> None:
        if self._tw is not None:
            with torch.no_grad():
                for dst, w in zip(self._tw, self.target.head_weights()):
                    dst.copy_(w)
            self._tw_key = tuple(p._version for p in self.target.parameters())

    def frame(self):
        if self._graph is not None:
            return self._replay_frame()
        env = self.env
        state = env.state.clone()
        target = env.target.clone()
        self.agent.act_q(self.epsilon)
        _, reward, flags = env.step_flipmask(use_current=True)
        done_all = (env.flags & (_lib.FLAG_TERMINATED | _lib.FLAG_TRUNCATED)) != 0
        # all n_alloc envs are stored (the padding envs of a ragged batch are real envs too)
        self.replay.store(state, target, self.agent.actions, env.reward, env.final_state, done_all)
        self._redraw_resets()
        self._track_stats()
        self._refresh_curriculum()
        done = done_all[: env.num_envs]
        self.frames += 1
        if self.replay.size >= self.learning_starts:
            self.epsilon = max(self.epsilon_final, self.epsilon - self.epsilon_step)
            if self.fused is not None and not self.prioritised:
                size_t = torch.full((1,), self.replay.size, dtype=torch.int64, device=env.device)
                self.replay.sample_rows(self._idx, self.seed, self._draw_t, size_t)
                self.draws += 1
            for u in range(self.updates_per_frame):
                if self.prioritised:
                    self.last_loss = self._update_prioritised()
                elif self.fused is not None:
                    self.last_loss = self.fused.update(self.replay, self._idx[u * self.batch_size:(u + 1) * self.batch_size])
                else:
                    self.last_loss = self._update(self.replay.sample_indices(self.batch_size, self.gen))
                self.updates += 1
                if self.updates % self.target_update == 0:
                    self._soft_update()
        return reward, done

    def refresh_weights(self) -> None:
        """Call after changing ``q`` / ``target`` weights outside frame() (e.g. loading a reference
        checkpoint, bdq_model/__init__.py:244, with load_state_dict): repacks the fused update's
        bilinear target tables, or the PyTorch path's cached target head weights.  A captured
        frame reads the same buffers, so it needs no re-capture."""
        if self.fused is not None:
            self.fused.pack()
        else:
            self._refresh_target_weights()

    def _update(self, idx: torch.Tensor) -> torch.Tensor:
        batch = self.replay.gather(idx, self.env.net)
        return bdq_update(self.q, self.target, self.opt, batch, self.gamma, target_weights=self._target_weights())

    def _update_prioritised(self, size_t: Optional[torch.Tensor] = None) -> torch.Tensor:
        """sample -> gather -> weighted update -> update_priorities (DDQNPER._learn_step)."""
        rp = self.replay
        idx, w = rp.sample(self.batch_size, size_t)
        if self.fused is not None:   # the weights into, and the priorities out of, the fused update's TD pass
            loss = self.fused.update(rp, idx, weights=w, priorities_out=self._prio,
                                     replay_constant=self.replay_constant)
        else:
            loss = bdq_update(self.q, self.target, self.opt, rp.gather(idx, self.env.net), self.gamma,
                              target_weights=self._target_weights(), weights=w, priorities_out=self._prio,
                              replay_constant=self.replay_constant)
        rp.update_priorities(idx, self._prio, size_t)
        return loss

    def _soft_update(self) -> None:
        if self.fused is not None:
            self.fused.soft_update()
        else:
            soft_update(self.target, self.q)
            self._refresh_target_weights()

    # ---- graph-captured frames -------------------------------------------------------------
    def capture(self, min_updates: int = 3) -> None:
        """Capture one whole learning frame (obs unpack, Q forward, epsilon-greedy flip masks,
        pbn_step_dev, replay store, epsilon decay, ``updates_per_frame`` update_policy steps)
        in a hipGraph; ``frame()`` replays it from then on.  The step index, epsilon, ring
        position and fill level live in device tensors the graph advances, mirrored on the
        host after every replay; target-network soft updates stay on the host (between
        replays), so ``target_update`` must be a multiple of ``updates_per_frame``.

        Frames run eagerly (on a side stream, as graph capture requires) until learning has
        started and ``min_updates`` updates have initialised Adam's state and library
        workspaces.  After capture, the env must only be stepped through ``frame()``."""
        if not self.graphable:
            raise ValueError("construct the learner with graphable=True to capture it")
        if self.target_update % self.updates_per_frame:
            raise ValueError("target_update must be a multiple of updates_per_frame")
        env = self.env
        dev = env.device
        # a loaded checkpoint that already learns runs no eager frame here; with the PyTorch update it
        # runs ``min_updates`` of them all the same: they initialise autograd's and the BLAS library's
        # workspaces in this process, which a capture cannot
        cold = self.fused is None and self._loaded_at is not None
        self._warm_up(lambda: self.replay.size >= self.learning_starts and self.updates >= min_updates
                      and not (cold and self.updates - self._loaded_at < min_updates))
        self._capture_counters(self.epsilon_final, self.epsilon_step, self.seed)
        self._done_buf = torch.zeros(env.n_alloc, dtype=torch.uint8, device=dev)
        self._capture_ring(_lib.FLAG_TERMINATED | _lib.FLAG_TRUNCATED, self._done_buf, self.agent.actions)
        self._adv = None
        if self.fused is not None and not self.prioritised:
            # the fused update's last launch advances the frame's counters and draws the next
            # frame's rows (pbn_frame_advance): the first replayed frame's rows are drawn now, over
            # the fill level its store will leave (what pbn_replay_advance drew inside the frame)
            self._adv = _lib.FrameAdvance(
                env.n_alloc, self.replay.capacity, self._pos_t.data_ptr(), self._size_t.data_ptr(),
                self._step_t.data_ptr(), self._eps64.data_ptr(), self._eps32.data_ptr(), float(self.epsilon_final),
                float(self.epsilon_step), self._idx.numel(), self.seed, self._draw_t.data_ptr(), self._idx.data_ptr())
            first = torch.full((1,), min(self.replay.size + env.n_alloc, self.replay.capacity), dtype=torch.int64,
                               device=dev)
            self.replay.sample_rows(self._idx, self.seed, self._draw_t, first)
        g = torch.cuda.CUDAGraph()
        g.register_generator_state(self.gen)
        if self.opt is not None:
            self.opt.zero_grad(set_to_none=True)
        with torch.cuda.graph(g):
            self._g_out = self._graph_body()
        self._graph = g
        # the capture recorded the frame without running it: nothing above advanced
        torch.cuda.current_stream(dev).synchronize()

    def _graph_body(self):
        env = self.env
        self.agent.act_q(step_t=self._step_t, epsilon_t=self._eps32)
        self._step_and_store()
        self._redraw_resets()
        self._track_stats()
        self._refresh_curriculum()
        # then the counters: the step index, the ring position and fill level, epsilon (and, fused,
        # the next frame's rows) advance in the update's last launch or in pbn_replay_advance.  A
        # prioritised frame, fused or not, advances them before its updates: its sample must see the
        # fill level after the frame's store, as the eager path does
        fused = self.fused is not None and not self.prioritised
        if not fused:   # (fused: the update's last launch advances them, pbn_frame_advance)
            self._advance_counters()
        loss = None
        B = self.batch_size
        U = self.updates_per_frame
        for u in range(U):
            if fused:
                loss = self.fused.update(self.replay, self._idx[u * B:(u + 1) * B],
                                         advance=self._adv if u == U - 1 else None)
            elif self.prioritised:
                loss = self._update_prioritised(self._size_t)
            else:
                loss = self._update(self.replay.sample_indices(B, self.gen, size_t=self._size_t))
        return env.reward[: env.num_envs], self._done_buf[: env.num_envs].view(torch.bool), loss

    def _replay_frame(self):
        rp = self.replay
        if self.fused is not None:
            self.fused.sync()            # weights loaded between replays: repack the tables
        else:
            self._target_weights()       # (refreshes the captured head-weight copies if stale)
        self._graph.replay()
        # the replayed update rewrote the online parameters in place (version counters: what
        # PyTorch and BatchedBDQ's eval-mode pack cache read)
        if self.fused is not None:
            self.fused.mark_updated()
        else:
            bump(self.q.parameters())
        self._mirror_frame()
        if self.prioritised:
            for _ in range(self.updates_per_frame):
                rp.mirror_beta()
        self.frames += 1
        self.updates += self.updates_per_frame
        if self._adv is not None:
            self.draws += 1
        if self.updates % self.target_update == 0:
            self._soft_update()
        reward, done, self.last_loss = self._g_out
        return reward, done

    def run(self, k: int):
        """``k`` captured frames replayed back to back (DDQNLearner.run's counterpart); returns the
        last frame's (reward, done), as ``frame()`` does.  The soft target update stays on the host
        (it falls due every ``target_update`` updates, 10,000 by default: a due test on the device
        would add a launch to every frame), so the ``k`` frames are split where one falls due: each
        segment is replayed with nothing on the host between its frames, then the host's copies
        move on by the segment's frames with ``_replay_frame``'s own arithmetic, and the soft update
        runs before the next segment."""
        if self._graph is None:
            raise ValueError("run() replays the captured frame: call capture() first")
        if k < 1:
            raise ValueError("k must be >= 1")
        rp, U, T = self.replay, self.updates_per_frame, self.target_update
        if self.fused is not None:
            self.fused.sync()            # weights loaded between replays: repack the tables
        else:
            self._target_weights()       # (refreshes the captured head-weight copies if stale)
        left = int(k)
        while left:
            # capture() made sure that T is a multiple of U, and updates moves by U a frame
            n = min(left, max(1, (T - self.updates % T) // U))
            for _ in range(n):
                self._graph.replay()
            if self.fused is not None:
                self.fused.mark_updated()
            else:
                bump(self.q.parameters())
            for _ in range(n):
                self._mirror_frame()
                if self.prioritised:
                    for _ in range(U):
                        rp.mirror_beta()
            self.frames += n
            self.updates += n * U
            if self._adv is not None:
                self.draws += n
            if self.updates % T == 0:
                self._soft_update()
            left -= n
        reward, done, self.last_loss = self._g_out
        return reward, done

    # ---- checkpoints (learner.py, checkpoint.py) ---------------------------------------------
    agent_kind = "bdq"

    def _predraws(self) -> bool:
        """The fused uniform learner: its rows come from the REPLAY Philox stream, a frame ahead
        when captured."""
        return self.fused is not None and not self.prioritised

    def _own_state(self) -> dict:
        own = {"frames": int(self.frames), "updates": int(self.updates), "epsilon": self.epsilon}
        if self._predraws():
            own["draws"] = int(self.draws)
            own["idx"] = cpu_copy(self._idx)
        return own

    def _check_loadable_captured(self, host: dict) -> None:
        if int(host["replay.size"]) < self.learning_starts:
            raise ValueError("the checkpoint was saved before learning started (fewer than learning_starts rows): "
                             "a captured frame always updates; load into a learner that is not captured yet")
        if int(host["learner.updates"]) % self.updates_per_frame:
            raise ValueError("checkpoint mismatch: updates is not a multiple of updates_per_frame")

    def _load_own_state(self, own: dict) -> None:
        self.frames, self.updates, self.epsilon = int(own["frames"]), int(own["updates"]), own["epsilon"]
        self._loaded_at = self.updates
        rp, env = self.replay, self.env
        if self.prioritised:
            rp.beta_t.fill_(rp.beta)     # (moved by every sample, eager or captured: the host's copy is it)
        if self.fused is None:
            self._refresh_target_weights()
        if not self._predraws():
            return
        self.draws = int(own["draws"])
        self._draw_t.fill_(self.draws)
        self._idx.copy_(own["idx"])
        if self._graph is None:
            return       # the eager frame draws at its start, capture() its first rows: both from draws
        if own["captured"]:
            self._draw_t.fill_(self.draws + 1)      # the saved rows are the next frame's: verbatim
        else:
            # an eager learner's rows are its last frame's: the next frame's are drawn now, over the
            # fill level that frame's store will leave (as capture() draws its first)
            first = torch.full((1,), min(rp.size + env.n_alloc, rp.capacity), dtype=torch.int64, device=env.device)
            rp.sample_rows(self._idx, self.seed, self._draw_t, first)

