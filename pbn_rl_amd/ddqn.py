"""The reference's other agent, DDQN / DDQNPER (ddqn_per/, driven by train_ddqn.py), on the device.

The reference steps one env per ``global_step`` (``DDQN.learn``, ddqn_per/__init__.py:308-403):
``predict`` runs ``DQN`` on one (state, target) pair, the env takes one int action (0 is the
no-op, :351; a > 0 flips node a - 1), the transition goes to ``ExperienceReplay`` or
``PrioritisedER`` with ``done = terminated``, and ``_learn_step`` (:275-278, :468-483) takes one
double-DQN / Huber / clip_grad_norm_ / Adam step.  Here one frame covers a whole ``VectorPBNEnv``:

    pbn_dqn_flipmask_from_state  packed state + target id -> Q -> epsilon-greedy -> action and
                                 flip-mask words, one launch                        (HIP, MFMA)
    pbn_step                     the PBN transition                                 (HIP)
    pbn_replay_store             the transitions into the device ring               (HIP)
    pbn_per_sample / _update     prioritised replay (replay.py, csrc/pbn_per.hip)   (HIP)
    pbn_ddqn_learn               _learn_step on a flat parameter buffer, 4 launches (HIP, MFMA)
    pbn_ddqn_schedule            a captured frame's beta step and due target copy   (HIP)
    pbn_rollout_dqn              n frames of the first two in one launch: the network runs inside
                                 the multi-step step kernel (BatchedDDQN.rollout)   (HIP, MFMA)

``DQN`` keeps ddqn_per/network.py's module tree and parameter names, so the ``"params"`` entry of
a reference ``ddqn_*.pt`` loads with ``load_state_dict``.  ``ddqn_update`` restates ``_get_loss`` +
``_back_propagate`` (with weights: ``DDQNPER._learn_step``) in PyTorch: the ``fused=False`` path
and what tests/golden/ddqn_update.npz pins.  ``FusedDDQNUpdate`` keeps its buffers as fused.py's
FusedUpdate does, and ``DDQNLearner``'s captured frame is built from learner.py's FrameLearner, as
the BDQ agent's are (replay.py).
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .fused import FusedUpdate
from .learner import FrameLearner
from .replay import DeviceReplay, PrioritisedDeviceReplay
from .vector_env import unpack_states

__all__ = ["DQN", "ddqn_update", "BatchedDDQN", "FusedDDQNUpdate", "ddqn_fused_supported", "DDQNLearner",
           "dqn_layout", "load_ddqn_checkpoint"]


class DQN(nn.Module):
    """ddqn_per/network.py:11-43, same parameter names: ``input`` (nn.Bilinear(N, N, net_arch[0][0])),
    ``linears.<i>`` (Linear(arch[0], arch[1]) per entry of ``net_arch``), ``output``; ReLU between.

    On the GPU the bilinear layer y[b, o] = bias[o] + sum_ij s[b, i] W[o, i, j] g[b, j] runs as
    two GEMMs (MyBilinear's contract form: T = g @ W.view(out * N, N)^T, then y = T.view(B, out, N)
    @ s); on the CPU it is ``nn.Bilinear`` itself."""

    def __init__(self, input_size: int, output_size: int, net_arch: Sequence[Tuple[int, int]]):
        super().__init__()
        net_arch = [tuple(int(x) for x in a) for a in net_arch]
        self.input = nn.Bilinear(input_size, input_size, net_arch[0][0], bias=True)
        self.linears = nn.ModuleList([nn.Linear(a[0], a[1], bias=True) for a in net_arch])
        self.output = nn.Linear(self.linears[-1].out_features, output_size, bias=True)
        self.input_size, self.output_size, self.net_arch = int(input_size), int(output_size), net_arch

    def _bilinear(self, state: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if not state.is_cuda or state.dim() < 2:
            return self.input(state, target)
        n, out = self.input_size, self.input.out_features
        s2, g2 = state.reshape(-1, n), target.reshape(-1, n)
        t = g2 @ self.input.weight.reshape(-1, n).t()                    # (B, out * N)
        y = torch.baddbmm(self.input.bias.view(1, -1, 1), t.view(-1, out, n), s2.unsqueeze(2)).squeeze(2)
        return y.reshape(*state.shape[:-1], out)

    def forward(self, state: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        x = F.relu(self._bilinear(state, target))
        for linear in self.linears:
            x = F.relu(linear(x))
        return self.output(x)


def ddqn_update(q: nn.Module, target: nn.Module, opt: torch.optim.Optimizer, batch: Dict[str, torch.Tensor],
                gamma: float, max_grad_norm: float, weights: Optional[torch.Tensor] = None,
                priorities_out: Optional[torch.Tensor] = None, replay_constant: float = 1e-5):
    """One ``_learn_step`` in PyTorch; returns (loss, total gradient norm before clipping).

    ``batch``: state, target, next_state float (B, N); action int64 (B, 1); reward, done float (B, 1).
    DDQN (ddqn_per/__init__.py:218-267): q_b = Q(s_b, g_b)[a_b], a'_b = argmax_a Q(s'_b, g_b),
    y_b = r_b + (1 - done_b) gamma Q_target(s'_b, g_b)[a'_b], loss = mean_b huber(q_b - y_b), then
    clip_grad_norm_ over all parameters and ``opt.step()``.  With ``weights`` (float32 [B];
    DDQNPER._learn_step, :468-483): l_b = w_b h_b, loss = mean_b l_b and ``priorities_out``
    (float32 [B], optional) receives |l_b| + ``replay_constant``."""
    if weights is None and priorities_out is not None:
        raise ValueError("priorities_out needs weights")
    with torch.no_grad():
        action_prime = q(batch["next_state"], batch["target"]).max(dim=1)[1].unsqueeze(1)
        target_q = batch["reward"] + (1 - batch["done"]) * gamma * target(
            batch["next_state"], batch["target"]).gather(1, action_prime)
    controller_q = q(batch["state"], batch["target"]).gather(1, batch["action"])
    if weights is None:
        loss = F.huber_loss(controller_q, target_q, reduction="mean")
    else:
        loss = F.huber_loss(controller_q, target_q, reduction="none") * weights.reshape(-1, 1)
        if priorities_out is not None:
            priorities_out.copy_(loss.detach().squeeze(1).abs() + replay_constant)
        loss = loss.mean()
    opt.zero_grad()
    loss.backward()
    norm = torch.nn.utils.clip_grad_norm_(q.parameters(), max_grad_norm)
    opt.step()
    return loss.detach(), norm.detach()


def dqn_layout(n_nodes: int, h0: int, h1: int) -> List[int]:
    """pbn_dqn_layout: the float offsets of the flat parameter buffer's 6 segments, then its size."""
    off = (ctypes.c_int64 * 7)()
    _lib.check(_lib.load().pbn_dqn_layout(n_nodes, h0, h1, off), "pbn_dqn_layout")
    return list(off)


def ddqn_fused_supported(n_nodes: int, net_arch, batch_size: int) -> bool:
    """Whether pbn_ddqn_learn runs this shape (its workspace query accepts it): one hidden Linear
    with both widths <= 64, N + 1 <= 128, a batch that is a multiple of 16 and <= 1024."""
    arch = [tuple(a) for a in net_arch]
    if len(arch) != 1 or len(arch[0]) != 2:
        return False
    h0, h1 = int(arch[0][0]), int(arch[0][1])
    nbytes = ctypes.c_int64()
    return _lib.load().pbn_ddqn_learn_workspace(int(n_nodes), h0, h1, int(batch_size), ctypes.byref(nbytes)) == 0


def _segments(q: DQN):
    """The parameters in pbn_dqn_layout's segment order."""
    lin = q.linears[0]
    return [q.input.weight, q.input.bias, lin.weight, lin.bias, q.output.weight, q.output.bias]


def _check_dqn(q: DQN, n_nodes: int) -> Tuple[int, int]:
    if not isinstance(q, DQN) or q.input_size != n_nodes or q.output_size != n_nodes + 1:
        raise ValueError("needs a DQN(N, N + 1, net_arch) for the env's N")
    if len(q.linears) != 1:
        raise ValueError("the HIP kernels run one hidden Linear (len(net_arch) == 1)")
    return int(q.linears[0].in_features), int(q.linears[0].out_features)


def _first_states(spec, device) -> torch.Tensor:
    """(256, N) float32: row t = the first state of attractor t, zeros past them (target id 255)."""
    tab = torch.zeros(256, spec.n, dtype=torch.float32)
    for t, a in enumerate(spec.attractors):
        tab[t] = torch.tensor(list(a[0]), dtype=torch.float32)
    return tab.to(device)


def _unpack(words: torch.Tensor, n_nodes: int) -> torch.Tensor:
    """Packed state words (W, B) int32 -> (B, N) float32 (bit i of word w = node 32 w + i)."""
    return unpack_states(words, n_nodes).to(torch.float32)


class BatchedDDQN:
    """DDQN.predict (ddqn_per/__init__.py:155-179) for a whole VectorPBNEnv.  ``act_q`` is one
    launch, pbn_dqn_flipmask_from_state: packed state + target id -> Q -> epsilon-greedy ->
    ``self.actions`` (int32 [n]) and ``env.flipmask``.  Epsilon-greedy follows the EXPLORE law of
    pbn_q_to_flipmask with one branch, so the actions equal that kernel's on the same Q.

    The kernel reads the network's image (pbn_dqn_pack); it is rebuilt when the parameters'
    version counters change, or supplied by a learner (``image_provider``, FusedDDQNUpdate).
    ``kernel`` (default: whenever the kernel takes the network, i.e. one hidden Linear, widths <= 64,
    N + 1 <= 128): False runs ``DQN.forward`` on pbn_obs_unpack's observation and pbn_q_to_flipmask
    instead (the PyTorch path, also the baseline of tools/ddqn_bench.py); True with another network
    is an error.  An env that is not on the GPU (a test stub) acts in PyTorch."""

    def __init__(self, env, dqn: Optional[DQN] = None, *, net_arch=((50, 50),), epsilon: float = 0.0,
                 kernel: Optional[bool] = None, generator: Optional[torch.Generator] = None):
        self.env = env
        N = env.n_nodes
        self.q = dqn if dqn is not None else DQN(N, N + 1, list(net_arch))
        self.q = self.q.to(env.device)
        if self.q.input_size != N or self.q.output_size != N + 1:
            raise ValueError("needs a DQN(N, N + 1, net_arch) for the env's N")
        self.epsilon = float(epsilon)
        self.on_gpu = torch.device(env.device).type == "cuda"
        supported = self.on_gpu and len(self.q.linears) == 1 and ddqn_fused_supported(N, self.q.net_arch, 16)
        if kernel and not supported:
            raise ValueError("the acting kernel needs a GPU env and one hidden Linear, widths <= 64, N + 1 <= 128")
        self.kernel = supported if kernel is None else bool(kernel)
        n = env.n_alloc
        self.actions = torch.zeros(n, dtype=torch.int32, device=env.device)
        self.qbuf = torch.empty(n, N + 1, dtype=torch.float32, device=env.device)
        self.first = _first_states(env.spec, env.device)
        self.image_provider = None
        self.gen = generator
        self._key = None
        if self.kernel:
            self.h0, self.h1 = _check_dqn(self.q, N)
            self.off = dqn_layout(N, self.h0, self.h1)
            self._flat = torch.zeros(self.off[6], dtype=torch.float32, device=env.device)
            nimg = ctypes.c_int64()
            _lib.check(_lib.load().pbn_dqn_image_floats(env.net.handle, self.h0, self.h1, ctypes.byref(nimg)),
                       "pbn_dqn_image_floats")
            self._image = torch.zeros(nimg.value, dtype=torch.float32, device=env.device)
        elif self.on_gpu:
            self.obs = torch.empty(2, n, N, dtype=torch.float32, device=env.device)

    def image(self) -> torch.Tensor:
        """The network image the acting kernel reads, up to date with the parameters."""
        if self.image_provider is not None:
            return self.image_provider()
        params = _segments(self.q)
        key = tuple((p.data_ptr(), p._version) for p in params)
        if key != self._key:
            with torch.no_grad():
                for p, at in zip(params, self.off):
                    self._flat[at:at + p.numel()].copy_(p.detach().reshape(-1))
            env = self.env
            with torch.cuda.device(env.device):
                _lib.check(_lib.load().pbn_dqn_pack(env.net.handle, self.h0, self.h1, self._flat.data_ptr(),
                                                    self._image.data_ptr(), env._stream()), "pbn_dqn_pack")
            self._key = key
        return self._image

    def observe(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(state, target) float32 (n, N) each: the envs' states and their targets' first states."""
        env = self.env
        if not self.on_gpu or self.kernel:
            return _unpack(env.state, env.n_nodes), self.first[env.target.long()]
        with torch.cuda.device(env.device):
            _lib.check(_lib.load().pbn_obs_unpack(env.net.handle, env.n_alloc, env.state.data_ptr(),
                                                  env.target.data_ptr(), self.obs.data_ptr(), env._stream()),
                       "pbn_obs_unpack")
        return self.obs[0], self.obs[1]

    def _launch(self, eps: float, step_t, epsilon_t, q_out) -> None:
        env = self.env
        image = self.image()
        with torch.cuda.device(env.device):
            _lib.check(_lib.load().pbn_dqn_flipmask_from_state(
                env.net.handle, env.seed, env.step_index, step_t.data_ptr() if step_t is not None else None,
                env.env_offset, env.n_alloc, env.state.data_ptr(), env.target.data_ptr(), self.h0, self.h1,
                image.data_ptr(), eps, epsilon_t.data_ptr() if epsilon_t is not None else None,
                q_out.data_ptr() if q_out is not None else None, env.flipmask.data_ptr(), self.actions.data_ptr(),
                env._stream()), "pbn_dqn_flipmask_from_state")

    @torch.no_grad()
    def q_values(self) -> torch.Tensor:
        """Q (n, N + 1) of every env's (state, target); with the kernel, its own Q output (the
        launch also rewrites ``actions`` and ``env.flipmask`` at the agent's epsilon)."""
        if self.kernel:
            self._launch(self.epsilon, None, None, self.qbuf)
            return self.qbuf
        s, g = self.observe()
        return self.q(s, g)

    @torch.no_grad()
    def act_q(self, epsilon: Optional[float] = None, step_t: Optional[torch.Tensor] = None,
              epsilon_t: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Epsilon-greedy actions of every env at the env's next step index -> ``env.flipmask`` and
        ``self.actions``.  ``step_t`` / ``epsilon_t``: optional one-element device tensors (int64 /
        float32) read when the kernel runs (graph replays)."""
        if step_t is not None and (step_t.dtype != torch.int64 or step_t.numel() != 1):
            raise ValueError("step_t must be a one-element int64 tensor")
        if epsilon_t is not None and (epsilon_t.dtype != torch.float32 or epsilon_t.numel() != 1):
            raise ValueError("epsilon_t must be a one-element float32 tensor")
        env = self.env
        eps = self.epsilon if epsilon is None else float(epsilon)
        if self.kernel:
            self._launch(eps, step_t, epsilon_t, None)
            return env.flipmask
        q = self.q_values().contiguous()
        if self.on_gpu:
            L = _lib.load()
            with torch.cuda.device(env.device):
                if step_t is None:
                    _lib.check(L.pbn_q_to_flipmask(env.net.handle, env.seed, env.step_index, env.env_offset,
                                                   env.n_alloc, 1, env.n_nodes + 1, q.data_ptr(), eps,
                                                   env.flipmask.data_ptr(), self.actions.data_ptr(), env._stream()),
                               "pbn_q_to_flipmask")
                else:
                    _lib.check(L.pbn_q_to_flipmask_dev(env.net.handle, env.seed, step_t.data_ptr(), env.env_offset,
                                                       env.n_alloc, 1, env.n_nodes + 1, q.data_ptr(), eps,
                                                       epsilon_t.data_ptr() if epsilon_t is not None else None,
                                                       env.flipmask.data_ptr(), self.actions.data_ptr(),
                                                       env._stream()), "pbn_q_to_flipmask_dev")
            return env.flipmask
        # no GPU (a stub env): torch's generator explores
        n, A = q.shape
        explore = torch.rand(n, generator=self.gen) < eps
        rand = torch.randint(0, A, (n,), generator=self.gen)
        a = torch.where(explore, rand, q.argmax(1)).to(torch.int32)
        self.actions.copy_(a)
        node = (a - 1).clamp(min=0)
        words = torch.arange(env.words, dtype=torch.int32).unsqueeze(1)
        bit = torch.ones_like(node) << (node & 31)
        env.flipmask.copy_(torch.where((a > 0).unsqueeze(0) & ((node >> 5).unsqueeze(0) == words), bit.unsqueeze(0),
                                       torch.zeros_like(bit).unsqueeze(0)))
        return env.flipmask

    @torch.no_grad()
    def step(self, epsilon: Optional[float] = None):
        """One frame for every env; returns (state', reward, flags) views as VectorPBNEnv.step_flipmask."""
        self.act_q(epsilon)
        return self.env.step_flipmask(use_current=True)

    @torch.no_grad()
    def rollout(self, n_steps: int, epsilon: Optional[float] = None, *, keep_obs: bool = False,
                keep_final: bool = True, keep_updates: bool = False, out: Optional[dict] = None) -> dict:
        """``n_steps`` frames of ``step()`` in one ``pbn_rollout_dqn`` launch: the wave that owns an
        env runs the network on its state and target before every step, so the state never leaves
        the chip.  Returns ``VectorPBNEnv.rollout``'s dict plus ``"actions"`` (int32 (n_steps,
        n_alloc)); every entry equals what ``n_steps`` calls of ``act_q`` + ``step_flipmask`` give,
        bit for bit.  The network is the agent's current image; ``env.step_index`` advances by
        ``n_steps``.  Pass ``out`` (a previous result) to reuse its buffers."""
        if not self.kernel:
            raise ValueError("rollout runs the policy inside the step kernel, which takes a GPU env and a DQN with "
                             "one hidden Linear, widths <= 64, N + 1 <= 128 (kernel=True)")
        env = self.env
        n_steps = int(n_steps)
        if out is None or out["_n_steps"] != n_steps or out.get("actions") is None:
            out = env.rollout_buffers(n_steps, keep_obs, keep_final, keep_updates, keep_actions=True)
        eps = self.epsilon if epsilon is None else float(epsilon)
        image = self.image()
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        with torch.cuda.device(env.device):
            _lib.check(_lib.load().pbn_rollout_dqn(
                env.net.handle, env.seed, env.step_index, env.env_offset, env.n_alloc, n_steps,
                _lib.MODE_AUTORESET if env.autoreset else 0, env.state.data_ptr(), env.target.data_ptr(),
                env.t.data_ptr(), self.h0, self.h1, image.data_ptr(), eps, out["flipmask"].data_ptr(),
                out["actions"].data_ptr(), ptr(out["obs"]), ptr(out["final_state"]), out["reward"].data_ptr(),
                out["flags"].data_ptr(), ptr(out.get("updates")), env._stream()), "pbn_rollout_dqn")
        env.step_index += n_steps
        return out


class FusedDDQNUpdate(FusedUpdate):
    """``_learn_step`` (ddqn_per/__init__.py:275-278, :468-483) as pbn_ddqn_learn's four HIP launches
    instead of PyTorch's forward / autograd / clip / Adam kernels.

    The buffers and their bookkeeping are FusedUpdate's (fused.py); the flat layout is
    ``pbn_dqn_layout``.  A network's image (pbn_dqn_pack) is the bilinear layer contracted with every
    attractor's first state, the padded biases and the dense weights as MFMA-fragment tiles.  Every
    update rewrites the online image; ``pack()`` rebuilds the images after weights change any other
    way (a loaded checkpoint); ``sync_target()`` is the hard target copy (:286-287), parameters and
    image, device to device.  Adam is torch.optim.Adam's arithmetic."""

    def __init__(self, q: DQN, target: DQN, net, *, batch_size: int, learning_rate: float = 1e-4,
                 gamma: float = 0.95, max_grad_norm: float = 10.0, betas=(0.9, 0.999), eps: float = 1e-8,
                 keep_grad: bool = False):
        N = net.spec.n
        self._require_gpu(q)
        self.h0, self.h1 = _check_dqn(q, N)
        if _check_dqn(target, N) != (self.h0, self.h1):
            raise ValueError("the target network must have the online network's shape")
        if not ddqn_fused_supported(N, [(self.h0, self.h1)], batch_size):
            raise ValueError("pbn_ddqn_learn: one hidden Linear, widths <= 64, N + 1 <= 128, batch a multiple "
                             "of 16 and <= 1024")
        self.max_grad_norm = float(max_grad_norm)
        self.off = dqn_layout(N, self.h0, self.h1)
        super().__init__(q, target, net, batch_size=batch_size, learning_rate=learning_rate, gamma=gamma, betas=betas,
                         eps=eps, keep_grad=keep_grad)
        self.grad_norm = torch.zeros(1, dtype=torch.float32, device=self.q_flat.device)

    _STATE_TENSORS = FusedUpdate._STATE_TENSORS + ("grad_norm",)

    def _sizes(self):
        L = _lib.load()
        nimg, nbytes = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(L.pbn_dqn_image_floats(self.net.handle, self.h0, self.h1, ctypes.byref(nimg)), "pbn_dqn_image_floats")
        _lib.check(L.pbn_ddqn_learn_workspace(self.N, self.h0, self.h1, self.B, ctypes.byref(nbytes)),
                   "pbn_ddqn_learn_workspace")
        return self.off[6], nimg.value, nbytes.value

    def _params(self, q: DQN):
        return list(zip(_segments(q), self.off))

    def _pack(self, flat: torch.Tensor, image: torch.Tensor) -> None:
        _lib.check(_lib.load().pbn_dqn_pack(self.net.handle, self.h0, self.h1, flat.data_ptr(), image.data_ptr(),
                                            self._stream()), "pbn_dqn_pack")

    def sync_target(self) -> None:
        """target <- online (``self.target.load_state_dict(self.controller.state_dict())``,
        ddqn_per/__init__.py:286-287): the parameters and the image, two pbn_copy_async launches."""
        self.sync()
        L = _lib.load()
        with torch.cuda.device(self.q_flat.device):
            _lib.check(L.pbn_copy_async(self.t_flat.data_ptr(), self.q_flat.data_ptr(), self.q_flat.numel() * 4,
                                        self._stream()), "pbn_copy_async")
            _lib.check(L.pbn_copy_async(self.t_image.data_ptr(), self.q_image.data_ptr(), self.q_image.numel() * 4,
                                        self._stream()), "pbn_copy_async")
        self.mark_target_updated()

    def acting_image(self) -> torch.Tensor:
        """BatchedDDQN's image provider: the online image, repacked first if the weights were
        changed outside update()."""
        self.sync()
        return self.q_image

    def update(self, replay: DeviceReplay, idx: torch.Tensor, weights: Optional[torch.Tensor] = None,
               priorities_out: Optional[torch.Tensor] = None, replay_constant: float = 1e-5) -> torch.Tensor:
        """One update on ring rows ``idx`` (int64, ``batch_size`` of them); returns the loss buffer's
        element (overwritten by the next update; ``grad_norm`` holds the total norm before
        clipping).  ``weights`` / ``priorities_out`` (float32 [B] on the device, both or neither):
        DDQNPER's importance weights by batch position in, |w_b h_b| + ``replay_constant`` out."""
        self._check_idx(idx)
        if replay.action.shape[1] != 1:
            raise ValueError("the replay ring must hold one action per transition")
        self.check_per_args(self.B, self.q_flat.device, weights, priorities_out)
        self.sync()
        b1, b2 = self.betas
        with torch.cuda.device(self.q_flat.device):
            _lib.check(_lib.load().pbn_ddqn_learn(
                self.net.handle, self.h0, self.h1, self.B, idx.contiguous().data_ptr(), replay.capacity,
                replay.state.data_ptr(), replay.next_state.data_ptr(), replay.target.data_ptr(),
                replay.action.data_ptr(), replay.reward.data_ptr(), replay.done.data_ptr(), self.q_flat.data_ptr(),
                self.q_image.data_ptr(), self.t_image.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                self.step.data_ptr(), self.lr, b1, b2, self.eps, self.gamma, self.max_grad_norm,
                self.work.data_ptr(), self.work.numel() * 4, self.loss.data_ptr(), self.grad_norm.data_ptr(),
                self.grad.data_ptr() if self.grad is not None else None,
                weights.data_ptr() if weights is not None else None, float(replay_constant),
                priorities_out.data_ptr() if priorities_out is not None else None, self._stream()), "pbn_ddqn_learn")
        if not torch.cuda.is_current_stream_capturing():
            self.mark_updated()
        return self.loss[0]


class DDQNLearner(FrameLearner):
    """``DDQN.learn`` / ``DDQNPER`` (ddqn_per/__init__.py:308-403, :431-539) over a VectorPBNEnv; the
    defaults are train_ddqn.py's.  One ``frame()`` is one reference ``global_step`` for every env:
    act at the current epsilon, step, store all ``n_alloc`` transitions with ``done`` = TERMINATED
    only (:380-389), one ``_learn_step`` if ``frames > learning_starts``, ``frame % train_frequency
    == 0`` and the ring holds ``batch_size`` rows, then the schedules of ``_schedule_step``
    (:283-290, :488-490): epsilon down by (max - min) / (exploration_fraction total_frames) to
    ``min_epsilon``, the hard target copy when ``(frame + 1) % target_update == 0``, and beta up by
    (max_beta - beta) / (beta_fraction total_frames) to 1 -- every frame, learning or not, so the
    sample of frame f uses the reference's BETA at that global_step.

    ``prioritised=True`` (GPU only): every update is PrioritisedDeviceReplay.sample -> the update
    with importance weights -> update_priorities with |w_b h_b| + ``replay_constant``.
    ``fused`` (default: when ``ddqn_fused_supported`` and the env is on the GPU) runs acting and the
    update as the HIP launches of csrc/pbn_ddqn.hip; ``fused=False`` acts through ``DQN.forward``
    and updates with ``ddqn_update`` + torch.optim.Adam.

    ``graphable=True`` allows ``capture()``: the fused, prioritised frame (``train_frequency`` 1) as
    one hipGraph, every counter and both schedules in device memory, the target copy decided on the
    device (pbn_ddqn_schedule).  ``frame()`` then replays it, and ``run(k)`` replays it ``k`` times
    with no host work between the replays.  Without ``capture()`` the frames are the eager ones.

    ``episode_stats=True`` keeps episode statistics on the device (``stats``, an EpisodeStats with
    ``log_every`` = ``stats_log_every``), tracked every frame, eager or captured: after ``run(k)``,
    ``stats.series()`` holds the windows that elapsed inside the replays.

    ``curriculum=True`` (needs ``episode_stats=True``) is the reference's ``env.rework_probas``: the envs
    a step reset restart from a (source, target) pair drawn by the per-pair statistics' weights
    (``curriculum``, a Curriculum; the table is rebuilt every ``curriculum_refresh`` frames), inside
    the frame, eager or captured."""

    def __init__(self, env, dqn: Optional[DQN] = None, *, net_arch=((50, 50),), total_frames: int,
                 capacity: int, batch_size: int = 64, target_update: int = 512, gamma: float = 0.95,
                 max_epsilon: float = 1.0, min_epsilon: float = 0.05, exploration_fraction: float = 0.1,
                 learning_rate: float = 1e-4, max_grad_norm: float = 10.0, learning_starts: int = 0,
                 train_frequency: int = 1, prioritised: bool = True, per_alpha: float = 0.6, per_beta: float = 0.4,
                 per_max_beta: float = 1.0, beta_fraction: float = 0.75, replay_constant: float = 1e-5,
                 fused: Optional[bool] = None, seed: int = 0, graphable: bool = False,
                 episode_stats: bool = False, stats_log_every: int = 0, curriculum: bool = False,
                 curriculum_refresh: int = 1000):
        dev = torch.device(env.device)
        on_gpu = dev.type == "cuda"
        if prioritised and not on_gpu:
            raise ValueError("prioritised replay runs on the GPU")
        if prioritised and batch_size > 1024:
            raise ValueError("prioritised replay samples at most 1024 rows per update")
        if not env.keep_final_state:
            raise ValueError("DDQNLearner needs the env's final_state (keep_final_state=True)")
        N = env.n_nodes
        self.env = env
        q = dqn if dqn is not None else DQN(N, N + 1, list(net_arch))
        can_fuse = on_gpu and len(q.linears) == 1 and ddqn_fused_supported(N, q.net_arch, batch_size)
        if fused and not can_fuse:
            raise ValueError("fused update: a GPU env and a shape ddqn_fused_supported accepts")
        use_fused = can_fuse if fused is None else bool(fused)
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(seed)
        self.seed = int(seed)
        self.agent = BatchedDDQN(env, q, kernel=use_fused, generator=self.gen)
        self.q = self.agent.q.train()
        self.target = DQN(N, N + 1, self.q.net_arch).to(dev)
        self.target.load_state_dict(self.q.state_dict())
        self.fused: Optional[FusedDDQNUpdate] = None
        self.opt = None
        if use_fused:
            self.fused = FusedDDQNUpdate(self.q, self.target, env.net, batch_size=batch_size,
                                         learning_rate=learning_rate, gamma=gamma, max_grad_norm=max_grad_norm)
            self.agent.image_provider = self.fused.acting_image
        else:
            self.opt = torch.optim.Adam(self.q.parameters(), lr=learning_rate)
        cap = max(int(capacity), env.n_alloc)
        self.prioritised = bool(prioritised)
        if self.prioritised:
            # beta is set before every sample (the reference moves it per global_step, not per sample)
            self.replay = PrioritisedDeviceReplay(cap, env.words, 1, dev, alpha=per_alpha, beta=per_beta,
                                                  max_beta=per_max_beta, beta_step=0.0, seed=seed)
            self._prio = torch.empty(batch_size, dtype=torch.float32, device=dev)
        else:
            self.replay = DeviceReplay(cap, env.words, 1, dev)
        self._pos_t = torch.zeros(1, dtype=torch.int64, device=dev)
        self._size_t = torch.zeros(1, dtype=torch.int64, device=dev)
        self.first = self.agent.first
        self.total_frames = int(total_frames)
        self.batch_size, self.gamma, self.target_update = int(batch_size), float(gamma), int(target_update)
        self.max_grad_norm, self.replay_constant = float(max_grad_norm), float(replay_constant)
        self.learning_starts, self.train_frequency = int(learning_starts), int(train_frequency)
        self.epsilon, self.min_epsilon = float(max_epsilon), float(min_epsilon)
        self.epsilon_decrement = (max_epsilon - min_epsilon) / (exploration_fraction * total_frames)
        self.beta = float(per_beta)
        self.beta_increment = (per_max_beta - per_beta) / (beta_fraction * total_frames)
        self.frames = 0
        self.updates = 0
        self.syncs: List[int] = []          # the frames whose schedule step copied the target
        self.last_loss: Optional[torch.Tensor] = None
        self.last_beta: Optional[float] = None   # the beta of the last prioritised sample
        self.per_max_beta = float(per_max_beta)
        self.graphable = bool(graphable)
        self._graph: Optional[torch.cuda.CUDAGraph] = None
        self._init_stats(episode_stats, stats_log_every)
        self._init_curriculum(curriculum, curriculum_refresh)

    def gather(self, idx: torch.Tensor) -> Dict[str, torch.Tensor]:
        """Rows ``idx`` of the ring as ``ddqn_update``'s batch (pbn_replay_batch when it takes the
        batch size, else PyTorch bit operations)."""
        rp, N, B = self.replay, self.env.n_nodes, idx.shape[0]
        if rp.device.type == "cuda" and B % 32 == 0:
            b = rp.gather(idx, self.env.net)
            x = b["x"]
            return {"state": x[0, :B], "target": x[1, :B], "next_state": x[0, B:], "action": b["actions"].view(B, 1),
                    "reward": b["rewards"], "done": b["masks"]}
        return {"state": _unpack(rp.state[:, idx], N), "target": self.first[rp.target[idx].long()],
                "next_state": _unpack(rp.next_state[:, idx], N), "action": rp.action[idx].long().view(B, 1),
                "reward": rp.reward[idx].view(B, 1), "done": rp.done[idx].to(torch.float32).view(B, 1)}

    def _learn_step(self) -> torch.Tensor:
        rp, B = self.replay, self.batch_size
        if self.prioritised:
            rp.beta_t.fill_(self.beta)
            rp.beta = self.last_beta = self.beta
            idx, w = rp.sample(B)
            if self.fused is not None:
                loss = self.fused.update(rp, idx, weights=w, priorities_out=self._prio,
                                         replay_constant=self.replay_constant)
            else:
                loss, _ = ddqn_update(self.q, self.target, self.opt, self.gather(idx), self.gamma, self.max_grad_norm,
                                      weights=w, priorities_out=self._prio, replay_constant=self.replay_constant)
            rp.update_priorities(idx, self._prio)
            return loss
        idx = rp.sample_indices(B, self.gen)
        if self.fused is not None:
            return self.fused.update(rp, idx)
        return ddqn_update(self.q, self.target, self.opt, self.gather(idx), self.gamma, self.max_grad_norm)[0]

    def sync_target(self) -> None:
        if self.fused is not None:
            self.fused.sync_target()
        else:
            self.target.load_state_dict(self.q.state_dict())

    def frame(self):
        """One global_step for every env; returns (reward, done) of the ``num_envs`` envs, ``done``
        = terminated or truncated (the episode ended; what is stored is terminated alone)."""
        if self._graph is not None:
            return self.run(1)
        env, rp = self.env, self.replay
        f = self.frames
        state = env.state.clone()
        target = env.target.clone()
        self.agent.act_q(self.epsilon)
        _, reward, flags = env.step_flipmask(use_current=True)
        rp.store_at(self._pos_t, self._size_t, state, target, self.agent.actions.view(-1, 1), env.reward,
                    env.final_state, env.flags, done_mask=_lib.FLAG_TERMINATED)
        self._redraw_resets()
        self._track_stats()
        self._refresh_curriculum()
        rp.pos = (rp.pos + env.n_alloc) % rp.capacity
        rp.size = min(rp.size + env.n_alloc, rp.capacity)
        if f > self.learning_starts and f % self.train_frequency == 0 and rp.size >= max(self.batch_size, 2):
            self.last_loss = self._learn_step()
            self.updates += 1
        # _schedule_step
        self.epsilon = max(self.min_epsilon, self.epsilon - self.epsilon_decrement)
        if (f + 1) % self.target_update == 0:
            self.sync_target()
            self.syncs.append(f)
        self.beta = min(self.beta + self.beta_increment, 1)
        self.frames = f + 1
        done = (flags & (_lib.FLAG_TERMINATED | _lib.FLAG_TRUNCATED)) != 0
        return reward, done

    # ---- graph-captured frames -------------------------------------------------------------
    def _check_capturable(self) -> None:
        """capture()'s refusals; nothing here touches the GPU."""
        if not self.graphable:
            raise ValueError("construct the learner with graphable=True to capture it")
        wrong = []
        if self.fused is None:
            wrong.append("fused: the captured frame runs the HIP update (fused=True), not the PyTorch one")
        if not self.prioritised:
            wrong.append("prioritised: the captured frame samples from prioritised replay (prioritised=True)")
        if self.train_frequency != 1:
            wrong.append(f"train_frequency: the captured frame updates every frame (1), not every {self.train_frequency}")
        if self.per_max_beta < 1.0:
            wrong.append("per_max_beta: the captured schedule moves replay.beta_t itself, which every sample clamps "
                         "to per_max_beta; it must be >= 1")
        if wrong:
            raise ValueError("capture() cannot take this learner -- " + "; ".join(wrong))

    def capture(self, min_updates: int = 1) -> None:
        """Capture one whole learning frame in a hipGraph; ``frame()`` replays it from then on and
        ``run(k)`` replays it ``k`` times back to back.  The frame is one chain of launches:

            pbn_dqn_flipmask_from_state  act at *step and *epsilon
            pbn_step_dev_store           the step, writing its transitions into the ring (settle law:
                                         pbn_step_dev, then pbn_replay_store, which also moves the
                                         stepped state into ``env.state``)
            pbn_per_store                the new rows' priorities
            pbn_replay_advance           ring position, fill level, step index, epsilon's decay
            pbn_per_sample               over the fill level the store left, at *beta
            pbn_ddqn_learn               weights in, priorities out
            pbn_per_update
            pbn_ddqn_schedule            beta's increment and, when due, the hard target copy

        The step index, epsilon, beta, the ring position and fill level, the draw counter and Adam's
        step count live in device memory; the host mirrors them after the replays with the eager
        frame's own arithmetic.  Frames run eagerly (on a side stream, as capture requires) until
        every later frame learns and ``min_updates`` updates are done.  Fused and prioritised with
        ``train_frequency`` 1 only; after capture the env must only be stepped through ``frame()`` /
        ``run()``.  Weights loaded between replays are repacked by the next replay (``sync()``)."""
        self._check_capturable()
        if self._graph is not None:
            raise ValueError("the frame is already captured")
        env, rp, dev = self.env, self.replay, torch.device(self.env.device)
        # (a loaded checkpoint that already learns every frame: no eager frame runs)
        self._warm_up(lambda: self._learns(self.frames, rp.size) and self.updates >= min_updates)
        self._capture_counters(self.min_epsilon, self.epsilon_decrement, 0)
        self._step_base = env.step_index - self.frames      # *step - base = the frames done
        rp.beta_t.fill_(self.beta)            # the next frame's beta; the schedule launch moves it from here on
        self._capture_ring(_lib.FLAG_TERMINATED, None, self.agent.actions.view(-1, 1))
        self.fused.sync()                         # (a repack belongs before the capture, not in it)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._graph_body()
        self._graph = g
        # the capture recorded the frame without running it: nothing above advanced
        torch.cuda.current_stream(dev).synchronize()

    def _graph_body(self) -> None:
        env, rp, fu = self.env, self.replay, self.fused
        self.agent.act_q(step_t=self._step_t, epsilon_t=self._eps32)
        self._step_and_store()
        self._redraw_resets()
        self._track_stats()
        self._refresh_curriculum()
        # the counters before the sample: it must see the fill level the store left, as the eager
        # frame's does
        self._advance_counters()
        self._g_idx, self._g_w = rp.sample(self.batch_size, size_t=self._size_t)
        fu.update(rp, self._g_idx, weights=self._g_w, priorities_out=self._prio,
                  replay_constant=self.replay_constant)
        rp.update_priorities(self._g_idx, self._prio, self._size_t)
        with torch.cuda.device(env.device):
            _lib.check(_lib.load().pbn_ddqn_schedule(
                rp.beta_t.data_ptr(), float(self.beta_increment), self._step_t.data_ptr(), self._step_base,
                self.target_update, fu.t_flat.data_ptr(), fu.q_flat.data_ptr(), fu.q_flat.numel(),
                fu.t_image.data_ptr(), fu.q_image.data_ptr(), fu.q_image.numel(), env._stream()), "pbn_ddqn_schedule")

    # ---- checkpoints (learner.py, checkpoint.py) ---------------------------------------------
    agent_kind = "ddqn"

    def _own_state(self) -> dict:
        return {"frames": int(self.frames), "updates": int(self.updates), "epsilon": self.epsilon, "beta": self.beta,
                "last_beta": self.last_beta, "syncs": [int(f) for f in self.syncs]}

    def _learns(self, frames: int, size: int) -> bool:
        """Whether every frame from ``frames`` on takes an update (what a captured frame does)."""
        return frames > self.learning_starts and size >= max(self.batch_size, 2)

    def _check_loadable_captured(self, host: dict) -> None:
        """Into a captured learner: the checkpoint's frames must all learn from here on, and its
        step index must count from the base the captured schedule launch holds."""
        if not self._learns(int(host["learner.frames"]), int(host["replay.size"])):
            raise ValueError("the checkpoint was saved before every frame learns (frames <= learning_starts, or "
                             "fewer than batch_size rows): a captured frame always updates; load into a learner "
                             "that is not captured yet")
        base = int(host["env.step_index"]) - int(host["learner.frames"])
        if base != self._step_base:
            raise ValueError(f"checkpoint mismatch: env.step_index - frames (file {base}, captured frame "
                             f"{self._step_base}): the captured target-copy schedule counts frames from it; load "
                             "into a fresh learner and capture() after the load")

    def _load_own_state(self, own: dict) -> None:
        self.frames, self.updates = int(own["frames"]), int(own["updates"])
        self.epsilon, self.beta, self.last_beta = own["epsilon"], own["beta"], own["last_beta"]
        self.syncs[:] = [int(f) for f in own["syncs"]]
        if self.prioritised:
            # beta_t across the frame boundary: an eager frame leaves its own beta there, a captured
            # one the next frame's (its schedule launch has moved it on)
            rp = self.replay
            if self._graph is not None:
                rp.beta_t.fill_(self.beta)
            else:
                rp.beta_t.fill_(self.last_beta if self.last_beta is not None else rp.beta)

    def _mirror(self, k: int) -> None:
        """The host's copies after ``k`` replays: the eager frame's own arithmetic, ``k`` times."""
        rp, fu = self.replay, self.fused
        synced = False
        for _ in range(k):
            f = self.frames
            self._mirror_frame()
            rp.beta = self.last_beta = self.beta     # the beta this frame's sample read
            rp.mirror_beta()
            self.updates += 1
            if (f + 1) % self.target_update == 0:
                self.syncs.append(f)
                synced = True
            self.beta = min(self.beta + self.beta_increment, 1)
            self.frames = f + 1
        # the replays rewrote the online parameters in place, and the target's on sync frames (the
        # version counters are what sync(), BatchedDDQN and PyTorch read)
        fu.mark_updated()
        if synced:
            fu.mark_target_updated()
        self.last_loss = fu.loss[0]

    def run(self, k: int):
        """``k`` captured frames replayed back to back, nothing on the host between them; then the
        host's copies move to their values after ``k`` frames.  Returns the last frame's (reward,
        done), as ``frame()`` does."""
        if self._graph is None:
            raise ValueError("run() replays the captured frame: call capture() first")
        if k < 1:
            raise ValueError("k must be >= 1")
        self.fused.sync()                # weights loaded since the last replay: repack their images
        for _ in range(k):
            self._graph.replay()
        self._mirror(k)
        env = self.env
        n = env.num_envs
        done = (env.flags[:n] & (_lib.FLAG_TERMINATED | _lib.FLAG_TRUNCATED)) != 0
        return env.reward[:n], done


def load_ddqn_checkpoint(path: str) -> DQN:
    """A ``DQN`` from the ``.npz`` export of a reference save dict (``DDQN._make_save_dict``,
    ddqn_per/__init__.py:130-148; tools/export_agent.py --ddqn): arrays ``params.<name>`` (the
    ``"params"`` state dict), ``net_arch`` (``policy_kwargs["net_arch"]``, int (L, 2)), ``input_size``
    and ``output_size``.  Arrays only; nothing in the file is executed."""
    with np.load(path, allow_pickle=False) as z:
        arch = [tuple(int(x) for x in row) for row in np.asarray(z["net_arch"]).reshape(-1, 2)]
        dqn = DQN(int(z["input_size"]), int(z["output_size"]), arch)
        sd = {k[len("params."):]: torch.from_numpy(np.asarray(z[k], dtype=np.float32)) for k in z.files
              if k.startswith("params.")}
    dqn.load_state_dict(sd)
    return dqn
