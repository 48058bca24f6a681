"""The ControlGBDQ agent (control_gbdq_model/, train_control_gbdq.py) over a VectorPBNEnv; DESIGN.md
"ControlGBDQ".

The reference's fourth agent gives one binary value per control node (gym-PBN/ControlPBNEnv's action
form, ``control_to_flipmask``).  Its three graph layers are GBDQ's up to attribute names, so
pbn_gbdq_pack and pbn_gbdq_front serve it unchanged; its tail is three 256-wide layers, a
``Linear(256, 1)`` value head and C ``Linear(256, 2)`` advantage heads (control_gbdq_model/network.py:
43-57), which pbn_cgbdq_flipmask (HIP, csrc/pbn_cgbdq.hip) runs in one MFMA launch that ends in the
control flip mask.

    ControlGraphBranchingQNetwork   the module tree under the reference's names: its state_dict loads
    cgbdq_update                    update_policy (:88-128) on a gathered batch: no gradient clamp
    BatchedControlGBDQ              predict (:64-86) for every env: pbn_gbdq_front, then pbn_cgbdq_flipmask
    ControlGBDQLearner              learn (:139-240) as frames over the batch, one replay ring

Stated departures are GBDQ's (gbdq.py): per-env BatchNorm statistics for batched acting, running
statistics left alone there, replay rows drawn with replacement.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .gbdq import BatchedGBDQ, EdgeConv, GBDQLearner, GraphBranchingQNetwork, _explore_words, ring_rows
from .replay import DeviceReplay
from .vector_env import control_to_flipmask

__all__ = ["ControlGraphBranchingQNetwork", "cgbdq_update", "stacked_heads", "combine_heads", "BatchedControlGBDQ",
           "ControlGBDQLearner", "EXPLORE_MODES"]

EXPLORE_MODES = {"reference": 0, "uniform": 1}     # pbn_cgbdq_flipmask's explore_mode


class ControlGraphBranchingQNetwork(nn.Module):
    """control_gbdq_model/network.py:10-82 under the reference's attribute names (``conv_model1..3``,
    ``conv1..3`` whose ``nn`` shares those parameters, ``model``, ``pooling``, ``bn1..3``,
    ``value_head``, ``adv_heads``): a reference ``state_dict`` loads with ``strict=True``.

    ``forward(x, edge_index, per_env=False)``: x (B, N, 2) -> Q (B, C, 2).  The BatchNorm law is
    GraphBranchingQNetwork's (gbdq.py): training mode always, ``per_env=True`` for batched acting."""

    def __init__(self, state: int, action_space_dimension: int, number_of_actions: int):
        super().__init__()
        self.ac_dim = action_space_dimension
        self.n = number_of_actions
        self.state = state
        self.in_size = state * state
        self.conv_model1 = nn.Sequential(nn.Linear(2 * 2, 64), nn.ReLU(), nn.Linear(64, state))
        self.conv_model2 = nn.Sequential(nn.Linear(2 * state, 64), nn.ReLU(), nn.Linear(64, state))
        self.conv_model3 = nn.Sequential(nn.Linear(2 * state, 64), nn.ReLU(), nn.Linear(64, state))
        self.conv1 = EdgeConv(self.conv_model1, aggr="add")
        self.conv2 = EdgeConv(self.conv_model2, aggr="add")
        self.conv3 = EdgeConv(self.conv_model3, aggr="add")
        self.model = nn.Sequential(nn.Linear(self.in_size, 256), nn.ReLU(), nn.Linear(256, 256), nn.ReLU(),
                                   nn.Linear(256, 256), nn.ReLU())
        self.pooling = nn.AvgPool1d(4)     # (unused, as in the reference)
        self.bn1 = nn.BatchNorm1d(state)
        self.bn2 = nn.BatchNorm1d(state)
        self.bn3 = nn.BatchNorm1d(state)
        self.value_head = nn.Linear(256, 1)
        self.adv_heads = nn.ModuleList([nn.Linear(256, action_space_dimension) for _ in range(number_of_actions)])

    _bn = staticmethod(GraphBranchingQNetwork._bn)
    conv_flat = GraphBranchingQNetwork.conv_flat

    def front(self, x: torch.Tensor, edges: torch.Tensor, per_env: bool = False) -> torch.Tensor:
        """The three graph layers: (B, N, 2) -> (B, N N), what pbn_gbdq_front computes (per_env)."""
        out = F.relu(self._bn(self.bn1, self.conv1(x, edges), per_env))
        out = F.relu(self._bn(self.bn2, self.conv2(out, edges), per_env))
        out = F.relu(self._bn(self.bn3, self.conv3(out, edges), per_env))
        return out.reshape((x.shape[0], self.in_size))

    def tail(self, front: torch.Tensor) -> torch.Tensor:
        """Trunk, heads and the dueling combination (:69-78): (B, N N) -> Q (B, C, 2)."""
        out = self.model(front)
        value = self.value_head(out)
        advantages = torch.stack([l(out) for l in self.adv_heads], dim=1)
        return value.unsqueeze(2) + advantages - advantages.mean(2, keepdim=True)

    def heads_raw(self, front: torch.Tensor) -> torch.Tensor:
        """Trunk and heads without the combination: (B, N N) -> (C + 1, B, 2), head 0 the value head
        zero-padded to 2 outputs (GraphBranchingQNetwork.heads_raw's layout)."""
        out = self.model(front)
        value = F.pad(self.value_head(out), (0, self.ac_dim - 1))
        return torch.stack([value] + [l(out) for l in self.adv_heads], dim=0)

    def forward(self, x: torch.Tensor, edges: torch.Tensor, per_env: bool = False) -> torch.Tensor:
        return self.tail(self.front(x, edges, per_env))

    def tail_parameters(self) -> list:
        """pbn_cgbdq_pack's ``d_tail`` in its order (csrc/cgbdq_tail.h)."""
        ps = []
        for i in (0, 2, 4):
            ps += [self.model[i].weight, self.model[i].bias]
        ps += [self.value_head.weight, self.value_head.bias]
        for hd in self.adv_heads:
            ps += [hd.weight, hd.bias]
        return ps

    def tail_flat(self) -> torch.Tensor:
        return torch.cat([p.detach().reshape(-1) for p in self.tail_parameters()]).contiguous()


def stacked_heads(raw: torch.Tensor) -> torch.Tensor:
    """``heads_raw``'s (C + 1, B, 2) as pbn_cgbdq_heads' (B, 1 + 2 C): the value, then head k's two
    outputs at columns 1 + 2 k and 2 + 2 k."""
    return torch.cat([raw[0, :, :1], raw[1:].transpose(0, 1).reshape(raw.shape[1], -1)], dim=1)


def combine_heads(heads: torch.Tensor) -> torch.Tensor:
    """The dueling combination in the kernel's stated order on (B, 1 + 2 C) stacked heads:
    mean = (adv_0 + adv_1) / 2, q_a = (v + adv_a) - mean -> (B, C, 2)."""
    v = heads[:, :1, None]
    adv = heads[:, 1:].reshape(heads.shape[0], -1, 2)
    mean = ((adv[..., 0] + adv[..., 1]) / 2)[..., None]
    return (v + adv) - mean


def cgbdq_update(q: ControlGraphBranchingQNetwork, target: ControlGraphBranchingQNetwork, opt: torch.optim.Optimizer,
                 batch: Dict[str, torch.Tensor], edges: torch.Tensor, gamma: float = 0.99) -> torch.Tensor:
    """``update_policy`` (control_gbdq_model/__init__.py:94-121) on a batch of ``states``, ``targets``,
    ``next_states`` (B, N) floats, ``actions`` (B, C, 1) int64, ``rewards`` and ``masks`` (B, 1):
    inputs ``stack((states, targets), dim=2)``, three forwards in the reference's order, q(s), q(s'),
    target(s'), each with its own batch statistics; the double-DQN target with ``masks = done``
    exactly as written; MSE over (b, k); no gradient clamp (it is commented out there); one optimiser
    step.  Returns the loss."""
    qvals = q(torch.stack((batch["states"], batch["targets"]), dim=2), edges)
    current = qvals.gather(2, batch["actions"]).squeeze(-1)
    with torch.no_grad():
        nxt = torch.stack((batch["next_states"], batch["targets"]), dim=2)
        argmax = torch.argmax(q(nxt, edges), dim=2)
        max_next = target(nxt, edges).gather(2, argmax.unsqueeze(2)).squeeze(-1)
    expected = batch["rewards"] + max_next * gamma * batch["masks"]
    loss = F.mse_loss(expected, current)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss.detach()


# ------------------------------------------------------------------------------------ acting
class BatchedControlGBDQ(BatchedGBDQ):
    """``ControlGBDQ.predict`` (control_gbdq_model/__init__.py:64-86) for every env of a VectorPBNEnv.
    On the GPU, where ``front_supported(N)`` holds, acting is two launches: pbn_gbdq_front, then
    pbn_cgbdq_flipmask (the tail, the dueling combination, the argmax over each head's two outputs,
    epsilon-greedy by the frozen EXPLORE law and the control flip mask).  On a CPU device, or an
    unsupported N, the restated forward, the numpy EXPLORE law and ``control_to_flipmask`` stand in and
    give the same actions and masks.

    ``control_nodes``: head k's node; an entry outside [0, N) keeps its head and its recorded action
    and sets no bit (train_control_gbdq.py lists node 14 of 14 genes).  ``explore``: "reference" gives
    every control node the value 0 when an env explores (the reference's ``np.random.randint(0, 1)``),
    "uniform" gives head k the value (EXPLORE word k + 1 times 2) >> 32."""

    def __init__(self, env, qnet: Optional[ControlGraphBranchingQNetwork] = None, control_nodes: Sequence[int] = (),
                 explore: str = "reference", *, epsilon: float = 0.0):
        if explore not in EXPLORE_MODES:
            raise ValueError("explore must be 'reference' or 'uniform'")
        self.control_nodes = [int(c) for c in control_nodes]
        C, N = len(self.control_nodes), env.n_nodes
        if not 1 <= C <= 128:
            raise ValueError("1 to 128 control nodes")
        self.explore = explore
        q = (qnet if qnet is not None else ControlGraphBranchingQNetwork(N, 2, C)).to(torch.device(env.device))
        if q.state != N or q.ac_dim != 2 or q.n != C:
            raise ValueError("BatchedControlGBDQ needs ControlGraphBranchingQNetwork(N, 2, len(control_nodes))")
        self._init_front(env, q, C, epsilon)
        self._valid = [k for k, c in enumerate(self.control_nodes) if 0 <= c < N]
        self._tail_image, self._tail_key = None, None
        if self.kernel:
            nf = ctypes.c_int64()
            _lib.check(_lib.load().pbn_cgbdq_image_floats(env.net.handle, C, ctypes.byref(nf)), "pbn_cgbdq_image_floats")
            self._tail_image = torch.zeros(nf.value, dtype=torch.float32, device=self.device)
            self._ctrl = torch.tensor(self.control_nodes, dtype=torch.int32, device=self.device)
            self._heads = torch.empty(env.n_alloc, 1 + 2 * C, dtype=torch.float32, device=self.device)

    def capture(self, *args, **kwargs):
        raise NotImplementedError("a captured ControlGBDQ frame is out of scope: the update is PyTorch's "
                                  "(DESIGN.md 'ControlGBDQ')")

    def pack(self) -> torch.Tensor:
        """Both images, each repacked when one of its parameters changed ((data_ptr, _version)); returns
        the tail's (pbn_cgbdq_pack)."""
        self._pack_front()
        ps = self.q.tail_parameters()
        key = tuple((p.data_ptr(), p._version) for p in ps)
        if key != self._tail_key:
            flat = self.q.tail_flat()
            with torch.cuda.device(self.device):
                _lib.check(_lib.load().pbn_cgbdq_pack(self.env.net.handle, flat.data_ptr(), self.branches,
                                                      self._tail_image.data_ptr(), self.env._stream()), "pbn_cgbdq_pack")
            self._tail_key = key
        return self._tail_image

    @torch.no_grad()
    def heads(self) -> torch.Tensor:
        """The raw head outputs (n, 1 + 2 C) of every env's observation (pbn_cgbdq_heads' layout)."""
        front = self.front()
        if not self.kernel:
            return stacked_heads(self.q.heads_raw(front)).contiguous()
        env, image = self.env, self.pack()
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pbn_cgbdq_heads(env.net.handle, env.n_alloc, front.data_ptr(), image.data_ptr(),
                                                   self.branches, self._heads.data_ptr(), env._stream()), "pbn_cgbdq_heads")
        return self._heads

    @torch.no_grad()
    def act(self, epsilon: Optional[float] = None, step_t: Optional[torch.Tensor] = None,
            epsilon_t: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Every env's values (``self.actions`` (n, C)) and flip masks (``env.flipmask`` (W, n)), keyed by
        the env's next step index; ``step_t`` / ``epsilon_t``: optional one-element device tensors (int64
        / float32) read when the kernel runs."""
        env = self.env
        eps = self.epsilon if epsilon is None else float(epsilon)
        C = self.branches
        if self.kernel:
            front, image = self.front(), self.pack()
            with torch.cuda.device(self.device):
                _lib.check(_lib.load().pbn_cgbdq_flipmask(
                    env.net.handle, env.seed, env.step_index, step_t.data_ptr() if step_t is not None else None,
                    env.env_offset, env.n_alloc, front.data_ptr(), image.data_ptr(), C, self._ctrl.data_ptr(),
                    EXPLORE_MODES[self.explore], eps, epsilon_t.data_ptr() if epsilon_t is not None else None,
                    env.state.data_ptr(), env.flipmask.data_ptr(), self.actions.data_ptr(), env._stream()),
                    "pbn_cgbdq_flipmask")
            return env.flipmask
        step = int(step_t.item()) if step_t is not None else env.step_index
        eps = float(epsilon_t.item()) if epsilon_t is not None else eps
        n = env.n_alloc
        greedy = torch.argmax(combine_heads(self.heads()), dim=2).cpu().numpy()
        w = _explore_words(env.seed, step, env.env_offset, n, (C + 1 + 3) // 4)
        eps_u = int(np.floor(np.float64(np.float32(eps)) * 4294967296.0))
        explore = w[0] < np.uint64(eps_u)
        if self.explore == "uniform":
            rnd = np.stack([(w[1 + k] * np.uint64(2)) >> np.uint64(32) for k in range(C)], axis=1).astype(np.int64)
        else:
            rnd = np.zeros((n, C), dtype=np.int64)
        acts = np.where(explore[:, None], rnd, greedy)
        self.actions.copy_(torch.from_numpy(acts.astype(np.int32)))
        if self._valid:
            env.flipmask.copy_(control_to_flipmask(env.state, self.actions[:, self._valid],
                                                   [self.control_nodes[k] for k in self._valid], env.n_nodes))
        else:
            env.flipmask.zero_()
        return env.flipmask


# ------------------------------------------------------------------------------------ the learner
class ControlGBDQLearner(GBDQLearner):
    """``ControlGBDQ.learn`` (control_gbdq_model/__init__.py:139-240) over a VectorPBNEnv; the defaults
    are ``AgentConfig``'s as train_control_gbdq.py runs it.  One ``frame()``: act for every env
    (BatchedControlGBDQ), step, store the transitions, ``decrement_epsilon`` (:130-137, once per frame),
    and one ``update_policy`` when ``frame > max(batch_size, learning_starts)`` (:221).

    One ring, not two: the reference stores every transition in ``memory_positive`` and never fills
    ``memory_negative`` (:173-189), so the batch is min(batch_size, len) rows of one DeviceReplay, drawn
    with replacement; the stored done is terminated | truncated.  ``target_update`` as GBDQLearner's:
    "reference" (the refresh at :127-128 assigns into a fresh ``state_dict()`` copy: a no-op) or "copy".
    The reference's epsilon bump to 0.3 when ``all_attractors`` grows (:194-196) never fires here: the
    batched env's attractor set is fixed.  The update is PyTorch's (``cgbdq_update`` +
    torch.optim.Adam); ``capture()`` is not implemented."""

    agent_kind = "cgbdq"

    def __init__(self, env, qnet: Optional[ControlGraphBranchingQNetwork] = None, *, control_nodes: Sequence[int],
                 explore: str = "reference", capacity: int = 10 ** 5, batch_size: int = 256, learning_rate: float = 1e-5,
                 gamma: float = 0.99, target_update: str = "reference", target_net_update_freq: int = 5000,
                 learning_starts: int = 288, epsilon_start: float = 1.0, epsilon_final: float = 0.0,
                 epsilon_decay: int = 5_000, seed: int = 0, episode_stats: bool = False, stats_log_every: int = 0,
                 curriculum: bool = False, curriculum_refresh: int = 1000):
        if target_update not in ("reference", "copy"):
            raise ValueError("target_update must be 'reference' or 'copy'")
        if not env.keep_final_state:
            raise ValueError("ControlGBDQLearner needs the env's final_state (keep_final_state=True)")
        self.env = env
        self.agent = BatchedControlGBDQ(env, qnet, control_nodes, explore)
        dev = self.agent.device
        self.q = self.agent.q.train()
        C = self.agent.branches
        self.target = ControlGraphBranchingQNetwork(env.n_nodes, 2, C).to(dev).train()
        self.target.load_state_dict(self.q.state_dict())
        self.opt = torch.optim.Adam(self.q.parameters(), lr=learning_rate)
        self.replay = DeviceReplay(max(int(capacity), env.n_alloc), env.words, C, dev)
        self.batch_size, self.gamma = int(batch_size), float(gamma)
        self.target_update, self.target_net_update_freq = target_update, int(target_net_update_freq)
        self.learning_starts = max(int(learning_starts), self.batch_size)
        self.epsilon, self.epsilon_final = float(epsilon_start), float(epsilon_final)
        self.epsilon_step = (epsilon_start - epsilon_final) / epsilon_decay
        self.time_steps = 0
        self.frames = 0
        self.updates = 0
        self.update_counter = 0
        self.seed = int(seed)
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(seed)
        self.last_loss: Optional[torch.Tensor] = None
        self._init_stats(episode_stats, stats_log_every)
        self._init_curriculum(curriculum, curriculum_refresh)

    def sample(self) -> Dict[str, torch.Tensor]:
        """min(batch_size, len) rows (:89) as cgbdq_update's batch."""
        rp = self.replay
        idx = rp.sample_indices(min(self.batch_size, rp.size), self.gen)
        cols = ring_rows(rp, idx, getattr(self.env, "net", None), self.env.spec)
        return dict(zip(("states", "targets", "next_states", "actions", "rewards", "masks"), cols))

    def update(self) -> torch.Tensor:
        loss = cgbdq_update(self.q, self.target, self.opt, self.sample(), self.agent.edges, self.gamma)
        self.updates += 1
        self.refresh_target()
        return loss

    def frame(self):
        env = self.env
        state = env.state.clone()
        target = env.target.clone()
        self.agent.act(self.epsilon)
        _, reward, flags = env.step_flipmask(use_current=True)
        done_all = (env.flags & (_lib.FLAG_TERMINATED | _lib.FLAG_TRUNCATED)) != 0
        self.replay.store(state, target, self.agent.actions, env.reward, env.final_state, done_all)
        self._redraw_resets()
        self._track_stats()
        self._refresh_curriculum()
        self.decrement_epsilon()
        f = self.frames
        self.frames += 1
        if f > max(self.batch_size, self.learning_starts):
            self.last_loss = self.update()
        return reward, done_all[: env.num_envs]

    def _load_counters(self) -> None:
        pass     # (the ring's position and fill level are host values)
