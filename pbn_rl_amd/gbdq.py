"""The GBDQ graph agent (gbdq_model/, train_gbdq.py) over a VectorPBNEnv; DESIGN.md "GBDQ".

The reference's third agent reads the PBN's own wiring: three ``EdgeConv(add)`` layers over the
predictor graph, each followed by ``BatchNorm1d`` (never put in eval mode) and ReLU, then a 512-wide
trunk and a value head and K advantage heads (gbdq_model/network.py:10-90).  ``torch_geometric`` is
not a dependency here: ``EdgeConv`` is restated below in PyG's documented convention.

    edge_index                gbdq_model/__init__.py:259-276 (get_adj_list) from the spec's functions
    GraphBranchingQNetwork    the module tree under the reference's names: its state_dict loads
    gbdq_update               update_policy (:98-138) on a gathered batch
    SplitDeviceReplay         memory_positive / memory_negative (:159-200) as two device rings, filled by
                              pbn_replay_store_split (HIP) in one stable partition per frame
    BatchedGBDQ               predict (:75-96) for every env: pbn_gbdq_front (HIP, csrc/pbn_gbdq.hip: the
                              three graph layers in one launch) -> trunk and heads (torch GEMMs) ->
                              pbn_heads_to_flipmask (HIP)
    GBDQLearner               learn (:149-251) as frames over the batch

Stated departures: batched acting normalises every env by its own statistics (``per_env=True``, what
the reference's B = 1 ``predict`` computes) and leaves BatchNorm's running statistics alone (they are
never read in training mode, and a batch has no sequential order to update them in); replay rows are
drawn with replacement, as DeviceReplay does.
"""
from __future__ import annotations


import ctypes
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .checkpoint import cpu_copy
from .learner import FrameLearner
from .replay import DeviceReplay
from .vector_env import actions_to_flipmask, unpack_states

__all__ = ["edge_index", "edge_csr", "EdgeConv", "GraphBranchingQNetwork", "gbdq_update", "front_supported",
           "ring_rows", "SplitDeviceReplay", "BatchedGBDQ", "GBDQLearner"]


# ------------------------------------------------------------------------------------ the graph
def edge_index(spec_or_env, device=None) -> torch.Tensor:
    """``GBDQ.get_adj_list`` (gbdq_model/__init__.py:259-276) as an int64 (2, E) tensor: for each node
    ``top`` in index order the pair (top, top), then over its functions in order and each function's
    inputs in order the pair (top, bot) for every input not yet seen for this node.  The ``done`` set
    starts empty, so a node that lists itself gets its self pair twice.  Row 0 = tops, row 1 = bots.
    The inputs are the functions' own (a network lowered to gates keeps them in ``Network.nodes``)."""
    spec = getattr(spec_or_env, "spec", spec_or_env)
    net = getattr(spec, "network", spec)
    tops, bots = [], []
    for top, funcs in enumerate(net.nodes):
        done = set()
        tops.append(top)
        bots.append(top)
        for f in funcs:
            for bot in f.inputs:
                if bot not in done:
                    done.add(bot)
                    tops.append(top)
                    bots.append(int(bot))
    return torch.tensor([tops, bots], dtype=torch.long, device=device)


def edge_csr(edges: torch.Tensor, n_nodes: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The edge list grouped by target node (row 1), edges of one node in list order: (start int32
    [N + 1], src int32 [E]); node i receives the messages of src[start[i]:start[i + 1]]."""
    e = edges.detach().cpu()
    order = torch.sort(e[1], stable=True).indices
    counts = torch.bincount(e[1], minlength=n_nodes)
    start = torch.zeros(n_nodes + 1, dtype=torch.int64)
    start[1:] = torch.cumsum(counts, 0)
    return start.to(torch.int32), e[0][order].to(torch.int32)


class EdgeConv(nn.Module):
    """``torch_geometric.nn.EdgeConv(nn, aggr="add")``, flow source -> target: for edge e with j =
    edge_index[0][e] and i = edge_index[1][e] the message is ``nn(cat[x_i, x_j - x_i])`` and node i's
    output the sum of the messages that end in it (zero without one).  x is (B, N, F) with one shared
    edge list.  The gathers and the sum are products with 0/1 matrices: exact for the gathers of finite
    values, and with a deterministic backward on the GPU (an index_add's atomics are not).  A NaN or
    infinite row of x reaches every node (0 * NaN), where an index gather, and pbn_gbdq_front, reach
    only the nodes that receive from it (DESIGN.md "Non-finite values")."""

    def __init__(self, nn_module: nn.Module, aggr: str = "add"):
        super().__init__()
        if aggr != "add":
            raise ValueError("only aggr='add' is restated")
        self.nn = nn_module
        self._sel: Optional[tuple] = None

    def _selectors(self, edges: torch.Tensor, n: int, like: torch.Tensor):
        key = (edges.data_ptr(), edges._version, edges.shape[1], n, like.device, like.dtype)
        if self._sel is None or self._sel[0] != key:
            gj = F.one_hot(edges[0], n).to(like.dtype)       # (E, N)
            gi = F.one_hot(edges[1], n).to(like.dtype)
            self._sel = (key, gi, gj, gi.t().contiguous())
        return self._sel[1:]

    def forward(self, x: torch.Tensor, edges: torch.Tensor) -> torch.Tensor:
        gi, gj, agg = self._selectors(edges, x.shape[-2], x)
        x_i = torch.matmul(gi, x)                             # (B, E, F)
        x_j = torch.matmul(gj, x)
        return torch.matmul(agg, self.nn(torch.cat([x_i, x_j - x_i], dim=-1)))


def _mlp3(i: int, o: int) -> nn.Sequential:
    return nn.Sequential(nn.Linear(i, 512), nn.ReLU(), nn.Linear(512, 512), nn.ReLU(), nn.Linear(512, o))


class GraphBranchingQNetwork(nn.Module):
    """gbdq_model/network.py:10-90 under the reference's attribute names (``conv_model1..3``,
    ``gconv1..3`` whose ``nn`` shares those parameters, ``bn1..3``, ``model``, ``pooling``,
    ``value_head``, ``adv_heads``): a reference ``state_dict`` loads with ``strict=True``.

    ``forward(x, edge_index, per_env=False)``: x (B, N, 2) = (state bit, target bit) per node -> Q
    (B, K, A).  ``BatchNorm1d(state)`` on (B, N, N) takes the node as the channel and its statistics
    over (batch, feature); the reference never calls ``eval()``, so every forward normalises by the
    batch's statistics.  ``per_env=True`` normalises every env by its own (mean and biased variance
    over the N features of each (env, node) row, eps 1e-5): a loop of B = 1 forwards, which is what
    ``predict`` runs; it leaves the running statistics alone."""

    def __init__(self, state: int, action_space_dimension: int, number_of_actions: int):
        super().__init__()
        self.ac_dim = action_space_dimension
        self.n = number_of_actions
        self.state = state
        self.in_size = state * state
        self.conv_model1 = nn.Sequential(nn.Linear(2 * 2, 64), nn.ReLU(), nn.Linear(64, state))
        self.conv_model2 = nn.Sequential(nn.Linear(2 * state, 64), nn.ReLU(), nn.Linear(64, state))
        self.conv_model3 = nn.Sequential(nn.Linear(2 * state, 64), nn.ReLU(), nn.Linear(64, state))
        self.gconv1 = EdgeConv(self.conv_model1, aggr="add")
        self.gconv2 = EdgeConv(self.conv_model2, aggr="add")
        self.gconv3 = EdgeConv(self.conv_model3, aggr="add")
        self.model = nn.Sequential(nn.Linear(self.in_size, 512), nn.ReLU(), nn.Linear(512, 512), nn.ReLU(),
                                   nn.Linear(512, 512), nn.ReLU(), nn.Linear(512, 512), nn.ReLU())
        self.pooling = nn.AvgPool1d(4)
        self.bn1 = nn.BatchNorm1d(state)
        self.bn2 = nn.BatchNorm1d(state)
        self.bn3 = nn.BatchNorm1d(state)
        self.value_head = _mlp3(512, 1)
        self.adv_heads = nn.ModuleList([_mlp3(512, action_space_dimension) for _ in range(number_of_actions)])

    @staticmethod
    def _bn(bn: nn.BatchNorm1d, x: torch.Tensor, per_env: bool) -> torch.Tensor:
        if not per_env:
            return bn(x)
        B, N, Fd = x.shape
        # every (env, node) row is a channel of its own: BatchNorm1d's training arithmetic at B = 1
        y = F.batch_norm(x.reshape(1, B * N, Fd), None, None, bn.weight.repeat(B), bn.bias.repeat(B), True, 0.0, bn.eps)
        return y.reshape(B, N, Fd)

    def front(self, x: torch.Tensor, edges: torch.Tensor, per_env: bool = False) -> torch.Tensor:
        """The three graph layers: (B, N, 2) -> (B, N N), what pbn_gbdq_front computes (per_env)."""
        out = F.relu(self._bn(self.bn1, self.gconv1(x, edges), per_env))
        out = F.relu(self._bn(self.bn2, self.gconv2(out, edges), per_env))
        out = F.relu(self._bn(self.bn3, self.gconv3(out, edges), per_env))
        return out.reshape((x.shape[0], self.in_size))

    def tail(self, front: torch.Tensor) -> torch.Tensor:
        """Trunk, heads and the dueling combination (:83-90): (B, N N) -> Q (B, K, A)."""
        out = self.model(front)
        value = self.value_head(out)
        advantages = torch.stack([l(out) for l in self.adv_heads], dim=1)
        return value.unsqueeze(2) + advantages - advantages.mean(2, keepdim=True)

    def heads_raw(self, front: torch.Tensor) -> torch.Tensor:
        """Trunk and heads without the combination: (B, N N) -> (K + 1, B, A), head 0 the value head
        zero-padded to A outputs, the layout pbn_heads_to_flipmask reads (as BDQ's)."""
        out = self.model(front)
        value = F.pad(self.value_head(out), (0, self.ac_dim - 1))
        return torch.stack([value] + [l(out) for l in self.adv_heads], dim=0)

    def forward(self, x: torch.Tensor, edges: torch.Tensor, per_env: bool = False) -> torch.Tensor:
        return self.tail(self.front(x, edges, per_env))

    def conv_flat(self) -> torch.Tensor:
        """pbn_gbdq_pack's ``d_conv``: the three conv models and the three BatchNorms, flat."""
        ps = []
        for m in (self.conv_model1, self.conv_model2, self.conv_model3):
            ps += [m[0].weight, m[0].bias, m[2].weight, m[2].bias]
        for bn in (self.bn1, self.bn2, self.bn3):
            ps += [bn.weight, bn.bias]
        return torch.cat([p.detach().reshape(-1) for p in ps]).contiguous()


def gbdq_update(q: GraphBranchingQNetwork, target: GraphBranchingQNetwork, opt: torch.optim.Optimizer,
                batch: Dict[str, torch.Tensor], edges: torch.Tensor, gamma: float = 1.8,
                grad_clamp: float = 10.0) -> torch.Tensor:
    """``update_policy`` (gbdq_model/__init__.py:104-131) on a batch of ``states``, ``targets``,
    ``next_states`` (B, N) floats, ``actions`` (B, K, 1) int64, ``rewards`` and ``masks`` (B, 1):
    inputs ``stack((states, targets), dim=2)``, the double-DQN target with ``masks = done`` exactly as
    written, MSE over (b, k), every gradient tensor clamped to [-10, 10], one optimiser step.  Three
    forwards in the reference's order, q(s), q(s'), target(s'), each with its own batch statistics
    (and its own running-statistics update).  Returns the loss."""
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
    for p in q.parameters():
        p.grad.data.clamp_(-grad_clamp, grad_clamp)
    opt.step()
    return loss.detach()


def front_supported(n_nodes: int) -> bool:
    """Whether pbn_gbdq_front's LDS carving (csrc/gbdq_front.h: act [Np][NS], u and v [Np][68], the
    table [16][N], the node codes) fits one block's 160 KiB; the entry point says the same with
    PBN_EINVAL."""
    N = int(n_nodes)
    if not 1 <= N <= 128:
        return False
    al16 = lambda v: (v + 15) & ~15  # noqa: E731
    Np, Kp = al16(N), (N + 3) & ~3
    NS = Kp + (4 - Kp % 32 + 32) % 32
    return 4 * (Np * NS + 2 * Np * 68 + al16(16 * N) + al16(N)) <= 160 * 1024


# ------------------------------------------------------------------------------------ the two rings
def ring_rows(ring: DeviceReplay, idx: torch.Tensor, net_handle=None, spec=None) -> tuple:
    """Rows ``idx`` of one ring as gbdq_update's columns (states, targets, next_states, actions, rewards,
    masks).  On the GPU through pbn_replay_batch (the index list padded to a multiple of 32, the result
    sliced); on the CPU the same rows unpacked in torch."""
    B = idx.shape[0]
    if ring.device.type == "cuda":
        pad = (-B) % 32
        full = torch.cat([idx, idx[:1].expand(pad)]) if pad else idx
        g = ring.gather(full, net_handle)
        Bp, x = full.shape[0], g["x"]
        return (x[0, :B], x[1, :B], x[0, Bp:Bp + B], g["actions"][:B], g["rewards"][:B], g["masks"][:B])
    spec = spec if spec is not None else net_handle.spec
    N = spec.n
    first = torch.zeros(len(spec.attractors) + 1, N)
    for a, att in enumerate(spec.attractors):
        first[a] = torch.tensor(list(att[0]), dtype=torch.float32)
    tg = ring.target[idx].long().clamp(max=len(spec.attractors))
    return (unpack_states(ring.state[:, idx], N).float(), first[tg], unpack_states(ring.next_state[:, idx], N).float(),
            ring.action[idx].long().unsqueeze(-1), ring.reward[idx].reshape(-1, 1), ring.done[idx].float().reshape(-1, 1))


class SplitDeviceReplay:
    """``memory_positive`` and ``memory_negative`` (gbdq_model/__init__.py:159-200): terminated
    transitions go to ``positive``, all others to ``negative`` (two DeviceReplay rings of ``capacity``
    rows each).  ``store`` is a stable partition in env order: the r-th terminated env of the frame goes
    to slot (pos + r) mod capacity of the positive ring, the others to the negative ring likewise; the
    stored ``done`` is terminated | truncated.  On the GPU it is pbn_replay_store_split, with both
    rings' positions and fill levels in device memory (nothing comes back to the host until a sample
    asks for the fill levels); on the CPU the same partition in torch."""

    def __init__(self, capacity: int, words: int, branches: int, device):
        self.capacity = int(capacity)
        self.device = torch.device(device)
        self.positive = DeviceReplay(capacity, words, branches, device)
        self.negative = DeviceReplay(capacity, words, branches, device)
        # pos_p, size_p, pos_n, size_n; then the last store's (positive, negative) counts
        self._ctr = torch.zeros(4, dtype=torch.int64, device=self.device)
        self.counts = torch.zeros(2, dtype=torch.int64, device=self.device)
        self._work: Optional[torch.Tensor] = None
        self._stale = False

    @property
    def action(self) -> torch.Tensor:
        return self.positive.action

    def sync(self) -> None:
        """The host's ``pos`` / ``size`` of both rings, from the device's (one small copy)."""
        if self._stale:
            p, sp, n_, sn = self._ctr.tolist()
            self.positive.pos, self.positive.size, self.negative.pos, self.negative.size = p, sp, n_, sn
            self._stale = False

    def __len__(self) -> int:
        self.sync()
        return self.positive.size + self.negative.size

    def store(self, state, target, action, reward, next_state, flags) -> None:
        """Append a frame: state / next_state (W, n) words, target (n,), action (n, K), reward (n,)
        and the env's ``flags`` (n,) uint8."""
        n = target.shape[0]
        if n > self.capacity:
            raise ValueError("more transitions than a ring holds")
        rp, rn = self.positive, self.negative
        if self.device.type == "cuda":
            if self._work is None or self._work.numel() < (n + 255) // 256:
                self._work = torch.empty((n + 255) // 256, dtype=torch.int32, device=self.device)
            ts = [t.contiguous() for t in (state, next_state, target, action, reward, flags)]
            dt = (torch.int32, torch.int32, torch.uint8, torch.int32, torch.float32, torch.uint8)
            if any(t.dtype != d for t, d in zip(ts, dt)):
                raise ValueError("store: int32 words and actions, uint8 targets and flags, float32 rewards")
            c = self._ctr
            ring = lambda r: (r.state.data_ptr(), r.next_state.data_ptr(), r.target.data_ptr(),  # noqa: E731
                              r.action.data_ptr(), r.reward.data_ptr(), r.done.data_ptr())
            with torch.cuda.device(self.device):
                _lib.check(_lib.load().pbn_replay_store_split(
                    n, rp.words, rp.action.shape[1], *(t.data_ptr() for t in ts), _lib.FLAG_TERMINATED,
                    _lib.FLAG_TERMINATED | _lib.FLAG_TRUNCATED,
                    rp.capacity, c[0:].data_ptr(), c[1:].data_ptr(), *ring(rp),
                    rn.capacity, c[2:].data_ptr(), c[3:].data_ptr(), *ring(rn),
                    self._work.data_ptr(), self.counts.data_ptr(),
                    torch.cuda.current_stream(self.device).cuda_stream), "pbn_replay_store_split")
            self._stale = True
            return
        term = (flags & _lib.FLAG_TERMINATED) != 0
        done = (flags & (_lib.FLAG_TERMINATED | _lib.FLAG_TRUNCATED)) != 0
        for ring, sel in ((rp, term), (rn, ~term)):
            idx = torch.nonzero(sel).reshape(-1)                  # ascending: env order
            ring.store(state[:, idx], target[idx], action[idx], reward[idx], next_state[:, idx], done[idx])
        self.counts.copy_(torch.tensor([int(term.sum()), int((~term).sum())]))
        self._ctr.copy_(torch.tensor([rp.pos, rp.size, rn.pos, rn.size]))

    def sample(self, batch: int, generator: Optional[torch.Generator] = None):
        """min(batch, len) rows of each ring (:99-100), each draw as DeviceReplay.sample_indices:
        (positive rows, negative rows), either possibly empty."""
        self.sync()
        out = []
        for ring in (self.positive, self.negative):
            k = min(int(batch), ring.size)
            out.append(ring.sample_indices(k, generator) if k else torch.zeros(0, dtype=torch.int64, device=self.device))
        return tuple(out)

    def gather(self, idx_p: torch.Tensor, idx_n: torch.Tensor, net_handle=None, spec=None) -> Dict[str, torch.Tensor]:
        """The rows as gbdq_update's batch, positive rows first (:101).  On the GPU through
        pbn_replay_batch (index lists padded to a multiple of 32, the result sliced)."""
        parts = [ring_rows(ring, idx, net_handle, spec) for ring, idx in ((self.positive, idx_p), (self.negative, idx_n))
                 if idx.shape[0]]
        cols = [torch.cat(c, 0) for c in zip(*parts)]
        return dict(zip(("states", "targets", "next_states", "actions", "rewards", "masks"), cols))

    def state_dict(self) -> dict:
        self.sync()
        out = {}
        for prefix, ring in (("positive", self.positive), ("negative", self.negative)):
            for k, v in ring.state_dict().items():
                out[f"{prefix}.{k}"] = v
        out["counts"] = cpu_copy(self.counts)
        return out

    def load_state_dict(self, sd: dict) -> None:
        for prefix, ring in (("positive", self.positive), ("negative", self.negative)):
            ring.load_state_dict({k[len(prefix) + 1:]: v for k, v in sd.items() if k.startswith(prefix + ".")})
        self.counts.copy_(sd["counts"])
        rp, rn = self.positive, self.negative
        self._ctr.copy_(torch.tensor([rp.pos, rp.size, rn.pos, rn.size]))
        self._stale = False


# ------------------------------------------------------------------------------------ acting
_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)


def _explore_words(seed: int, step: int, env_offset: int, n: int, calls: int):
    """The EXPLORE stream's words per env (DESIGN.md "RNG": Philox4x32-7, stream 4, keyed by the seed,
    counters (env id, step, stream << 28 | call)): the CPU stand-in for what the acting kernels draw."""
    mask = np.uint64(0xFFFFFFFF)
    ge = np.arange(n, dtype=np.uint64) + np.uint64(env_offset)
    out = []
    for call in range(calls):
        c0, c1 = ge & mask, np.full(n, step & 0xFFFFFFFF, dtype=np.uint64)
        c2 = np.full(n, (4 << 28) | call, dtype=np.uint64)
        c3 = ((ge >> np.uint64(32)) & np.uint64(0xFFFF)) | np.uint64(((step >> 32) & 0xFFFF) << 16)
        k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
        for _ in range(7):
            p0, p1 = _PHILOX_M0 * c0, _PHILOX_M1 * c2
            c0, c1, c2, c3 = (((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)) & mask, p1 & mask,
                              ((p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)) & mask, p0 & mask)
            k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
        out += [c0, c1, c2, c3]
    return out


class BatchedGBDQ:
    """``GBDQ.predict`` (gbdq_model/__init__.py:75-96) for every env of a VectorPBNEnv: the front
    kernel (pbn_gbdq_front: the packed state -> the (n, N N) activations after bn3, one launch), the
    trunk and heads as torch GEMMs, then pbn_heads_to_flipmask (dueling combination, epsilon-greedy by
    the frozen EXPLORE law -- the reference's ``random.choice(range(action_count))`` per bin is that
    law's uniform draw -- and flip masks).  Where ``front_supported`` says no, and on a CPU device,
    the restated ``per_env=True`` forward stands in for the kernel."""

    def __init__(self, env, qnet: Optional[GraphBranchingQNetwork] = None, branches: int = 5, *, epsilon: float = 0.0):
        N = env.n_nodes
        q = (qnet if qnet is not None else GraphBranchingQNetwork(N, N + 1, int(branches))).to(torch.device(env.device))
        if q.state != N or q.ac_dim != N + 1 or q.n != int(branches):
            raise ValueError("BatchedGBDQ needs GraphBranchingQNetwork(N, N + 1, branches)")
        self._init_front(env, q, branches, epsilon)

    def _init_front(self, env, q, branches: int, epsilon: float) -> None:
        """What every agent on this front shares: the edge list, the action buffer, the targets' first
        states and, where the kernel runs, its image and output."""
        self.env = env
        N = env.n_nodes
        self.branches = int(branches)
        self.device = torch.device(env.device)
        self.q = q
        self.epsilon = float(epsilon)
        self.edges = edge_index(env.spec, device=self.device)
        n = env.n_alloc
        self.actions = torch.empty(n, self.branches, dtype=torch.int32, device=self.device)
        atts = env.spec.attractors
        self._first = torch.zeros(len(atts) + 1, N, dtype=torch.float32, device=self.device)
        for a, att in enumerate(atts):
            self._first[a] = torch.tensor(list(att[0]), dtype=torch.float32)
        self.kernel = self.device.type == "cuda" and front_supported(N)
        self._image, self._image_key = None, None
        if self.kernel:
            start, src = edge_csr(self.edges, N)
            self._csr = (start.to(self.device), src.to(self.device))
            nf = ctypes.c_int64()
            _lib.check(_lib.load().pbn_gbdq_image_floats(env.net.handle, src.numel(), ctypes.byref(nf)),
                       "pbn_gbdq_image_floats")
            self._image = torch.zeros(nf.value, dtype=torch.float32, device=self.device)
            self._front = torch.empty(n, N * N, dtype=torch.float32, device=self.device)

    def capture(self, *args, **kwargs):
        raise NotImplementedError("a captured GBDQ frame is out of scope: the trunk and heads are torch GEMMs and the "
                                  "update is PyTorch's (DESIGN.md 'GBDQ')")

    def pack(self) -> torch.Tensor:
        return self._pack_front()

    def _pack_front(self) -> torch.Tensor:
        """The front kernel's image, repacked (pbn_gbdq_pack) when a graph-layer parameter changed."""
        q = self.q
        ps = [p for m in (q.conv_model1, q.conv_model2, q.conv_model3, q.bn1, q.bn2, q.bn3) for p in m.parameters()]
        key = tuple((p.data_ptr(), p._version) for p in ps)
        if key != self._image_key:
            flat = q.conv_flat()
            start, src = self._csr
            with torch.cuda.device(self.device):
                _lib.check(_lib.load().pbn_gbdq_pack(self.env.net.handle, flat.data_ptr(), src.numel(), start.data_ptr(),
                                                     src.data_ptr(), self._image.data_ptr(), self.env._stream()),
                           "pbn_gbdq_pack")
            self._image_key = key
        return self._image

    def observe(self) -> torch.Tensor:
        """(n, N, 2) fp32: per node the state bit and the bit of the target attractor's first state."""
        env = self.env
        s = unpack_states(env.state, env.n_nodes).float()
        t = self._first[env.target.long().clamp(max=self._first.shape[0] - 1)]
        return torch.stack((s, t), dim=2)

    @torch.no_grad()
    def front(self) -> torch.Tensor:
        """(n, N N): the activations after bn3 + ReLU of every env."""
        env = self.env
        if not self.kernel:
            return self.q.front(self.observe(), self.edges, per_env=True)
        image = self._pack_front()
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pbn_gbdq_front(env.net.handle, env.n_alloc, env.state.data_ptr(), env.target.data_ptr(),
                                                  image.data_ptr(), self._front.data_ptr(), env._stream()),
                       "pbn_gbdq_front")
        return self._front

    @torch.no_grad()
    def heads(self) -> torch.Tensor:
        """The raw head outputs (K + 1, n, A) of every env's observation."""
        return self.q.heads_raw(self.front()).contiguous()

    @torch.no_grad()
    def act(self, epsilon: Optional[float] = None, step_t: Optional[torch.Tensor] = None,
            epsilon_t: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Every env's actions (``self.actions`` (n, K)) and flip masks (``env.flipmask`` (W, n)), keyed
        by the env's next step index; ``step_t`` / ``epsilon_t``: optional one-element device tensors
        (int64 / float32) read when the kernel runs, as BatchedBDQ.act_heads."""
        env = self.env
        eps = self.epsilon if epsilon is None else float(epsilon)
        heads = self.heads()
        A = env.n_nodes + 1
        if self.device.type == "cuda":
            with torch.cuda.device(self.device):
                _lib.check(_lib.load().pbn_heads_to_flipmask(
                    env.net.handle, env.seed, env.step_index, step_t.data_ptr() if step_t is not None else None,
                    env.env_offset, env.n_alloc, self.branches, A, heads.data_ptr(), eps,
                    epsilon_t.data_ptr() if epsilon_t is not None else None, env.flipmask.data_ptr(),
                    self.actions.data_ptr(), env._stream()), "pbn_heads_to_flipmask")
            return env.flipmask
        step = int(step_t.item()) if step_t is not None else env.step_index
        eps = float(epsilon_t.item()) if epsilon_t is not None else eps
        n, K = env.n_alloc, self.branches
        adv = heads[1:].transpose(0, 1)                                  # (n, K, A)
        qv = heads[0, :, :1].unsqueeze(2) + adv - adv.mean(2, keepdim=True)
        w = _explore_words(env.seed, step, env.env_offset, n, (K + 1 + 3) // 4)
        eps_u = int(np.floor(np.float64(np.float32(eps)) * 4294967296.0))
        explore = w[0] < np.uint64(eps_u)
        rnd = np.stack([(w[1 + k] * np.uint64(A)) >> np.uint64(32) for k in range(K)], axis=1).astype(np.int64)
        acts = np.where(explore[:, None], rnd, torch.argmax(qv, dim=2).numpy())
        self.actions.copy_(torch.from_numpy(acts.astype(np.int32)))
        env.flipmask.copy_(actions_to_flipmask(self.actions, env.n_nodes, check=False))
        return env.flipmask

    @torch.no_grad()
    def step(self, epsilon: Optional[float] = None):
        """One frame for every env; returns (state', reward, flags) as VectorPBNEnv.step_flipmask."""
        self.act(epsilon)
        return self.env.step_flipmask(use_current=True)


# ------------------------------------------------------------------------------------ the learner
class GBDQLearner(FrameLearner):
    """``GBDQ.learn`` (gbdq_model/__init__.py:149-251) over a VectorPBNEnv; the defaults are
    ``AgentConfig``'s as train_gbdq.py runs it.  One ``frame()``: act for every env (BatchedGBDQ), step,
    store the transitions in the split replay, ``decrement_epsilon`` (:140-147), and one
    ``update_policy`` when ``frame > max(batch_size, learning_starts)`` (:232; ``frame`` counts from 0).
    ``batch_size`` rows are drawn from each ring.

    ``target_update``: the reference's refresh (:134-138) assigns into a fresh ``state_dict()`` copy and
    so changes nothing; "reference" (the default, as ``mask = done`` is kept for BDQ) leaves the target
    network at its initial weights, "copy" does the hard copy every ``target_net_update_freq`` updates.
    The update is PyTorch's (``gbdq_update`` + torch.optim.Adam); ``capture()`` is not implemented."""

    agent_kind = "gbdq"
    fused = None
    prioritised = False
    _graph = None

    def __init__(self, env, qnet: Optional[GraphBranchingQNetwork] = None, *, branches: int = 5, capacity: int = 10 ** 4,
                 batch_size: int = 512, learning_rate: float = 1e-4, gamma: float = 1.8, target_update: str = "reference",
                 target_net_update_freq: int = 1000, learning_starts: int = 518, epsilon_start: float = 0.0,
                 epsilon_final: float = 0.0, epsilon_decay: int = 10_000, seed: int = 0, episode_stats: bool = False,
                 stats_log_every: int = 0, curriculum: bool = False, curriculum_refresh: int = 1000):
        if target_update not in ("reference", "copy"):
            raise ValueError("target_update must be 'reference' or 'copy'")
        if not env.keep_final_state:
            raise ValueError("GBDQLearner needs the env's final_state (keep_final_state=True)")
        self.env = env
        self.agent = BatchedGBDQ(env, qnet, branches)
        dev = self.agent.device
        self.q = self.agent.q.train()
        N = env.n_nodes
        self.target = GraphBranchingQNetwork(N, N + 1, self.agent.branches).to(dev).train()
        self.target.load_state_dict(self.q.state_dict())
        self.opt = torch.optim.Adam(self.q.parameters(), lr=learning_rate)
        self.replay = SplitDeviceReplay(max(int(capacity), env.n_alloc), env.words, self.agent.branches, dev)
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

    def capture(self, *args, **kwargs):
        self.agent.capture()

    def decrement_epsilon(self) -> float:
        self.time_steps += 1
        if self.time_steps > self.learning_starts:
            self.epsilon = max(self.epsilon_final, self.epsilon - self.epsilon_step)
        return self.epsilon

    def refresh_target(self) -> None:
        """update_policy's tail (:133-138): the counter, and in "copy" mode the hard copy."""
        self.update_counter += 1
        if self.update_counter % self.target_net_update_freq == 0:
            self.update_counter = 0
            if self.target_update == "copy":
                self.target.load_state_dict(self.q.state_dict())

    def update(self) -> torch.Tensor:
        idx_p, idx_n = self.replay.sample(self.batch_size, self.gen)
        batch = self.replay.gather(idx_p, idx_n, getattr(self.env, "net", None), self.env.spec)
        loss = gbdq_update(self.q, self.target, self.opt, batch, self.agent.edges, self.gamma)
        self.updates += 1
        self.refresh_target()
        return loss

    def frame(self):
        env = self.env
        state = env.state.clone()
        target = env.target.clone()
        self.agent.act(self.epsilon)
        _, reward, flags = env.step_flipmask(use_current=True)
        self.replay.store(state, target, self.agent.actions, env.reward, env.final_state, env.flags)
        self._redraw_resets()
        self._track_stats()
        self._refresh_curriculum()
        done = (env.flags[: env.num_envs] & (_lib.FLAG_TERMINATED | _lib.FLAG_TRUNCATED)) != 0
        self.decrement_epsilon()
        f = self.frames
        self.frames += 1
        if f > max(self.batch_size, self.learning_starts):
            self.last_loss = self.update()
        return reward, done

    # ---- checkpoints (learner.py, checkpoint.py)
    def _own_state(self) -> dict:
        return {"frames": int(self.frames), "updates": int(self.updates), "update_counter": int(self.update_counter),
                "time_steps": int(self.time_steps), "epsilon": float(self.epsilon)}

    def _load_own_state(self, own: dict) -> None:
        self.frames, self.updates = int(own["frames"]), int(own["updates"])
        self.update_counter, self.time_steps = int(own["update_counter"]), int(own["time_steps"])
        self.epsilon = float(own["epsilon"])

    def load_state_dict(self, sd: dict) -> None:
        sd = dict(sd)
        for prefix, net in (("q", self.q), ("target", self.target)):
            for k, v in net.state_dict().items():     # (BatchNorm's 0-d num_batches_tracked comes back as [1])
                sd[f"{prefix}.{k}"] = sd[f"{prefix}.{k}"].reshape(v.shape)
        super().load_state_dict(sd)

    def _load_counters(self) -> None:
        pass     # (the split replay refills its own device counters)
