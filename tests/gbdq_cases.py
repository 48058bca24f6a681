"""Shared pieces of the GBDQ tests (test_gbdq_host.py, test_gpu_gbdq.py): the reference's edge
routine restated, a synthetic network with a duplicate self pair and a hub, the literal per-edge
forward in any dtype, the numpy stable partition of the split replay, and an oracle-backed CPU env."""
import types
from fractions import Fraction

import numpy as np
import torch

from oracle import oracle
from pbn_rl_amd import _lib
from pbn_rl_amd.attractors import load_attractors
from pbn_rl_amd.env import _Graph
from pbn_rl_amd.gbdq import GraphBranchingQNetwork
from pbn_rl_amd.network import Network, NodeFunction, load_network
from pbn_rl_amd.spec import EnvSpec

TERM, TRUNC = _lib.FLAG_TERMINATED, _lib.FLAG_TRUNCATED


def ref_adj_list(spec):
    """GBDQ.get_adj_list (gbdq_model/__init__.py:259-276), its arithmetic over PBNEnv.graph."""
    graph = _Graph(types.SimpleNamespace(spec=spec))
    top_nodes, bot_nodes = [], []
    for top_node in graph.nodes:
        done = set()
        top_nodes.append(top_node.index)
        bot_nodes.append(top_node.index)
        for predictor, _, _ in top_node.predictors:
            for bot_node_id in predictor:
                if bot_node_id not in done:
                    done.add(bot_node_id)
                    top_nodes.append(top_node.index)
                    bot_nodes.append(graph.getNodeByID(bot_node_id).index)
    return torch.tensor([top_nodes, bot_nodes], dtype=torch.long)


def hub_spec(n_nodes: int = 9, **kw) -> EnvSpec:
    """Every node lists node 0 (the hub) and itself: each node has its self pair twice, and node 0
    in-degree N + 1 (the N nodes that list it, and its own self pair)."""
    nodes = [[NodeFunction((0,), 0b10, Fraction(1), [])]]
    nodes += [[NodeFunction((0, i), 0b0110, Fraction(1), [])] for i in range(1, n_nodes)]
    net = Network([f"g{i}" for i in range(n_nodes)], nodes, name=f"hub{n_nodes}")
    rng = np.random.default_rng(5)
    states = sorted({tuple(int(b) for b in rng.integers(0, 2, size=n_nodes)) for _ in range(6)})
    return EnvSpec(net, [[s] for s in states], **kw)


def named_spec(name: str, **kw) -> EnvSpec:
    if name == "hub":
        return hub_spec(**kw)
    return EnvSpec(load_network(name), load_attractors(name), **kw)


def make_q(n_nodes: int, branches: int, seed: int, bn: str = "unit", adv_scale: float = 1.0) -> GraphBranchingQNetwork:
    """A seeded network; bn = "random": gamma in [0.5, 1.5] (some negative), beta in [-0.5, 0.5]."""
    torch.manual_seed(seed)
    q = GraphBranchingQNetwork(n_nodes, n_nodes + 1, branches)
    with torch.no_grad():
        if bn == "random":
            for m in (q.bn1, q.bn2, q.bn3):
                m.weight.copy_((torch.rand(n_nodes) + 0.5) * torch.where(torch.rand(n_nodes) < 0.2, -1.0, 1.0))
                m.bias.copy_(torch.rand(n_nodes) - 0.5)
        for hd in q.adv_heads:
            hd[4].weight.mul_(adv_scale)
    return q


def literal_front(q: GraphBranchingQNetwork, x: torch.Tensor, edges: torch.Tensor, dtype) -> torch.Tensor:
    """The per_env front written literally in ``dtype``: one row per (env, edge), index_add, and the
    per-row BatchNorm from its definition.  (B, N, 2) -> (B, N N)."""
    sd = {k: v.detach().to(dtype) for k, v in q.state_dict().items()}
    top, bot = edges[0], edges[1]
    out = x.to(dtype)
    for l in (1, 2, 3):
        x_i, x_j = out[:, bot], out[:, top]
        h = torch.relu(torch.cat([x_i, x_j - x_i], -1) @ sd[f"conv_model{l}.0.weight"].t() + sd[f"conv_model{l}.0.bias"])
        m = h @ sd[f"conv_model{l}.2.weight"].t() + sd[f"conv_model{l}.2.bias"]
        agg = torch.zeros(out.shape[0], out.shape[1], m.shape[-1], dtype=dtype).index_add_(1, bot, m)
        mean = agg.mean(-1, keepdim=True)
        var = ((agg - mean) ** 2).mean(-1, keepdim=True)
        y = (agg - mean) / torch.sqrt(var + 1e-5)
        out = torch.relu(y * sd[f"bn{l}.weight"][None, :, None] + sd[f"bn{l}.bias"][None, :, None])
    return out.reshape(x.shape[0], -1)


def observation(spec, state_words: np.ndarray, target: np.ndarray) -> torch.Tensor:
    """(n, N, 2) float32 from packed words (W, n) uint32 and target ids (zeros without an attractor)."""
    N = spec.n
    W, n = state_words.shape
    bits = (state_words.T[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
    s = bits.reshape(n, 32 * W)[:, :N].astype(np.float32)
    first = np.zeros((len(spec.attractors) + 1, N), dtype=np.float32)
    for a, att in enumerate(spec.attractors):
        first[a] = np.asarray(att[0], dtype=np.float32)
    tg = np.minimum(np.asarray(target).astype(np.int64), len(spec.attractors))
    return torch.from_numpy(np.stack([s, first[tg]], axis=2))


def random_inputs(spec, n: int, seed: int):
    """State words (W, n) uint32 and targets (n,) uint8: random states, env 0 all zeros, env 1 all
    ones, env 2 (and every 7th) with target id 255."""
    rng = np.random.default_rng(seed)
    N, W = spec.n, spec.words
    bits = rng.integers(0, 2, size=(n, 32 * W)).astype(np.uint64)
    bits[:, N:] = 0
    bits[0] = 0
    bits[1, :N] = 1
    words = (bits.reshape(n, W, 32) << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32).T.copy()
    target = rng.integers(0, max(1, len(spec.attractors)), size=n).astype(np.uint8)
    target[2::7] = 255
    return words, target


def split_partition(n_prev, flags: np.ndarray):
    """The numpy statement of the split store: (positive env indices, negative env indices), each
    ascending (a stable partition in env order)."""
    term = (flags & TERM) != 0
    return np.nonzero(term)[0], np.nonzero(~term)[0]


def expected_rings(rings, pos, size, cap, fields, flags):
    """Apply one frame to numpy copies of both rings: rings = {"p": {field: array}, "n": ...}."""
    ip, in_ = split_partition(None, flags)
    done = ((flags & (TERM | TRUNC)) != 0).astype(np.uint8)
    for key, idx in (("p", ip), ("n", in_)):
        slots = (pos[key] + np.arange(len(idx))) % cap[key]
        r = rings[key]
        r["state"][:, slots] = fields["state"][:, idx]
        r["next_state"][:, slots] = fields["next_state"][:, idx]
        r["target"][slots] = fields["target"][idx]
        r["action"][slots] = fields["action"][idx]
        r["reward"][slots] = fields["reward"][idx]
        r["done"][slots] = done[idx]
        pos[key] = (pos[key] + len(idx)) % cap[key]
        size[key] = min(size[key] + len(idx), cap[key])
    return len(ip), len(in_)


class CpuVectorEnv:
    """VectorPBNEnv's surface on CPU tensors, stepped by the C oracle (the learner's CPU path)."""

    def __init__(self, spec, num_envs: int, seed: int = 0):
        assert num_envs % 32 == 0
        self.spec, self.num_envs, self.n_alloc, self.seed, self.env_offset = spec, num_envs, num_envs, seed, 0
        self.n_nodes, self.words, self.device, self.keep_final_state = spec.n, spec.words, torch.device("cpu"), True
        W, n = self.words, num_envs
        self.state = torch.zeros(W, n, dtype=torch.int32)
        self.final_state = torch.zeros(W, n, dtype=torch.int32)
        self.flipmask = torch.zeros(W, n, dtype=torch.int32)
        self.target = torch.zeros(n, dtype=torch.uint8)
        self.t = torch.zeros(n, dtype=torch.uint8)
        self.reward = torch.zeros(n, dtype=torch.float32)
        self.flags = torch.zeros(n, dtype=torch.uint8)
        self.step_index = 0

    def reset(self):
        st, tg, t = oracle.reset(self.spec, self.seed, self.step_index, 0, self.n_alloc)
        self.state.copy_(torch.from_numpy(st.view(np.int32)))
        self.target.copy_(torch.from_numpy(tg))
        self.t.copy_(torch.from_numpy(t))
        self.step_index += 1

    def step_flipmask(self, use_current=True):
        out = oracle.step(self.spec, self.seed, self.step_index, 0, self.state.numpy().view(np.uint32),
                          self.flipmask.numpy().view(np.uint32), self.target.numpy(), self.t.numpy(), 1)
        self.step_index += 1
        self.state.copy_(torch.from_numpy(out["state_out"].view(np.int32)))
        self.final_state.copy_(torch.from_numpy(out["final_state"].view(np.int32)))
        self.target.copy_(torch.from_numpy(out["target"]))
        self.t.copy_(torch.from_numpy(out["t"]))
        self.reward.copy_(torch.from_numpy(out["reward"]))
        self.flags.copy_(torch.from_numpy(out["flags"]))
        return self.state, self.reward, self.flags

    _STATE = ("state", "target", "t", "flags", "reward", "final_state", "flipmask")

    def state_dict(self):
        out = {k: getattr(self, k).clone() for k in self._STATE}
        out.update(step_index=int(self.step_index), seed=int(self.seed), env_offset=0)
        return out

    def load_state_dict(self, sd):
        for k in self._STATE:
            getattr(self, k).copy_(sd[k])
        self.step_index, self.seed = int(sd["step_index"]), int(sd["seed"])


# ---- the acting test's network and inputs (test_gpu_gbdq.py; their gap budget is checked on the CPU)
ACT_SEED = 31
ACT_ADV_SCALE = 20.0     # wider advantage spreads: fewer near-ties among the top two


def act_inputs(spec, n: int = 96):
    return random_inputs(spec, n, 12)


def act_reference(spec, q, words, target):
    """(keep (n, K) bool: the float64 forward's top-two Q gap exceeds 1e-4; its greedy actions (n, K))."""
    import copy

    from pbn_rl_amd.gbdq import edge_index
    q64 = copy.deepcopy(q).double()
    qv = q64(observation(spec, words, target).double(), edge_index(spec), per_env=True)
    top = qv.topk(2, dim=2).values
    return (top[..., 0] - top[..., 1]) > 1e-4, torch.argmax(qv, dim=2)
