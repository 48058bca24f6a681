"""Shared pieces of the GBDQ tests (test_gbdq_host.py, test_gpu_gbdq.py, test_gbdq_edges_host.py,
test_gpu_gbdq_edges.py): the reference's edge routine restated, a synthetic network with a duplicate
self pair and a hub, the literal per-edge forward in any dtype, the edge sweep's cases (node counts at
the layout's edges, edge lists no spec gives, planted NaNs and infinities), the front kernel's raw ABI
with its canaries, the numpy stable partition of the split replay, and an oracle-backed CPU env."""
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
    if name.startswith("size"):
        return size_spec(int(name[4:]))
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


# ---- the edge sweep's cases (test_gbdq_edges_host.py, test_gpu_gbdq_edges.py) -------------------------
# Node counts at the edges of csrc/gbdq_front.h's layout.  1 is the smallest N a pbn_net accepts
# (net_image.h: 1..128): one feature per row, so every deviation is zero and the output relu(beta)
# exactly.  16 = Np (full MFMA tiles, no zero padding), 4 and 64 = Kp steps (no k tail), 64 / 65 =
# bn_relu's second feature per lane, 36 and 100 (and 1, 4, 65) = Kp % 32 == 4 (NS == Kp: act has no
# padding columns), 97.. = four state words, 128 = the ceiling (RT = 8, 146 KB of LDS).
SIZE_N = [1, 4, 15, 16, 17, 36, 63, 64, 65, 100, 127, 128]
_SIZE_SPECS = {}


def size_spec(N: int) -> EnvSpec:
    """random_network(N, 700 + N, max_funcs=2) with min(5, 2^N) random single-state attractors (cached)."""
    from pbn_rl_amd.attractors import random_state_targets
    from tests.synthetic import random_network
    if N not in _SIZE_SPECS:
        _SIZE_SPECS[N] = EnvSpec(random_network(N, 700 + N, max_funcs=2), random_state_targets(N, min(5, 2 ** N), 701 + N))
    return _SIZE_SPECS[N]


EDGE_KINDS = ["isolated", "dense", "empty"]


def custom_edges(N: int, kind: str) -> torch.Tensor:
    """A (2, E) int64 edge tensor in edge_index's convention (row 0 = tops: the sources, row 1 = bots:
    the node that receives the message) that no EnvSpec gives:
      "isolated"  nodes 0 and N - 1 receive nothing, not even their self pair; every other node i its
                  self pair and the nodes i + 1, 3 i mod N and 0 or N - 1 (the isolated nodes still send)
      "dense"     node 0 receives every node twice (in-degree 2 N); the others their self pair only
      "empty"     E = 0"""
    tops, bots = [], []
    if kind == "isolated":
        for i in range(1, N - 1):
            for j in (i, (i + 1) % N, (3 * i) % N, 0 if i & 1 else N - 1):
                tops.append(j)
                bots.append(i)
    elif kind == "dense":
        for j in list(range(N)) * 2:
            tops.append(j)
            bots.append(0)
        for i in range(1, N):
            tops.append(i)
            bots.append(i)
    elif kind != "empty":
        raise ValueError(kind)
    return torch.tensor([tops, bots], dtype=torch.long).reshape(2, len(tops))


NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")
# The planted indices: hidden unit 5, output feature 2, input feature 1 (and N + 1: the Bm half), node 2.
NF_C, NF_O, NF_K, NF_I = 5, 2, 1, 2


def nonfinite_front_cases(N: int):
    """[(name, mutate(q))]: each plants one NaN or infinity in a graph-layer parameter (N >= 3).

    What the literal forward gives for them (NONFINITE_REACH; test_gbdq_edges_host.py asserts it):
    BatchNorm normalises a node's row over its features, and a conv model's parameters are shared by
    every edge, so one non-finite conv parameter reaches one feature (or, from the first Linear, every
    feature) of every node that receives a message, the row's mean and variance, and through them the
    whole row: every entry of the output is NaN ("all") wherever every node has its self pair.  Only
    the BatchNorm parameters are per node: NaN in bn2.weight[i] makes row i NaN after layer 2 and,
    after layer 3, the rows of the nodes that receive from i ("rows"); +inf in bn3.bias[i] makes row i
    +inf ("rows"); -inf in bn1.bias[i] is taken to 0 by the ReLU, as F.relu does, and the output stays
    finite ("none": the case holds the kernel to not inventing a NaN).  The output is behind a ReLU, so
    no case can give -inf."""
    def plant(get, index, value):
        def mutate(q):
            with torch.no_grad():
                get(q)[index] = value
        return mutate
    return [
        ("nan conv1.0.weight", plant(lambda q: q.conv_model1[0].weight, (NF_C, 0), NAN)),
        ("nan conv1.2.bias", plant(lambda q: q.conv_model1[2].bias, NF_O, NAN)),
        ("nan conv2.0.weight A", plant(lambda q: q.conv_model2[0].weight, (NF_C, NF_K), NAN)),
        ("nan conv2.0.weight Bm", plant(lambda q: q.conv_model2[0].weight, (NF_C, N + NF_K), NAN)),
        ("+inf conv3.0.bias", plant(lambda q: q.conv_model3[0].bias, NF_C, PINF)),
        ("-inf conv2.2.weight", plant(lambda q: q.conv_model2[2].weight, (NF_O, NF_C), NINF)),
        ("nan bn2.weight", plant(lambda q: q.bn2.weight, NF_I, NAN)),
        ("+inf bn3.bias", plant(lambda q: q.bn3.bias, NF_I, PINF)),
        ("-inf bn1.bias", plant(lambda q: q.bn1.bias, NF_I, NINF)),
        ("nan bn3.weight", plant(lambda q: q.bn3.weight, NF_I, NAN)),       # beyond the issue's list: one NaN row
    ]


NONFINITE_REACH = {"nan conv1.0.weight": "all", "nan conv1.2.bias": "all", "nan conv2.0.weight A": "all",
                   "nan conv2.0.weight Bm": "all", "+inf conv3.0.bias": "all", "-inf conv2.2.weight": "all",
                   "nan bn2.weight": "rows", "+inf bn3.bias": "rows", "-inf bn1.bias": "none", "nan bn3.weight": "rows"}
NONFINITE_NAMES = list(NONFINITE_REACH)
# q.front gathers x_i and x_j with 0/1 matrix products (EdgeConv), and 0 * NaN is NaN: a NaN row that
# enters a layer reaches every node there, not only the nodes that receive from it.  The literal
# forward (and PyG's EdgeConv, and the kernel) gather by index.
ONEHOT_SPREADS = {"nan bn2.weight"}


def pattern(x: torch.Tensor):
    x = x.detach().cpu()
    return torch.isnan(x), torch.isposinf(x), torch.isneginf(x)


def same_pattern(a: torch.Tensor, b: torch.Tensor) -> bool:
    return all(torch.equal(u, v) for u, v in zip(pattern(a), pattern(b)))


_FRONT_REFS = {}


def front_refs(key, spec, q, n: int, seed: int, edges: torch.Tensor, inputs=None):
    """(words, target, f32, f64, e_ref) of random_inputs(spec, n, seed) (or of ``inputs``): the fp32 and
    float64 literal forwards and e_ref, their maximum distance over the entries finite in both.
    Computed once per ``key`` and shared (callers leave the tensors unchanged)."""
    if key not in _FRONT_REFS:
        words, target = random_inputs(spec, n, seed) if inputs is None else inputs
        x = observation(spec, words, target)
        f32, f64 = literal_front(q, x, edges, torch.float32), literal_front(q, x, edges, torch.float64)
        fin = torch.isfinite(f32) & torch.isfinite(f64)
        e_ref = float((f32.double() - f64)[fin].abs().max()) if bool(fin.any()) else 0.0
        _FRONT_REFS[key] = (words, target, f32, f64, e_ref)
    return _FRONT_REFS[key]


def sweep_case(name: str, kind: str = None, nonfinite: str = None):
    """One case of the edge sweep, its references computed once: (spec, q, edges, words, target, f32,
    f64, e_ref).  ``name``: named_spec's ("size65", "pbn7", "hub"); the network make_q(N, 5, 40 + N,
    bn="random"), 32 envs of random_inputs(seed 6); ``kind``: custom_edges' in place of the spec's
    edge list; ``nonfinite``: the name of a nonfinite_front_cases entry, planted in q."""
    from pbn_rl_amd.gbdq import edge_index
    spec = named_spec(name)
    N = spec.n
    q = make_q(N, 5, 40 + N, bn="random")
    if nonfinite is not None:
        dict(nonfinite_front_cases(N))[nonfinite](q)
    edges = edge_index(spec) if kind is None else custom_edges(N, kind)
    return (spec, q, edges) + front_refs((name, kind, nonfinite), spec, q, 32, 6, edges)


REUSE_ENVS = 2048 + 32      # pbn_gbdq_front launches min(n_envs, 2048) blocks: blocks 0..31 take a second env


def reuse_case(name: str):
    """The block-reuse case: sweep_case's network on 32 distinct inputs whose target ids include
    n_attr - 1, n_attr (no such attractor: zeros, as 255) and 255; (spec, q, edges, words, target, f32,
    f64, e_ref, env_input) with env_input[e] = (e + e // 2048) % 32 for the REUSE_ENVS envs."""
    from pbn_rl_amd.gbdq import edge_index
    spec = named_spec(name)
    N = spec.n
    q = make_q(N, 5, 40 + N, bn="random")
    words, target = random_inputs(spec, 32, 6)
    if N < 16:      # few states: 32 distinct ones
        words[0] = np.random.default_rng(7).permutation(2 ** N)[:32].astype(np.uint32)
    n_attr = len(spec.attractors)
    target[3], target[4], target[5] = n_attr - 1, n_attr, 255
    assert len({(tuple(words[:, e]), int(target[e])) for e in range(32)}) == 32
    e = np.arange(REUSE_ENVS)
    edges = edge_index(spec)
    return (spec, q, edges) + front_refs((name, "reuse"), spec, q, 32, 6, edges, (words, target)) + ((e + e // 2048) % 32,)


def m1_table_numpy(q) -> np.ndarray:
    """csrc/pbn_gbdq.hip's M1[16][N] = W2 relu(W1 in + b1) + b2 in sequential, unfused fp32 sums, with
    F.relu's law (x < 0 ? 0 : x: a NaN stays)."""
    f32 = np.float32
    N = q.state
    w1, b1 = q.conv_model1[0].weight.detach().numpy(), q.conv_model1[0].bias.detach().numpy()
    w2, b2 = q.conv_model1[2].weight.detach().numpy(), q.conv_model1[2].bias.detach().numpy()
    want = np.zeros((16, N), dtype=f32)
    with np.errstate(invalid="ignore"):
        for code in range(16):
            si, ti, sj, tj = (f32((code >> b) & 1) for b in range(4))
            inp = [si, ti, f32(sj - si), f32(tj - ti)]
            acc = np.zeros(N, dtype=f32)
            for c in range(64):
                h = f32(w1[c, 0] * inp[0])
                for k in (1, 2, 3):
                    h = f32(h + f32(w1[c, k] * inp[k]))
                h = f32(h + b1[c])
                h = f32(0) if h < 0 else h
                acc = (acc + (w2[:, c] * h).astype(f32)).astype(f32)
            want[code] = (acc + b2).astype(f32)
    return want


# ---- the raw ABI of the front kernel on the GPU (test_gpu_gbdq.py, test_gpu_gbdq_edges.py) -----------
CANARY = -12345.5
DEV = "cuda"


def _al16(v):
    return (v + 15) & ~15


def image_offsets(N):
    """csrc/gbdq_front.h's image layout."""
    Np, Kp = _al16(N), (N + 3) & ~3
    o = {"m1": 0}
    at = _al16(16 * N)
    o["bn"] = at
    at += _al16(6 * N)
    for l in (0, 1):
        o[f"wu{l}"] = at
        at += _al16(Kp * 128)
        o[f"b1{l}"] = at
        at += 64
        o[f"w2t{l}"] = at
        at += _al16(64 * Np)
        o[f"b2{l}"] = at
        at += _al16(N)
    o["csr_start"] = at
    at += _al16(N + 1)
    o["csr_src"] = at
    return o, Np, Kp


def pack_image(net, spec, q, edges=None, csr=None):
    """pbn_gbdq_pack into an image with 64 canary floats behind it: (image, its floats).  ``edges``: a
    (2, E) tensor in place of edge_index(spec); ``csr``: raw (start, src) int32 tensors in place of
    edge_csr's.  With E = 0 the entry point gets a null d_csr_src."""
    import ctypes

    from pbn_rl_amd.gbdq import edge_csr, edge_index
    L = _lib.load()
    N = spec.n
    start, src = csr if csr is not None else edge_csr(edge_index(spec) if edges is None else edges, N)
    E = src.numel()
    nf = ctypes.c_int64()
    _lib.check(L.pbn_gbdq_image_floats(net.handle, E, ctypes.byref(nf)), "pbn_gbdq_image_floats")
    assert nf.value == image_offsets(N)[0]["csr_src"] + _al16(E)
    image = torch.full((nf.value + 64,), CANARY, dtype=torch.float32, device=DEV)
    flat = q.conv_flat().to(DEV)
    start_d, src_d = start.to(DEV), src.to(DEV)
    _lib.check(L.pbn_gbdq_pack(net.handle, flat.data_ptr(), E, start_d.data_ptr(), src_d.data_ptr() if E else None,
                               image.data_ptr(), torch.cuda.current_stream().cuda_stream), "pbn_gbdq_pack")
    torch.cuda.synchronize()
    assert torch.equal(image[nf.value:].cpu(), torch.full((64,), CANARY))
    return image, nf.value


def run_front(net, spec, image, words, target):
    """pbn_gbdq_front on (W, n) uint32 words and (n,) uint8 targets: (n, N N) on the CPU; 256 canary
    floats behind the output."""
    L = _lib.load()
    n, N = words.shape[1], spec.n
    st = torch.from_numpy(words.view(np.int32)).to(DEV)
    tg = torch.from_numpy(target).to(DEV)
    out = torch.full((n * N * N + 256,), CANARY, dtype=torch.float32, device=DEV)
    _lib.check(L.pbn_gbdq_front(net.handle, n, st.data_ptr(), tg.data_ptr(), image.data_ptr(), out.data_ptr(),
                                torch.cuda.current_stream().cuda_stream), "pbn_gbdq_front")
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(got[n * N * N:], torch.full((256,), CANARY))
    return got[: n * N * N].reshape(n, N * N)


def split_partition(n_prev, flags: np.ndarray, term_mask: int = TERM):
    """The numpy statement of the split store: (positive env indices, negative env indices), each
    ascending (a stable partition in env order).  Positive: any bit of ``term_mask`` set."""
    term = (flags & np.uint8(term_mask)) != 0
    return np.nonzero(term)[0], np.nonzero(~term)[0]


def expected_rings(rings, pos, size, cap, fields, flags, term_mask: int = TERM, done_mask: int = TERM | TRUNC):
    """Apply one frame to numpy copies of both rings: rings = {"p": {field: array}, "n": ...}; cap =
    {"p": capacity_p, "n": capacity_n} (they may differ); the stored done is (flags & done_mask) != 0."""
    ip, in_ = split_partition(None, flags, term_mask)
    done = ((flags & np.uint8(done_mask)) != 0).astype(np.uint8)
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


SPLIT_FLAGS = np.array([0, 1, 2, 3, 4, 17, 18, 33], dtype=np.uint8)     # the env's flag bytes the store tests draw from
SPLIT_FRAMES = ["mixed", "all", "none", "last", "first", "mixed", "all", "none"]


def split_frame(rng, n: int, words: int, K: int, kind: str, flag_values=SPLIT_FLAGS, term_value: int = 1,
                other_value: int = 2):
    """One frame of random transitions, (fields, flags): "mixed" draws every flag from ``flag_values``;
    "all" / "none" set every env to ``term_value`` / ``other_value``; "last" / "first" terminate only
    env n - 1 / env 0; "third" terminates each env with probability 1 / 3."""
    flags = rng.choice(flag_values, size=n).astype(np.uint8)
    if kind == "all":
        flags[:] = term_value
    elif kind == "none":
        flags[:] = other_value
    elif kind in ("last", "first"):
        flags[:] = 0
        flags[n - 1 if kind == "last" else 0] = term_value
    elif kind == "third":
        flags[:] = np.where(rng.random(n) < 1 / 3, term_value, other_value).astype(np.uint8)
    elif kind != "mixed":
        raise ValueError(kind)
    fields = {"state": rng.integers(-2 ** 31, 2 ** 31, size=(words, n)).astype(np.int32),
              "next_state": rng.integers(-2 ** 31, 2 ** 31, size=(words, n)).astype(np.int32),
              "target": rng.integers(0, 255, size=n).astype(np.uint8),
              "action": rng.integers(0, 8, size=(n, K)).astype(np.int32),
              "reward": rng.standard_normal(n).astype(np.float32)}
    return fields, flags


RING_CANARY = {"state": -7, "next_state": -8, "target": 99, "action": -9, "reward": -12345.5, "done": 77}


def canary_rings(cap_p: int, cap_n: int, words: int, K: int):
    """numpy rings filled with RING_CANARY (rows never stored to keep it), and zeroed pos / size."""
    def ring(cap):
        return {"state": np.full((words, cap), -7, np.int32), "next_state": np.full((words, cap), -8, np.int32),
                "target": np.full(cap, 99, np.uint8), "action": np.full((cap, K), -9, np.int32),
                "reward": np.full(cap, -12345.5, np.float32), "done": np.full(cap, 77, np.uint8)}
    return {"p": ring(cap_p), "n": ring(cap_n)}, {"p": 0, "n": 0}, {"p": 0, "n": 0}, {"p": cap_p, "n": cap_n}


def expected_rings_rowwise(rings, pos, size, cap, fields, flags, term_mask: int, done_mask: int):
    """expected_rings stated one env at a time (the law as DESIGN.md words it: the r-th positive env of
    the frame goes to slot (pos + r) mod capacity of the positive ring, the others likewise)."""
    count = {"p": 0, "n": 0}
    for e in range(len(flags)):
        key = "p" if int(flags[e]) & term_mask else "n"
        j = (pos[key] + count[key]) % cap[key]
        count[key] += 1
        r = rings[key]
        r["state"][:, j], r["next_state"][:, j] = fields["state"][:, e], fields["next_state"][:, e]
        r["target"][j], r["action"][j], r["reward"][j] = fields["target"][e], fields["action"][e], fields["reward"][e]
        r["done"][j] = 1 if int(flags[e]) & done_mask else 0
    for key in "pn":
        pos[key] = (pos[key] + count[key]) % cap[key]
        size[key] = min(size[key] + count[key], cap[key])
    return count["p"], count["n"]


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
