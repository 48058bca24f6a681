"""The inputs and the float64 references of the fused updates' edge tests, shared by
test_gpu_learn_edges.py, test_gpu_ddqn_edges.py and test_gpu_adam_state.py: seeded networks built on
the CPU generator, rings with their edge rows, the batch unpacked here (not by the library), and the
PyTorch update on float64 copies.  Every helper takes the device, so the input conditions of a case
(no argmax tie in Q(s')) can be evaluated without a GPU (test_adam_state_seeds_host.py)."""
import copy

import numpy as np
import torch

from pbn_rl_amd.agent import BranchingQNetwork
from pbn_rl_amd.ddqn import DQN, ddqn_update
from pbn_rl_amd.replay import DeviceReplay, bdq_update, soft_update
from tests.edge_shapes import edge_spec, u32
from tests.test_gpu_learn import _filled_replay

# ---- BDQ (pbn_bdq_learn) ----------------------------------------------------------------------------
CAP = 256
ZERO_ROW, ONES_ROW = 0, 1


def make_nets(N, K, seed):
    """The online network and a perturbed target, both built on the CPU generator."""
    torch.manual_seed(seed)
    q = BranchingQNetwork((N, N), N + 1, K)
    tgt = copy.deepcopy(q)
    with torch.no_grad():
        for p in tgt.parameters():
            p.add_(0.01 * torch.randn_like(p))
    return q, tgt


def edge_rows(spec, R):
    """One ring row whose state is all zeros and one whose state has all N bits set."""
    N, W = spec.n, spec.words
    ones = np.full(W, 0xFFFFFFFF, np.uint32)
    if N % 32:
        ones[W - 1] = np.uint32((1 << (N % 32)) - 1)
    R.state[:, ZERO_ROW] = 0
    R.state[:, ONES_ROW] = torch.from_numpy(ones.view(np.int32)).to(R.state.device)


def pick_rows(R, B, seed):
    """B ring rows: the two edge rows, one row without a target, then seeded draws."""
    idx = np.random.default_rng(seed).integers(0, CAP, size=B)
    idx[0], idx[1] = ZERO_ROW, ONES_ROW
    none = np.flatnonzero(R.target.cpu().numpy() == 255)
    idx[2] = none[none > ONES_ROW][0]
    return idx


def bits(words, N):
    """(W, B) uint32 -> (B, N) float64"""
    w = words.T[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]
    return (w & 1).reshape(words.shape[1], -1)[:, :N].astype(np.float64)


def batch_of(spec, R, idx, device, dtype):
    """Rows idx of the ring as bdq_update's batch, unpacked here (not by the library)."""
    N = spec.n
    first = np.zeros((256, N))
    for t, att in enumerate(spec.attractors):
        first[t] = att[0]
    it = torch.from_numpy(idx).to(R.state.device)
    g = first[R.target[it].cpu().numpy()]
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)  # noqa: E731
    return {"obs": to(np.stack([bits(u32(R.state[:, it]), N), g])),
            "next_obs": to(np.stack([bits(u32(R.next_state[:, it]), N), g])),
            "actions": R.action[it].to(device=device, dtype=torch.int64).unsqueeze(-1),
            "rewards": R.reward[it].to(device=device, dtype=dtype).reshape(-1, 1),
            "masks": R.done[it].to(device=device, dtype=dtype).reshape(-1, 1)}


def bdq_ring(spec, K, seed, device="cuda"):
    """test_gpu_learn.py's ring of CAP random transitions, with the two edge rows."""
    R = _filled_replay(spec, K, CAP, seed=seed, device=device)
    edge_rows(spec, R)
    return R


def bdq_top2_gap(q64, b64):
    """The smallest gap between the two largest entries of an online Q(s') row."""
    with torch.no_grad():
        top2 = q64(b64["next_obs"]).topk(2, dim=2)[0]
        return float((top2[..., 0] - top2[..., 1]).min())


def bdq_reference_update(q64, tgt64, b64, lr, gamma, opt=None, **kw):
    """bdq_update on the float64 networks (torch.optim.Adam unless ``opt`` is given); returns the
    loss, and leaves the clamped gradient in the parameters' .grad."""
    opt64 = opt if opt is not None else torch.optim.Adam(q64.parameters(), lr=lr)
    return float(bdq_update(q64, tgt64, opt64, b64, gamma, **kw))


def bdq_trajectory_gaps(N, B, K, lr, ring_seed, row_seed, steps, soft_after=2, gamma=0.9):
    """A pure float64 PyTorch trajectory on the CPU (bdq_update + torch.optim.Adam, the soft target
    update after update ``soft_after``), rows pick_rows(row_seed + k) at update k: the top-2 gap of
    Q(s') before every update."""
    spec = edge_spec(N)
    R = bdq_ring(spec, K, ring_seed, device="cpu")
    q64, tgt64 = (m.double() for m in make_nets(N, K, seed=7))
    opt = torch.optim.Adam(q64.parameters(), lr=lr)
    gaps = []
    for k in range(steps):
        b64 = batch_of(spec, R, pick_rows(R, B, row_seed + k), "cpu", torch.float64)
        gaps.append(bdq_top2_gap(q64, b64))
        bdq_reference_update(q64, tgt64, b64, lr, gamma, opt=opt)
        if k + 1 == soft_after:
            soft_update(tgt64, q64)
    return gaps


# ---- DDQN (pbn_ddqn_learn) --------------------------------------------------------------------------
DDQN_CAP = 1024
ZERO_AT = 5                       # the batch position whose importance weight is 0


def _ring(spec, cap, seed, device="cuda"):
    """A ring of random transitions (one action each; one target in ten missing) and its arrays."""
    dev = torch.device(device)
    R = DeviceReplay(cap, spec.words, 1, dev)
    rng = np.random.default_rng(seed)
    N, W = spec.n, spec.words
    st = rng.integers(0, 2 ** 32, size=(W, cap), dtype=np.uint64).astype(np.uint32)
    nst = rng.integers(0, 2 ** 32, size=(W, cap), dtype=np.uint64).astype(np.uint32)
    if N % 32:
        st[W - 1] &= np.uint32((1 << (N % 32)) - 1)
        nst[W - 1] &= np.uint32((1 << (N % 32)) - 1)
    tg = rng.integers(0, len(spec.attractors), size=cap).astype(np.uint8)
    tg[rng.random(cap) < 0.1] = 255
    a = dict(st=st, nst=nst, tg=tg, act=rng.integers(0, N + 1, size=(cap, 1)).astype(np.int32),
             rew=(1.5 * rng.standard_normal(cap)).astype(np.float32), done=(rng.random(cap) < 0.3).astype(np.uint8))
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    R.store(to(st.view(np.int32)), to(tg), to(a["act"]), to(a["rew"]), to(nst.view(np.int32)), to(a["done"]))
    return R, a


def _bits(words, N):
    """(W, B) uint32 -> (B, N) float32"""
    w = words.T[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]
    return (w & 1).reshape(words.shape[1], -1)[:, :N].astype(np.float32)


def _batch(spec, a, idx, device="cuda"):
    """Rows idx of the ring's arrays as ddqn_update's batch, unpacked here (not by the library)."""
    first = np.zeros((256, spec.n), np.float32)
    for t, att in enumerate(spec.attractors):
        first[t] = att[0]
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)  # noqa: E731
    return {"state": to(_bits(a["st"][:, idx], spec.n)), "target": to(first[a["tg"][idx]]),
            "next_state": to(_bits(a["nst"][:, idx], spec.n)), "action": to(a["act"][idx].astype(np.int64)),
            "reward": to(a["rew"][idx].reshape(-1, 1)), "done": to(a["done"][idx].astype(np.float32).reshape(-1, 1))}


def make_dqn_nets(N, arch, seed):
    """The online network and a perturbed target, both built on the CPU generator."""
    torch.manual_seed(seed)
    q = DQN(N, N + 1, [arch])
    tgt = copy.deepcopy(q)
    with torch.no_grad():
        for p in tgt.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return q, tgt


def ddqn_inputs(N, B, ring_seed, device="cuda"):
    """test_gpu_ddqn.py's _inputs on an edge spec, the weights drawn on the host."""
    spec = edge_spec(N)
    R, a = _ring(spec, DDQN_CAP, seed=ring_seed, device=device)
    rng = np.random.default_rng(B + N)
    idx = rng.integers(0, DDQN_CAP, size=B)
    idx[3] = idx[7] = idx[1]                    # one ring row three times, each with its own weight
    w = (rng.random(B) + 0.05).astype(np.float32)
    w[ZERO_AT] = 0.0
    return spec, B, R, a, idx, w


def batch64_of(batch):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}


def ddqn_conditions(q64, tgt64, batch64, gamma):
    """The reference's input conditions: the smallest top-2 gap of the online Q(s') rows, and |delta|
    per row."""
    with torch.no_grad():
        qn = q64(batch64["next_state"], batch64["target"])
        top2 = qn.topk(2, dim=1)[0]
        gap = float((top2[:, 0] - top2[:, 1]).min())
        y = batch64["reward"] + (1 - batch64["done"]) * gamma * tgt64(batch64["next_state"], batch64["target"]).gather(
            1, qn.argmax(1, keepdim=True))
        delta = (q64(batch64["state"], batch64["target"]).gather(1, batch64["action"]) - y).abs()
    return gap, delta


def ddqn_trajectory_rows(B, row_seed, k):
    """The ring rows of a trajectory's update k."""
    return np.random.default_rng(row_seed + k).integers(0, DDQN_CAP, size=B)


def ddqn_trajectory_gaps(N, arch, B, lr, ring_seed, row_seed, steps, clip_half=False, sync_after=2, gamma=0.95):
    """A pure float64 PyTorch trajectory on the CPU (ddqn_update + torch.optim.Adam, the hard target
    copy after update ``sync_after``): the top-2 gap of Q(s') before every update and every update's
    gradient norm; ``clip_half`` clips at half the first update's norm."""
    spec = edge_spec(N)
    _, a = _ring(spec, DDQN_CAP, seed=ring_seed, device="cpu")
    q64, tgt64 = (m.double() for m in make_dqn_nets(N, arch, seed=7))
    opt = torch.optim.Adam(q64.parameters(), lr=lr)
    gaps, norms, max_norm = [], [], 1e30
    for k in range(steps):
        b64 = batch64_of(_batch(spec, a, ddqn_trajectory_rows(B, row_seed, k), device="cpu"))
        gaps.append(ddqn_conditions(q64, tgt64, b64, gamma)[0])
        if k == 0 and clip_half:
            probe = copy.deepcopy(q64)
            no_step = torch.optim.SGD(probe.parameters(), lr=0.0)
            max_norm = 0.5 * float(ddqn_update(probe, tgt64, no_step, b64, gamma, 1e30)[1])
        norms.append(float(ddqn_update(q64, tgt64, opt, b64, gamma, max_norm)[1]))
        if k + 1 == sync_after:
            tgt64.load_state_dict(q64.state_dict())
    return gaps, norms, max_norm
