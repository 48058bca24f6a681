"""Inputs and float64 references of the replay-path edge sweeps (test_gpu_replay_edges.py,
test_gpu_per_edges.py, the store of test_gpu_grid_caps.py), built on the CPU so that test_replay_edges_host.py can check, from the oracle
and the references alone, the conditions under which a wrong kernel cannot pass:

  TD loss      synthetic head tensors at every (B, K, A) where td_loss_kernel changes path: a partial
               last block (B not a multiple of kTdRows = 8), K = 1 and 7, A = 1 .. 128, and a dynamic
               LDS request either side of 64 KB.  Every random case keeps the float64 top-two gap of
               each next-state Q row >= MIN_GAP (an fp32 argmax cannot legitimately differ); the
               tie case is exact in fp32 by construction; the +inf case has one NaN per marked row.
  PER samples  (capacity, size, seed, batches): priorities spread over six decades, the seed picked
               so that p_total's association matters and every large batch reaches both halves;
               and one constructed tree on which the association decides a sampled row.
  ring store   random transitions and the ring pbn_replay_store leaves of them, in numpy (the store past
               its grid cap: test_gpu_grid_caps.py).
  gather       rings over edge_spec(N) whose rows set and clear bit N - 1, with target ids on both
               sides of n_attr.
"""
import itertools

import numpy as np
import torch

from oracle import agent_oracle
from tests.edge_shapes import edge_spec
from tests.per_oracle import PerOracle, replay_uniforms

# ---- TD loss ---------------------------------------------------------------------------------

GAMMA = 0.9
GAMMA32 = float(np.float32(GAMMA))     # what the kernel multiplies by
RC = 1e-5
RC32 = float(np.float32(RC))
MIN_GAP = 1e-3
TD_ROWS = 8                            # csrc/pbn_agent.hip kTdRows

# (B, K, A): partial and single blocks; branch extremes; action extremes (A = 1 skips the argmax
# loop); A = 128 at K = 4 / 5 (61,696 B / 74,048 B of LDS: either side of 64 KB); the largest shape
TD_CASES = ([(B, 3, 29) for B in (1, 7, 8, 9, 33)] + [(9, 1, 29), (9, 7, 29)] +
            [(9, 3, A) for A in (1, 2, 16, 71, 128)] + [(9, 4, 128), (9, 5, 128), (9, 7, 128)])


def td_lds_bytes(K, A):
    """pbn_bdq_td_loss's dynamic LDS request: online rows of both halves and target rows of K + 1
    heads, plus g and the squared error per (row, branch)."""
    return ((K + 1) * 3 * TD_ROWS * A + 2 * TD_ROWS * K) * 4


def dueling(heads):
    """(K + 1, R, A) raw heads -> Q (K, R, A) = (v + adv) - mean(adv) (bdq_model/network.py:59-61)."""
    adv = heads[1:]
    return (heads[0, :, :1].unsqueeze(0) + adv) - adv.mean(2, keepdim=True)


def next_q64(inp):
    """The next-state online Q (K, B, A) in float64."""
    on = inp["online"].double()
    return dueling(on[:, on.shape[1] // 2:])


def top_two_gap(inp):
    q = next_q64(inp)
    if q.shape[2] == 1:
        return float("inf")
    top = q.topk(2, dim=2).values
    return float((top[..., 0] - top[..., 1]).min())


def _td_draw(B, K, A, seed):
    g = torch.Generator().manual_seed(seed)
    inp = {"online": torch.randn(K + 1, 2 * B, A, generator=g), "target": torch.randn(K + 1, B, A, generator=g),
           "actions": torch.randint(0, A, (B, K), generator=g), "rewards": torch.randn(B, generator=g),
           "masks": torch.randint(0, 2, (B,), generator=g).float(), "weights": torch.rand(B, generator=g) + 0.05}
    inp["masks"][0] = 1.0                  # the double-DQN term is live in at least one row ...
    if B > 1:
        inp["masks"][1] = 0.0              # ... and masked in another
    return inp


def td_inputs(B, K, A):
    """Unit-scale head tensors (CPU, fp32): online (K+1, 2B, A), target (K+1, B, A), actions int64
    (B, K), rewards, masks (0 / 1), weights in [0.05, 1.05); reseeded until the float64 top-two gap of
    every next-state Q row is at least MIN_GAP."""
    for s in itertools.count():
        inp = _td_draw(B, K, A, (B * 131 + K) * 257 + A + 100003 * s)
        if top_two_gap(inp) >= MIN_GAP:
            return inp


TIE_SHAPE = (9, 3, 16)


def td_tie_inputs():
    """Every next-state online advantage row holds its maximum at two positions j1 < j2, and the
    target advantage differs there by 0.5.  The next-state rows are multiples of 1/8 of magnitude
    <= 2.5 with A = 16: the sum over A, the division by 16, v + adv and the subtraction are exact in
    fp32, so the fp32 Q row equals the float64 one and ties exactly.  Masks are all 1."""
    B, K, A = TIE_SHAPE
    inp = _td_draw(B, K, A, 7)
    rng = np.random.default_rng(7)
    nxt = rng.integers(-16, 17, size=(K + 1, B, A)).astype(np.float32) / 8
    j = np.sort(np.stack([rng.permutation(A)[:2] for _ in range(B * K)]).reshape(B, K, 2), axis=2)
    j[0, 0] = (0, A - 1)
    for b in range(B):
        for k in range(K):
            nxt[k + 1, b, j[b, k]] = 2.5
            inp["target"][k + 1, b, j[b, k, 1]] = inp["target"][k + 1, b, j[b, k, 0]] + 0.5
    inp["online"][:, B:] = torch.from_numpy(nxt)
    inp["masks"][:] = 1.0
    inp["j1"], inp["j2"] = torch.from_numpy(j[..., 0].copy()), torch.from_numpy(j[..., 1].copy())
    return inp


INF_SHAPE = (9, 3, 29)
INF_AT = [(2, 1, 5), (6, 0, 28), (4, 2, 1)]    # (row b, branch k, position j > 0)


def td_inf_inputs():
    """td_inputs with one +inf in the next-state online advantage row of each INF_AT entry: that
    row's mean is +inf, q_j = inf - inf = NaN and every other q is -inf, so torch.argmax picks j."""
    B, K, A = INF_SHAPE
    inp = {k: v.clone() for k, v in td_inputs(B, K, A).items()}
    for b, k, j in INF_AT:
        inp["online"][k + 1, B + b, j] = float("inf")
        inp["masks"][b] = 1.0
    return inp


def td_reference(inp, dtype=torch.float64, weighted=False, device="cpu"):
    """The comment block above td_loss_kernel in PyTorch at ``dtype``: (loss, priorities or None,
    d loss / d online (K+1, 2B, A) from autograd, a* (K, B)).  Only the first half's rows carry
    gradient; the rest of the gradient buffer is exactly 0."""
    on = inp["online"].to(device=device, dtype=dtype)
    tg = inp["target"].to(device=device, dtype=dtype)
    B = tg.shape[1]
    now = on[:, :B].clone().requires_grad_()
    a = inp["actions"].to(device).t().unsqueeze(2)                       # (K, B, 1)
    cur = dueling(now).gather(2, a).squeeze(2)                           # (K, B)
    am = dueling(on[:, B:]).argmax(2)
    nq = dueling(tg).gather(2, am.unsqueeze(2)).squeeze(2)
    r, m = (inp[k].to(device=device, dtype=dtype) for k in ("rewards", "masks"))
    sq = ((r + (nq * GAMMA32) * m) - cur) ** 2
    prio = None
    if weighted:
        w = inp["weights"].to(device=device, dtype=dtype)
        wl = w * sq.mean(0)
        loss = wl.mean()
        prio = (wl.abs() + RC32).detach()
    else:
        loss = sq.mean()
    grad = torch.zeros_like(on)
    grad[:, :B] = torch.autograd.grad(loss, now)[0]
    return loss.detach(), prio, grad, am


# ---- priority trees --------------------------------------------------------------------------

ALPHA = 0.6
PER_SEED = 99                      # test_gpu_per.SEED: the REPLAY stream's seed

# capacity -> tree_size and what it reaches
PER_CAPACITIES = {2: 2, 3: 4, 200: 256, 300: 512, 512: 512, 513: 1024, 1500: 2048}


def six_decades(rng, n):
    return (10.0 ** rng.uniform(-3.0, 3.0, size=n)).astype(np.float32)


def varied_updates(size, seed):
    """Update batches that give every row of [0, size) a strictly positive priority spread over six
    decades: the rows in a seeded random order, at most 1024 (all distinct) per batch."""
    rng = np.random.default_rng(seed)
    rows, prio = rng.permutation(size).astype(np.int64), six_decades(rng, size)
    return [(rows[i:i + 1024], prio[i:i + 1024]) for i in range(0, size, 1024)]


# (capacity, size, seed of the priorities, batches in draw order, PrioritisedDeviceReplay keywords).
# size 2: only row 0 can be drawn.  size = tree_size / 2 + 1: the prefix walk leaves at node 2
# (rem == w, one term).  size = capacity = tree_size: log2 T terms.  The seeds are the first that
# meet the conditions of test_replay_edges_host.py.
PER_SAMPLE_CASES = [
    (2, 2, 0, (1, 64), {}),
    (200, 2, 0, (65,), {}),
    (200, 200, 1, (1, 63, 1024), {}),
    (200, 129, 0, (64,), {}),
    (300, 257, 0, (65, 1024), {}),
    (512, 512, 0, (1, 63, 64, 65, 1024), {}),
    (512, 511, 5, (64,), {}),
    (513, 513, 0, (63, 1024), {}),
    (1024, 513, 0, (65,), {}),
    (1024, 1024, 0, (1024, 64), {}),
    (1500, 1500, 1, (63, 1024), {}),
    (1500, 1499, 1, (65,), {}),
    (1500, 1025, 0, (64,), {}),
    (512, 512, 1, (64, 64), {"beta": 0.5, "max_beta": 0.5, "beta_step": 0.04}),
]


def per_sample_oracle(cap, size, seed):
    """The oracle after ``size`` rows are stored from position 0 and every row is updated."""
    o = PerOracle(cap, ALPHA)
    o.store(size)
    for idx, prio in varied_updates(size, seed):
        o.update(idx, prio)
    return o


def sequential_prefix(o):
    """The left-to-right fp64 sum of leaves [0, size - 2]: what p_total must not be taken for."""
    s = 0.0
    for x in o.sum_leaves()[:o.size - 1].tolist():
        s += x
    return s


def per_sample_rows(o, batches, beta=0.4):
    """The oracle's rows of each batch, the draw counter starting at 0."""
    return [o.sample(B, beta, replay_uniforms(PER_SEED, c, B))[0] for c, B in enumerate(batches)]


def association_tree():
    """(draw counter, the 8 leaves of a capacity-8 tree) on which one sampled row depends on the
    association of p_total.  The seeded cases above cannot show it: a p_total that is one ulp off
    moves a row only if a search mass lies within an ulp of a node boundary.  Here the prefix terms
    are t = [1, 2^-53, 2^-53]: t_1 + (t_2 + t_3) = 1 + 2^-52, while (t_1 + t_2) + t_3 = 1.  With
    batch 1 the mass is u * p_total for the draw's uniform u in (1/2, 1), a multiple of 2^-53:
    u + 2^-53 =: c for the right p_total, u for the wrong one; and leaves 0 and 1 add up to c exactly
    (leaves 2 and 3 to 1 - c), so ``left > mass`` at node 2 is false for the right p_total (row 2) and
    true for the wrong one (row 1).  The counter is the first whose uniform lies in (1/2, 1)."""
    for ctr in itertools.count():
        u = float(replay_uniforms(PER_SEED, ctr, 1)[0])
        if 0.5 < u < 1.0 - 2.0 ** -52:
            break
    c = u + 2.0 ** -53
    e = 2.0 ** -54
    return ctr, np.array([c / 2, c / 2, (1 - c) / 2, (1 - c) / 2, e, e, 2 * e, 2 * e])


def association_oracle():
    ctr, leaves = association_tree()
    o = PerOracle(8, ALPHA)
    o.size = 8
    o.adopt_leaves(leaves, leaves)
    return ctr, o


# ---- ring store ------------------------------------------------------------------------------

STORE_FIELDS = ("state", "next_state", "target", "action", "reward", "done")
STORE_CANARY = {"state": 0xF9F9F9F9, "next_state": 0xF9F9F9F9, "target": 0xEE, "action": -7, "reward": -7.0,
                "done": 0xEE}


def store_transitions(n, W, K, seed):
    """n random transitions as numpy arrays: state / next_state (W, n) uint32, target (n,) uint8,
    action (n, K) int32, reward (n,) float32, done (n,) uint8 flag bytes (any of the low six bits)."""
    rng = np.random.default_rng(seed)
    word = lambda: rng.integers(0, 2 ** 32, size=(W, n), dtype=np.uint64).astype(np.uint32)  # noqa: E731
    return {"state": word(), "next_state": word(), "target": rng.integers(0, 256, size=n).astype(np.uint8),
            "action": rng.integers(0, 129, size=(n, K)).astype(np.int32),
            "reward": rng.standard_normal(n).astype(np.float32), "done": rng.integers(0, 64, size=n).astype(np.uint8)}


def store_expected(cap, W, K, pos, t, done_mask=0):
    """(ring fields after pbn_replay_store of transitions t at slots (pos + e) mod cap into a ring
    of STORE_CANARY values, the 0 / 1 done values by row): done is flags & done_mask != 0, or
    flags != 0 when done_mask is 0."""
    n = t["target"].shape[0]
    slots = (pos + np.arange(n, dtype=np.int64)) % cap
    done01 = ((t["done"] & np.uint8(done_mask)) != 0 if done_mask else t["done"] != 0).astype(np.uint8)
    ring = {"state": np.full((W, cap), STORE_CANARY["state"], np.uint32),
            "next_state": np.full((W, cap), STORE_CANARY["next_state"], np.uint32),
            "target": np.full(cap, STORE_CANARY["target"], np.uint8),
            "action": np.full((cap, K), STORE_CANARY["action"], np.int32),
            "reward": np.full(cap, STORE_CANARY["reward"], np.float32),
            "done": np.full(cap, STORE_CANARY["done"], np.uint8)}
    ring["state"][:, slots] = t["state"]
    ring["next_state"][:, slots] = t["next_state"]
    ring["target"][slots] = t["target"]
    ring["action"][slots] = t["action"]
    ring["reward"][slots] = t["reward"]
    ring["done"][slots] = done01
    return ring, done01


# ---- batch gather ----------------------------------------------------------------------------

GATHER_N =[31, 32, 33, 64, 65, 96, 97, 127]
GATHER_CAP = 61
GATHER_B = [1, 33, 96]


def gather_ring(N, K, cap=GATHER_CAP):
    """A ring over edge_spec(N) as numpy arrays: random words masked to N bits (row 0 clears and
    row cap - 1 sets bit N - 1 of the state; the next state the other way round), target ids on
    both sides of n_attr (row 0: an attractor whose first state has bit N - 1 set; row 7: 255; row 9:
    n_attr), actions, rewards and 0 / 1 done flags."""
    spec = edge_spec(N)
    W, n_attr = spec.words, len(spec.attractors)
    rng = np.random.default_rng(1000 * N + K)
    last = np.uint32((1 << (N - 32 * (W - 1))) - 1) if N % 32 else np.uint32(0xFFFFFFFF)
    ring = {}
    for name in ("state", "next_state"):
        a = rng.integers(0, 2 ** 32, size=(W, cap), dtype=np.uint64).astype(np.uint32)
        a[W - 1] &= last
        ring[name] = a
    w, bit = (N - 1) >> 5, np.uint32(1 << ((N - 1) & 31))
    ring["state"][w, 0] &= ~bit
    ring["state"][w, cap - 1] |= bit
    ring["next_state"][w, 0] |= bit
    ring["next_state"][w, cap - 1] &= ~bit
    tg = rng.choice(list(range(n_attr)) + [n_attr, n_attr + 1, 200, 255], size=cap).astype(np.uint8)
    high = [a for a, att in enumerate(spec.attractors) if att[0][N - 1]]
    tg[0] = high[0] if high else 0
    tg[7], tg[9] = 255, n_attr
    ring["target"] = tg
    ring["action"] = rng.integers(0, N + 1, size=(cap, K)).astype(np.int32)
    ring["reward"] = rng.standard_normal(cap).astype(np.float32)
    ring["done"] = rng.integers(0, 2, size=cap).astype(np.uint8)
    return spec, ring


def gather_idx(B, cap=GATHER_CAP, seed=0):
    """Rows with duplicates, 0 and cap - 1, and from B = 33 the rows without a target (7 and 9)."""
    rng = np.random.default_rng(seed + B)
    idx = rng.integers(0, cap, size=B).astype(np.int64)
    idx[0] = 0
    if B > 1:
        idx[1] = cap - 1
    if B >= 8:
        idx[2] = idx[3] = idx[4]
        idx[5], idx[6] = 7, 9
    return idx


def gather_expected(spec, ring, idx):
    """x (2, 2B, N) of pbn_replay_batch from agent_oracle.obs_unpack, then actions int64, rewards, masks."""
    obs = agent_oracle.obs_unpack(spec, ring["state"][:, idx], ring["target"][idx])
    nxt = agent_oracle.obs_unpack(spec, ring["next_state"][:, idx], ring["target"][idx])
    return (np.concatenate([obs, nxt], axis=1), ring["action"][idx].astype(np.int64), ring["reward"][idx],
            ring["done"][idx].astype(np.float32))
