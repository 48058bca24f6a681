"""Every launch of pbn_rl_amd/csrc that clamps its grid, run past the clamp: some thread takes a second
(or third) trip of the grid-stride loop, at sizes just past each cap (tests/grid_caps.py states the
caps and holds the cases; tests/test_grid_caps_host.py holds both to the sources).

All comparisons are exact, over the whole output, against plain numpy on the host: bins, bytes, bit
patterns, with canaries or zeros around what is written.  The one float comparison is the DQN's Q on
an image whose last rows only a second trip of dqn_pack_kernel writes: against the module in float64
at the project's Q tolerance (rtol 1e-5 / atol 1e-5, edge_shapes.check_close)."""
import copy

import numpy as np
import pytest
import torch

from oracle import agent_oracle
from pbn_rl_amd import _lib
from pbn_rl_amd.ddqn import BatchedDDQN, FusedDDQNUpdate
from pbn_rl_amd.replay import DeviceReplay
from pbn_rl_amd.ssd import state_histogram
from pbn_rl_amd.state_table import StateTable
from pbn_rl_amd.vector_env import VectorPBNEnv
from tests import grid_caps as G
from tests import replay_edge_cases as C
from tests import table_limits as tl
from tests.edge_shapes import check_close, edge_spec, u32
from tests.edge_updates import _ring, make_dqn_nets
from tests.test_gpu_evaluate import reduce_np
from tests.test_gpu_state_table import unique_counts

pytestmark = pytest.mark.gpu


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    """A numpy array on the device; uint32 as the int32 the library's tensors hold."""
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def host(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(dtype) if dtype is not None else a


# ---- a. histogram -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", G.HIST_MIXES)
@pytest.mark.parametrize("n_bits", G.HIST_BITS)
@pytest.mark.parametrize("shape", G.HIST_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_histogram_past_the_cap(shape, n_bits, mix):
    """One element past 4096 x 256, a ragged last wave on the second trip, a third trip; every
    element equal (a whole-wave merge each round), five hot bins, and all distinct within a wave (the
    per-lane fallback).  The bin of the uncounted columns stays 0."""
    rows, stride, cols = shape
    assert G.past("hist", rows * cols)
    st = G.hist_input(shape, n_bits, mix)
    if mix == "distinct" and n_bits >= 7:
        assert G.distinct_per_wave(st, cols, n_bits) > 4
    hist = torch.zeros(1 << n_bits, dtype=torch.int32, device="cuda")
    state_histogram(dev(st), cols, n_bits, hist)
    got = host(hist, np.uint32)
    want = G.hist_expected(st, cols, n_bits)
    assert int(want.sum()) == rows * cols
    assert np.array_equal(got, want), (int(got.sum(dtype=np.int64)), rows * cols, np.flatnonzero(got != want)[:8])
    empty = G.hist_empty_bin(shape, n_bits)
    if empty is not None:
        assert got[empty] == 0


# ---- b. copy ----------------------------------------------------------------------------------------
def test_copy_past_one_trip_of_the_capped_grid():
    """pbn_copy_async at 4S - 1 .. 8S + 1 vectors, S the stride of its capped grid: the unrolled
    trip and the single-vector tail both run, for one thread or for all; dst + 16 equals the source
    and the bytes on both sides of it stay zero."""
    L = _lib.load()
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    S, sizes = G.copy_sizes(n_cus)
    assert all(G.copy_stride(n, n_cus) == S for n in sizes)
    assert all(G.past("copy", n, n_cus) for n in sizes[-4:])
    pad = 4096
    top = 16 * max(sizes)
    src = torch.randint(0, 256, (top,), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(7))
    src_np = host(src)
    dst = torch.zeros(16 + top + pad, dtype=torch.uint8, device="cuda")
    for n16 in sizes:
        nbytes = 16 * n16
        dst.zero_()
        _lib.check(L.pbn_copy_async(dst.data_ptr() + 16, src.data_ptr(), nbytes, stream()), "pbn_copy_async")
        got = host(dst)
        assert np.array_equal(got[16:16 + nbytes], src_np[:nbytes]), (n16, S)
        assert not got[:16].any() and not got[16 + nbytes:].any(), (n16, S)


# ---- c. pbn_eval_reduce -----------------------------------------------------------------------------
@pytest.mark.parametrize("max_steps", G.REDUCE_MAX_STEPS)
@pytest.mark.parametrize("n_pairs,runs", G.REDUCE_SHAPES)
def test_eval_reduce_past_2048_blocks(n_pairs, runs, max_steps):
    """2,048 pairs (the last one-trip size) and four sizes past it, up to 254^2 pairs: a block's LDS
    histogram and its s_sum / s_fail slots carry over its pairs.  All-fail and all-zero pairs on the
    first and on a later trip; one shape with counts outside 0..max_steps + 1, which are clamped.  A
    second launch accumulates into the same hist."""
    assert G.past("eval_reduce", n_pairs) != ((n_pairs, runs) == G.REDUCE_AT_CAP)
    L = _lib.load()
    given, clamped, planted = G.reduce_counts(n_pairs, runs, max_steps)
    want_sum, want_fail, want_hist = reduce_np(clamped, max_steps)
    for name, p in planted.items():
        assert want_fail[p] == (runs if name.startswith("fail") else 0), name
        assert want_sum[p] == (runs * (max_steps + 1) if name.startswith("fail") else 0), name
    d_count = dev(given)
    hist = torch.zeros(max_steps + 2, dtype=torch.int64, device="cuda")
    for launch in (1, 2):
        pair_sum = torch.full((n_pairs,), -1, dtype=torch.int64, device="cuda")
        pair_fail = torch.full((n_pairs,), -1, dtype=torch.int32, device="cuda")
        rc = L.pbn_eval_reduce(d_count.data_ptr(), n_pairs, runs, max_steps, pair_sum.data_ptr(), pair_fail.data_ptr(),
                               hist.data_ptr(), stream())
        assert rc == 0, L.pbn_last_error()
        assert np.array_equal(host(pair_sum), want_sum), launch
        assert np.array_equal(host(pair_fail), want_fail), launch
        assert np.array_equal(host(hist), launch * want_hist), launch


# ---- d. pbn_obs_unpack ------------------------------------------------------------------------------
@pytest.mark.parametrize("N,n", G.OBS_CASES)
def test_obs_unpack_past_the_cap(N, n):
    """n * N just past 8192 x 256 float4: the last float4s, which straddle two envs (N mod 4 != 0),
    are written on a second trip.  Both planes, every element."""
    assert G.past("obs_unpack", n * N)
    spec = edge_spec(N)
    st, tg = G.obs_input(spec, n)
    env = VectorPBNEnv(spec, 64)
    guard = 64
    buf = torch.full((guard + 2 * n * N + guard,), -777.0, dtype=torch.float32, device="cuda")
    obs = buf[guard:guard + 2 * n * N]
    d_st, d_tg = dev(st), dev(tg)
    _lib.check(_lib.load().pbn_obs_unpack(env.net.handle, n, d_st.data_ptr(), d_tg.data_ptr(), obs.data_ptr(), stream()),
               "pbn_obs_unpack")
    got = host(buf)
    want = agent_oracle.obs_unpack(spec, st, tg)
    assert np.array_equal(got[guard:-guard].reshape(2, n, N), want)
    assert (got[:guard] == -777.0).all() and (got[-guard:] == -777.0).all()
    A = len(spec.attractors)
    assert not want[1][tg >= A].any() and all(want[1][tg == a].any() for a in range(A) if any(spec.attractors[a][0]))
    env.close()


# ---- e. pbn_replay_store ----------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(G.STORE_VARIANTS))
@pytest.mark.parametrize("W,K", G.STORE_WK)
def test_replay_store_past_the_cap(W, K, variant):
    """1,048,833 rows into a ring of 13 more, from a position that makes the write wrap on the
    second trip; with and without done_mask, done_out and the in-pass state / target copies.
    Every ring field bit for bit; the 13 slots not written keep the canary."""
    n, cap, pos = G.STORE_N, G.STORE_CAPACITY, G.STORE_POS
    assert G.past("replay_store", n)
    done_mask, with_out, with_copies = G.STORE_VARIANTS[variant]
    t = C.store_transitions(n, W, K, seed=W + K + done_mask)
    want, done01 = C.store_expected(cap, W, K, pos, t, done_mask)
    r = DeviceReplay(cap, W, K, torch.device("cuda"))
    for f in C.STORE_FIELDS:
        v = np.array(C.STORE_CANARY[f], want[f].dtype)
        getattr(r, f).fill_(v.view(np.int32).item() if v.dtype == np.uint32 else v.item())
    d = {f: dev(t[f]) for f in C.STORE_FIELDS}
    obuf = torch.full((64 + n + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    kw = {}
    if with_out:
        kw["done_out"] = obuf[64:64 + n]
    if with_copies:      # the destination is the stored state / target itself: read before it is overwritten
        new_tg = ((t["target"].astype(np.int32) + 1) % 256).astype(np.uint8)
        kw["state_copy"] = (d["state"], d["next_state"])
        kw["target_copy"] = (d["target"], dev(new_tg))
    pos_t = torch.tensor([pos], dtype=torch.int64, device="cuda")
    size_t = torch.zeros(1, dtype=torch.int64, device="cuda")
    r.store_at(pos_t, size_t, d["state"], d["target"], d["action"], d["reward"], d["next_state"], d["done"],
               done_mask=done_mask, advance=False, **kw)
    torch.cuda.synchronize()
    assert int(pos_t) == pos and int(size_t) == 0
    for f in C.STORE_FIELDS:
        assert np.array_equal(host(getattr(r, f)).view(np.uint8), want[f].view(np.uint8)), (variant, f)
    assert int((want["done"] == C.STORE_CANARY["done"]).sum()) == cap - n
    out = host(obuf)
    if with_out:
        assert np.array_equal(out[64:64 + n], done01)
    else:
        assert (out[64:64 + n] == 0xAB).all()
    assert (out[:64] == 0xAB).all() and (out[64 + n:] == 0xAB).all()
    if with_copies:
        assert np.array_equal(host(d["state"], np.uint32), t["next_state"]) and np.array_equal(host(d["target"]), new_tg)
    else:
        assert np.array_equal(host(d["state"], np.uint32), t["state"]) and np.array_equal(host(d["target"]), t["target"])


# ---- f. pbn_table_insert ----------------------------------------------------------------------------
@pytest.mark.parametrize("with_counts", [False, True], ids=["ones", "row_counts"])
@pytest.mark.parametrize("W", [1, 4])
def test_table_insert_past_the_cap(W, with_counts):
    """33 x 32,771 rows in one launch into a sized table (grow=False): a ragged last wave on the
    second trip, merges in every wave, row counts with zeros that skip rows.  items() equals
    np.unique weighted by the row counts; nothing is lost."""
    rows, stride, cols = G.TABLE_SHAPE
    assert G.past("table_insert", rows * cols)
    n_bits = 32 * W - 3
    st, mult = G.table_input(W)
    table = StateTable(n_bits, "cuda", capacity=G.TABLE_CAPACITY, grow=False)
    table.add(dev(st), cols, row_counts=torch.from_numpy(mult.view(np.int64)).cuda() if with_counts else None)
    want = unique_counts(st, cols, n_bits, mult if with_counts else None)
    assert 2900 < len(want[0]) <= G.TABLE_POOL
    if with_counts:
        assert int((mult == 0).sum()) > rows * cols // 5 and int(want[1].sum()) == int(mult.sum())
    else:
        assert int(want[1].sum()) == rows * cols
    words, counts = table.items()
    assert table.n_lost == 0 and table.n_growths == 0
    assert np.array_equal(words, want[0]) and np.array_equal(counts, want[1])
    assert len(table) == len(want[0])


# ---- g. DQN pack and target sync --------------------------------------------------------------------
def test_dqn_image_and_target_sync_past_the_caps():
    """hold70_a254 with a (64, 16) DQN: the image's T section alone is 254 x 70 x 64 floats, so the rows
    of targets 235..253 are written by a second trip of dqn_pack_kernel, and parameters + image pass
    ddqn_schedule_kernel's 1024 x 256 vectors.  Q of envs aimed at targets on both sides of that
    offset against the module in float64; the update's image against a fresh pack; the hard target
    copy eager (two pbn_copy_async) and through pbn_ddqn_schedule, due and not due."""
    spec = tl.limit_spec(G.DQN_SPEC)
    N, A, arch, n = spec.n, len(spec.attractors), G.DQN_ARCH, G.DQN_ENVS
    env = VectorPBNEnv(spec, n, seed=17)
    env.reset()
    tg = np.array([G.DQN_TARGETS[e % len(G.DQN_TARGETS)] for e in range(n)], np.uint8)
    tg[list(G.DQN_NO_TARGET)] = 255
    rng = np.random.default_rng(70)
    st = rng.integers(0, 2 ** 32, size=(spec.words, n), dtype=np.uint64).astype(np.uint32)
    st[spec.words - 1] &= np.uint32((1 << (N % 32)) - 1)
    env.set_state(dev(st), dev(tg))
    q_cpu, tgt_cpu = make_dqn_nets(N, arch, seed=3)
    q, tgt = q_cpu.cuda(), tgt_cpu.cuda()
    agent = BatchedDDQN(env, q)
    assert agent.kernel and env.n_alloc == n
    one = G.CAPS["dqn_pack"].elements()
    n_image = agent._image.numel()
    assert G.past("dqn_pack", n_image) and n_image == G.dqn_image_layout(N, A, *arch)[2]
    for t in G.DQN_TARGETS:
        assert (G.dqn_t_row(N, arch[0], t) >= one) == (t >= 235)
    qk = agent.q_values().clone()
    obs = agent_oracle.obs_unpack(spec, st, tg)
    s, g = torch.from_numpy(obs[0]).cuda(), torch.from_numpy(obs[1]).cuda()
    assert float(g[list(G.DQN_NO_TARGET)].abs().sum()) == 0.0
    with torch.no_grad():
        want = copy.deepcopy(q).double()(s.double(), g.double())
        mod = q(s, g)
    check_close(f"Q {G.DQN_SPEC} arch={arch}", qk, want, mod, 1e-5, 1e-5, ("dqn_q", G.DQN_SPEC, arch))

    # one update: the image it leaves equals a fresh pack, bit for bit
    B = 16
    fused = FusedDDQNUpdate(q, tgt, env.net, batch_size=B, learning_rate=1e-3, gamma=0.95)
    assert fused.q_image.numel() == n_image
    R, _ = _ring(spec, 1024, seed=170)
    R.target[:B] = dev(np.array([0, 1, 233, 234, 235, 236, 253, 255] * 2, np.uint8))
    idx = torch.arange(B, dtype=torch.int64, device="cuda")
    before = fused.q_image.clone()
    fused.update(R, idx)
    upd = fused.q_image.clone()
    assert bool((upd[one:] != before[one:]).any())          # the update moved image floats past the cap
    fused.pack("online")
    torch.cuda.synchronize()
    assert torch.equal(upd.view(torch.int32), fused.q_image.view(torch.int32))

    # the hard target copy, eager
    n_flat = fused.q_flat.numel()
    assert G.past("ddqn_schedule", n_flat + n_image)
    bits = lambda x: host(x, np.uint32).copy()  # noqa: E731
    assert not np.array_equal(bits(fused.t_flat), bits(fused.q_flat))
    assert not np.array_equal(bits(fused.t_image)[one:], bits(fused.q_image)[one:])
    fused.sync_target()
    assert np.array_equal(bits(fused.t_flat), bits(fused.q_flat))
    assert np.array_equal(bits(fused.t_image), bits(fused.q_image))

    # and through pbn_ddqn_schedule: a frame that is not due leaves the target alone, a due one copies
    with torch.no_grad():
        fused.t_flat.add_(1.0)
        fused.t_image.fill_(-3.0)
    t_flat0, t_image0 = bits(fused.t_flat), bits(fused.t_image)
    q_flat0, q_image0 = bits(fused.q_flat), bits(fused.q_image)
    beta = torch.tensor([0.5], dtype=torch.float64, device="cuda")
    step = torch.tensor([1007], dtype=torch.int64, device="cuda")
    L = _lib.load()

    def schedule():
        _lib.check(L.pbn_ddqn_schedule(beta.data_ptr(), 0.125, step.data_ptr(), 1000, 4, fused.t_flat.data_ptr(),
                                       fused.q_flat.data_ptr(), n_flat, fused.t_image.data_ptr(),
                                       fused.q_image.data_ptr(), n_image, stream()), "pbn_ddqn_schedule")
        torch.cuda.synchronize()

    schedule()                                               # (1007 - 1000) % 4 != 0
    assert float(beta) == 0.625
    assert np.array_equal(bits(fused.t_flat), t_flat0) and np.array_equal(bits(fused.t_image), t_image0)
    step.fill_(1008)
    schedule()
    assert float(beta) == 0.75
    assert np.array_equal(bits(fused.t_flat), q_flat0) and np.array_equal(bits(fused.t_image), q_image0)
    assert np.array_equal(bits(fused.q_flat), q_flat0) and np.array_equal(bits(fused.q_image), q_image0)
    env.close()
