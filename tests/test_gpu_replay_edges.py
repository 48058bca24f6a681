"""The replay data path of csrc/pbn_agent.hip at the shapes where its kernels change path
(tests/replay_edge_cases.py; the conditions on the inputs: tests/test_replay_edges_host.py).

TD loss (pbn_bdq_td_loss, pbn_bdq_td_loss_per) on synthetic head tensors, no Q-network involved,
against the comment block above td_loss_kernel evaluated in float64 by PyTorch on the same fp32
inputs, the head gradient from autograd: the loss and the priorities to rtol 1e-5, the whole
gradient buffer to rtol 1e-4 / atol 1e-7 (the project's tolerances for these quantities;
edge_shapes.FLOAT_BOUNDS would list a shape that needs another bound, and none does), rows B..2B-1
of every head and outputs 1..A-1 of head 0 exactly 0.

Ring store (pbn_replay_store) against index_copy_ of the same transitions, batch gather
(pbn_replay_batch) against agent_oracle.obs_unpack and plain indexing, frame advance
(pbn_replay_advance) against the host arithmetic and agent_oracle.replay_rows: all bit for bit, with
canaries around everything written."""
import numpy as np
import pytest
import torch

from oracle import agent_oracle
from pbn_rl_amd import _lib
from pbn_rl_amd.replay import DeviceReplay, _TDLoss, _TDLossPER
from pbn_rl_amd.vector_env import VectorPBNEnv
from tests import replay_edge_cases as C
from tests.edge_shapes import check_close

pytestmark = pytest.mark.gpu

SLACK = 64
GRID = 4096 * 256          # threads of the largest grid the store and the gather launch


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(n, dtype, sentinel):
    """(buffer, its middle n elements): SLACK sentinel elements on either side."""
    buf = torch.full((SLACK + n + SLACK,), sentinel, dtype=dtype, device="cuda")
    return buf, buf[SLACK:SLACK + n]


def assert_guards(buf, n, sentinel, what):
    assert bool((buf[:SLACK] == sentinel).all()) and bool((buf[SLACK + n:] == sentinel).all()), what


# ---- TD loss ---------------------------------------------------------------------------------

def td_kernel(inp, weighted):
    """(loss, priorities or None, d loss / d online) of the HIP entry through its autograd function."""
    on = inp["online"].cuda().requires_grad_()
    a = [inp[k].cuda() for k in ("target", "actions", "rewards", "masks")]
    prio = None
    if weighted:
        prio = torch.full((a[0].shape[1],), -1.0, device="cuda")
        loss = _TDLossPER.apply(on, *a, inp["weights"].cuda(), C.GAMMA, C.RC, prio)
    else:
        loss = _TDLoss.apply(on, *a, C.GAMMA)
    grad, = torch.autograd.grad(loss, on)
    torch.cuda.synchronize()
    return loss.detach(), prio, grad


def check_td(inp, weighted, shape):
    B = inp["target"].shape[1]
    name = f"td{'_per' if weighted else ''} {shape}"
    loss, prio, grad = td_kernel(inp, weighted)
    l64, p64, g64, _ = C.td_reference(inp, weighted=weighted)
    l32, p32, g32, _ = C.td_reference(inp, torch.float32, weighted, device="cuda")
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
    check_close(f"{name} loss", loss.cpu().reshape(1), l64.reshape(1), l32.cpu().reshape(1), 1e-5, 0.0,
                key=("td_loss",) + shape)
    if weighted:
        check_close(f"{name} priorities", prio.cpu(), p64, p32.cpu(), 1e-5, 0.0, key=("td_priorities",) + shape)
    check_close(f"{name} gradient", grad.cpu(), g64, g32.cpu(), 1e-4, 1e-7, key=("td_gradient",) + shape)
    assert not grad[:, B:].any(), "rows B..2B-1 of every head are exactly 0"
    assert not grad[0, :, 1:].any(), "outputs 1..A-1 of the value head are exactly 0"
    return loss, prio, grad


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("B,K,A", C.TD_CASES)
def test_td_loss_at_every_shape(B, K, A, weighted):
    """Partial and single blocks (B = 1, 7, 9, 33 beside 8), K = 1 and 7, A = 1 (no argmax loop) to
    128, and the dynamic LDS request on both sides of 64 KB up to 98,752 B at (9, 7, 128)."""
    check_td(C.td_inputs(B, K, A), weighted, (B, K, A))


@pytest.mark.parametrize("weighted", [False, True])
def test_td_loss_takes_the_first_of_two_maxima(weighted):
    """Every next-state row ties exactly at j1 < j2 (exact in fp32 by construction) and the target
    Q differs there by 0.5 under a mask of 1: taking j2 moves every TD error by 0.45."""
    check_td(C.td_tie_inputs(), weighted, C.TIE_SHAPE)


@pytest.mark.parametrize("weighted", [False, True])
def test_td_loss_takes_a_nan_as_the_maximum(weighted):
    """One +inf in a next-state advantage row: q_j is NaN, the others -inf, a* = j as
    torch.argmax has it; the loss and the gradient stay finite and match."""
    check_td(C.td_inf_inputs(), weighted, C.INF_SHAPE)


@pytest.mark.parametrize("B,K,A", [(9, 3, 29), (33, 1, 29), (9, 7, 128)])
def test_td_loss_per_with_unit_weights_is_the_unweighted_kernel(B, K, A):
    """Weights of exactly 1: the gradient equals pbn_bdq_td_loss's bit for bit (g is scaled by
    1.0f, every other expression is the same).  The loss is not bit-equal by construction: the
    unweighted kernel adds a block's B K squared errors in pair order and scales by 1 / (B K), the
    weighted one adds each row's K terms, divides by K, and adds the rows; it is held to the
    project's rtol 1e-5.  priority = |1 * l_b| + rc against float64."""
    inp = dict(C.td_inputs(B, K, A))
    inp["weights"] = torch.ones(B)
    loss_1, prio_1, grad_1 = check_td(inp, True, (B, K, A))
    loss_0, _, grad_0 = td_kernel(inp, False)
    assert torch.equal(grad_1, grad_0)
    assert torch.allclose(loss_1, loss_0, rtol=1e-5, atol=0), (loss_1.item(), loss_0.item())
    assert torch.allclose(prio_1.mean() - C.RC32, loss_0, rtol=1e-4)


@pytest.mark.parametrize("B,K,A", [(9, 3, 29), (1, 3, 29), (9, 7, 128)])
def test_td_loss_writes_nothing_outside_its_buffers(B, K, A):
    """The C entries on guarded buffers at a partial last block: the gradient, the priorities, the
    per-block partial sums and the loss are all that is written."""
    inp = C.td_inputs(B, K, A)
    on, tg, act, rew, msk, w = (inp[k].cuda() for k in ("online", "target", "actions", "rewards", "masks", "weights"))
    L = _lib.load()
    nb = (B + C.TD_ROWS - 1) // C.TD_ROWS
    for weighted in (False, True):
        gbuf, grad = guarded(on.numel(), torch.float32, -777.0)
        pbuf, prio = guarded(B, torch.float32, -777.0)
        sbuf, scratch = guarded(nb, torch.float32, -777.0)
        lbuf, loss = guarded(1, torch.float32, -777.0)
        if weighted:
            rc = L.pbn_bdq_td_loss_per(on.data_ptr(), tg.data_ptr(), act.data_ptr(), rew.data_ptr(), msk.data_ptr(),
                                       w.data_ptr(), B, K, A, C.GAMMA, C.RC, loss.data_ptr(), grad.data_ptr(),
                                       prio.data_ptr(), scratch.data_ptr(), stream())
        else:
            rc = L.pbn_bdq_td_loss(on.data_ptr(), tg.data_ptr(), act.data_ptr(), rew.data_ptr(), msk.data_ptr(), B, K, A,
                                   C.GAMMA, loss.data_ptr(), grad.data_ptr(), scratch.data_ptr(), stream())
        _lib.check(rc, "pbn_bdq_td_loss")
        torch.cuda.synchronize()
        assert_guards(gbuf, on.numel(), -777.0, "gradient")
        assert_guards(sbuf, nb, -777.0, "partial sums")
        assert_guards(lbuf, 1, -777.0, "loss")
        assert_guards(pbuf, B, -777.0, "priorities")
        assert bool((prio == -777.0).all()) != weighted
        l64, _, g64, _ = C.td_reference(inp, weighted=weighted)
        assert torch.allclose(loss.cpu().double(), l64.reshape(1), rtol=1e-5, atol=0)
        assert torch.allclose(grad.cpu().double().view_as(g64), g64, rtol=1e-4, atol=1e-7)


# ---- ring store ------------------------------------------------------------------------------

FIELDS = ("state", "next_state", "target", "action", "reward", "done")


def canary_ring(cap, W, K):
    r = DeviceReplay(cap, W, K, torch.device("cuda"))
    r.state.fill_(-7)
    r.next_state.fill_(-7)
    r.target.fill_(0xEE)
    r.action.fill_(-7)
    r.reward.fill_(-7.0)
    r.done.fill_(0xEE)
    return r


def transitions(n, W, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    word = lambda: torch.randint(-2 ** 31, 2 ** 31 - 1, (W, n), device="cuda", generator=g,   # noqa: E731
                                 dtype=torch.int64).to(torch.int32)
    return {"state": word(), "next_state": word(),
            "target": torch.randint(0, 256, (n,), device="cuda", generator=g).to(torch.uint8),
            "action": torch.randint(0, 129, (n, K), device="cuda", generator=g).to(torch.int32),
            "reward": torch.randn(n, device="cuda", generator=g),
            "done": torch.randint(0, 2, (n,), device="cuda", generator=g).to(torch.uint8)}


def ring_after(r, pos, t):
    """The ring's fields after index_copy_ of transitions t at slots (pos + e) mod capacity."""
    n = t["target"].shape[0]
    slots = (torch.arange(n, device="cuda") + pos) % r.capacity
    want = {f: getattr(r, f).clone() for f in FIELDS}
    for f in FIELDS:
        want[f].index_copy_(1 if f in ("state", "next_state") else 0, slots, t[f])
    return want, slots


def bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def assert_ring(r, want, what):
    torch.cuda.synchronize()
    for f in FIELDS:
        assert torch.equal(bits(getattr(r, f)), bits(want[f])), (what, f)


def store(r, pos, t, **kw):
    pos_t = torch.tensor([pos], dtype=torch.int64, device="cuda")
    size_t = torch.zeros(1, dtype=torch.int64, device="cuda")
    r.store_at(pos_t, size_t, t["state"], t["target"], t["action"], t["reward"], t["next_state"], t["done"],
               advance=False, **kw)
    assert int(pos_t) == pos and int(size_t) == 0


STORE_CASES = ([(W, K, n, n + 13, n + 13 - (n + 1) // 2) for W, K in ((3, 1), (4, 7)) for n in (1, 255, 257)] +
               [(3, 1, 70, 70, 31), (4, 7, 70, 70, 31), (1, 1, GRID + 33, GRID + 38, GRID - 962)])


@pytest.mark.parametrize("W,K,n,cap,pos", STORE_CASES)
def test_replay_store_matches_index_copy(W, K, n, cap, pos):
    """Three and four state words, one and seven branches, one transition, a block more or less
    one (255, 257), the whole ring from a mid-ring position, and n > 4096 * 256 (the grid-stride
    loop): every field bit for bit, every other ring row still the canary."""
    r = canary_ring(cap, W, K)
    t = transitions(n, W, K, n + W)
    want, slots = ring_after(r, pos, t)
    assert n == 1 or int(slots.min()) == 0                 # (the range wraps)
    store(r, pos, t)
    assert_ring(r, want, (W, K, n))
    assert int((r.done != 0xEE).sum()) == n


def test_replay_store_done_from_flags_at_four_words():
    """done_mask != 0 with done_out at W = 4, K = 7, across the wrap: the ring's done and done_out
    are flags & mask != 0; done_out is written in [0, n) only."""
    n, cap, pos, W, K = 257, 300, 200, 4, 7
    r = canary_ring(cap, W, K)
    t = transitions(n, W, K, 5)
    g = torch.Generator(device="cuda").manual_seed(6)
    flags = torch.randint(0, 64, (n,), device="cuda", generator=g).to(torch.uint8)
    done01 = ((flags & 5) != 0).to(torch.uint8)
    assert bool(done01.any()) and not bool(done01.all()) and bool(((flags != 0) & (done01 == 0)).any())
    want, _ = ring_after(r, pos, dict(t, done=done01))
    obuf, out = guarded(n, torch.uint8, 0xAB)
    store(r, pos, dict(t, done=flags), done_mask=5, done_out=out)
    assert_ring(r, want, "done_mask")
    assert torch.equal(out, done01)
    assert_guards(obuf, n, 0xAB, "done_out")


def test_replay_store_in_pass_copies_at_four_words():
    """state_copy / target_copy at W = 4 with the destination the stored state / target itself:
    the ring gets the values read before the same pass overwrites them."""
    n, cap, pos, W, K = 257, 300, 200, 4, 7
    r = canary_ring(cap, W, K)
    t = transitions(n, W, K, 8)
    want, _ = ring_after(r, pos, t)
    st, tg = t["state"].clone(), t["target"].clone()
    tg_new = ((t["target"].to(torch.int32) + 1) % 256).to(torch.uint8)
    store(r, pos, dict(t, state=st, target=tg), state_copy=(st, t["next_state"]), target_copy=(tg, tg_new))
    assert_ring(r, want, "in-pass copies")
    assert torch.equal(st, t["next_state"]) and torch.equal(tg, tg_new)


# ---- batch gather ----------------------------------------------------------------------------

_NETS = {}


def net_of(spec):
    if id(spec) not in _NETS:
        _NETS[id(spec)] = VectorPBNEnv(spec, 64)
    return _NETS[id(spec)].net


def run_gather(spec, ring, idx, K):
    """pbn_replay_batch through the C entry (any B) into guarded buffers, against gather_expected."""
    B, N, cap = len(idx), spec.n, ring["target"].shape[0]
    dev = {f: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for f, a in ring.items()}
    xb, x = guarded(2 * 2 * B * N, torch.float32, -777.0)
    ab, act = guarded(B * K, torch.int64, -777)
    rb, rew = guarded(B, torch.float32, -777.0)
    mb, msk = guarded(B, torch.float32, -777.0)
    idx_t = torch.from_numpy(idx).cuda()
    _lib.check(_lib.load().pbn_replay_batch(
        net_of(spec).handle, B, idx_t.data_ptr(), cap, dev["state"].data_ptr(), dev["next_state"].data_ptr(),
        dev["target"].data_ptr(), dev["action"].data_ptr(), K, dev["reward"].data_ptr(), dev["done"].data_ptr(),
        x.data_ptr(), act.data_ptr(), rew.data_ptr(), msk.data_ptr(), stream()), "pbn_replay_batch")
    torch.cuda.synchronize()
    want_x, want_a, want_r, want_m = C.gather_expected(spec, ring, idx)
    what = (N, K, B)
    got_x = x.cpu().numpy().reshape(2, 2 * B, N)
    assert np.array_equal(got_x[0], want_x[0]), what
    assert np.array_equal(got_x[1], want_x[1]), what
    assert np.array_equal(act.cpu().numpy().reshape(B, K), want_a), what
    assert np.array_equal(rew.cpu().numpy().view(np.int32), want_r.view(np.int32)), what
    assert np.array_equal(msk.cpu().numpy(), want_m), what
    for buf, n, s in ((xb, 4 * B * N, -777.0), (ab, B * K, -777), (rb, B, -777.0), (mb, B, -777.0)):
        assert_guards(buf, n, s, what)
    return got_x


@pytest.mark.parametrize("N", C.GATHER_N)
def test_replay_batch_at_every_word_edge(N):
    """N on both sides of every state word (W = 1 .. 4), K = 1 and 7, B = 1, 33 and 96 (two of
    them batches DeviceReplay.gather refuses): rows with duplicates, 0 and capacity - 1; target ids
    n_attr and 255 give an all-zero plane 1."""
    for K in (1, 7):
        spec, ring = C.gather_ring(N, K)
        n_attr = len(spec.attractors)
        for B in C.GATHER_B:
            idx = C.gather_idx(B)
            x = run_gather(spec, ring, idx, K)
            none = np.flatnonzero(ring["target"][idx] >= n_attr)
            assert B == 1 or len(none) >= 2
            assert not x[1][none].any() and not x[1][B + none].any()


def test_replay_batch_grid_stride():
    """B = 8192 at N = 70: 2 B N = 1,146,880 elements of a plane against 4096 * 256 threads."""
    spec, ring = C.gather_ring(70, 1)
    assert 2 * 8192 * 70 > GRID
    run_gather(spec, ring, C.gather_idx(8192), 1)


# ---- frame advance ---------------------------------------------------------------------------

def i64(v):
    return torch.tensor([v], dtype=torch.int64, device="cuda")


def advance(n_store, cap, pos, size, step, e64, e32, floor, estep, n_idx, seed, ctr, idx):
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    _lib.check(_lib.load().pbn_replay_advance(n_store, cap, ptr(pos), ptr(size), ptr(step), ptr(e64), ptr(e32), floor,
                                              estep, n_idx, seed, ptr(ctr), ptr(idx), stream()), "pbn_replay_advance")
    torch.cuda.synchronize()


def test_replay_advance_empty_ring_draws_row_zero():
    """Fill level 0 and n_store = 0 (d_pos null): every row is 0, nothing else moves but the counter."""
    size, ctr = i64(0), i64(3)
    ibuf, idx = guarded(300, torch.int64, -777)
    advance(0, 1000, None, size, None, None, None, 0.0, 0.0, 300, 11, ctr, idx)
    assert int(size) == 0 and int(ctr) == 4 and not idx.any()
    assert_guards(ibuf, 300, -777, "idx")


def test_replay_advance_without_rows_keeps_the_counter():
    """n_idx = 0: *counter stays (given or null), while position, fill level and step advance."""
    pos, size, step, ctr = i64(990), i64(995), i64(41), i64(9)
    ibuf, idx = guarded(8, torch.int64, -777)
    advance(40, 1000, pos, size, step, None, None, 0.0, 0.0, 0, 11, ctr, idx)
    assert (int(pos), int(size), int(step), int(ctr)) == (30, 1000, 42, 9)
    assert bool((ibuf == -777).all())
    advance(40, 1000, pos, size, step, None, None, 0.0, 0.0, 0, 11, None, None)
    assert (int(pos), int(size), int(step)) == (70, 1000, 43)


@pytest.mark.parametrize("n_idx", [1, 255, 256, 257])
def test_replay_advance_row_counts_around_the_block(n_idx):
    """One row, and a row fewer, as many and one more than the block's 256 threads; d_step,
    d_eps64 and d_eps32 null."""
    pos, size, ctr = i64(5), i64(700), i64(2 ** 33 + 5)
    ibuf, idx = guarded(n_idx, torch.int64, -777)
    advance(33, 1000, pos, size, None, None, None, 0.0, 0.0, n_idx, 123, ctr, idx)
    assert (int(pos), int(size), int(ctr)) == (38, 733, 2 ** 33 + 6)
    assert np.array_equal(idx.cpu().numpy(), agent_oracle.replay_rows(123, 2 ** 33 + 5, n_idx, 733))
    assert_guards(ibuf, n_idx, -777, "idx")


def test_replay_advance_capacity_one():
    pos, size, step, ctr = i64(0), i64(0), i64(0), i64(0)
    idx = torch.full((65,), -777, dtype=torch.int64, device="cuda")
    for k in range(2):
        advance(1, 1, pos, size, step, None, None, 0.0, 0.0, 65, 5, ctr, idx)
        assert (int(pos), int(size), int(step), int(ctr)) == (0, 1, k + 1, k + 1) and not idx.any()


def test_replay_advance_fill_level_beyond_32_bits():
    """A fill level of 2^40 + 12345 in a ring of 2^41 rows (counters only; no ring memory is
    touched): the rows are the 64-bit multiply-high of the oracle, some above 2^32."""
    size0, cap = 2 ** 40 + 12345, 2 ** 41
    pos, size, ctr = i64(cap - 3), i64(size0), i64(17)
    idx = torch.empty(257, dtype=torch.int64, device="cuda")
    advance(7, cap, pos, size, None, None, None, 0.0, 0.0, 257, 77, ctr, idx)
    assert (int(pos), int(size), int(ctr)) == (4, size0 + 7, 18)
    want = agent_oracle.replay_rows(77, 17, 257, size0 + 7)
    assert want.max() > 2 ** 39 and want.min() < 2 ** 34
    assert np.array_equal(idx.cpu().numpy(), want)


@pytest.mark.parametrize("eps,step,floor", [(0.5, 0.25, 0.25), (0.1, 0.25, 0.25), (0.75, 0.25, 0.25),
                                            (0.30000000000000004, 0.1, 0.2)])
def test_replay_advance_epsilon_at_the_floor(eps, step, floor):
    """Epsilon landing exactly on the floor, already below it, above it, and one rounding away
    from it: max(floor, eps - step) of the host, and its fp32 copy."""
    e64 = torch.tensor([eps], dtype=torch.float64, device="cuda")
    e32 = torch.full((1,), -7.0, dtype=torch.float32, device="cuda")
    size = i64(10)
    advance(0, 100, None, size, None, e64, e32, floor, step, 0, 0, None, None)
    want = max(floor, eps - step)
    assert float(e64) == want and float(e32) == float(np.float32(want)) and int(size) == 10
    e32.fill_(-7.0)
    advance(0, 100, None, size, None, e64, None, floor, step, 0, 0, None, None)
    assert float(e64) == max(floor, want - step) and float(e32) == -7.0
