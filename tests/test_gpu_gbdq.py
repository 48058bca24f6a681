"""The GBDQ agent on the GPU (csrc/pbn_gbdq.hip, pbn_rl_amd/gbdq.py; DESIGN.md "GBDQ").

pbn_gbdq_front is held to this rule: with e_ref the maximum distance of the fp32 literal forward (CPU
torch, one row per (env, edge)) to the float64 literal forward on the same inputs, the kernel's maximum
distance to float64 is at most 8 e_ref.  The margin covers the reordered sums, the pre-combined A - Bm
and the division by a small per-row deviation; the measured ratios are in DESIGN.md "GBDQ"."""
import copy

import numpy as np
import pytest
import torch

from oracle import agent_oracle, oracle
from pbn_rl_amd import _lib
from pbn_rl_amd.gbdq import BatchedGBDQ, GBDQLearner, SplitDeviceReplay, edge_csr, edge_index, gbdq_update
from pbn_rl_amd.vector_env import VectorPBNEnv
from tests import gbdq_cases as gc

pytestmark = pytest.mark.gpu

CANARY, DEV = gc.CANARY, gc.DEV
image_offsets, pack_image, run_front = gc.image_offsets, gc.pack_image, gc.run_front      # (shared with the edge sweep)


@pytest.fixture(scope="module")
def nets():
    cache = {}

    def get(name):
        if name not in cache:
            spec = gc.named_spec(name)
            cache[name] = (spec, _lib.NetHandle(spec))
        return cache[name]
    yield get
    for _, h in cache.values():
        h.close()


@pytest.mark.parametrize("bn", ["unit", "random"])
@pytest.mark.parametrize("name,n", [("pbn7", 32), ("pbn28", 96), ("bb33", 32), ("pbn70", 32), ("hub", 96)])
def test_front_kernel_within_eight_times_the_fp32_error(nets, name, n, bn):
    """N = 7 (one partly filled tile), 28, 33 (two words), 70 (three words, a k tail), and the hub
    network (duplicate self pairs, in-degree N + 1); all-zero and all-one states; target id 255."""
    spec, net = nets(name)
    q = gc.make_q(spec.n, 5, 40 + spec.n, bn=bn)
    words, target = gc.random_inputs(spec, n, 6)
    x = gc.observation(spec, words, target)
    e = edge_index(spec)
    f64 = gc.literal_front(q, x, e, torch.float64)
    e_ref = float((gc.literal_front(q, x, e, torch.float32).double() - f64).abs().max())
    image, _ = pack_image(net, spec, q)
    got = run_front(net, spec, image, words, target)
    err = float((got.double() - f64).abs().max())
    print(f"gbdq front {name} n={n} bn={bn}: e_ref {e_ref:.3e} kernel {err:.3e} ratio {err / e_ref:.2f}")
    assert torch.isfinite(got).all()
    assert err <= 8 * e_ref
    again = run_front(net, spec, image, words, target)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))       # two runs, equal bits


@pytest.mark.parametrize("name", ["pbn7", "pbn70", "hub", "size64", "size65", "size128"])
def test_front_kernel_zero_variance_gives_relu_beta(nets, name):
    """Zero conv weights with constant biases: every (env, node) row is constant, its variance zero,
    and the output relu(beta) exactly, without a NaN.  (size64 / size65: the last N with one feature
    per lane and the first with two; size128: both features on every lane.)"""
    spec, net = nets(name)
    N = spec.n
    q = gc.make_q(N, 5, 3, bn="random")
    with torch.no_grad():
        for m in (q.conv_model1, q.conv_model2, q.conv_model3):
            m[0].weight.zero_()
            m[2].weight.zero_()
            m[0].bias.fill_(0.5)
            m[2].bias.fill_(0.25)
    words, target = gc.random_inputs(spec, 32, 8)
    image, _ = pack_image(net, spec, q)
    got = run_front(net, spec, image, words, target)
    want = torch.relu(q.bn3.bias.detach())[None, :, None].expand(32, N, N).reshape(32, N * N)
    diff = (got - want).abs()
    print(f"gbdq front zero variance {name}: max |got - relu(beta)| {float(diff.max()):.3e} at {int(diff.argmax())}")
    assert torch.isfinite(got).all() and torch.equal(got, want)


@pytest.mark.parametrize("name", ["pbn7", "pbn70", "size16", "size65", "size128"])
def test_pack_table_and_segments_bit_for_bit(nets, name):
    """M1 against the sequential, unfused fp32 sums the header states; the [A - Bm | Bm] and transposed
    second-Linear segments with their zero padding; the edge list.  (size16, size128: full tiles, no
    zero padding at all; size65: a Kp-row tail of three zero rows and 15 zero tile columns.)"""
    spec, net = nets(name)
    N = spec.n
    q = gc.make_q(N, 5, 17, bn="random")
    image, nf = pack_image(net, spec, q)
    img = image[:nf].cpu().numpy()
    off, Np, Kp = image_offsets(N)
    want = gc.m1_table_numpy(q)     # (F.relu's law, x < 0 ? 0 : x: equal to max(x, 0) on these finite sums)
    assert np.array_equal(img[: 16 * N].reshape(16, N), want)
    for l, m in ((0, q.conv_model2), (1, q.conv_model3)):
        W1, W2 = m[0].weight.detach().numpy(), m[2].weight.detach().numpy()
        wu = img[off[f"wu{l}"]: off[f"wu{l}"] + Kp * 128].reshape(Kp, 128)
        assert np.array_equal(wu[:N, :64], (W1[:, :N] - W1[:, N:]).T) and np.array_equal(wu[:N, 64:], W1[:, N:].T)
        assert not wu[N:].any()
        w2t = img[off[f"w2t{l}"]: off[f"w2t{l}"] + 64 * Np].reshape(64, Np)
        assert np.array_equal(w2t[:, :N], W2.T) and not w2t[:, N:].any()
        assert np.array_equal(img[off[f"b1{l}"]: off[f"b1{l}"] + 64], m[0].bias.detach().numpy())
        assert np.array_equal(img[off[f"b2{l}"]: off[f"b2{l}"] + N], m[2].bias.detach().numpy())
    start, src = edge_csr(edge_index(spec), N)
    ints = img.view(np.int32)
    assert np.array_equal(ints[off["csr_start"]: off["csr_start"] + N + 1], start.numpy())
    assert np.array_equal(ints[off["csr_src"]: off["csr_src"] + src.numel()], src.numpy())


def test_front_rejects_bad_arguments(nets):
    spec, net = nets("pbn7")
    L = _lib.load()
    buf = torch.zeros(64 * 49, dtype=torch.float32, device=DEV)
    assert L.pbn_gbdq_front(net.handle, 33, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None) == -22
    assert b"multiple of 32" in L.pbn_last_error()
    assert L.pbn_gbdq_front(net.handle, 32, None, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None) == -22
    assert L.pbn_gbdq_front(None, 32, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None) == -22


# ------------------------------------------------------------------------------------ acting
@pytest.mark.parametrize("name,K", [("pbn7", 1), ("pbn28", 5)])
def test_act_equals_heads_to_flipmask_on_the_cpu_forward(name, K):
    spec = gc.named_spec(name)
    N, n = spec.n, 96
    env = VectorPBNEnv(spec, n, seed=9)
    env.reset()
    words, target = gc.act_inputs(spec, n)
    env.set_state(torch.from_numpy(words.view(np.int32)).to(DEV), torch.from_numpy(target).to(DEV))
    q = gc.make_q(N, K, gc.ACT_SEED, adv_scale=gc.ACT_ADV_SCALE)
    keep, _ = gc.act_reference(spec, q, words, target)
    assert float((~keep).float().mean()) <= 0.01
    q_cpu = copy.deepcopy(q)
    agent = BatchedGBDQ(env, q, branches=K)
    assert agent.kernel
    x = gc.observation(spec, words, target)
    assert torch.equal(agent.observe().cpu(), x)
    heads_cpu = q_cpu.heads_raw(q_cpu.front(x, edge_index(spec), per_env=True)).detach().contiguous().to(DEV)
    L = _lib.load()
    for eps in (0.0, 1.0):
        agent.act(eps)
        torch.cuda.synchronize()
        acts, flip = agent.actions.cpu().numpy().copy(), env.flipmask.cpu().numpy().copy()
        flip_ref = torch.zeros_like(env.flipmask)
        acts_ref = torch.zeros_like(agent.actions)
        _lib.check(L.pbn_heads_to_flipmask(env.net.handle, env.seed, env.step_index, None, 0, n, K, N + 1,
                                           heads_cpu.data_ptr(), eps, None, flip_ref.data_ptr(), acts_ref.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream), "pbn_heads_to_flipmask")
        torch.cuda.synchronize()
        kp = keep.numpy() if eps == 0.0 else np.ones((n, K), dtype=bool)
        assert np.array_equal(acts[kp], acts_ref.cpu().numpy()[kp]), eps
        rows = kp.all(1)
        assert np.array_equal(flip[:, rows], flip_ref.cpu().numpy()[:, rows]), eps
        if eps == 1.0:      # the EXPLORE law's draws exactly
            qv = np.zeros((n, K, N + 1), dtype=np.float32)
            want_flip, want_acts = agent_oracle.q_to_flipmask(spec, qv, env.seed, env.step_index, 0, 1.0)
            assert np.array_equal(acts, want_acts) and np.array_equal(flip.view(np.uint32), want_flip)
    with pytest.raises(NotImplementedError):
        agent.capture()
    env.close()


# ------------------------------------------------------------------------------------ the split store
def _numpy_rings(rp):
    return {k: {f: getattr(r, f).cpu().numpy().copy() for f in ("state", "next_state", "target", "action", "reward", "done")}
            for k, r in (("p", rp.positive), ("n", rp.negative))}


@pytest.mark.parametrize("n,cap,words", [(32, 32, 1), (32, 80, 3), (4096, 4096, 1), (4096, 10000, 3)])
def test_replay_store_split_equals_the_numpy_partition(n, cap, words):
    """All terminated, none, one terminated env at index n - 1, mixed frames until each ring wraps;
    capacity == n; one and three state words; rows not stored to keep their canary values."""
    rng = np.random.default_rng(n + words)
    K = 5
    rp = SplitDeviceReplay(cap, words, K, DEV)
    for r in (rp.positive, rp.negative):
        r.state.fill_(-7), r.next_state.fill_(-8), r.target.fill_(99), r.action.fill_(-9), r.reward.fill_(CANARY)
        r.done.fill_(77)
    rings = _numpy_rings(rp)
    pos, size, capd = {"p": 0, "n": 0}, {"p": 0, "n": 0}, {"p": cap, "n": cap}
    frames = ["mixed", "all", "none", "last", "mixed", "mixed", "all", "none"]
    for kind in frames:
        flags = rng.choice(np.array([0, 1, 2, 3, 4, 17, 18, 33], dtype=np.uint8), size=n)
        if kind == "all":
            flags[:] = 1
        elif kind == "none":
            flags[:] = 2
        elif kind == "last":
            flags[:] = 0
            flags[n - 1] = 1
        fields = {"state": rng.integers(-2 ** 31, 2 ** 31, size=(words, n)).astype(np.int32),
                  "next_state": rng.integers(-2 ** 31, 2 ** 31, size=(words, n)).astype(np.int32),
                  "target": rng.integers(0, 255, size=n).astype(np.uint8),
                  "action": rng.integers(0, 8, size=(n, K)).astype(np.int32),
                  "reward": rng.standard_normal(n).astype(np.float32)}
        t = {k: torch.from_numpy(v).to(DEV) for k, v in fields.items()}
        rp.store(t["state"], t["target"], t["action"], t["reward"], t["next_state"], torch.from_numpy(flags).to(DEV))
        cp, cn = gc.expected_rings(rings, pos, size, capd, fields, flags)
        assert rp.counts.tolist() == [cp, cn], kind
        assert rp._ctr.tolist() == [pos["p"], size["p"], pos["n"], size["n"]], kind
        got = _numpy_rings(rp)
        for key in "pn":
            for f, want in rings[key].items():
                assert np.array_equal(got[key][f].view(np.uint8), want.view(np.uint8)), (kind, key, f)
    rp.sync()
    assert (rp.positive.pos, rp.positive.size, rp.negative.pos, rp.negative.size) == (pos["p"], size["p"], pos["n"], size["n"])
    assert size["p"] == cap and size["n"] == cap      # both rings wrapped


def test_replay_store_split_leaves_unwritten_rows_alone():
    rp = SplitDeviceReplay(64, 1, 5, DEV)
    rp.positive.reward.fill_(CANARY), rp.negative.reward.fill_(CANARY)
    n = 32
    flags = torch.zeros(n, dtype=torch.uint8, device=DEV)
    flags[5] = 1
    z = torch.zeros(1, n, dtype=torch.int32, device=DEV)
    rp.store(z, flags, torch.zeros(n, 5, dtype=torch.int32, device=DEV), torch.ones(n, device=DEV), z, flags)
    assert rp.positive.reward.tolist() == [1.0] + [CANARY] * 63
    assert rp.negative.reward.tolist() == [1.0] * 31 + [CANARY] * 33
    assert len(rp) == 32 and rp.positive.done[0].item() == 1 and int(rp.negative.done.sum()) == 0
    L = _lib.load()
    assert L.pbn_replay_store_split(*([0] * 2 + [1] + [None] * 6 + [0, 0] + [0, None, None] + [None] * 6
                                      + [0, None, None] + [None] * 6 + [None, None, None])) == -22


# ------------------------------------------------------------------------------------ the learner
def _gpu_learner(seed=4, n=64, **kw):
    spec = gc.named_spec("pbn7", horizon=5)
    env = VectorPBNEnv(spec, n, seed=seed)
    env.reset()
    args = dict(batch_size=32, learning_starts=0, capacity=512, epsilon_start=0.5, epsilon_final=0.1, epsilon_decay=10,
                target_update="copy", target_net_update_freq=3, seed=seed)
    args.update(kw)
    return GBDQLearner(env, gc.make_q(7, 5, 8), **args)


def test_learner_stores_the_oracle_transitions():
    """Twenty frames on pbn7 with 64 envs: both rings hold what the oracle chain gives for the agent's
    actions, terminated rows in the positive ring, in env order."""
    n, seed = 64, 4
    lr = _gpu_learner(seed=seed, n=n, learning_starts=1000)      # no update: the rings alone
    spec, env = lr.env.spec, lr.env
    st, tg, t = oracle.reset(spec, seed, 0, 0, n)
    rows = {"p": [], "n": []}
    for k in range(20):
        step = env.step_index
        lr.frame()
        torch.cuda.synchronize()
        acts = lr.agent.actions.cpu().numpy()
        flip = np.zeros((1, n), dtype=np.uint32)
        for b in range(5):
            a = acts[:, b].astype(np.int64)
            flip[0] |= np.where(a > 0, np.left_shift(np.uint32(1), np.maximum(a - 1, 0).astype(np.uint32)), 0).astype(np.uint32)
        ref = oracle.step(spec, seed, step, 0, st, flip, tg, t, 1)
        for e in range(n):
            key = "p" if ref["flags"][e] & 1 else "n"
            rows[key].append((int(st[0, e]), int(tg[e]), tuple(acts[e]), float(ref["reward"][e]),
                              int(ref["final_state"][0, e]), int((ref["flags"][e] & 3) != 0)))
        st, tg, t = ref["state_out"], ref["target"], ref["t"]
    assert len(rows["p"]) > 0 and len(rows["n"]) > 0 and len(lr.replay) == min(len(rows["p"]), 512) + min(len(rows["n"]), 512)
    for key, ring in (("p", lr.replay.positive), ("n", lr.replay.negative)):
        want = rows[key]
        assert ring.size == min(len(want), 512)
        S, T, A = ring.state.cpu().numpy().view(np.uint32), ring.target.cpu().numpy(), ring.action.cpu().numpy()
        R, NS, D = ring.reward.cpu().numpy(), ring.next_state.cpu().numpy().view(np.uint32), ring.done.cpu().numpy()
        for r, w in enumerate(want):
            if r < len(want) - 512:
                continue                                              # overwritten since
            j = r % 512
            assert (int(S[0, j]), int(T[j]), tuple(A[j]), float(R[j]), int(NS[0, j]), int(D[j])) == w, (key, r)


def test_gpu_update_matches_the_cpu_update():
    """The GPU update's loss and clamped gradients against the CPU gbdq_update on the same rows: the
    loss to rtol 1e-5, the gradients to rtol 1e-3 / atol 1e-6 (test_gpu_learn.py's for the PyTorch path)."""
    lr = _gpu_learner(learning_starts=1000)
    for _ in range(10):
        lr.frame()
    idx_p, idx_n = lr.replay.sample(32, lr.gen)
    assert idx_p.numel() > 0 and idx_n.numel() == 32
    batch = lr.replay.gather(idx_p, idx_n, lr.env.net, lr.env.spec)
    cpu_batch = {k: v.cpu() for k, v in batch.items()}
    q_cpu, t_cpu = copy.deepcopy(lr.q).cpu(), copy.deepcopy(lr.target).cpu()
    opt_cpu = torch.optim.Adam(q_cpu.parameters(), lr=1e-4)
    loss = gbdq_update(lr.q, lr.target, lr.opt, batch, lr.agent.edges, 1.8)
    loss_cpu = gbdq_update(q_cpu, t_cpu, opt_cpu, cpu_batch, edge_index(lr.env.spec), 1.8)
    print(f"gbdq update: loss gpu {float(loss):.8e} cpu {float(loss_cpu):.8e}")
    assert torch.allclose(loss.cpu(), loss_cpu, rtol=1e-5)
    for (name, p), pc in zip(lr.q.named_parameters(), q_cpu.parameters()):
        assert torch.allclose(p.grad.cpu(), pc.grad, rtol=1e-3, atol=1e-6), (name, (p.grad.cpu() - pc.grad).abs().max().item())


def test_gpu_learner_resume_is_bit_equal(tmp_path):
    k = 40
    a = _gpu_learner()
    for _ in range(k):
        a.frame()
    assert a.updates == k - 33
    path = str(tmp_path / "gbdq.npz")
    a.save(path)
    for _ in range(k):
        a.frame()
    b = _gpu_learner()
    b.load(path)
    for _ in range(k):
        b.frame()
    torch.cuda.synchronize()
    want, got = a.state_dict(), b.state_dict()
    assert want.keys() == got.keys()
    for key, v in want.items():
        assert torch.equal(v, got[key]) if isinstance(v, torch.Tensor) else v == got[key], key
    assert a.updates == 2 * k - 33 and torch.isfinite(a.last_loss)
