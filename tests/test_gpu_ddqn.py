"""The DDQN / DDQNPER agent on the GPU (pbn_rl_amd/ddqn.py, csrc/pbn_ddqn.hip): the acting launch
against DQN.forward and pbn_q_to_flipmask, the fused update against the PyTorch update it replaces
(ddqn_update + torch.optim.Adam) and against the reference's own update (tests/golden/ddqn_update.npz),
weights and determinism, DDQNLearner against the oracle chain, and evaluate_control with a DQN.

Tolerances are those of the BDQ tests for the same comparisons: the kernel's Q against the module's
rtol 1e-5 / atol 1e-5 (test_gpu_agent.py); loss, norm and priorities rtol 1e-5; the clipped gradient
rtol 1e-3 / atol 1e-6; the Adam step from the kernel's own gradient rtol 1e-5 / atol 1e-7; the image
after an update bit-equal to a fresh pack (test_gpu_learn.py, test_gpu_learn_per.py)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle
from pbn_rl_amd import _lib
from pbn_rl_amd.attractors import load_attractors
from pbn_rl_amd.ddqn import DQN, BatchedDDQN, DDQNLearner, FusedDDQNUpdate, ddqn_update
from pbn_rl_amd.evaluate import evaluate_control
from pbn_rl_amd.network import load_network
from pbn_rl_amd.replay import DeviceReplay
from pbn_rl_amd.spec import EnvSpec
from pbn_rl_amd.vector_env import VectorPBNEnv
from tests.edge_updates import ZERO_AT, _batch, _ring
from tests.golden_parts import load_parts

pytestmark = pytest.mark.gpu

RC = 1e-5
N_ENVS, CAP = 96, 1024
# (network, net_arch, B): one tile; train_ddqn.py's; A = 34 crosses the 32-output tile; W = 3 state
# words; unequal widths, neither a multiple of 16
SHAPES = [("pbn7", [(8, 8)], 16), ("pbn28", [(50, 50)], 64), ("bb33", [(50, 50)], 32), ("pbn70", [(64, 64)], 16),
          ("pbn7", [(20, 40)], 16)]
IDS = ["pbn7-8x8", "pbn28-50x50", "bb33-50x50", "pbn70-64x64", "pbn7-20x40"]
_SPECS = {}


def make_spec(net):
    if net not in _SPECS:
        _SPECS[net] = EnvSpec(load_network(net), load_attractors(net))
    return _SPECS[net]


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def _nets(N, arch, seed):
    torch.manual_seed(seed)
    q = DQN(N, N + 1, arch)
    tgt = copy.deepcopy(q)
    with torch.no_grad():
        for p in tgt.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return q.cuda(), tgt.cuda()


def _inputs(net, B):
    spec = make_spec(net)
    env = VectorPBNEnv(spec, N_ENVS)
    R, a = _ring(spec, CAP, seed=100 + B + spec.n)
    idx = np.random.default_rng(B).integers(0, CAP, size=B)
    idx[3] = idx[7] = idx[1]                    # one ring row three times, each with its own weight
    w = torch.rand(B, device="cuda", generator=torch.Generator(device="cuda").manual_seed(B)) + 0.05
    w[ZERO_AT] = 0.0
    return spec, env, R, a, idx, torch.from_numpy(idx).cuda(), w


# ---- acting ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,arch,B", SHAPES, ids=IDS)
def test_acting_launch_matches_the_module_and_the_explore_law(net, arch, B):
    spec = make_spec(net)
    N, seed = spec.n, 17
    env = VectorPBNEnv(spec, N_ENVS, seed=seed)
    env.reset()
    env.target[5] = 255                              # envs without a target
    env.target[64] = 255
    q, _ = _nets(N, arch, seed=3)
    agent = BatchedDDQN(env, q)
    assert agent.kernel
    qk = agent.q_values().clone()
    assert qk.shape == (N_ENVS, N + 1)
    s, g = BatchedDDQN(env, q, kernel=False).observe()   # pbn_obs_unpack's observation
    assert float(g[5].abs().sum()) == 0.0
    with torch.no_grad():
        want = q(s, g)
    assert torch.allclose(qk, want, rtol=1e-5, atol=1e-5), (qk - want).abs().max().item()
    L = _lib.load()
    flip_ref = torch.zeros_like(env.flipmask)
    act_ref = torch.zeros(N_ENVS, dtype=torch.int32, device="cuda")
    step_t = torch.full((1,), env.step_index, dtype=torch.int64, device="cuda")
    for eps in (0.0, 0.3, 1.0):
        agent.act_q(eps)
        acts, flip = agent.actions.clone(), env.flipmask.clone()
        _lib.check(L.pbn_q_to_flipmask(env.net.handle, env.seed, env.step_index, env.env_offset, N_ENVS, 1, N + 1,
                                       qk.data_ptr(), eps, flip_ref.data_ptr(), act_ref.data_ptr(), None),
                   "pbn_q_to_flipmask")
        torch.cuda.synchronize()
        assert torch.equal(acts, act_ref), eps
        assert torch.equal(flip, flip_ref), eps
        if eps == 0.0:
            assert torch.equal(acts.long(), qk.argmax(1))
        agent.actions.zero_()
        agent.act_q(0.9, step_t=step_t, epsilon_t=torch.full((1,), eps, device="cuda"))   # the device's values win
        assert torch.equal(agent.actions, act_ref) and torch.equal(env.flipmask, flip_ref), eps
    assert 0 < int((act_ref != qk.argmax(1)).sum())      # eps = 1 explored
    # the flip mask is the action's node bit
    a = act_ref.cpu().numpy()
    fm = u32(flip_ref)
    for e in range(N_ENVS):
        want_w = np.zeros(spec.words, np.uint32)
        if a[e] > 0:
            want_w[(a[e] - 1) >> 5] = np.uint32(1) << np.uint32((a[e] - 1) & 31)
        assert np.array_equal(fm[:, e], want_w), e


def test_image_holds_the_contracted_bilinear_layer():
    spec = make_spec("bb33")
    env = VectorPBNEnv(spec, 32)
    q, _ = _nets(spec.n, [(20, 40)], seed=5)
    agent = BatchedDDQN(env, q)
    img = agent.image()
    n_attr, N = len(spec.attractors), spec.n
    T = img[:n_attr * N * 32].view(n_attr, N, 32)
    x = torch.tensor([list(a[0]) for a in spec.attractors], dtype=torch.float32, device="cuda")
    want = torch.einsum("tj,oij->tio", x, q.input.weight.detach())
    assert torch.allclose(T[:, :, :20], want, rtol=1e-5, atol=1e-6)
    assert float(T[:, :, 20:].abs().sum()) == 0.0


# ---- the update against PyTorch -------------------------------------------------------------------
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("net,arch,B", SHAPES, ids=IDS)
def test_fused_update_matches_pytorch(net, arch, B, clip):
    spec, env, R, a, idx, idx_t, w = _inputs(net, B)
    N = spec.n
    q, tgt = _nets(N, arch, seed=7)
    q_ref, tgt_ref = copy.deepcopy(q), copy.deepcopy(tgt)
    lr, gamma = 1e-3, 0.95
    max_norm = 0.02 if clip else 10.0
    batch = _batch(spec, a, idx)
    # the PyTorch side's input conditions: no argmax tie in Q(s'), |delta| on both sides of 1
    with torch.no_grad():
        qn = q_ref(batch["next_state"], batch["target"])
        top2 = qn.topk(2, dim=1)[0]
        assert float((top2[:, 0] - top2[:, 1]).min()) > 1e-4
        y = batch["reward"] + (1 - batch["done"]) * gamma * tgt_ref(batch["next_state"], batch["target"]).gather(
            1, qn.argmax(1, keepdim=True))
        delta = (q_ref(batch["state"], batch["target"]).gather(1, batch["action"]) - y).abs()
        assert bool((delta < 1).any()) and bool((delta > 1).any())
    fused = FusedDDQNUpdate(q, tgt, env.net, batch_size=B, learning_rate=lr, gamma=gamma, max_grad_norm=max_norm,
                            keep_grad=True)
    p0 = [p.detach().clone() for p in q.parameters()]
    versions = [p._version for p in q.parameters()]
    prio = torch.full((B,), -1.0, device="cuda")
    loss = float(fused.update(R, idx_t, weights=w, priorities_out=prio, replay_constant=RC))
    torch.cuda.synchronize()
    # the module's parameters alias the flat buffer, and the in-place update moved their versions
    assert q.input.weight.data_ptr() == fused.q_flat.data_ptr()
    assert all(p._version > v for p, v in zip(q.parameters(), versions))
    opt = torch.optim.Adam(q_ref.parameters(), lr=lr)
    prio_ref = torch.full((B,), -1.0, device="cuda")
    loss_ref, norm_ref = ddqn_update(q_ref, tgt_ref, opt, batch, gamma, max_norm, weights=w, priorities_out=prio_ref,
                                     replay_constant=RC)
    loss_ref, norm_ref = float(loss_ref), float(norm_ref)
    assert (norm_ref > max_norm) == clip, norm_ref
    norm = float(fused.grad_norm)
    print(f"{net} {arch} B={B} clip={clip}: loss {loss!r} ref {loss_ref!r}; norm {norm!r} ref {norm_ref!r}; "
          f"priorities max rel {((prio - prio_ref).abs() / prio_ref).max().item():.3g}")
    assert abs(loss - loss_ref) <= 1e-5 * abs(loss_ref), (loss, loss_ref)
    assert abs(norm - norm_ref) <= 1e-5 * norm_ref, (norm, norm_ref)
    assert torch.allclose(prio, prio_ref, rtol=1e-5, atol=0), ((prio - prio_ref).abs() / prio_ref).max().item()
    assert prio[ZERO_AT].item() == torch.tensor(RC, dtype=torch.float32).item()      # |0 * h| + rc, exactly
    assert (prio > 0).all() and not torch.equal(prio[1], prio[3])                    # one row, two weights
    names = [n for n, _ in q.named_parameters()]
    for name, g, p in zip(names, fused.grads(), q_ref.parameters()):
        assert torch.allclose(g, p.grad, rtol=1e-3, atol=1e-6), (name, (g - p.grad).abs().max().item())
    b1, b2, eps = 0.9, 0.999, 1e-8
    for name, g, before, after in zip(names, fused.grads(), p0, q.parameters()):
        m, v = (1 - b1) * g, (1 - b2) * g * g
        want = before - (lr / (1 - b1)) * m / (v.sqrt() / (1 - b2) ** 0.5 + eps)
        assert torch.allclose(after, want, rtol=1e-5, atol=1e-7), (name, (after - want).abs().max().item())
    assert float(fused.step) == 1.0
    upd = fused.q_image.clone()
    fused.pack("online")
    torch.cuda.synchronize()
    assert torch.equal(upd, fused.q_image)


# ---- the update against the reference's own ---------------------------------------------------------
@pytest.mark.parametrize("call", ["ddqn_a", "ddqn_b", "per_a", "per_b"])
@pytest.mark.parametrize("prefix,net,N,B", [("s7", "pbn7", 7, 16), ("s28", "pbn28", 28, 64)])
def test_fused_update_matches_the_reference_learn_step(prefix, net, N, B, call):
    """pbn_ddqn_learn held to DDQN._learn_step / DDQNPER._learn_step through tests/golden/ddqn_update.npz
    (tools/gen_ddqn_golden.py; ddqn_update is held to it in tests/test_ddqn_host.py).  Loss, norm and
    priorities rtol 1e-5; clipped gradients rtol 1e-3 / atol 1e-6; parameters after Adam atol 1e-5
    where the reference gradient exceeds 1e-4 (one Adam step is ~lr there), else within two steps."""
    d = load_parts(__file__.replace("test_gpu_ddqn.py", "golden/ddqn_update.npz"))
    spec = make_spec(net)
    env = VectorPBNEnv(spec, 32)
    dev = torch.device("cuda")
    arch = [tuple(int(x) for x in r) for r in d[prefix + ".arch"]]
    names = [str(n) for n in d[prefix + ".names"]]
    q, tgt = DQN(N, N + 1, arch).to(dev), DQN(N, N + 1, arch).to(dev)
    q.load_state_dict({n: torch.from_numpy(d[f"{prefix}.q0.{n}"]) for n in names})
    tgt.load_state_dict({n: torch.from_numpy(d[f"{prefix}.t0.{n}"]) for n in names})
    key, p = f"{prefix}.{call}", prefix + ".b."
    lr = float(d["lr"])
    fused = FusedDDQNUpdate(q, tgt, env.net, batch_size=B, learning_rate=lr, gamma=float(d["gamma"]),
                            max_grad_norm=float(d[key + ".max_grad_norm"]), keep_grad=True)
    bits = (1 << np.arange(N, dtype=np.uint32))
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    R = DeviceReplay(B, 1, 1, dev)
    st = (d[p + "states"].astype(np.uint32) * bits).sum(1).astype(np.uint32)[None]
    nst = (d[p + "next_states"].astype(np.uint32) * bits).sum(1).astype(np.uint32)[None]
    R.store(to(st.view(np.int32)), to(d[p + "target_ids"]), to(d[p + "actions"].astype(np.int32).reshape(B, 1)),
            to(d[p + "rewards"]), to(nst.view(np.int32)), to(d[p + "done"]))
    idx = torch.arange(B, dtype=torch.int64, device=dev)
    per = call.startswith("per")
    w = to(d[p + "weights"]) if per else None
    prio = torch.empty(B, device=dev) if per else None
    loss = float(fused.update(R, idx, weights=w, priorities_out=prio, replay_constant=float(d["replay_constant"])))
    torch.cuda.synchronize()
    want, want_norm = float(d[key + ".loss"]), float(d[key + ".norm"])
    print(f"{key}: loss {loss!r} ref {want!r}; norm {float(fused.grad_norm)!r} ref {want_norm!r}")
    assert abs(loss - want) <= 1e-5 * abs(want), (loss, want)
    assert abs(float(fused.grad_norm) - want_norm) <= 1e-5 * want_norm
    if per:
        assert torch.allclose(prio, to(d[key + ".priorities"]), rtol=1e-5, atol=0)
    for n, g, wt in zip(names, fused.grads(), q.parameters()):
        g_ref = to(d[f"{key}.g.{n}"])
        assert torch.allclose(g, g_ref, rtol=1e-3, atol=1e-6), (n, (g - g_ref).abs().max().item())
        err = (wt.detach() - to(d[f"{key}.q1.{n}"])).abs()
        big = g_ref.abs() > 1e-4
        assert err[big].max().item() <= 1e-5 if big.any() else True, (n, err[big].max().item())
        assert err.max().item() <= 2.1 * lr, (n, err.max().item())


# ---- weights and determinism ----------------------------------------------------------------------
@pytest.mark.parametrize("net,arch,B", SHAPES[:3], ids=IDS[:3])
def test_unit_weights_and_reruns_are_bit_equal(net, arch, B):
    spec, env, R, a, idx, idx_t, _ = _inputs(net, B)
    q1, t1 = _nets(spec.n, arch, seed=7)
    nets = [(q1, t1)] + [(copy.deepcopy(q1), copy.deepcopy(t1)) for _ in range(2)]
    kw = dict(batch_size=B, learning_rate=1e-3, gamma=0.95, max_grad_norm=0.3, keep_grad=True)
    f = [FusedDDQNUpdate(q, t, env.net, **kw) for q, t in nets]
    ones = torch.ones(B, device="cuda")
    prio = torch.full((B,), -1.0, device="cuda")
    for u in range(2):
        f[0].update(R, idx_t)
        f[1].update(R, idx_t, weights=ones, priorities_out=prio, replay_constant=RC)
        f[2].update(R, idx_t)
        torch.cuda.synchronize()
        for name in ("q_flat", "m", "v", "step", "q_image", "grad", "loss", "grad_norm"):
            assert torch.equal(getattr(f[0], name), getattr(f[2], name)), (u, name)      # two runs, one state
            assert torch.equal(getattr(f[0], name), getattr(f[1], name)), (u, name)      # unit weights
        assert (prio >= RC).all()
    assert float(f[0].step) == 2.0


def test_sync_target_copies_parameters_and_image():
    spec, env, R, a, idx, idx_t, _ = _inputs("bb33", 32)
    q, t = _nets(33, [(50, 50)], seed=2)
    fused = FusedDDQNUpdate(q, t, env.net, batch_size=32)
    fused.update(R, idx_t)
    assert not torch.equal(fused.q_flat, fused.t_flat) and not torch.equal(fused.q_image, fused.t_image)
    versions = [p._version for p in t.parameters()]
    fused.sync_target()
    torch.cuda.synchronize()
    assert torch.equal(fused.q_flat, fused.t_flat) and torch.equal(fused.q_image, fused.t_image)
    assert all(torch.equal(a_, b_) for a_, b_ in zip(t.state_dict().values(), q.state_dict().values()))
    assert all(p._version > v for p, v in zip(t.parameters(), versions))
    with torch.no_grad():                       # weights changed outside update(): the next use repacks
        q.output.bias.add_(1.0)
    before = fused.q_image.clone()
    assert fused.acting_image() is fused.q_image
    torch.cuda.synchronize()
    assert not torch.equal(before, fused.q_image)


def test_acting_falls_to_pytorch_for_a_network_the_kernel_does_not_take():
    spec = make_spec("pbn7")
    env = VectorPBNEnv(spec, 32, seed=1)
    env.reset()
    torch.manual_seed(0)
    deep = DQN(7, 8, [(8, 8), (8, 8)]).cuda()
    agent = BatchedDDQN(env, deep)
    assert not agent.kernel
    agent.act_q(0.0)
    torch.cuda.synchronize()
    assert torch.equal(agent.actions.long(), agent.q_values().argmax(1))
    with pytest.raises(ValueError, match="one hidden Linear"):
        BatchedDDQN(env, deep, kernel=True)


def test_update_refuses_bad_arguments():
    spec, env, R, a, idx, idx_t, w = _inputs("pbn7", 16)
    q, t = _nets(7, [(8, 8)], seed=1)
    fused = FusedDDQNUpdate(q, t, env.net, batch_size=16)
    with pytest.raises(ValueError, match="priorities_out is required with weights"):
        fused.update(R, idx_t, weights=w)
    with pytest.raises(ValueError, match="16 int64 ring indices"):
        fused.update(R, idx_t[:8])
    L = _lib.load()
    nb = ctypes.c_int64()
    assert L.pbn_ddqn_learn_workspace(7, 8, 8, 16, ctypes.byref(nb)) == 0
    args = lambda work, nbytes, image: (  # noqa: E731
        env.net.handle, 8, 8, 16, idx_t.data_ptr(), R.capacity, R.state.data_ptr(), R.next_state.data_ptr(),
        R.target.data_ptr(), R.action.data_ptr(), R.reward.data_ptr(), R.done.data_ptr(), fused.q_flat.data_ptr(),
        image, fused.t_image.data_ptr(), fused.m.data_ptr(), fused.v.data_ptr(), fused.step.data_ptr(), 1e-3, 0.9,
        0.999, 1e-8, 0.95, 10.0, work, nbytes, fused.loss.data_ptr(), fused.grad_norm.data_ptr(), None, None, RC,
        None, None)
    assert L.pbn_ddqn_learn(*args(fused.work.data_ptr(), nb.value - 4, fused.q_image.data_ptr())) == -22
    assert "workspace too small" in L.pbn_last_error().decode()
    assert L.pbn_ddqn_learn(*args(fused.work.data_ptr() + 4, nb.value, fused.q_image.data_ptr())) == -22
    assert "16-byte aligned" in L.pbn_last_error().decode()
    assert L.pbn_ddqn_learn(*args(fused.work.data_ptr(), nb.value, None)) == -22
    assert "null network image" in L.pbn_last_error().decode()
    assert float(fused.step) == 0.0


# ---- the learner ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "pytorch"])
@pytest.mark.parametrize("prioritised", [True, False], ids=["per", "uniform"])
def test_learner_frames_follow_the_oracle_and_the_schedules(prioritised, fused):
    spec = make_spec("pbn28")
    seed, frames = 23, 12
    torch.manual_seed(1)
    env = VectorPBNEnv(spec, N_ENVS, seed=seed)
    lr = DDQNLearner(env, net_arch=[(50, 50)], total_frames=frames, capacity=CAP, batch_size=64, target_update=4,
                     exploration_fraction=0.5, prioritised=prioritised, fused=fused, seed=5)
    assert (lr.fused is not None) == fused
    env.reset()
    st, tg, t = oracle.reset(spec, seed, 0, 0, N_ENVS)
    rp = lr.replay
    for f in range(frames):
        eps = max(0.05, 1.0 - f * 0.95 / (0.5 * frames))
        beta = min(1.0, 0.4 + f * 0.6 / (0.75 * frames))
        assert lr.epsilon == pytest.approx(eps, abs=1e-12) and lr.beta == pytest.approx(beta, abs=1e-12)
        step, pos = env.step_index, rp.pos
        lr.frame()
        torch.cuda.synchronize()
        # the stored transitions are the oracle's for the same actions, done = TERMINATED only
        acts = lr.agent.actions.cpu().numpy()
        flip = np.zeros((spec.words, N_ENVS), np.uint32)
        flip[0, acts > 0] = np.uint32(1) << (acts[acts > 0] - 1).astype(np.uint32)
        assert np.array_equal(u32(env.flipmask), flip), f
        ref = oracle.step(spec, seed, step, 0, st, flip, tg, t, 1)
        rows = (pos + torch.arange(N_ENVS, device="cuda")) % CAP          # (the ring wraps in frame 10)
        assert np.array_equal(u32(rp.state[:, rows]), st), f
        assert np.array_equal(rp.target[rows].cpu().numpy(), tg), f
        assert np.array_equal(rp.action[rows, 0].cpu().numpy(), acts), f
        assert np.array_equal(u32(rp.next_state[:, rows]), ref["final_state"]), f
        assert np.array_equal(rp.reward[rows].cpu().numpy(), ref["reward"]), f
        assert np.array_equal(rp.done[rows].cpu().numpy(), ref["flags"] & 1), f
        assert np.array_equal(u32(env.state), ref["state_out"]), f
        st, tg, t = ref["state_out"], ref["target"], ref["t"]
        # the target is the online network exactly on sync frames, and not between them
        same = all(torch.equal(a, b) for a, b in zip(lr.target.state_dict().values(), lr.q.state_dict().values()))
        assert same == ((f + 1) % 4 == 0 or lr.updates == 0), f
        if lr.fused is not None:
            assert torch.equal(lr.fused.q_image, lr.fused.t_image) == same, f
        if prioritised and lr.updates:
            assert lr.last_beta == pytest.approx(beta, abs=1e-12)       # the reference's BETA at this global_step
            assert float(rp.beta_t) == pytest.approx(beta, abs=1e-12)
    assert lr.syncs == [3, 7, 11] and lr.updates == frames - 1
    assert rp.size == CAP and torch.isfinite(lr.last_loss)


@pytest.mark.parametrize("prioritised", [True, False], ids=["per", "uniform"])
def test_fused_and_pytorch_learners_agree_on_the_first_update(prioritised):
    spec = make_spec("pbn28")
    torch.manual_seed(2)
    q0 = DQN(28, 29, [(50, 50)])
    losses = []
    for fused in (True, False):
        env = VectorPBNEnv(spec, N_ENVS, seed=9)
        lr = DDQNLearner(env, copy.deepcopy(q0), net_arch=[(50, 50)], total_frames=100, capacity=CAP, batch_size=64,
                         target_update=50, max_epsilon=1.0, exploration_fraction=1.0, prioritised=prioritised,
                         fused=fused, seed=5)
        env.reset()
        lr.epsilon = 1.0          # both explore with the EXPLORE stream: the same actions and ring
        lr.epsilon_decrement = 0.0
        lr.frame()
        lr.frame()                # the first update (frame 1), from equal weights and equal rings
        torch.cuda.synchronize()
        assert lr.updates == 1
        losses.append(float(lr.last_loss))
    print("first-update losses (fused, pytorch):", losses)
    assert abs(losses[0] - losses[1]) <= 1e-4 * abs(losses[1]), losses


# ---- evaluate_control -----------------------------------------------------------------------------
def test_evaluate_control_takes_a_dqn():
    spec = make_spec("bb33")
    torch.manual_seed(4)
    dqn = DQN(33, 34, [(50, 50)]).cuda()

    def policy(state_bits, target_bits):
        with torch.no_grad():
            return dqn(state_bits.float(), target_bits.float()).argmax(1)

    a = evaluate_control(spec, dqn, runs=3, max_steps=20, seed=6, record_actions=True)
    b = evaluate_control(spec, policy, runs=3, max_steps=20, seed=6, graph=False, record_actions=True)
    assert a.total == b.total > 0
    assert np.array_equal(a.counts, b.counts)
    assert np.array_equal(a.matrix, b.matrix) and a.data == b.data
    assert np.array_equal(a.hit_states, b.hit_states)
    assert a.strategies.shape[2] == 1 and np.array_equal(a.strategies, b.strategies)
