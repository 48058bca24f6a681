"""The ControlGBDQ agent on the GPU (csrc/pbn_cgbdq.hip, pbn_rl_amd/cgbdq.py; DESIGN.md "ControlGBDQ").

pbn_cgbdq_heads is held to the project's rule: with e_ref the maximum distance of the fp32 CPU module
to the float64 module on the same fp32 front, the kernel's maximum distance to float64 is at most
8 e_ref (layer 1 sums its N N terms in three levels; the measured ratios are in DESIGN.md
"ControlGBDQ").  pbn_cgbdq_flipmask is held exactly to the stated combination and argmax on
pbn_cgbdq_heads' output, and to float64 wherever the float64 gap exceeds 16 e_ref."""
import copy

import numpy as np
import pytest
import torch

from oracle import oracle
from pbn_rl_amd import _lib
from pbn_rl_amd.cgbdq import BatchedControlGBDQ, ControlGBDQLearner, cgbdq_update, combine_heads
from pbn_rl_amd.gbdq import edge_index
from pbn_rl_amd.vector_env import VectorPBNEnv
from tests import cgbdq_cases as cc
from tests import gbdq_cases as gc

pytestmark = pytest.mark.gpu

DEV = cc.DEV


@pytest.fixture(scope="module")
def nets():
    cache = {}

    def get(name):
        if name not in cache:
            spec = cc.named_spec(name)
            cache[name] = (spec, _lib.NetHandle(spec))
        return cache[name]
    yield get
    for _, h in cache.values():
        h.close()


@pytest.fixture(scope="module")
def images(nets):
    """(name, C) -> the packed tail image of the case's network (case_q: the same for every n)."""
    cache = {}

    def get(name, C):
        if (name, C) not in cache:
            _, net = nets(name)
            cache[(name, C)] = cc.pack_tail(net, cc.case_q(name, C), C)[0]
        return cache[(name, C)]
    return get


# ------------------------------------------------------------------------------------ the heads
@pytest.mark.parametrize("n", [32, 96])
@pytest.mark.parametrize("name,C", cc.HEAD_CASES)
def test_heads_within_eight_times_the_fp32_error(nets, images, name, C, n):
    _, net = nets(name)
    _, q, _, _, front32, h32, h64, e_ref = cc.head_refs(name, C, n)
    got = cc.run_heads(net, images(name, C), front32, C)
    err = float((got.double() - h64).abs().max())
    print(f"cgbdq heads {name} C={C} n={n}: e_ref {e_ref:.3e} kernel {err:.3e} ratio {err / e_ref:.2f}")
    assert torch.isfinite(got).all() and e_ref > 0
    assert err <= 8 * e_ref
    again = cc.run_heads(net, images(name, C), front32, C)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))       # two runs, equal bits


@pytest.mark.parametrize("name,C", [("size3", 3), ("size16", 7), ("size65", 65)])
def test_pack_image_bit_for_bit(nets, name, C):
    """The whole image against csrc/cgbdq_tail.h restated in numpy: N = 3 (a k tail of 7 zeros, 7 head
    rows), 16 (K = 256: no k tail; 15 rows), 65 (K = 4,225: a tail of 15; 131 rows)."""
    spec, net = nets(name)
    q = cc.make_cq(spec.n, C, 17)
    image, nf = cc.pack_tail(net, q, C)
    want = cc.tail_image_numpy(q)
    assert nf == want.size
    assert np.array_equal(image[:nf].cpu().numpy().view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------ fused against unfused
def _ctrl_for(name, N, C):
    if name == "size65":        # word edges, an entry = N, an entry = -1, a duplicate
        return [31, 32, 63, 64, 65, -1, 32] + [(k * 65) // C for k in range(7, C)]
    return cc.ctrl_nodes(name, N, C)


@pytest.mark.parametrize("name,C", [("pbn7", 3), ("muscle", 8), ("pbn28", 16), ("size65", 65), ("size128", 128)])
def test_flipmask_equals_the_stated_law_on_the_heads_kernel_output(nets, images, name, C):
    """Every (env, head) pair: the fused launch's actions are the numpy fp32 combination and argmax of
    pbn_cgbdq_heads' output (bit-equal heads), its masks control_to_flipmask of those actions; epsilon 0,
    1 and 0.5 in both modes (C = 128 uniform: 33 EXPLORE calls); the d_step / d_epsilon forms; canaries
    behind every output (run_flipmask); equal bits twice."""
    spec, net = nets(name)
    n, N = 96, spec.n
    _, q, words, _, front32, _, _, _ = cc.head_refs(name, C, n)
    image = images(name, C)
    heads = cc.run_heads(net, image, front32, C).numpy()
    ctrl = _ctrl_for(name, N, C)
    seed, step, off = 0x1234567890ABCDEF, (1 << 33) + 5, 64
    for mode in ("reference", "uniform"):
        for eps in (0.0, 1.0, 0.5):
            acts, mask = cc.run_flipmask(net, image, front32, ctrl, words, seed=seed, step=step, eps=eps, mode=mode,
                                         env_offset=off)
            want = cc.expected_actions(heads, seed, step, off, eps, mode)
            assert np.array_equal(acts, want), (mode, eps)
            assert np.array_equal(mask, cc.expected_masks(words, want, ctrl, N)), (mode, eps)
            if eps == 0.5:
                explore, _ = cc.explore_numpy(seed, step, off, n, C, eps, mode)
                assert 0 < int(explore.sum()) < n
                a2, m2 = cc.run_flipmask(net, image, front32, ctrl, words, seed=seed, step=step, eps=eps, mode=mode,
                                         env_offset=off)
                assert np.array_equal(acts, a2) and np.array_equal(mask, m2)
                a3, m3 = cc.run_flipmask(net, image, front32, ctrl, words, seed=seed, step=step, eps=eps, mode=mode,
                                         env_offset=off, dev_scalars=True)
                assert np.array_equal(acts, a3) and np.array_equal(mask, m3)
    if name == "size128":
        assert (C + 1 + 3) // 4 == 33


@pytest.mark.parametrize("name,C", cc.ACTION_CASES)
def test_greedy_actions_equal_float64_outside_the_near_ties(nets, images, name, C):
    spec, net = nets(name)
    n = cc.ACTION_N
    _, q, words, _, front32, _, h64, e_ref = cc.head_refs(name, C, n)
    keep = cc.gap_keep(h64, e_ref)
    assert float((~keep).mean()) <= 0.01
    acts, _ = cc.run_flipmask(net, images(name, C), front32, cc.ctrl_nodes(name, spec.n, C), words, seed=3, step=9, eps=0.0,
                              mode="reference")
    assert np.array_equal(acts[keep], cc.greedy64(h64)[keep])


# ------------------------------------------------------------------------------------ non-finite values
NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")


def _plant(where, value):
    def mutate(q, front):
        with torch.no_grad():
            if where == "model.0.bias":
                q.model[0].bias[5] = value
            elif where == "model.2.weight":
                q.model[2].weight[7, 11] = value
            elif where == "value_head.bias":
                q.value_head.bias[0] = value
            elif where == "last head bias":
                q.adv_heads[-1].bias[1] = value
            elif where == "front":
                front[3, 1] = NAN
                front[3, front.shape[1] - 1] = PINF
    return mutate


NONFINITE = [(w, v) for w in ("model.0.bias", "model.2.weight", "value_head.bias", "last head bias") for v in (NAN, PINF, NINF)]
NONFINITE.append(("front", NAN))


@pytest.mark.parametrize("name,C", [("pbn7", 3), ("pbn28", 8)])
@pytest.mark.parametrize("where,value", NONFINITE, ids=[f"{w} {v}" for w, v in NONFINITE])
def test_nonfinite_values_follow_pytorch(nets, name, C, where, value):
    """A NaN or an infinity in a tail parameter, or in one row of the front: the heads' NaN / +inf / -inf
    pattern is the fp32 module's (the float64 module checked to share it first), the finite entries are
    within 8 e_ref (of this case's finite entries), and the fused launch's actions are torch.argmax's of
    the stated combination of the kernel's heads."""
    spec, net = nets(name)
    n = 32
    _, q0, words, _, front0, _, _, _ = cc.head_refs(name, C, n)
    q, front = copy.deepcopy(q0), front0.clone()
    _plant(where, value)(q, front)
    h32, h64 = cc.heads32(q, front), cc.heads64(q, front)
    assert gc.same_pattern(h32, h64.float())
    image, _ = cc.pack_tail(net, q, C)
    got = cc.run_heads(net, image, front, C)
    assert gc.same_pattern(got, h32), (where, value)
    fin = torch.isfinite(h64)
    e_ref = cc.e_ref_of(h32, h64)
    if bool(fin.any()):
        err = float((got.double() - h64)[fin].abs().max())
        print(f"cgbdq nonfinite {name} {where} {value}: e_ref {e_ref:.3e} kernel {err:.3e}")
        assert err <= 8 * e_ref
    acts, mask = cc.run_flipmask(net, image, front, cc.ctrl_nodes(name, spec.n, C), words, seed=1, step=2, eps=0.0,
                                 mode="uniform")
    want = torch.argmax(combine_heads(got), dim=2).numpy()
    assert np.array_equal(acts, want)
    assert np.array_equal(mask, cc.expected_masks(words, want, cc.ctrl_nodes(name, spec.n, C), spec.n))


# ------------------------------------------------------------------------------------ rejections
def test_entry_points_reject_bad_arguments(nets):
    spec, net = nets("pbn7")
    L = _lib.load()
    buf = torch.zeros(4096, dtype=torch.float32, device=DEV)
    p = buf.data_ptr()
    EINVAL = -22
    assert L.pbn_cgbdq_heads(net.handle, 33, p, p, 3, p, None) == EINVAL and b"multiple of 32" in L.pbn_last_error()
    assert L.pbn_cgbdq_heads(net.handle, 32, None, p, 3, p, None) == EINVAL
    assert L.pbn_cgbdq_heads(net.handle, 32, p, None, 3, p, None) == EINVAL
    assert L.pbn_cgbdq_heads(net.handle, 32, p, p, 3, None, None) == EINVAL
    assert L.pbn_cgbdq_heads(net.handle, 32, p, p, 0, p, None) == EINVAL and b"n_ctrl" in L.pbn_last_error()
    assert L.pbn_cgbdq_heads(net.handle, 32, p, p, 129, p, None) == EINVAL
    assert L.pbn_cgbdq_heads(net.handle, 32, p, p + 4, 3, p, None) == EINVAL and b"16-byte" in L.pbn_last_error()
    assert L.pbn_cgbdq_heads(None, 32, p, p, 3, p, None) == EINVAL
    assert L.pbn_cgbdq_pack(net.handle, None, 3, p, None) == EINVAL
    assert L.pbn_cgbdq_pack(net.handle, p, 3, p + 8, None) == EINVAL
    assert L.pbn_cgbdq_pack(net.handle, p, 0, p, None) == EINVAL
    assert L.pbn_cgbdq_image_floats(net.handle, 3, None) == EINVAL
    fm = lambda **kw: L.pbn_cgbdq_flipmask(*[kw.get(k, d) for k, d in (  # noqa: E731
        ("net", net.handle), ("seed", 1), ("step", 2), ("d_step", None), ("off", 0), ("n", 32), ("front", p), ("image", p),
        ("C", 3), ("ctrl", p), ("mode", 0), ("eps", 0.5), ("d_eps", None), ("state", p), ("mask", p), ("acts", None),
        ("stream", None))])
    assert fm(n=48) == EINVAL
    assert fm(off=16) == EINVAL
    assert fm(C=0) == EINVAL
    assert fm(mode=2) == EINVAL and b"explore_mode" in L.pbn_last_error()
    assert fm(eps=1.5) == EINVAL
    assert fm(eps=float("nan")) == EINVAL
    assert fm(ctrl=None) == EINVAL
    assert fm(state=None) == EINVAL
    assert fm(mask=None) == EINVAL
    assert fm(front=None) == EINVAL
    assert fm(image=p + 4) == EINVAL
    assert fm(d_step=p + 4) == EINVAL
    assert fm(n=0) == 0


# ------------------------------------------------------------------------------------ the agent and the learner
CTRL7 = [0, 2, 5, 7, 2, -1]


def test_agent_act_is_front_then_the_fused_tail():
    """BatchedControlGBDQ on the muscle network with the reference script's control nodes: the kernel
    path's actions and masks are the stated law on its own heads(), which are within 8 e_ref of the
    float64 module on the kernel's front."""
    spec = cc.named_spec("muscle")
    n, C = 64, 8
    env = VectorPBNEnv(spec, n, seed=9)
    env.reset()
    agent = BatchedControlGBDQ(env, cc.make_cq(14, C, 5), cc.MUSCLE_CTRL, "uniform")
    assert agent.kernel
    front = agent.front().cpu()
    heads = agent.heads().cpu()
    q_cpu = copy.deepcopy(agent.q).cpu()
    h32, h64 = cc.heads32(q_cpu, front), cc.heads64(q_cpu, front)
    assert float((heads.double() - h64).abs().max()) <= 8 * cc.e_ref_of(h32, h64)
    state = env.state.cpu().numpy().view(np.uint32)
    for eps in (0.0, 0.5):
        agent.act(eps)
        torch.cuda.synchronize()
        want = cc.expected_actions(heads.numpy(), env.seed, env.step_index, 0, eps, "uniform")
        assert np.array_equal(agent.actions.cpu().numpy(), want)
        assert np.array_equal(env.flipmask.cpu().numpy().view(np.uint32), cc.expected_masks(state, want, cc.MUSCLE_CTRL, 14))
    # a changed tail parameter repacks the image
    with torch.no_grad():
        agent.q.value_head.bias.add_(1.0)
    assert torch.allclose(agent.heads().cpu()[:, 0], heads[:, 0] + 1.0, atol=1e-6)
    with pytest.raises(NotImplementedError):
        agent.capture()
    env.close()


def _gpu_learner(seed=4, n=64, **kw):
    spec = gc.named_spec("pbn7", horizon=5)
    env = VectorPBNEnv(spec, n, seed=seed)
    env.reset()
    args = dict(control_nodes=CTRL7, explore="uniform", batch_size=32, learning_starts=0, capacity=512, epsilon_start=0.5,
                epsilon_final=0.1, epsilon_decay=10, target_update="copy", target_net_update_freq=3, seed=seed)
    args.update(kw)
    return ControlGBDQLearner(env, cc.make_cq(7, len(CTRL7), 8), **args)


def test_learner_stores_the_oracle_transitions():
    """Twenty frames on pbn7 with 64 envs: the ring holds what the oracle chain gives for the agent's
    actions, in env order (the pattern of test_gpu_gbdq.py's)."""
    n, seed = 64, 4
    lr = _gpu_learner(seed=seed, n=n, learning_starts=1000)
    spec, env = lr.env.spec, lr.env
    st, tg, t = oracle.reset(spec, seed, 0, 0, n)
    rows = []
    for _ in range(20):
        step = env.step_index
        lr.frame()
        torch.cuda.synchronize()
        acts = lr.agent.actions.cpu().numpy()
        flip = cc.expected_masks(st, acts, CTRL7, 7)
        ref = oracle.step(spec, seed, step, 0, st, flip, tg, t, 1)
        for e in range(n):
            rows.append((int(st[0, e]), int(tg[e]), tuple(acts[e]), float(ref["reward"][e]), int(ref["final_state"][0, e]),
                         int((ref["flags"][e] & 3) != 0)))
        st, tg, t = ref["state_out"], ref["target"], ref["t"]
    rp = lr.replay
    assert rp.size == 512 and len(rows) == 1280
    S, T, A = rp.state.cpu().numpy().view(np.uint32), rp.target.cpu().numpy(), rp.action.cpu().numpy()
    R, NS, D = rp.reward.cpu().numpy(), rp.next_state.cpu().numpy().view(np.uint32), rp.done.cpu().numpy()
    assert any(r[5] for r in rows[-512:]) and any(any(r[2]) for r in rows[-512:])
    for r in range(len(rows) - 512, len(rows)):
        j = r % 512
        assert (int(S[0, j]), int(T[j]), tuple(A[j]), float(R[j]), int(NS[0, j]), int(D[j])) == rows[r], r


def test_gpu_update_matches_the_cpu_update():
    """The GPU update's loss and gradients against the CPU cgbdq_update on the same rows: the loss to
    rtol 1e-5, the gradients to rtol 1e-3 / atol 1e-6 (test_gpu_gbdq.py's tolerances)."""
    lr = _gpu_learner(learning_starts=1000)
    for _ in range(10):
        lr.frame()
    batch = lr.sample()
    assert batch["states"].shape == (32, 7) and batch["actions"].shape == (32, len(CTRL7), 1)
    cpu_batch = {k: v.cpu() for k, v in batch.items()}
    q_cpu, t_cpu = copy.deepcopy(lr.q).cpu(), copy.deepcopy(lr.target).cpu()
    opt_cpu = torch.optim.Adam(q_cpu.parameters(), lr=1e-5)
    loss = cgbdq_update(lr.q, lr.target, lr.opt, batch, lr.agent.edges, 0.99)
    loss_cpu = cgbdq_update(q_cpu, t_cpu, opt_cpu, cpu_batch, edge_index(lr.env.spec), 0.99)
    print(f"cgbdq update: loss gpu {float(loss):.8e} cpu {float(loss_cpu):.8e}")
    assert torch.allclose(loss.cpu(), loss_cpu, rtol=1e-5)
    for (name, p), pc in zip(lr.q.named_parameters(), q_cpu.parameters()):
        assert torch.allclose(p.grad.cpu(), pc.grad, rtol=1e-3, atol=1e-6), (name, (p.grad.cpu() - pc.grad).abs().max().item())


def test_gpu_learner_resume_is_bit_equal(tmp_path):
    k = 40
    a = _gpu_learner()
    for _ in range(k):
        a.frame()
    assert a.updates == k - 33
    path = str(tmp_path / "cgbdq.npz")
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
