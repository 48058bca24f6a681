"""The BDQ acting kernels (csrc/pbn_qnet.hip, pbn_agent.hip) at every action-tile and state-word
edge (tests/edge_shapes.py): seeded random networks of N = 15 .. 127 nodes, so A = N + 1 lies on
both sides of each 16- and 32-action tile and the state takes 1 .. 4 words, where the bundled
networks give A in {8, 29, 34, 71} only.

Exact: flip masks and actions of the one-launch forms (pbn_qnet_flipmask_from_state,
pbn_qnet_flipmask) and of pbn_qnet_heads* -> pbn_heads_to_flipmask against the oracle's restatement
of the heads arithmetic; pbn_bilinear_targets' LDS kernel against its L2 kernel.  Float: the head
outputs, Q and the bilinear layer against the PyTorch module evaluated in float64 on the same
unpacked observation, at the project's tolerances for these quantities (rtol 1e-5 / atol 1e-5;
edge_shapes.FLOAT_BOUNDS lists any shape that needs another bound and why)."""
import copy

import numpy as np
import pytest
import torch

from oracle import agent_oracle
from pbn_rl_amd import _lib
from pbn_rl_amd.agent import BatchedBDQ, BranchingQNetwork
from pbn_rl_amd.vector_env import VectorPBNEnv
from tests.edge_shapes import EDGE_N, ENVS, NO_TARGET, check_close, edge_spec, u32

pytestmark = pytest.mark.gpu

SEED, STEP = 13, 29
SENTINEL, SLACK = 0x5A5A5A5A, 64
# K = 3 at every edge with both env counts; K >= 4 takes the second EXPLORE call, K = 7 fills all
# eight heads
CASES = [(N, 3, n) for N in EDGE_N for n in ENVS] + [(N, K, 160) for N in (32, 96, 127) for K in (1, 5, 7)]


def make_agent(N, K, n, n_targets=4):
    spec = edge_spec(N, n_targets)
    torch.manual_seed(17 + N)
    env = VectorPBNEnv(spec, n, seed=SEED)
    agent = BatchedBDQ(env, BranchingQNetwork((N, N), N + 1, K), branches=K)
    env.reset()
    for _ in range(2):
        env.step_flipmask(random_actions=True)
    for e in NO_TARGET:
        env.target[e] = 255
    env.step_index = STEP
    return spec, env, agent


def heads_path_fits(K, A):
    """pbn_heads_to_flipmask stages 64 envs' (K + 1) x A head rows and K actions in one block's
    160 KB of LDS and refuses what does not fit."""
    return 64 * ((K + 1) * A + K) * 4 <= 160 * 1024


def guarded_actions(agent):
    """agent.actions as the middle of a sentinel-filled buffer: (buffer, the view)."""
    n, K = agent.actions.shape
    buf = torch.full((SLACK + n * K + SLACK,), SENTINEL, dtype=torch.int32, device=agent.actions.device)
    agent.actions = buf[SLACK:SLACK + n * K].view(n, K)
    return buf


def assert_guards(buf, n_k, what):
    assert bool((buf[:SLACK] == SENTINEL).all()) and bool((buf[SLACK + n_k:] == SENTINEL).all()), what


@pytest.mark.parametrize("N,K,n", CASES)
def test_flipmasks_and_actions_are_the_oracles(N, K, n):
    """act_q (one launch, from the packed state), q_heads() -> act_heads(), and the y forms
    (pbn_bilinear_targets -> pbn_qnet_flipmask / pbn_qnet_heads) against
    agent_oracle.q_to_flipmask(heads_q(heads)): flip masks and the whole actions tensor bit for
    bit at epsilon 0, 0.3 and 1 and through the device step / epsilon forms; nothing outside the
    actions' [0, n K) is written; the greedy rows include negative and positive value-head
    outputs."""
    spec, env, agent = make_agent(N, K, n)
    A = N + 1
    assert agent.fused_tail and env.n_alloc == n
    with torch.no_grad():
        # value-head outputs of both signs: shift its last bias by their median
        agent.q.value_head[2].bias.sub_(agent.q_heads()[0, :, 0].median())
        heads = agent.q_heads().clone()
    v = heads[0, :, 0]
    assert bool((v < 0).any()) and bool((v > 0).any())
    assert not heads[0, :, 1:].any()                       # the value head's padding
    q = agent_oracle.heads_q(heads.cpu().numpy())
    buf = guarded_actions(agent)
    step_t = torch.full((1,), STEP, dtype=torch.int64, device="cuda")
    L = _lib.load()
    for eps in (0.0, 0.3, 1.0):
        flip, acts = agent_oracle.q_to_flipmask(spec, q, SEED, STEP, 0, eps)
        eps_t = torch.full((1,), eps, dtype=torch.float32, device="cuda")

        def check(what):
            torch.cuda.synchronize()
            assert np.array_equal(u32(env.flipmask), flip), (what, eps)
            assert np.array_equal(agent.actions.cpu().numpy(), acts), (what, eps)
            assert_guards(buf, n * K, (what, eps))
            env.flipmask.fill_(-1)
            agent.actions.fill_(SENTINEL)

        env.flipmask.fill_(-1)
        agent.act_q(eps)
        check("act_q")
        env.step_index = STEP + 5                          # ignored: the device step wins
        agent.act_q(0.77, step_t=step_t, epsilon_t=eps_t)
        env.step_index = STEP
        check("act_q device forms")
        if heads_path_fits(K, A):
            agent.act_heads(heads, eps)
            check("act_heads")
            agent.act_heads(heads, 0.77, step_t=step_t, epsilon_t=eps_t)
            check("act_heads device forms")
        else:
            with pytest.raises(_lib.PbnError, match="n_branches \\* n_actions too large"):
                agent.act_heads(heads, eps)
            assert bool((agent.actions == SENTINEL).all()) and bool((env.flipmask == -1).all())
    # the y forms: the bilinear layer from pbn_bilinear_targets, then the tail alone
    with torch.no_grad():
        hw = agent.bilinear()
        m = agent.q.model
        ts = [t.detach().contiguous() for t in (m[2].weight, m[2].bias, m[4].weight, m[4].bias, m[6].weight,
                                                m[6].bias, *hw)]
        ptrs = [t.data_ptr() for t in ts]
        h_y = torch.full_like(heads, float("nan"))
        _lib.check(L.pbn_qnet_heads(env.net.handle, n, agent._y.data_ptr(), *ptrs, K + 1, A, agent._slope,
                                    h_y.data_ptr(), None), "pbn_qnet_heads")
        torch.cuda.synchronize()
        assert not h_y[0, :, 1:].any() and bool(torch.isfinite(h_y).all())
        q_y = agent_oracle.heads_q(h_y.cpu().numpy())
        for eps in (0.0, 0.3, 1.0):
            flip, acts = agent_oracle.q_to_flipmask(spec, q_y, SEED, STEP, 0, eps)
            env.flipmask.fill_(-1)
            agent.actions.fill_(SENTINEL)
            _lib.check(L.pbn_qnet_flipmask(env.net.handle, SEED, STEP, None, 0, n, agent._y.data_ptr(), *ptrs, K, A,
                                           agent._slope, eps, None, env.flipmask.data_ptr(),
                                           agent.actions.data_ptr(), None), "pbn_qnet_flipmask")
            torch.cuda.synchronize()
            assert np.array_equal(u32(env.flipmask), flip), eps
            assert np.array_equal(agent.actions.cpu().numpy(), acts), eps
            assert_guards(buf, n * K, ("pbn_qnet_flipmask", eps))
    env.close()


@pytest.mark.parametrize("N", EDGE_N)
def test_heads_and_q_match_the_module_in_float64(N):
    """q_heads() (pbn_qnet_heads_from_state), the y form (pbn_qnet_heads) and q_values() against
    copy.deepcopy(q).double() on observe().double(): rtol 1e-5 / atol 1e-5."""
    spec, env, agent = make_agent(N, 3, 160)
    L = _lib.load()
    with torch.no_grad():
        heads = agent.q_heads().clone()
        qv = agent.q_values().clone()
        hw = agent.bilinear()
        m = agent.q.model
        ts = [t.detach().contiguous() for t in (m[2].weight, m[2].bias, m[4].weight, m[4].bias, m[6].weight,
                                                m[6].bias, *hw)]
        h_y = torch.empty_like(heads)
        _lib.check(L.pbn_qnet_heads(env.net.handle, env.n_alloc, agent._y.data_ptr(), *[t.data_ptr() for t in ts],
                                    4, N + 1, agent._slope, h_y.data_ptr(), None), "pbn_qnet_heads")
        obs = agent.observe()
        q64 = copy.deepcopy(agent.q).double()
        ref_heads = q64.forward_heads(q64.model[0](obs.double()))
        ref_q = q64(obs.double())
        mod_heads = agent.q.forward_heads(agent.q.model[0](obs))
        mod_q = agent.q(obs)
    torch.cuda.synchronize()
    check_close(f"heads from state N={N}", heads, ref_heads, mod_heads, 1e-5, 1e-5, ("heads", N))
    check_close(f"heads from y N={N}", h_y, ref_heads, mod_heads, 1e-5, 1e-5, ("heads", N))
    check_close(f"Q N={N}", qv, ref_q, mod_q, 1e-5, 1e-5, ("q", N))
    env.close()


@pytest.mark.parametrize("N,n_targets", [(N, 4) for N in EDGE_N] + [(95, 8), (97, 8), (127, 8)])
def test_bilinear_lds_equals_l2_and_the_module_in_float64(N, n_targets, monkeypatch):
    """pbn_bilinear_targets at W = 1 .. 4: the LDS-staged kernel (n_targets = 4: n_attr N <= 556)
    against the L2 kernel (PBN_BILINEAR=l2) bit for bit, and both against the float64 module's
    bilinear layer + LeakyReLU at rtol 1e-5 / atol 1e-5; with n_targets = 8 (N >= 70) the table does
    not fit and both launches are the L2 kernel.  Ragged last block, envs without a target."""
    spec, env, agent = make_agent(N, 3, 160, n_targets)
    lds_bytes = (2 * n_targets * N * 32 + 256) * 4
    assert (lds_bytes <= 140 * 1024) == (n_targets == 4)
    env.target[::7] = 0xFF
    with torch.no_grad():
        agent.bilinear()
        y_lds = agent._y.clone()
        monkeypatch.setenv("PBN_BILINEAR", "l2")
        agent.bilinear()
        y_l2 = agent._y.clone()
        obs = agent.observe()
        q64 = copy.deepcopy(agent.q).double()
        ref = q64.model[1](q64.model[0](obs.double()))
        mod = agent.q.model[1](agent.q.model[0](obs))
    torch.cuda.synchronize()
    assert torch.equal(y_lds, y_l2)
    check_close(f"y N={N} targets={n_targets}", y_lds, ref, mod, 1e-5, 1e-5, ("y", N))
    env.close()


def test_129_actions_fall_back_to_pytorch_and_the_kernels_refuse():
    """N = 128 (A = 129, one past the qnet kernels' four action tiles): BatchedBDQ runs the tail in
    PyTorch, its flip masks are the oracle's on its own Q, and the raw pbn_qnet_* entry points
    refuse n_actions = 129 without writing."""
    N, K, n = 128, 3, 96
    spec, env, agent = make_agent(N, K, n)
    assert not agent.fused_tail and spec.words == 4
    buf = guarded_actions(agent)
    with torch.no_grad():
        heads = agent.q_heads().clone()
        q = agent_oracle.heads_q(heads.cpu().numpy())
        for eps in (0.0, 0.3):
            env.flipmask.fill_(-1)
            agent.act_q(eps)
            torch.cuda.synchronize()
            flip, acts = agent_oracle.q_to_flipmask(spec, q, SEED, STEP, 0, eps)
            assert np.array_equal(u32(env.flipmask), flip) and np.array_equal(agent.actions.cpu().numpy(), acts)
            assert_guards(buf, n * K, eps)
        obs = agent.observe()
        q64 = copy.deepcopy(agent.q).double()
        check_close("heads N=128 (PyTorch tail)", heads, q64.forward_heads(q64.model[0](obs.double())),
                    agent.q.forward_heads(agent.q.model[0](obs)), 1e-5, 1e-5, ("heads", N))
        L = _lib.load()
        ptrs, _keep = agent._tail_operands()
        hw = agent.bilinear()
        m = agent.q.model
        ts = [t.detach().contiguous() for t in (m[2].weight, m[2].bias, m[4].weight, m[4].bias, m[6].weight,
                                                m[6].bias, *hw)]
        yp = [agent._y.data_ptr()] + [t.data_ptr() for t in ts]
        out = torch.full((K + 1, n, N + 1), -7.5, device="cuda")
        env.flipmask.fill_(-1)
        agent.actions.fill_(SENTINEL)
        h, st, tg = env.net.handle, env.state.data_ptr(), env.target.data_ptr()
        fm, ac = env.flipmask.data_ptr(), agent.actions.data_ptr()
        calls = [lambda: L.pbn_qnet_heads(h, n, *yp, K + 1, N + 1, 0.01, out.data_ptr(), None),
                 lambda: L.pbn_qnet_heads_from_state(h, n, st, tg, *ptrs, K + 1, N + 1, 0.01, out.data_ptr(), None),
                 lambda: L.pbn_qnet_flipmask(h, SEED, STEP, None, 0, n, *yp, K, N + 1, 0.01, 0.0, None, fm, ac, None),
                 lambda: L.pbn_qnet_flipmask_from_state(h, SEED, STEP, None, 0, n, st, tg, *ptrs, K, N + 1, 0.01, 0.0,
                                                        None, fm, ac, None)]
        for i, call in enumerate(calls):
            assert call() == -22, i
            assert "n_actions must be 1..128" in L.pbn_last_error().decode(), i
        torch.cuda.synchronize()
        assert bool((out == -7.5).all()) and bool((env.flipmask == -1).all())
        assert bool((buf == SENTINEL).all())
    env.close()
