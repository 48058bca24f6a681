"""Prioritised replay, host side (no GPU): the numpy restatement of the law (tests/per_oracle.py)
against traces of the reference's own PrioritisedER (tests/golden/per_trace.npz, written by
tools/gen_per_golden.py), bit for bit; the C entries and the Python classes refusing bad arguments
before they touch a device; and bdq_update's weighted CPU expressions."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from pbn_rl_amd import _lib
from pbn_rl_amd.agent import BranchingQNetwork
from pbn_rl_amd.replay import BDQLearner, PrioritisedDeviceReplay, bdq_update

from .per_oracle import PerOracle, replay_uniforms
from .test_replay_host import batch_for

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "per_trace.npz")
EINVAL = -22


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name,shape", [("c1000", (1000, 40, 32)), ("c1024", (1024, 64, 256)), ("c100", (100, 70, 32))])
def test_restatement_equals_the_reference_trace(golden, name, shape):
    """Every round of the trace: the roots and max_priority after each of store, sample and update,
    the sampled indices and float32 weights, and (at the snapshot rounds) all leaves of both trees
    -- all equal as bits."""
    cap, n, B, rounds, snap_every = (int(x) for x in golden[name + ".meta"])
    assert (cap, n, B) == shape
    o = PerOracle(cap, float(golden[name + ".alpha"]))
    roots, maxp = golden[name + ".roots"], golden[name + ".maxp"]
    snap = 0
    wrapped = False
    for r in range(rounds):
        before = o.pos
        o.store(n)
        wrapped |= o.pos < before
        assert (o.sum[1], o.min[1], o.max_priority) == (roots[r, 0, 0], roots[r, 0, 1], maxp[r, 0]), (r, "store")
        idx, w = o.sample(B, float(golden[name + ".betas"][r]), golden[name + ".u"][r])
        assert np.array_equal(idx, golden[name + ".idx"][r]), (r, "indices")
        assert np.array_equal(w.view(np.int32), golden[name + ".w"][r].view(np.int32)), (r, "weights")
        upd_idx = golden[name + ".upd_idx"][r]
        assert upd_idx[3] == upd_idx[1] == upd_idx[7]       # the trace's forced duplicates
        ok = o.update(upd_idx, golden[name + ".upd_p"][r])
        assert ok.all()
        assert (o.sum[1], o.min[1], o.max_priority) == (roots[r, 2, 0], roots[r, 2, 1], maxp[r, 2]), (r, "update")
        if (r + 1) % snap_every == 0:
            assert np.array_equal(o.sum_leaves(), golden[name + ".sum_leaves"][snap]), r
            assert np.array_equal(o.min_leaves(), golden[name + ".min_leaves"][snap]), r
            snap += 1
    assert wrapped and snap == len(golden[name + ".sum_leaves"])
    assert o.max_priority == 12.25                           # a duplicate that lost its leaf still counts


def test_oracle_conventions():
    o = PerOracle(100, 0.6)
    assert o.T == 128 and 1.0 ** o.alpha == 1.0
    leaves = o.store(3)
    assert leaves.tolist() == [1, 2, 3] and o.pos == 3 and o.size == 3      # the slot after each row
    assert o.sum[1] == 3.0 and o.min[1] == 1.0 and o.sum[o.T] == 0.0 and np.isinf(o.min[o.T])
    assert o.p_total() == 1.0                                # leaves [0, size - 2] = [0, 1]
    ok = o.update([1, 1, 50, -1], np.array([4.0, 2.0, 9.0, 9.0], dtype=np.float32))
    assert ok.tolist() == [True, True, False, False]
    assert o.sum[o.T + 1] == 2.0 ** 0.6 and o.max_priority == 4.0            # last pair wins; max counts both
    s, m = o.sum_leaves().copy(), o.min_leaves().copy()
    s[2] = m[2] = 0.5
    o.adopt_leaves(s, m)
    assert o.min[1] == 0.5 and o.sum[1] == (0.0 + 2.0 ** 0.6) + (0.5 + 1.0)
    u = replay_uniforms(7, 3, 5)
    assert u.shape == (5,) and ((u >= 0) & (u < 1)).all() and len(set(u.tolist())) == 5
    assert not np.array_equal(u, replay_uniforms(7, 4, 5))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


P = 0x10000     # a non-null, 8-byte aligned address: every call below must return before using it


def _store(lib, n=40, pos=P, cap=1000, T=1024, maxp=P, s=P, m=P):
    return lib.pbn_per_store(n, pos, cap, T, 0.6, maxp, s, m, None)


def _sample(lib, B=32, cap=1000, T=1024, size=P, s=P, m=P, beta=P, ctr=P, idx=P, w=P):
    return lib.pbn_per_sample(B, cap, T, size, s, m, beta, 1.0, 0.0, 0, ctr, idx, w, None)


def _update(lib, B=32, cap=1000, T=1024, size=P, idx=P, p=P, maxp=P, s=P, m=P):
    return lib.pbn_per_update(B, cap, T, 0.6, size, idx, p, maxp, s, m, None)


def _td(lib, on=P, tg=P, act=P, rew=P, msk=P, w=P, B=32, K=3, A=29, loss=P, grad=P, prio=P, scratch=P):
    return lib.pbn_bdq_td_loss_per(on, tg, act, rew, msk, w, B, K, A, 0.9, 1e-5, loss, grad, prio, scratch, None)


@pytest.mark.parametrize("call,bad", [
    (_store, dict(pos=None)), (_store, dict(maxp=None)), (_store, dict(s=None)), (_store, dict(m=None)),
    (_store, dict(T=1000)), (_store, dict(T=512)), (_store, dict(cap=1, T=1)), (_store, dict(n=0)),
    (_store, dict(n=1001)), (_store, dict(pos=P + 4)), (_store, dict(s=P + 4)), (_store, dict(m=P + 2)),
    (_sample, dict(size=None)), (_sample, dict(s=None)), (_sample, dict(m=None)), (_sample, dict(beta=None)),
    (_sample, dict(ctr=None)), (_sample, dict(idx=None)), (_sample, dict(w=None)), (_sample, dict(T=1536)),
    (_sample, dict(T=256)), (_sample, dict(cap=1, T=2)), (_sample, dict(B=0)), (_sample, dict(B=1025)),
    (_sample, dict(idx=P + 4)), (_sample, dict(w=P + 2)), (_sample, dict(beta=P + 4)),
    (_update, dict(size=None)), (_update, dict(idx=None)), (_update, dict(p=None)), (_update, dict(maxp=None)),
    (_update, dict(s=None)), (_update, dict(m=None)), (_update, dict(T=1000)), (_update, dict(cap=0)),
    (_update, dict(B=0)), (_update, dict(B=1025)), (_update, dict(idx=P + 4)), (_update, dict(p=P + 1)),
    (_td, dict(w=None)), (_td, dict(prio=None)), (_td, dict(on=None)), (_td, dict(B=0)), (_td, dict(K=8)),
    (_td, dict(A=129)), (_td, dict(w=P + 2)), (_td, dict(act=P + 4)),
])
def test_entries_reject_bad_arguments(lib, call, bad):
    assert call(lib, **bad) == EINVAL, bad
    assert lib.pbn_last_error()


def test_python_classes_reject_bad_arguments():
    with pytest.raises(ValueError, match="GPU"):
        PrioritisedDeviceReplay(100, 1, 3, "cpu")
    with pytest.raises(ValueError, match="fused"):
        BDQLearner(None, fused=True, prioritised=True)
    with pytest.raises(ValueError, match="1024"):
        BDQLearner(None, prioritised=True, batch_size=2048)
    N, B = 7, 32
    q = BranchingQNetwork((N, N), N + 1, 3)
    opt = torch.optim.Adam(q.parameters(), lr=1e-3)
    b = batch_for(N, B)
    with pytest.raises(ValueError, match="weights"):
        bdq_update(q, q, opt, b, priorities_out=torch.empty(B))
    with pytest.raises(ValueError, match="weights"):
        bdq_update(q, q, opt, b, weights=torch.ones(B, dtype=torch.float64))
    with pytest.raises(ValueError, match="weights"):
        bdq_update(q, q, opt, b, weights=torch.ones(B + 1))
    with pytest.raises(ValueError, match="priorities_out"):
        bdq_update(q, q, opt, b, weights=torch.ones(B), priorities_out=torch.empty(B, 1))


def _nets(N, seed):
    torch.manual_seed(seed)
    q = BranchingQNetwork((N, N), N + 1, 3)
    tgt = copy.deepcopy(q)
    for p in tgt.parameters():
        p.data.add_(0.01)
    return q, tgt


def test_unit_weights_give_todays_update_exactly():
    """bdq_update on CPU tensors: weights = 1 is the unweighted update, loss, clamped gradients
    and stepped parameters equal as bits; the priorities are l_b + replay_constant."""
    N, B = 7, 64
    q1, t1 = _nets(N, 0)
    q2, t2 = copy.deepcopy(q1), copy.deepcopy(t1)
    o1 = torch.optim.Adam(q1.parameters(), lr=1e-3)
    o2 = torch.optim.Adam(q2.parameters(), lr=1e-3)
    b = batch_for(N, B)
    prio = torch.empty(B)
    for _ in range(2):
        l1 = bdq_update(q1, t1, o1, b, gamma=0.9)
        l2 = bdq_update(q2, t2, o2, b, gamma=0.9, weights=torch.ones(B), priorities_out=prio, replay_constant=1e-3)
        assert torch.equal(l1, l2)
        for a, c in zip(q1.parameters(), q2.parameters()):
            assert torch.equal(a.grad, c.grad) and torch.equal(a, c)
    assert (prio >= 1e-3).all() and torch.isfinite(prio).all()
    assert torch.allclose((prio - 1e-3).mean(), l2, rtol=1e-5)


def test_weighted_update_matches_longhand():
    """DDQNPER._learn_step's arithmetic with BDQ's MSE, written out: l_b = mean_k (y - q)^2,
    loss = mean_b w_b l_b, priority_b = |w_b l_b| + replay_constant."""
    N, B = 7, 64
    q, tgt = _nets(N, 1)
    q2 = copy.deepcopy(q)
    opt = torch.optim.Adam(q.parameters(), lr=1e-3)
    b = batch_for(N, B, seed=2)
    w = torch.rand(B, generator=torch.Generator().manual_seed(3)) + 0.1
    prio = torch.empty(B)
    loss = bdq_update(q, tgt, opt, b, gamma=0.9, weights=w, priorities_out=prio)
    cur = q2(b["obs"]).gather(2, b["actions"]).squeeze(-1)
    with torch.no_grad():
        am = q2(b["next_obs"]).argmax(dim=2)
        nxt = tgt(b["next_obs"]).gather(2, am.unsqueeze(2)).squeeze(-1)
    lb = ((b["rewards"] + nxt * 0.9 * b["masks"] - cur) ** 2).mean(1)
    want = (w * lb).mean()
    grads = torch.autograd.grad(want, list(q2.parameters()), allow_unused=True)
    assert torch.allclose(loss, want.detach(), rtol=1e-6)
    assert torch.allclose(prio, (w * lb.detach()).abs() + 1e-5, rtol=1e-6)
    for p, g in zip(q.parameters(), grads):
        if g is not None:
            assert torch.allclose(p.grad, g.clamp(-1.0, 1.0), rtol=1e-5, atol=1e-8)
