"""compute_ssd_hist(sparse=True): the visited-state table == the dense histogram (N <= 32) and the
oracle's counts (networks of two, three and four state words), for every model form; and
attractor discovery's table path == its torch.unique path."""
import numpy as np
import pytest
import torch

from oracle import oracle
from pbn_rl_amd.attractors import load_attractors
from pbn_rl_amd.ddqn import DQN
from pbn_rl_amd.discovery import simulate_visits
from pbn_rl_amd.network import load_network
from pbn_rl_amd.spec import EnvSpec
from pbn_rl_amd.ssd import SparseSSD, compute_ssd_hist
from pbn_rl_amd.state_table import sort_states

from .synthetic import random_spec

pytestmark = pytest.mark.gpu

# test_gpu_ssd.py's shape: 70 chains in 96 allocated envs, three launches of 9, 9 and 5 counted steps
SHAPE = dict(resets=70, iters=23, burn_in=4, seed=5, chunk=9)


@pytest.mark.parametrize("name", ["pbn7", "pbn28"])
def test_sparse_equals_dense(name):
    spec = EnvSpec(load_network(name), load_attractors(name), perturbation=0.02)
    dense, _ = compute_ssd_hist(spec, None, **SHAPE)
    stats = {}
    ssd, plot = compute_ssd_hist(spec, None, sparse=True, capacity=64, stats=stats, **SHAPE)
    assert plot is None and isinstance(ssd, SparseSSD)
    assert ssd.total == 70 * 23 and ssd.n_nodes == spec.n
    assert np.array_equal(ssd.to_dense(), dense)
    assert np.array_equal(np.nonzero(dense)[0].astype(np.uint32), ssd.words[:, 0])
    assert stats["n_states"] == len(ssd) and stats["capacity"] >= 2 * len(ssd) and stats["n_growths"] >= 1


def four_word_spec():
    return random_spec(100, 41, perturbation=0.02)


@pytest.mark.parametrize("name", ["bb33", "pbn70", "rand100"])
def test_sparse_matches_oracle_beyond_32_nodes(name):
    """bb33: two words, gates (the wave kernels); pbn70: three words (the pipelined kernel); a
    100-node random network: four words."""
    spec = four_word_spec() if name == "rand100" else EnvSpec(load_network(name), load_attractors(name),
                                                              perturbation=0.02)
    resets, iters, burn_in, seed = SHAPE["resets"], SHAPE["iters"], SHAPE["burn_in"], SHAPE["seed"]
    ssd, _ = compute_ssd_hist(spec, None, sparse=True, **SHAPE)
    n, W = 96, (spec.n + 31) // 32
    st, tg, t = oracle.reset(spec, seed, 0, 0, n)
    visited = []
    for k in range(burn_in + iters):
        out = oracle.step(spec, seed, 1 + k, 0, st, np.zeros_like(st), tg, t, 0)
        if k >= burn_in:
            visited.append(np.asarray(out["final_state"]).view(np.uint32).reshape(W, n)[:, :resets].T)
        st, tg, t = out["state_out"], out["target"], out["t"]
    uniq, cnt = np.unique(np.concatenate(visited), axis=0, return_counts=True)
    order = sort_states(uniq)
    assert ssd.words.shape[1] == W and len(uniq) > 1
    assert np.array_equal(ssd.words, uniq[order]) and np.array_equal(ssd.counts, cnt[order].astype(np.uint64))
    assert ssd.total == resets * iters and np.array_equal(ssd.probs, cnt[order] / (resets * iters))
    assert ssd.bits.shape == (len(uniq), spec.n) and abs(ssd.probs.sum() - 1.0) < 1e-12


def same(a, b):
    return np.array_equal(a.words, b.words) and np.array_equal(a.counts, b.counts) and a.total == b.total


def test_pbn70_dqn_fused_equals_per_step():
    spec = EnvSpec(load_network("pbn70"), load_attractors("pbn70"), perturbation=0.02)
    torch.manual_seed(4)
    q = DQN(70, 71, [(16, 16)]).cuda()
    fused, _ = compute_ssd_hist(spec, q, sparse=True, fused=True, **SHAPE)
    step, _ = compute_ssd_hist(spec, q, sparse=True, fused=False, **SHAPE)
    free, _ = compute_ssd_hist(spec, None, sparse=True, **SHAPE)
    assert fused.total == step.total == 70 * 23
    assert same(fused, step)
    assert not same(fused, free)          # the policy intervened


def test_callable_policy_graph_equals_eager_with_a_partial_last_chunk():
    """25 counted steps staged in chunks of 9: two full chunks and a last one of 7."""
    spec = EnvSpec(load_network("pbn70"), load_attractors("pbn70"), perturbation=0.05)

    def policy(bits):   # flip node 2 whenever node 1 is on, else node 69 whenever node 68 is on
        a = bits[:, 1].to(torch.int64) * 3
        return torch.where(a > 0, a, bits[:, 68].to(torch.int64) * 70)[:, None]

    kw = dict(resets=100, iters=25, burn_in=7, seed=3, chunk=9, sparse=True)
    a, _ = compute_ssd_hist(spec, policy, graph=True, **kw)
    b, _ = compute_ssd_hist(spec, policy, graph=False, **kw)
    free, _ = compute_ssd_hist(spec, None, **kw)
    assert a.total == b.total == 100 * 25
    assert same(a, b) and not same(a, free)


def test_callable_policy_sparse_equals_dense():
    spec = EnvSpec(load_network("pbn7"), load_attractors("pbn7"), perturbation=0.02)

    def policy(bits):
        return (bits[:, 1].to(torch.int64) * 1)[:, None]

    kw = dict(resets=40, iters=25, burn_in=2, seed=8, chunk=9)
    dense, _ = compute_ssd_hist(spec, policy, **kw)
    ssd, _ = compute_ssd_hist(spec, policy, sparse=True, **kw)
    assert np.array_equal(ssd.to_dense(), dense)


def test_simulate_visits_table_equals_default():
    net = load_network("pbn10")
    kw = dict(chains=256, burn_in=20, window=40)
    want = simulate_visits(net, **kw)
    got = simulate_visits(net, table=True, window_chunk=16, **kw)
    assert got.dtype == want.dtype and np.array_equal(got, want) and len(want) > 1


def test_simulate_visits_table_keeps_the_order_beyond_one_word():
    """pbn70 (three words, states with bit 31 of a word set): the same rows in the same order."""
    net = load_network("pbn70")
    kw = dict(chains=64, burn_in=3, window=10)
    want = simulate_visits(net, **kw)
    got = simulate_visits(net, table=True, window_chunk=4, **kw)
    assert np.array_equal(got, want) and len(want) > 64
