"""compute_ssd_hist with a DQN policy (pbn_rl_amd/ssd.py): the fused path (BatchedDDQN.rollout
chunks, the network evaluated inside the step kernel) against the per-step path (act_q +
pbn_step_dev + histogram, captured or eager) and against the CPU oracle.  Exact comparisons."""
import numpy as np
import pytest
import torch

from oracle import oracle
from pbn_rl_amd.attractors import load_attractors
from pbn_rl_amd.ddqn import DQN, BatchedDDQN
from pbn_rl_amd.network import load_network
from pbn_rl_amd.spec import EnvSpec
from pbn_rl_amd.ssd import compute_ssd_hist
from pbn_rl_amd.vector_env import VectorPBNEnv

pytestmark = pytest.mark.gpu


def make_dqn(N, arch):
    torch.manual_seed(11)
    return DQN(N, N + 1, arch).cuda()


def test_fused_ssd_equals_the_per_step_ssd():
    spec = EnvSpec(load_network("pbn10"), load_attractors("pbn10"), perturbation=0.05)
    q = make_dqn(10, [(16, 16)])
    # the chunk divides neither the burn-in nor the counted steps
    kw = dict(resets=100, iters=60, burn_in=7, chunk=9, seed=5)
    ssd, plot = compute_ssd_hist(spec, q, **kw)
    assert plot is None and ssd.shape == (1 << 10,) and ssd.dtype == np.float64
    assert abs(float(ssd.sum()) - 1.0) < 1e-12
    assert np.array_equal(ssd, compute_ssd_hist(spec, q, fused=True, **kw)[0])
    assert np.array_equal(ssd, compute_ssd_hist(spec, q, fused=False, graph=True, **kw)[0])
    assert np.array_equal(ssd, compute_ssd_hist(spec, q, fused=False, graph=False, **kw)[0])
    # a BatchedDDQN: its network is taken
    env = VectorPBNEnv(spec, 32)
    assert np.array_equal(ssd, compute_ssd_hist(spec, BatchedDDQN(env, q), **kw)[0])
    env.close()
    # the policy intervenes: the distribution is not the uncontrolled chain's
    free = compute_ssd_hist(spec, None, **kw)[0]
    assert not np.array_equal(ssd, free)
    with pytest.raises(ValueError, match="fused=True needs a DQN"):
        compute_ssd_hist(spec, lambda bits: torch.zeros(bits.shape[0], 1, dtype=torch.int64), fused=True, **kw)


def test_fused_ssd_counts_the_oracles_chain():
    spec = EnvSpec(load_network("pbn7"), load_attractors("pbn7"), perturbation=0.05)
    N, resets, iters, seed = spec.n, 40, 12, 9
    q = make_dqn(N, [(8, 8)])
    ssd, _ = compute_ssd_hist(spec, q, resets=resets, iters=iters, seed=seed)
    # the same chains' actions from an identical rollout, then the chains again on the CPU
    env = VectorPBNEnv(spec, resets, seed=seed, autoreset=False)
    env.reset()
    first = env.step_index
    out = BatchedDDQN(env, q).rollout(iters, 0.0)
    actions = out["actions"].cpu().numpy()
    n = env.n_alloc
    env.close()
    st, tg, t = oracle.reset(spec, seed, 0, 0, n)
    counts = np.zeros(1 << N, dtype=np.uint32)
    acted = 0
    for k in range(iters):
        a = actions[k]
        flip = np.where(a > 0, np.uint32(1) << (np.maximum(a, 1) - 1).astype(np.uint32), np.uint32(0))
        ref = oracle.step(spec, seed, first + k, 0, st, flip.astype(np.uint32)[None, :], tg, t, 0)
        np.add.at(counts, ref["final_state"][0, :resets], 1)
        st, tg, t = ref["state_out"], ref["target"], ref["t"]
        acted += int((a[:resets] > 0).sum())
    assert acted > 0                     # the policy intervened
    total = int(counts.sum(dtype=np.uint64))
    assert total == resets * iters
    assert np.array_equal(ssd, np.divide(counts, total))
