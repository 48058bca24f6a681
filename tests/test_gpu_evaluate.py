"""pbn_rl_amd.evaluate on the GPU: the two bookkeeping kernels against a numpy restatement, the
reference's recorded bb33 evaluation through the product call, the pbn7 agent's evaluation against
a CPU replay over the oracle bit for bit, the loop forms against each other, and the exact law.

The protocol is model_tester.py:587-658 (tests/protocol.py restates it); the CPU replay below runs
it over oracle.step at the product's coordinates: env i = pair * runs + run, env ids from 0,
protocol step k at step index k, the env's target = the target attractor's id.
"""
import copy
import functools
import itertools

import numpy as np
import pytest
import torch

from oracle import law, oracle
from pbn_rl_amd import _lib
from pbn_rl_amd.attractors import load_attractors
from pbn_rl_amd.evaluate import evaluate_control
from pbn_rl_amd.network import load_network
from pbn_rl_amd.spec import EnvSpec

from .protocol import load_agent, pack, unpack
from .test_bn_pin import reference_result
from .test_law_pin import pbn7_agent, q_numpy, ref_pbn7_attractors

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TERMINATED = 1


# ------------------------------------------------------------------ 1. the kernels, directly
def track(L, n_alloc, n_real, W, K, max_steps, step_t, step0, flags, actions, state, count, open_, hit, strategy,
          open_after):
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    return L.pbn_eval_track(n_alloc, n_real, W, K, max_steps, ptr(step_t), step0, ptr(flags), ptr(actions),
                            ptr(state), ptr(count), ptr(open_), ptr(hit), ptr(strategy), ptr(open_after),
                            torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("optional", [True, False])
@pytest.mark.parametrize("W", [1, 2])
@pytest.mark.parametrize("n_real", [70, 64])
def test_track_kernel_exact(n_real, W, optional):
    """Scripted flags / actions / states for max_steps = 5 (and one launch past the end) against the
    rule restated in numpy; padding entries and closed envs' rows hold canaries throughout."""
    L = _lib.load()
    n_alloc, K, max_steps, step0 = 96, 3, 5, 11
    rng = np.random.default_rng(100 * n_real + W)
    open_np = np.ones(n_alloc, np.uint8)                     # the padding's 1s are canaries: never read
    open_np[:n_real] = rng.random(n_real) < 0.8
    count_np = np.where(np.arange(n_alloc) < n_real, 0, -7).astype(np.int32)
    hit_np = np.full((W, n_alloc), 0xDEADBEEF, np.uint32)
    strat_np = np.full((max_steps, n_alloc, K), -1, np.int16)
    after_np = np.zeros(max_steps + 1, np.int32)
    dev = lambda a: torch.from_numpy(a.copy()).to(DEV)  # noqa: E731
    count, open_, after = dev(count_np), dev(open_np), dev(after_np)
    hit = dev(hit_np.view(np.int32)) if optional else None
    strategy = dev(strat_np) if optional else None
    step_t = torch.zeros(1, dtype=torch.int64, device=DEV)
    real = np.arange(n_alloc) < n_real
    for k in range(1, max_steps + 2):                        # k = max_steps + 1: outside, touches nothing
        flags_np = (rng.integers(0, 32, n_alloc) * 2).astype(np.uint8)        # every other flag bit, as noise
        flags_np |= (rng.random(n_alloc) < 0.3).astype(np.uint8) * TERMINATED
        acts_np = rng.integers(0, 34, (n_alloc, K)).astype(np.int32)
        state_np = rng.integers(0, 1 << 32, (W, n_alloc), dtype=np.uint64).astype(np.uint32)
        step_t.fill_(step0 + k - 1)
        rc = track(L, n_alloc, n_real, W, K, max_steps, step_t, step0, dev(flags_np), dev(acts_np),
                   dev(state_np.view(np.int32)), count, open_, hit, strategy, after)
        assert rc == 0, L.pbn_last_error()
        if k <= max_steps:
            live = real & (open_np != 0)
            strat_np[k - 1, live] = acts_np[live]
            term = live & ((flags_np & TERMINATED) != 0)
            count_np[term] = k
            hit_np[:, term] = state_np[:, term]
            last = live & ~term & (k == max_steps)
            count_np[last] = max_steps + 1
            open_np[term | last] = 0
            after_np[k] = int((real & (open_np != 0)).sum())
        torch.cuda.synchronize()
        assert np.array_equal(count.cpu().numpy(), count_np), k
        assert np.array_equal(open_.cpu().numpy(), open_np), k
        assert np.array_equal(after.cpu().numpy(), after_np), k
        if optional:
            assert np.array_equal(hit.cpu().numpy().view(np.uint32), hit_np), k
            assert np.array_equal(strategy.cpu().numpy(), strat_np), k
    assert after_np[max_steps] == 0 and (open_np[:n_real] == 0).all() and (open_np[n_real:] == 1).all()
    assert (count_np[n_real:] == -7).all() and (count_np[:n_real] == max_steps + 1).any()
    assert (hit_np[:, n_real:] == 0xDEADBEEF).all() and (strat_np[:, n_real:] == -1).all()


def reduce_np(counts, max_steps):
    return (counts.sum(axis=1, dtype=np.int64), (counts == max_steps + 1).sum(axis=1).astype(np.int32),
            np.bincount(counts.ravel(), minlength=max_steps + 2).astype(np.int64))


@pytest.mark.parametrize("n_pairs,runs", [(10, 7), (3, 300)])
def test_reduce_kernel_exact(n_pairs, runs):
    """Pair sums, failures and the histogram; an all-fail pair and an all-zero pair; runs below a
    wave and above a block."""
    L = _lib.load()
    max_steps = 5
    rng = np.random.default_rng(runs)
    counts = rng.integers(0, max_steps + 2, (n_pairs, runs)).astype(np.int32)
    counts[1] = max_steps + 1
    counts[2] = 0
    d_count = torch.from_numpy(counts).to(DEV)
    pair_sum = torch.full((n_pairs,), -1, dtype=torch.int64, device=DEV)
    pair_fail = torch.full((n_pairs,), -1, dtype=torch.int32, device=DEV)
    hist = torch.zeros(max_steps + 2, dtype=torch.int64, device=DEV)
    rc = L.pbn_eval_reduce(d_count.data_ptr(), n_pairs, runs, max_steps, pair_sum.data_ptr(), pair_fail.data_ptr(),
                           hist.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.pbn_last_error()
    torch.cuda.synchronize()
    want_sum, want_fail, want_hist = reduce_np(counts, max_steps)
    assert want_sum[1] == runs * (max_steps + 1) and want_fail[1] == runs and want_sum[2] == 0
    assert np.array_equal(pair_sum.cpu().numpy(), want_sum)
    assert np.array_equal(pair_fail.cpu().numpy(), want_fail)
    assert np.array_equal(hist.cpu().numpy(), want_hist)


def test_eval_kernels_reject_bad_arguments():
    L = _lib.load()
    n, K, W, ms = 96, 3, 1, 5
    z = lambda *s, dtype=torch.int32: torch.zeros(*s, dtype=dtype, device=DEV)  # noqa: E731
    step_t, flags, acts, state = z(1, dtype=torch.int64), z(n, dtype=torch.uint8), z(n, K), z(W, n)
    count, open_, hit, strat, after = z(n + 1), z(n, dtype=torch.uint8), z(W, n), z(ms, n, K + 1, dtype=torch.int16), z(ms + 2)
    good = dict(n_alloc=n, n_real=70, max_steps=ms, count=count.data_ptr(), strategy=strat.data_ptr(),
                after=after.data_ptr(), acts=acts.data_ptr(), flags=flags.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return L.pbn_eval_track(a["n_alloc"], a["n_real"], W, K, a["max_steps"], step_t.data_ptr(), 0, a["flags"],
                                a["acts"], state.data_ptr(), a["count"], open_.data_ptr(), hit.data_ptr(),
                                a["strategy"], a["after"], None)

    bad = [dict(max_steps=0), dict(max_steps=255), dict(n_real=n + 1), dict(n_real=-1), dict(n_alloc=80),
           dict(count=count.data_ptr() + 1), dict(count=count.data_ptr() + 2), dict(after=after.data_ptr() + 2),
           dict(acts=acts.data_ptr() + 1), dict(strategy=strat.data_ptr() + 1), dict(flags=None), dict(count=None),
           dict(acts=None)]
    for kw in bad:
        assert call(**kw) == -22, kw
        assert L.pbn_last_error()
    psum, pfail, hist = z(10, dtype=torch.int64), z(11), z(ms + 3, dtype=torch.int64)

    def red(count_p=count.data_ptr(), n_pairs=10, runs=7, max_steps=ms, psum_p=psum.data_ptr(),
            pfail_p=pfail.data_ptr(), hist_p=hist.data_ptr()):
        return L.pbn_eval_reduce(count_p, n_pairs, runs, max_steps, psum_p, pfail_p, hist_p, None)

    for kw in [dict(max_steps=0), dict(max_steps=255), dict(n_pairs=0), dict(runs=0), dict(count_p=None),
               dict(count_p=count.data_ptr() + 2), dict(pfail_p=pfail.data_ptr() + 1), dict(psum_p=psum.data_ptr() + 4),
               dict(hist_p=hist.data_ptr() + 4), dict(hist_p=None)]:
        assert red(**kw) == -22, kw
    torch.cuda.synchronize()
    assert call() == 0 and red() == 0                         # the unmodified arguments are accepted
    torch.cuda.synchronize()


# -------------------------------------------------- 2. the reference's bb33 result, by the product
def test_bb33_evaluation_reproduces_reference():
    """data/results/pbn_33_3.pkl (model_tester.py --mode bn, 3 attractors, 10 runs) from
    evaluate_control: settle law, no perturbation, attractor order (0, 2, 1), the golden agent."""
    atts = load_attractors("bb33")
    chosen = [atts[i] for i in (0, 2, 1)]
    spec = EnvSpec(load_network("bb33"), atts, perturbation=0.0, settle=64)
    ev = evaluate_control(spec, load_agent("bb33", 33), attractors=chosen, runs=10, device=DEV)
    ref, ref_data = reference_result()
    assert ev.counts.shape == (9, 10)
    assert (ev.counts == ev.counts[:, :1]).all()              # every run of a pair has the same length
    assert np.array_equal(ev.matrix / 10, ref)
    assert {k: v for k, v in ev.data.items() if v} == ref_data
    assert ev.failed == 0 and ev.data[101] == 0
    assert ev.open_after[0] == 60 and ev.open_after[2] == 0


# ------------------------------------------------- 3. pbn7 against the CPU replay, bit for bit
P7, RUNS7, SEED7, MAX_STEPS = 0.01, 6, 7, 100


def pbn7_spec(settle):
    return EnvSpec(load_network("pbn7"), ref_pbn7_attractors(), perturbation=P7, horizon=0, settle=settle)


@functools.lru_cache(maxsize=None)
def cpu_replay(settle):
    """The protocol over oracle.step with the CPU module's greedy actions.  Returns counts
    (n_pairs, runs), hit states (n_pairs, runs, W), strategies (n, max_steps, K) and the top-2 Q
    gap of every decision taken (n, max_steps, K; inf where no step was taken)."""
    spec = pbn7_spec(settle)
    atts, N, W = spec.attractors, spec.n, spec.words
    q = pbn7_agent()
    pairs = list(itertools.product(range(len(atts)), repeat=2))
    n = len(pairs) * RUNS7
    assert n % 32 == 0                                        # no padding envs to restate
    src = [a for a, _ in pairs for _ in range(RUNS7)]
    tgt = [t for _, t in pairs for _ in range(RUNS7)]
    start = np.array([atts[a][0] for a in src], dtype=np.int64)
    tbits = np.array([atts[t][0] for t in tgt], dtype=np.float32)
    words = pack(start)
    target = np.array(tgt, dtype=np.uint8)
    t = np.zeros(n, np.uint8)
    count = np.zeros(n, np.int32)
    open_ = np.array([atts[a][0] not in atts[t] for a, t in zip(src, tgt)])
    hit = np.where(~open_[None, :], words, 0).astype(np.uint32)
    strategies = np.full((n, MAX_STEPS, 3), -1, np.int16)
    gaps = np.full((n, MAX_STEPS, 3), np.inf)
    for k in range(1, MAX_STEPS + 1):
        if not open_.any():
            break
        bits = unpack(words, N)
        with torch.no_grad():
            qv = q(torch.from_numpy(np.stack([bits.astype(np.float32), tbits]))).numpy()      # (n, 3, N + 1)
        acts = qv.argmax(axis=2)
        top = np.sort(qv, axis=2)
        flip_bits = np.zeros((n, N), np.int64)
        for a in acts.T:
            sel = a > 0
            flip_bits[np.nonzero(sel)[0], a[sel] - 1] = 1
        out = oracle.step(spec, SEED7, k, 0, words, pack(flip_bits), target, t, 0, want_final=False)
        words, t = out["state_out"], out["t"]
        live = open_.copy()
        strategies[live, k - 1] = acts[live]
        gaps[live, k - 1] = (top[:, :, -1] - top[:, :, -2])[live]
        term = live & ((out["flags"] & TERMINATED) != 0)
        count[term] = k
        hit[:, term] = words[:, term]
        last = live & ~term & (k == MAX_STEPS)
        count[last] = MAX_STEPS + 1
        open_[term | last] = False
    return (count.reshape(len(pairs), RUNS7), hit.T.reshape(len(pairs), RUNS7, W).copy(), strategies, gaps)


@functools.lru_cache(maxsize=None)
def gpu_base(settle):
    return evaluate_control(pbn7_spec(settle), pbn7_agent(), runs=RUNS7, seed=SEED7, record_actions=True, device=DEV)


@pytest.mark.parametrize("settle", [0, 64])
def test_pbn7_evaluation_equals_cpu_replay(settle):
    """p = 0.01, 96 envs, both step laws: counts, hit states and every recorded action equal the
    CPU replay's.  The fused network and the module agree to 1e-5 on the heads; the replay's
    smallest top-2 gap is printed, and a differing action prints its own."""
    counts, hit, strategies, gaps = cpu_replay(settle)
    ev = gpu_base(settle)
    taken = np.isfinite(gaps)
    print(f"settle={settle}: {int(taken.sum())} decisions, smallest top-2 gap {gaps[taken].min():.3g}, "
          f"{int((counts == MAX_STEPS + 1).sum())} failures, longest run {int(counts[counts <= MAX_STEPS].max())}")
    diff = np.argwhere(ev.strategies != strategies)
    if len(diff):
        i, k, b = diff[np.lexsort((diff[:, 2], diff[:, 0], diff[:, 1]))][0]      # the earliest step first
        print(f"first differing action: env {i} step {k + 1} branch {b}: gpu {ev.strategies[i, k, b]} "
              f"cpu {strategies[i, k, b]} top-2 gap {gaps[i, k, b]:.3g}")
    assert np.array_equal(ev.strategies, strategies)
    assert np.array_equal(ev.counts, counts)
    assert np.array_equal(ev.hit_states, hit)
    assert ev.failed == int((counts == MAX_STEPS + 1).sum())
    assert ev.open_after[0] == 72                              # 12 off-diagonal pairs x 6 runs


# ------------------------------------------------------------------- 4. the loop forms agree
def assert_same_evaluation(a, b):
    for name in ("counts", "matrix", "pair_fail", "open_after", "hit_states", "strategies"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert a.data == b.data


def module_policy():
    q = copy.deepcopy(pbn7_agent()).to(DEV)

    def policy(bits, tbits):
        with torch.no_grad():
            return q(torch.stack([bits, tbits]).to(torch.float32)).argmax(dim=2)
    return policy


@pytest.mark.parametrize("form", ["eager", "poll1", "poll7", "poll200", "module", "callable", "callable_eager"])
def test_loop_forms_give_the_same_evaluation(form):
    kw = {"eager": dict(graph=False), "poll1": dict(poll=1), "poll7": dict(poll=7), "poll200": dict(poll=200),
          "module": dict(fused=False), "callable": dict(), "callable_eager": dict(graph=False)}[form]
    model = module_policy() if form.startswith("callable") else pbn7_agent()
    ev = evaluate_control(pbn7_spec(0), model, runs=RUNS7, seed=SEED7, record_actions=True, device=DEV, **kw)
    assert_same_evaluation(ev, gpu_base(0))


# ------------------------------------------------------- 5. the law, through the product call
def test_evaluation_matches_exact_law():
    """pbn7, p = 0.01, one-update law, 2,048 runs per pair: every pair's mean length (from
    pbn_eval_reduce's sums) within 5 standard errors of oracle/law.py's exact mean."""
    runs = 2048
    spec = pbn7_spec(0)
    ev = evaluate_control(spec, pbn7_agent(), runs=runs, seed=5, device=DEV)
    exact = law.evaluate_protocol(load_network("pbn7"), ref_pbn7_attractors(), q_numpy(pbn7_agent()), P7)
    assert np.array_equal(ev.matrix, ev.counts.sum(axis=1, dtype=np.int64).reshape(4, 4))
    for (a, t), dist in exact.items():
        mean, var, _ = law.pair_statistics(dist)
        se = np.sqrt(var / runs)
        got = ev.matrix[a, t] / runs
        print(f"pair {(a, t)}: mean {got:.4f} exact {mean:.4f} se {se:.4f}")
        assert abs(got - mean) <= 5 * se + 1e-9, ((a, t), got, mean, se)
