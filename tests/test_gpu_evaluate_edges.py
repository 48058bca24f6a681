"""The evaluation bookkeeping at its limits: pbn_eval_track at three and four state words, one and
64 branches, max_steps 1 and 254 (failure count 255, last strategy row 253), blocks partly past
n_alloc and waves of padding only, launches outside 1..max_steps; and evaluate_control over all
254^2 pairs of hold28_a254 (uint8 target ids to 253, 31 trips of pbn_eval_reduce's 2,048 blocks)
against a CPU replay through the oracle.

test_gpu_evaluate.py's scripted-step harness and its numpy rule, at these shapes; all comparisons
exact.  pbn_eval_reduce's own sweep past its grid cap is in test_gpu_grid_caps.py."""
import itertools

import numpy as np
import pytest
import torch

from oracle import oracle
from pbn_rl_amd import _lib
from pbn_rl_amd.evaluate import evaluate_control

from . import table_limits as tl
from .protocol import pack
from .test_gpu_evaluate import DEV, TERMINATED, track

pytestmark = pytest.mark.gpu

# (n_alloc, n_real): one env in a 32-env block; two blocks, the second one wave wide; the same with a
# ragged n_real (the second block's wave partly padding); 17 blocks, the last 32 wide, 28 padding envs
SHAPES = [(32, 1), (288, 288), (288, 257), (4128, 4100)]
FULL = [(W, K, ms, shape, "full") for W in (3, 4) for K in (1, 64) for ms in (1, 254) for shape in SHAPES]
FORMS = [(4, 64, 254, (288, 257), "no_strategy"), (4, 64, 254, (288, 257), "no_hit_state"),
         (4, 1, 1, (4128, 4100), "no_strategy"), (4, 1, 1, (4128, 4100), "no_hit_state"),
         (4, 64, 254, (4128, 4100), "neither")]
STEP0 = 11


@pytest.mark.parametrize("W,K,max_steps,shape,form", FULL + FORMS,
                         ids=[f"W{W}-K{K}-T{ms}-{a}of{b}-{f}" for W, K, ms, (b, a), f in FULL + FORMS])
def test_track_kernel_at_its_limits(W, K, max_steps, shape, form):
    """Scripted flags / actions / states for every protocol step, with launches before step0 and
    more than one past the end, against the rule restated in numpy.  count, open, open_after and the
    hit states are compared after every launch, the strategy row of the step after every launch and
    the whole strategy array at the first two steps, every 64th and the end; padding entries and
    closed envs' rows hold canaries throughout."""
    L = _lib.load()
    n_alloc, n_real = shape
    rng = np.random.default_rng(1000 * n_real + 10 * W + K + max_steps)
    p_term = min(0.3, 2.0 / max_steps)                       # some runs end, some reach the failure rule
    open_np = np.ones(n_alloc, np.uint8)                     # the padding's 1s are canaries: never read
    open_np[:n_real] = rng.random(n_real) < 0.8
    if n_real == 1:
        open_np[0] = 1
    count_np = np.where(np.arange(n_alloc) < n_real, 0, -7).astype(np.int32)
    hit_np = np.full((W, n_alloc), 0xDEADBEEF, np.uint32)
    strat_np = np.full((max_steps, n_alloc, K), -1, np.int16)
    after_np = np.zeros(max_steps + 1, np.int32)
    dev = lambda a: torch.from_numpy(a.copy()).to(DEV)  # noqa: E731
    count, open_, after = dev(count_np), dev(open_np), dev(after_np)
    hit = dev(hit_np.view(np.int32)) if form in ("full", "no_strategy") else None
    strategy = dev(strat_np) if form in ("full", "no_hit_state") else None
    step_t = torch.zeros(1, dtype=torch.int64, device=DEV)
    real = np.arange(n_alloc) < n_real
    # protocol steps k; those outside 1..max_steps touch nothing
    steps = [0, -4] + list(range(1, max_steps + 1)) + [max_steps + 1, max_steps + 3, 2 ** 33]
    for k in steps:
        flags_np = (rng.integers(0, 32, n_alloc) * 2).astype(np.uint8)        # every other flag bit, as noise
        flags_np |= (rng.random(n_alloc) < p_term).astype(np.uint8) * TERMINATED
        acts_np = rng.integers(0, 129, (n_alloc, K)).astype(np.int32)
        state_np = rng.integers(0, 1 << 32, (W, n_alloc), dtype=np.uint64).astype(np.uint32)
        step_t.fill_(STEP0 + k - 1)
        rc = track(L, n_alloc, n_real, W, K, max_steps, step_t, STEP0, dev(flags_np), dev(acts_np),
                   dev(state_np.view(np.int32)), count, open_, hit, strategy, after)
        assert rc == 0, L.pbn_last_error()
        inside = 1 <= k <= max_steps
        if inside:
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
        if hit is not None:
            assert np.array_equal(hit.cpu().numpy().view(np.uint32), hit_np), k
        if strategy is not None:
            if inside:
                assert np.array_equal(strategy[k - 1].cpu().numpy(), strat_np[k - 1]), k
            if not inside or k <= 2 or k % 64 == 0 or k == max_steps:
                assert np.array_equal(strategy.cpu().numpy(), strat_np), k
    assert after_np[max_steps] == 0 and (open_np[:n_real] == 0).all() and (open_np[n_real:] == 1).all()
    assert (count_np[n_real:] == -7).all()
    assert (hit_np[:, n_real:] == 0xDEADBEEF).all() and (strat_np[:, n_real:] == -1).all()
    if n_real > 1:
        assert (count_np[:n_real] == max_steps + 1).any()    # the failure rule ran (255 at max_steps = 254)
        assert (count_np[:n_real] == 0).any()                # closed from the start: rows of canaries
        if max_steps > 1:
            assert ((count_np[:n_real] > 0) & (count_np[:n_real] < max_steps)).any()
    else:
        assert 1 <= count_np[0] <= max_steps + 1             # the one real env was open and ended
    if max_steps == 254 and n_real > 1:
        assert count_np.max() == 255 and (strat_np[253, :n_real] != -1).any()


# ------------------------------------------------ the product call over 254^2 pairs
SEED, MAX_STEPS = 9, 2


def cpu_replay(spec, n_alloc):
    """test_gpu_evaluate.py's cpu_replay for a policy that never intervenes, runs = 1: the protocol
    over oracle.step with zero flip masks at the product's coordinates (env i = pair, env ids from 0,
    protocol step k at step index k).  The padding envs n_real..n_alloc - 1 are restated too: they
    keep the state, target and t the reset at step index 0 gave them, and step along."""
    atts, W = spec.attractors, spec.words
    pairs = list(itertools.product(range(len(atts)), repeat=2))
    n = len(pairs)
    words, target, t = oracle.reset(spec, SEED, 0, 0, n_alloc)
    first = pack(np.array([a[0] for a in atts], dtype=np.int64))                  # (W, A)
    src = np.array([a for a, _ in pairs])
    tgt = np.array([b for _, b in pairs])
    words[:, :n] = first[:, src]
    target[:n] = tgt.astype(np.uint8)
    t[:n] = 0
    sets = [set(a) for a in atts]
    open_ = np.zeros(n_alloc, bool)
    open_[:n] = [atts[a][0] not in sets[b] for a, b in pairs]
    count = np.zeros(n_alloc, np.int32)
    hit = np.where(~open_[None, :] & (np.arange(n_alloc) < n)[None, :], words, 0).astype(np.uint32)
    strategies = np.full((n, MAX_STEPS, 1), -1, np.int16)
    open_after = np.zeros(MAX_STEPS + 1, np.int32)
    open_after[0] = int(open_.sum())
    zero = np.zeros_like(words)
    for k in range(1, MAX_STEPS + 1):
        out = oracle.step(spec, SEED, k, 0, words, zero, target, t, 0, want_final=False)
        words, t = out["state_out"], out["t"]
        live = open_.copy()
        strategies[live[:n], k - 1] = 0
        term = live & ((out["flags"] & TERMINATED) != 0)
        count[term] = k
        hit[:, term] = words[:, term]
        last = live & ~term & (k == MAX_STEPS)
        count[last] = MAX_STEPS + 1
        open_[term | last] = False
        open_after[k] = int(open_.sum())
    return pairs, count[:n].reshape(n, 1), hit[:, :n].T.reshape(n, 1, W).copy(), strategies, open_after


def test_all_pairs_of_254_attractors_equal_the_cpu_replay():
    """evaluate_control on hold28_a254 over all 64,516 pairs, one run each, a policy that always
    returns the no-op, p = 0, max_steps = 2: target ids up to 253 and 31 trips of pbn_eval_reduce's
    grid through the whole path.  Counts, hit states, open_after, matrix, pair_fail, data and the
    recorded actions equal the CPU replay's."""
    spec = tl.limit_spec("hold28_a254", perturbation=0.0, horizon=0)
    A = len(spec.attractors)
    n = A * A
    assert A == 254 and n > 2048
    n_alloc = (n + 31) // 32 * 32
    assert n_alloc - n == 28                                  # padding envs, restated in the replay

    def policy(bits, tbits):
        assert bits.shape == tbits.shape == (n, spec.n)
        return torch.zeros(n, 1, dtype=torch.int64, device=bits.device)

    ev = evaluate_control(spec, policy, runs=1, max_steps=MAX_STEPS, seed=SEED, record_actions=True, device=DEV)
    pairs, counts, hit, strategies, open_after = cpu_replay(spec, n_alloc)
    assert ev.pairs == pairs and ev.runs == 1
    assert np.array_equal(ev.counts, counts)
    assert np.array_equal(ev.hit_states, hit)
    assert np.array_equal(ev.open_after, open_after)
    assert np.array_equal(ev.strategies, strategies)
    want_matrix = counts.sum(axis=1, dtype=np.int64).reshape(A, A).astype(np.float64)
    assert np.array_equal(ev.matrix, want_matrix)
    assert np.array_equal(ev.pair_fail, (counts == MAX_STEPS + 1).sum(axis=1).astype(np.int32))
    want_data = {int(k): int(v) for k, v in enumerate(np.bincount(counts.ravel(), minlength=MAX_STEPS + 2)) if v}
    want_data.setdefault(MAX_STEPS + 1, 0)
    assert ev.data == want_data
    # what the replay must have found on a network that holds its state: the diagonal ends at once
    assert ev.data == {0: A, MAX_STEPS + 1: n - A} and open_after.tolist() == [n - A, n - A, 0]
    assert np.array_equal(np.diag(ev.matrix), np.zeros(A)) and ev.matrix[253, 0] == MAX_STEPS + 1
