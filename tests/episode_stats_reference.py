"""A numpy restatement of the episode-statistics contract (include/pbn_env.h pbn_episode_begin /
pbn_episode_track), the seeded cases that the host and the GPU tests share, and the C oracle's
trajectory of a case.  TEST INFRASTRUCTURE ONLY.

``episode_stats`` is fed per-frame ``(reward, flags, state_after, target_after)`` -- the GPU's own
outputs, or the C oracle's -- with the starting ``(state, target)`` and an ``attractor_id`` function,
and returns every aggregate, the per-env state and the series rows.  Returns are accumulated in
np.float32 in frame order; the fixed-point conversion is np.rint(np.float64(ret) * 2**20).
"""
import functools

import numpy as np

NO_TARGET = 0xFF
TERMINATED, TRUNCATED = 1, 2
FIXED_ONE = 2 ** 20
TOTALS = ("frames", "episodes", "successes", "missed", "len_sum", "ret_sum", "last_reward_sum", "unpaired")


def to_fixed(x) -> int:
    return int(np.rint(np.float64(np.float32(x)) * FIXED_ONE))


def spec_attractor_id(spec):
    """state words (a sequence of W ints) -> attractor id or -1: EnvSpec.attractor_id on the packed
    form the device holds."""
    W = spec.words
    starts = spec.arrays["attractor_start"]
    states = spec.arrays["attractor_states"]
    table = {}
    for a in range(len(spec.attractors)):
        for k in range(int(starts[a]), int(starts[a + 1])):
            table[tuple(int(x) for x in states[k * W:(k + 1) * W])] = a
    return lambda words: table.get(tuple(int(x) for x in words), -1)


def episode_stats(frames, state0, target0, attractor_id, n_attr, *, done_mask=TERMINATED | TRUNCATED, log_every=0,
                  series_rows=1):
    """frames: a sequence of (reward float32 [n], flags uint8 [n], state_after uint32 [W][n],
    target_after uint8 [n]).  Returns a dict: totals int64 [8], pairs int64 [A][A][4], hist int64 [256],
    ret float32 [n], len uint32 [n], src / tgt uint8 [n], series int64 [R][8], and closes: per frame
    the list of (env, src, tgt, flags) closed in it."""
    state0 = np.asarray(state0)
    n = state0.shape[1]
    A = n_attr

    def source(state, i):
        a = attractor_id(state[:, i])
        return NO_TARGET if a < 0 else a

    ret = np.zeros(n, dtype=np.float32)
    length = np.zeros(n, dtype=np.uint32)
    src = np.array([source(state0, i) for i in range(n)], dtype=np.uint8)
    tgt = np.asarray(target0, dtype=np.uint8).copy()
    totals = np.zeros(8, dtype=np.int64)
    pairs = np.zeros((A, A, 4), dtype=np.int64)
    hist = np.zeros(256, dtype=np.int64)
    series = np.zeros((series_rows if log_every else 0, 8), dtype=np.int64)
    closes = []
    for reward, flags, state, target in frames:
        reward = np.asarray(reward, dtype=np.float32)
        ret = (ret + reward).astype(np.float32)
        length = length + np.uint32(1)
        closed = []
        for i in np.nonzero(np.asarray(flags) & done_mask)[0]:
            f, s, t = int(flags[i]), int(src[i]), int(tgt[i])
            success = bool(f & TERMINATED)
            miss = bool(f & TRUNCATED) and not success
            L, fx = int(length[i]), to_fixed(ret[i])
            totals[1:7] += (1, success, miss, L, fx, to_fixed(reward[i]))
            hist[min(L, 255)] += 1
            if s < A and t < A:
                pairs[s, t] += (1, miss, L, fx)
            else:
                totals[7] += 1
            closed.append((int(i), s, t, f))
            ret[i], length[i] = 0.0, 0
            src[i], tgt[i] = source(np.asarray(state), i), target[i]
        closes.append(closed)
        totals[0] += 1
        if log_every and totals[0] % log_every == 0:
            series[(totals[0] // log_every - 1) % series_rows] = totals
    return {"totals": totals, "pairs": pairs, "hist": hist, "ret": ret, "len": length, "src": src, "tgt": tgt,
            "series": series, "closes": closes}


# ---------------------------------------------------------------- the seeded cases
def _bundled(name, **kw):
    from pbn_rl_amd.attractors import load_attractors
    from pbn_rl_amd.network import load_network
    from pbn_rl_amd.spec import EnvSpec
    return EnvSpec(load_network(name), load_attractors(name), **kw)


def _pbn7(**kw):
    return _bundled("pbn7", **{"horizon": 5, "perturbation": 0.01, **kw})


def _pbn7_attractors(k):
    from pbn_rl_amd.attractors import load_attractors
    from pbn_rl_amd.network import load_network
    from pbn_rl_amd.spec import EnvSpec
    return EnvSpec(load_network("pbn7"), load_attractors("pbn7")[:k], horizon=5, perturbation=0.01)


def _words4():
    from tests.synthetic import random_spec
    return random_spec(100, 5, n_targets=4, max_funcs=3, horizon=4, perturbation=0.01)


def _a254():
    from tests.synthetic import many_attractor_spec
    return many_attractor_spec(40, 254, seed=3, horizon=3, perturbation=0.01)


# what a case's oracle trajectory must contain (tests/test_episode_stats_host.py checks it, so that
# the GPU comparisons of tests/test_gpu_episode_stats.py are known to cover these events)
ALL = ("terminated", "truncated", "same_pair_in_wave", "different_pairs_in_wave", "target_changed")
SOLO = ("terminated", "truncated", "target_changed")        # one env: no second closer in its wave

# name -> (spec factory, num_envs, frames, seed, required events)
CASES = {
    "pbn7_1": (_pbn7, 1, 40, 11, SOLO),
    "pbn7_33": (_pbn7, 33, 40, 12, ALL),
    "pbn7_70": (_pbn7, 70, 40, 13, ALL),
    "pbn70_w3": (lambda: _bundled("pbn70", horizon=5, perturbation=0.01), 70, 24, 14, ("truncated", "same_pair_in_wave",
                                                                                     "different_pairs_in_wave",
                                                                                     "target_changed")),
    "rand100_w4": (_words4, 70, 24, 15, ("truncated", "same_pair_in_wave", "different_pairs_in_wave",
                                          "target_changed")),
    "one_attractor": (lambda: _pbn7_attractors(1), 70, 24, 16, ("terminated", "same_pair_in_wave")),
    "two_attractors": (lambda: _pbn7_attractors(2), 70, 24, 17, ALL),
    "a254": (_a254, 70, 12, 18, ("truncated", "different_pairs_in_wave", "target_changed")),
    "no_attractors": (lambda: _pbn7_attractors(0), 70, 24, 19, ("truncated",)),
}


@functools.lru_cache(maxsize=None)
def case_spec(name):
    return CASES[name][0]()


def oracle_trajectory(spec, n, n_frames, seed, random_actions=True):
    """(state0, target0, frames) of the C oracle for a VectorPBNEnv(spec, n, seed=seed) that is reset
    (step 0) and then stepped n_frames times with autoreset and in-kernel random actions."""
    from oracle import oracle
    n_alloc = (n + 31) // 32 * 32        # the oracle steps whole 32-env groups, as the env's padding does
    st, tg, t = oracle.reset(spec, seed, 0, 0, n_alloc)
    state0, target0, frames = st[:, :n].copy(), tg[:n].copy(), []
    for k in range(n_frames):
        out = oracle.step(spec, seed, 1 + k, 0, st, np.zeros_like(st), tg, t, 1 | (2 if random_actions else 0))
        st, tg, t = out["state_out"], out["target"], out["t"]
        frames.append((out["reward"][:n].copy(), out["flags"][:n].copy(), st[:, :n].copy(), tg[:n].copy()))
    return state0, target0, frames


@functools.lru_cache(maxsize=None)
def case_oracle(name):
    """(state0, target0, frames, reference statistics) of a case, from the C oracle alone."""
    _, n, n_frames, seed, _ = CASES[name]
    spec = case_spec(name)
    state0, target0, frames = oracle_trajectory(spec, n, n_frames, seed)
    ref = episode_stats(frames, state0, target0, spec_attractor_id(spec), len(spec.attractors))
    return state0, target0, frames, ref


def events(ref, target0, frames, wave=64):
    """The set of ALL's events that a trajectory's statistics show."""
    got = set()
    tgt_before = target0
    for closed, (_, flags, _, target) in zip(ref["closes"], frames):
        by_wave = {}
        for i, s, t, f in closed:
            got.add("terminated" if f & TERMINATED else "truncated")
            by_wave.setdefault(i // wave, []).append((s, t))
            if tgt_before[i] != target[i]:
                got.add("target_changed")
        for keys in by_wave.values():
            if len(keys) != len(set(keys)):
                got.add("same_pair_in_wave")
            if len(set(keys)) > 1:
                got.add("different_pairs_in_wave")
        tgt_before = target
    return got
