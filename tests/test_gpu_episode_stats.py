"""Episode statistics on the device (csrc/pbn_episode.hip, pbn_rl_amd/episode_stats.py, the learners'
``episode_stats=True``) against the numpy restatement of the contract (tests/episode_stats_reference.py).

Every comparison is exact: the aggregates are integers written by integer atomics, and a per-env
return is the float32 sum of its rewards in frame order, compared bit for bit.  The restatement is fed
twice: with the GPU's own per-frame outputs, and with the C oracle's trajectory of the same seed
(tests/test_episode_stats_host.py shows, from the oracle alone, which closing events each seeded case
contains)."""
import numpy as np
import pytest
import torch

from pbn_rl_amd import _lib
from pbn_rl_amd.attractors import load_attractors
from pbn_rl_amd.episode_stats import EpisodeStats
from pbn_rl_amd.network import load_network
from pbn_rl_amd.spec import EnvSpec
from pbn_rl_amd.vector_env import VectorPBNEnv
from tests import episode_stats_reference as R

pytestmark = pytest.mark.gpu

CANARY = {"ret": -777.5, "len": 0x5A5A5A5A, "src": 0xA5, "tgt": 0x5A}


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _plant_canaries(st, n):
    for k, v in CANARY.items():
        getattr(st, k)[n:] = v


def _frame_of(env, n):
    return (env.reward[:n].cpu().numpy().copy(), env.flags[:n].cpu().numpy().copy(), _u32(env.state[:, :n]).copy(),
            env.target[:n].cpu().numpy().copy())


def _run(spec, n, n_frames, seed, *, random_actions=True, prepare=None, **kw):
    """An env reset and stepped n_frames times with track() after every step.  Returns (env, stats,
    state0, target0, frames): what the restatement is fed with."""
    env = VectorPBNEnv(spec, n, seed=seed)
    env.reset()
    if prepare is not None:
        prepare(env)
    st = EpisodeStats(env, **kw)
    _plant_canaries(st, n)
    state0, target0 = _u32(env.state[:, :n]).copy(), env.target[:n].cpu().numpy().copy()
    frames = []
    for _ in range(n_frames):
        env.step_flipmask(random_actions=random_actions)
        st.track()
        frames.append(_frame_of(env, n))
    torch.cuda.synchronize()
    return env, st, state0, target0, frames


def _device(st, n):
    A = st.n_attractors
    return {"totals": st.totals_t.cpu().numpy(), "hist": st.hist_t.cpu().numpy(),
            "pairs": st.pairs_t.cpu().numpy() if A else np.zeros((0, 0, 4), dtype=np.int64),
            "ret": st.ret[:n].cpu().numpy(), "len": _u32(st.len[:n]), "src": st.src[:n].cpu().numpy(),
            "tgt": st.tgt[:n].cpu().numpy(),
            "series": st.series_t.cpu().numpy() if st.series_t is not None else np.zeros((0, 8), dtype=np.int64)}


def _assert_equal(got, ref, what):
    for k in ("totals", "pairs", "hist", "len", "src", "tgt", "series"):
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), (what, k, got[k], ref[k])
    assert got["ret"].dtype == np.float32 and ref["ret"].dtype == np.float32
    assert np.array_equal(got["ret"].view(np.uint32), ref["ret"].view(np.uint32)), (what, "ret", got["ret"], ref["ret"])


def _assert_canaries(st, n):
    assert bool((st.ret[n:] == CANARY["ret"]).all())
    assert np.array_equal(_u32(st.len[n:]), np.full(st.len.numel() - n, CANARY["len"], dtype=np.uint32))
    assert bool((st.src[n:] == CANARY["src"]).all()) and bool((st.tgt[n:] == CANARY["tgt"]).all())


def _check_case(name):
    _, n, n_frames, seed, _ = R.CASES[name]
    spec = R.case_spec(name)
    env, st, state0, target0, frames = _run(spec, n, n_frames, seed)
    A = len(spec.attractors)
    got = _device(st, n)
    own = R.episode_stats(frames, state0, target0, R.spec_attractor_id(spec), A)
    _assert_equal(got, own, (name, "restatement on the GPU's outputs"))
    o_state0, o_target0, o_frames, oracle_ref = R.case_oracle(name)
    assert np.array_equal(state0, o_state0) and np.array_equal(target0, o_target0)
    _assert_equal(got, oracle_ref, (name, "restatement on the C oracle's outputs"))
    assert (st.pairs_t is None) == (A == 0)
    if n < env.n_alloc:
        _assert_canaries(st, n)
    return env, st, own


@pytest.mark.parametrize("name", ["pbn7_1", "pbn7_33", "pbn7_70"])
def test_ragged_and_paired(name):
    env, st, ref = _check_case(name)
    n = env.num_envs
    # the readers, on the same numbers
    tot = dict(zip(R.TOTALS, (int(x) for x in ref["totals"])))
    got = st.totals()
    assert {k: got[k] for k in R.TOTALS} == tot and got["steps"] == tot["frames"] * n
    assert all(isinstance(got[k], int) for k in R.TOTALS)
    e = tot["episodes"]
    assert got["ep_len_mean"] == tot["len_sum"] / e and got["ep_rew_mean"] == tot["ret_sum"] / 2 ** 20 / e
    assert got["ep_last_reward_mean"] == tot["last_reward_sum"] / 2 ** 20 / e
    assert got["success_rate"] == tot["successes"] / e
    pairs = st.pairs()
    assert np.array_equal(pairs["episodes"], ref["pairs"][..., 0]) and np.array_equal(pairs["missed"], ref["pairs"][..., 1])
    seen = ref["pairs"][..., 0] > 0
    assert np.array_equal(pairs["mean_len"][seen], ref["pairs"][..., 2][seen] / ref["pairs"][..., 0][seen])
    assert np.isnan(pairs["mean_ret"][~seen]).all()
    assert np.array_equal(st.length_hist(), ref["hist"])
    # the facade's rework_probas rule: every pair starts at (horizon, 1) and adds (length, 1) per episode
    w = (5.0 + ref["pairs"][..., 2]) / (1.0 + ref["pairs"][..., 0])
    np.fill_diagonal(w, 0.0)
    assert np.array_equal(st.pair_weights(), w / w.sum())
    # window(): everything since construction, then nothing
    win = st.window()
    assert (win["frames"], win["episodes"], win["missed"]) == (tot["frames"], e, tot["missed"])
    assert win["missed_pairs"] == int((ref["pairs"][..., 1] > 0).sum()) and win["ep_len_mean"] == got["ep_len_mean"]
    again = st.window()
    assert (again["frames"], again["episodes"], again["missed_pairs"]) == (0, 0, 0) and np.isnan(again["ep_rew_mean"])
    # reset(): aggregates zeroed, episodes reopened on the current state
    st.reset()
    torch.cuda.synchronize()
    assert int(st.totals_t.abs().sum()) == 0 and int(st.hist_t.sum()) == 0 and int(st.pairs_t.abs().sum()) == 0
    lookup = R.spec_attractor_id(env.spec)
    state = _u32(env.state[:, :n])
    assert st.src[:n].cpu().tolist() == [lookup(state[:, i]) & 0xFF for i in range(n)]
    assert torch.equal(st.tgt[:n], env.target[:n]) and int(st.len[:n].abs().sum()) == 0


@pytest.mark.parametrize("name", ["pbn70_w3", "rand100_w4"])
def test_state_word_edge(name):
    env, _, _ = _check_case(name)
    assert env.words == {"pbn70_w3": 3, "rand100_w4": 4}[name]


@pytest.mark.parametrize("name", ["one_attractor", "two_attractors", "a254", "no_attractors"])
def test_attractor_count_edge(name):
    env, st, ref = _check_case(name)
    assert st.n_attractors == {"one_attractor": 1, "two_attractors": 2, "a254": 254, "no_attractors": 0}[name]
    if name == "no_attractors":
        assert st.pairs_t is None and ref["totals"][7] == ref["totals"][1] > 0 and st.pair_weights() is None
    if name == "one_attractor":
        assert ref["pairs"][0, 0, 0] == ref["totals"][1] and ref["totals"][7] == 0


@pytest.mark.parametrize("n", [64, 96, 4096])
def test_horizon_one_every_env_closes_every_frame(n):
    spec = EnvSpec(load_network("pbn7"), load_attractors("pbn7"), horizon=1, perturbation=0.01)
    env, st, state0, target0, frames = _run(spec, n, 8, seed=29)
    ref = R.episode_stats(frames, state0, target0, R.spec_attractor_id(spec), len(spec.attractors))
    _assert_equal(_device(st, n), ref, f"horizon 1, {n} envs")
    assert st.totals()["episodes"] == 8 * n and int(st.hist_t[1]) == 8 * n
    assert int(st.pairs_t[..., 0].sum()) == 8 * n and int(st.pairs_t[..., 2].sum()) == 8 * n


def test_length_cap():
    """bb33 without perturbation or interventions, horizon 255: the episodes that truncate have 255
    steps, land in bin 255 and count 255 each in len_sum."""
    spec = EnvSpec(load_network("bb33"), load_attractors("bb33"), horizon=255, perturbation=0.0)
    n = 32
    env, st, state0, target0, frames = _run(spec, n, 256, seed=31, random_actions=False)
    ref = R.episode_stats(frames, state0, target0, R.spec_attractor_id(spec), len(spec.attractors))
    _assert_equal(_device(st, n), ref, "length cap")
    tot = st.totals()
    truncated = sum(1 for c in ref["closes"] for _, _, _, f in c if f & R.TRUNCATED and not f & R.TERMINATED)
    assert truncated > 0 and tot["missed"] == truncated and int(st.hist_t[255]) == truncated
    short = sum(int(b) * int(c) for b, c in enumerate(st.length_hist()[:255]))
    assert tot["len_sum"] == 255 * truncated + short


def test_series_ring():
    spec = R.case_spec("pbn7_70")
    n, seed = 70, 13
    # four windows elapse in 19 frames; the ring keeps the last three
    env, st, state0, target0, frames = _run(spec, n, 19, seed, log_every=4, series_rows=3)
    ref = R.episode_stats(frames, state0, target0, R.spec_attractor_id(spec), 4, log_every=4, series_rows=3)
    _assert_equal(_device(st, n), ref, "series 4 x 3")
    s = st.series()
    assert s["lost"] == 1 and [w["frames"] for w in s["windows"]] == [8, 12, 16]
    rows = [ref["series"][1], ref["series"][2], ref["series"][0]]          # windows 2, 3, 4 live in rows 1, 2, 0
    for w, row in zip(s["windows"], rows):
        assert [w[k] for k in R.TOTALS] == row.tolist()
    assert s["windows"][0]["window"] is None                                # its predecessor was overwritten
    for prev, cur, w in zip(rows, rows[1:], s["windows"][1:]):
        d = cur - prev
        assert w["window"]["episodes"] == d[1] > 0 and w["window"]["missed"] == d[3]
        assert w["window"]["ep_len_mean"] == d[4] / d[1] and w["window"]["ep_rew_mean"] == d[5] / 2 ** 20 / d[1]
    # one row, every frame: the row is the totals themselves
    env, st, state0, target0, frames = _run(spec, n, 7, seed, log_every=1, series_rows=1)
    ref = R.episode_stats(frames, state0, target0, R.spec_attractor_id(spec), 4, log_every=1, series_rows=1)
    _assert_equal(_device(st, n), ref, "series 1 x 1")
    assert np.array_equal(st.series_t[0].cpu().numpy(), ref["totals"]) and st.series()["lost"] == 6
    # a ring that has not wrapped: every window has its own means, the first from zero
    env, st, *_ = _run(spec, n, 6, seed, log_every=3, series_rows=4)
    s = st.series()
    assert s["lost"] == 0 and [w["frames"] for w in s["windows"]] == [3, 6]
    assert s["windows"][0]["window"]["episodes"] == s["windows"][0]["episodes"]
    # log_every 0: no series buffer at all, frames still advance
    env, st, *_ = _run(spec, n, 5, seed, log_every=0)
    assert st.series_t is None and st.totals()["frames"] == 5 and st.series() == {"windows": [], "lost": 0}


def _outside_state(spec):
    for m in range(1 << spec.n):
        s = tuple((m >> i) & 1 for i in range(spec.n))
        if spec.attractor_id(s) < 0:
            return s
    raise AssertionError("every state is an attractor state")


def test_begin_after_set_state_and_spec_change():
    spec = R.case_spec("pbn7_33")
    n = 33
    out = _outside_state(spec)
    word = int(spec.network.pack(out)[0])

    def place(env):
        state = env.state[:, :n].clone()
        state[0, 0] = word
        env.set_state(state, t=torch.zeros(n, dtype=torch.uint8, device=env.device))

    env, st, state0, target0, frames = _run(spec, n, 6, seed=37, prepare=place)
    assert state0[0, 0] == word
    ref = R.episode_stats(frames, state0, target0, R.spec_attractor_id(spec), 4)
    _assert_equal(_device(st, n), ref, "begin after set_state")
    first = next(c for closed in ref["closes"] for c in closed if c[0] == 0)
    assert first[1] == R.NO_TARGET and st.totals()["unpaired"] == ref["totals"][7] >= 1
    # begin() again: the episodes reopen on the current state without touching the aggregates
    before = st.totals_t.clone()
    st.begin()
    torch.cuda.synchronize()
    assert torch.equal(st.totals_t, before) and int(st.len[:n].abs().sum()) == 0 and torch.equal(st.tgt[:n], env.target[:n])
    # a grown attractor set: the pair matrix no longer fits
    env.set_spec(EnvSpec(spec.network, list(spec.attractors) + [[out]], horizon=5, perturbation=0.01))
    with pytest.raises(ValueError, match="5 attractors"):
        st.track()
    with pytest.raises(ValueError, match="5 attractors"):
        st.begin()


# ---------------------------------------------------------------- the learners
N_ENVS, FRAMES, LOG = 96, 12, 3


def _pbn7(settle):
    return EnvSpec(load_network("pbn7"), load_attractors("pbn7"), horizon=5, perturbation=0.01, settle=settle)


def _ddqn(graphable, stats):
    from pbn_rl_amd.ddqn import DQN, DDQNLearner
    env = VectorPBNEnv(_pbn7(0), N_ENVS, seed=23)
    torch.manual_seed(11)
    lr = DDQNLearner(env, DQN(7, 8, [(16, 16)]), net_arch=[(16, 16)], total_frames=16, capacity=256, batch_size=16,
                     target_update=4, exploration_fraction=0.5, beta_fraction=0.75, prioritised=True, fused=True, seed=5,
                     graphable=graphable, episode_stats=stats, stats_log_every=LOG)
    env.reset()
    return lr


def _bdq(settle):
    def make(graphable, stats):
        from pbn_rl_amd.agent import BranchingQNetwork
        from pbn_rl_amd.replay import BDQLearner
        env = VectorPBNEnv(_pbn7(settle), N_ENVS, seed=23)
        torch.manual_seed(4)
        lr = BDQLearner(env, BranchingQNetwork((7, 7), 8, 3), capacity=4 * N_ENVS, learning_starts=N_ENVS, batch_size=16,
                        target_update=4, epsilon_start=1.0, epsilon_final=0.5, epsilon_decay=8, seed=11,
                        graphable=graphable, fused=True, episode_stats=stats, stats_log_every=LOG)
        env.reset()
        return lr
    return make


def _learner_fields(lr):
    env, rp, fu = lr.env, lr.replay, lr.fused
    return {"env.state": env.state, "env.target": env.target, "env.t": env.t, "env.flags": env.flags,
            "env.reward": env.reward, "ring.state": rp.state, "ring.next_state": rp.next_state,
            "ring.target": rp.target, "ring.action": rp.action, "ring.reward": rp.reward, "ring.done": rp.done,
            "loss": lr.last_loss.reshape(1) if lr.last_loss is not None else fu.loss.new_zeros(0),
            "q_flat": fu.q_flat, "t_flat": fu.t_flat, "adam.m": fu.m, "adam.v": fu.v}


@pytest.mark.parametrize("make", [_ddqn, _bdq(0), _bdq(3)], ids=["ddqn-per", "bdq-settle0", "bdq-settle3"])
def test_learners_track_without_changing_the_frame(make):
    n = N_ENVS
    # eager, stats off: the frame as it is today
    off = make(False, False)
    assert off.stats is None
    want = []
    for _ in range(FRAMES):
        off.frame()
        torch.cuda.synchronize()
        want.append({k: v.clone() for k, v in _learner_fields(off).items()})
    # eager, stats on: the same frames bit for bit, and the statistics of exactly those frames
    on = make(False, True)
    on.stats.begin()                      # (the env was reset after the learner was built)
    state0, target0 = _u32(on.env.state[:, :n]).copy(), on.env.target[:n].cpu().numpy().copy()
    frames = []
    for f in range(FRAMES):
        on.frame()
        torch.cuda.synchronize()
        for k, v in _learner_fields(on).items():
            assert torch.equal(v, want[f][k]), ("eager", f, k)
        frames.append(_frame_of(on.env, n))
    spec = on.env.spec
    ref = R.episode_stats(frames, state0, target0, R.spec_attractor_id(spec), 4, log_every=LOG, series_rows=1024)
    eager = _device(on.stats, n)
    _assert_equal(eager, ref, "eager learner")
    assert ref["totals"][0] == FRAMES and ref["totals"][1] > n and ref["totals"][2] > 0 and ref["totals"][3] > 0
    # captured, stats on: capture() runs its warm-up frames eagerly, the replays do the rest
    cap = make(True, True)
    cap.stats.begin()
    cap.capture()
    k = FRAMES - cap.frames
    assert k >= 8
    if hasattr(cap, "run"):
        cap.run(k)                        # k replays back to back: the windows elapse inside them
    else:
        for _ in range(k):
            cap.frame()
    torch.cuda.synchronize()
    for key, v in _learner_fields(cap).items():
        assert torch.equal(v, want[-1][key]), ("captured", key)
    _assert_equal(_device(cap.stats, n), eager, "captured learner")
    s = cap.stats.series()
    assert s["lost"] == 0 and [w["frames"] for w in s["windows"]] == [3, 6, 9, 12]
    assert s == on.stats.series()


# ---------------------------------------------------------------- the entry points' rejections
def test_rejections():
    spec = R.case_spec("pbn7_33")
    env = VectorPBNEnv(spec, 64, seed=1)
    env.reset()
    st = EpisodeStats(env, log_every=2, series_rows=4)
    bare = VectorPBNEnv(R.case_spec("no_attractors"), 64, seed=1)
    L = _lib.load()
    stream = env._stream()
    p = lambda t: t.data_ptr()  # noqa: E731
    begin = dict(net=env.net.handle, n_alloc=64, n_real=64, d_state=p(env.state), d_target=p(env.target), d_ret=p(st.ret),
                 d_len=p(st.len), d_src=p(st.src), d_tgt=p(st.tgt), stream=stream)
    track = dict(net=env.net.handle, n_alloc=64, n_real=64, done_mask=3, d_reward=p(env.reward), d_flags=p(env.flags),
                 d_state=p(env.state), d_target=p(env.target), d_ret=p(st.ret), d_len=p(st.len), d_src=p(st.src),
                 d_tgt=p(st.tgt), d_totals=p(st.totals_t), d_pairs=p(st.pairs_t), d_hist=p(st.hist_t), log_every=2,
                 series_rows=4, d_series=p(st.series_t), stream=stream)

    def rejected(fn, base, message, code=-22, **change):
        args = {**base, **change}
        decl = _lib.declared()[fn]
        rc = getattr(L, fn)(*[args[k] for k in decl.params])
        assert rc == code, (fn, change, rc)
        assert L.pbn_last_error().decode() == message, (fn, change, L.pbn_last_error().decode())

    before = st.totals_t.clone()
    group = "n_alloc must be a positive multiple of 32 below 2^31"
    for fn, base in (("pbn_episode_begin", begin), ("pbn_episode_track", track)):
        rejected(fn, base, "null net", net=None)
        rejected(fn, base, group, n_alloc=0)
        rejected(fn, base, group, n_alloc=48)
        rejected(fn, base, group, n_alloc=1 << 31)
        rejected(fn, base, "n_real must be in 1..n_alloc", n_real=0)
        rejected(fn, base, "n_real must be in 1..n_alloc", n_real=65)
        for k in ("d_state", "d_target", "d_ret", "d_len", "d_src", "d_tgt"):
            rejected(fn, base, "null buffer", **{k: None})
        for k in ("d_state", "d_ret", "d_len"):
            rejected(fn, base, "d_state, d_ret and d_len must be 4-byte aligned", **{k: base[k] + 2})
    mask = "done_mask must be a non-zero subset of TERMINATED | TRUNCATED"
    rejected("pbn_episode_track", track, mask, done_mask=0)
    rejected("pbn_episode_track", track, mask, done_mask=4)
    rejected("pbn_episode_track", track, mask, done_mask=7)
    for k in ("d_reward", "d_flags", "d_totals", "d_hist"):
        rejected("pbn_episode_track", track, "null buffer", **{k: None})
    rejected("pbn_episode_track", track, "d_pairs may be null only when the net has no attractors", d_pairs=None)
    rejected("pbn_episode_track", track, "d_reward must be 4-byte aligned", d_reward=track["d_reward"] + 1)
    for k in ("d_totals", "d_pairs", "d_hist", "d_series"):
        rejected("pbn_episode_track", track, "d_totals, d_pairs, d_hist and d_series must be 8-byte aligned",
                 **{k: track[k] + 4})
    rejected("pbn_episode_track", track, "log_every must be >= 0", log_every=-1)
    rejected("pbn_episode_track", track, "series_rows must be >= 1 when log_every > 0", series_rows=0)
    rejected("pbn_episode_track", track, "d_series may be null only when log_every is 0", d_series=None)
    torch.cuda.synchronize()
    assert torch.equal(st.totals_t, before)               # a rejected call launches nothing
    # what is allowed: a null series without logging, a null pair matrix on a net without attractors
    ok = {**track, "log_every": 0, "series_rows": 0, "d_series": None}
    assert L.pbn_episode_track(*[ok[k] for k in _lib.declared()["pbn_episode_track"].params]) == 0
    ok = {**ok, "net": bare.net.handle, "d_pairs": None, "d_state": p(bare.state), "d_target": p(bare.target)}
    assert L.pbn_episode_track(*[ok[k] for k in _lib.declared()["pbn_episode_track"].params]) == 0
    torch.cuda.synchronize()
    assert int(st.totals_t[0]) == int(before[0]) + 2
    with pytest.raises(ValueError):
        EpisodeStats(env, log_every=-1)
    with pytest.raises(ValueError):
        EpisodeStats(env, log_every=1, series_rows=0)
