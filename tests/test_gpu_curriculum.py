"""Curriculum resets on the device (csrc/pbn_curriculum.hip, pbn_rl_amd/curriculum.py, the learners'
``curriculum=True``) against the Python restatement of the law (tests/curriculum_reference.py).

Every comparison is exact: the table is integers built in a fixed association, and a restart is a
function of one Philox call and the table.  tests/test_curriculum_host.py holds the statistical test
of the law itself; nothing here is statistical.
"""
import functools

import numpy as np
import pytest
import torch

from pbn_rl_amd import _lib
from pbn_rl_amd.attractors import load_attractors
from pbn_rl_amd.curriculum import Curriculum, read_table, table_layout
from pbn_rl_amd.episode_stats import EpisodeStats
from pbn_rl_amd.network import load_network
from pbn_rl_amd.spec import EnvSpec
from pbn_rl_amd.vector_env import VectorPBNEnv
from tests import curriculum_reference as C
from tests.synthetic import many_attractor_spec, multi_state_spec, random_spec

pytestmark = pytest.mark.gpu

RESET = _lib.FLAG_RESET
BIG_OFFSET = (1 << 33) + 64
TARGET_CANARY, COPY_CANARY = 0xEE, 0x5A


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _pbn7(k=4, **kw):
    return EnvSpec(load_network("pbn7"), load_attractors("pbn7")[:k], **{"horizon": 4, "perturbation": 0.01, **kw})


@functools.lru_cache(maxsize=None)
def _spec(name):
    return {"a2": lambda: _pbn7(2), "a3": lambda: _pbn7(3),
            "pbn7": _pbn7,                                             # attractors of 1, 1, 4 and 1 states
            "w3": lambda: EnvSpec(load_network("pbn70"), load_attractors("pbn70"), horizon=5, perturbation=0.01),
            "w4": lambda: random_spec(100, 5, n_targets=4, max_funcs=3, horizon=4, perturbation=0.01),
            "a254": lambda: many_attractor_spec(40, 254, seed=3, horizon=3, perturbation=0.01),
            "multi": lambda: multi_state_spec(horizon=6)}[name]()     # two words; 3, 1, 5 and 2 states


def _seeded_pairs(A, seed):
    rng = np.random.default_rng(seed)
    pairs = np.zeros((A, A, 4), dtype=np.int64)
    pairs[..., 0] = rng.integers(0, 40, size=(A, A))
    pairs[..., 2] = pairs[..., 0] * rng.integers(1, 30, size=(A, A))
    return pairs


def _assert_table(got, ref, what):
    assert np.array_equal(got["rowcdf"], ref["rowcdf"]), (what, "rowcdf")
    assert np.array_equal(got["cdf"], ref["cdf"]), (what, "cdf")
    assert (got["total"], got["refreshes"]) == (ref["total"], ref["refreshes"]), (what, got["total"], got["refreshes"])


# ---------------------------------------------------------------- redraw
def _flag_patterns(n_alloc, n, rng):
    """No RESET, every env RESET, mixed; the other flag bits vary, and the padding envs always carry
    RESET (they must not be touched)."""
    other = rng.choice(np.array([0, 1, 2, 3, 4, 5, 8, 32, 47], dtype=np.uint8), size=(3, n_alloc))
    none, every, mixed = other[0].copy(), other[1] | RESET, other[2].copy()
    mixed[rng.random(n_alloc) < 0.4] |= RESET
    for f in (none, every, mixed):
        f[n:] |= RESET
    return {k: f.astype(np.uint8) for k, f in (("none", none), ("every", every), ("mixed", mixed))}


@pytest.mark.parametrize("name,n", [("a2", 1), ("a3", 33), ("pbn7", 70), ("w3", 33), ("w4", 70), ("a254", 70),
                                    ("multi", 33), ("pbn7", 300)])
def test_redraw_equals_the_reference(name, n):
    spec = _spec(name)
    A, W = len(spec.attractors), spec.words
    assert W == {"a2": 1, "a3": 1, "pbn7": 1, "w3": 3, "w4": 4, "a254": 2, "multi": 2}[name]
    rng = np.random.default_rng(100 * A + n)
    pairs = _seeded_pairs(A, 7 + A)
    ref_table = C.build_table(pairs, C.horizon_of(spec), refreshes=2)
    steps = iter([1, 5, (3 << 32) | 7, 12, 2, 900, 33, 34, 35, 36, 37, 38])
    seen = set()
    for env_offset in (0, BIG_OFFSET):
        env = VectorPBNEnv(spec, n, seed=977 + n, env_offset=env_offset)
        env.reset()
        stats = EpisodeStats(env)
        cur = Curriculum(env, stats, refresh_every=0)
        stats.pairs_t.copy_(torch.from_numpy(pairs))
        cur.refresh(force=True)
        _assert_table(cur.table(), ref_table, (name, "forced"))
        patterns = _flag_patterns(env.n_alloc, n, rng)
        for by_tensor in (False, True):
            for kind, flags in patterns.items():
                step = next(steps)
                with_copy = (kind == "mixed") != by_tensor            # both ways under both step forms
                state0 = rng.integers(0, 1 << 32, size=(W, env.n_alloc), dtype=np.uint64).astype(np.uint32)
                env.state.copy_(torch.from_numpy(state0.view(np.int32)))
                env.target.fill_(TARGET_CANARY)
                env.flags.copy_(torch.from_numpy(flags))
                copy = torch.full((env.n_alloc,), COPY_CANARY, dtype=torch.uint8, device=env.device) if with_copy else None
                if by_tensor:     # the tensor's value counts, not the scalar beside it
                    cur.redraw(step=step + 1, step_t=torch.tensor([step], dtype=torch.int64, device=env.device),
                               target_copy=copy)
                else:
                    cur.redraw(step=step, target_copy=copy)
                torch.cuda.synchronize()
                what = (name, n, env_offset, by_tensor, kind)
                real = np.zeros(env.n_alloc, dtype=np.uint8)
                real[:n] = flags[:n]
                want_state, want_target, picks = C.redraw(ref_table, spec, env.seed, env_offset, step, real, state0,
                                                          np.full(env.n_alloc, TARGET_CANARY, dtype=np.uint8))
                assert np.array_equal(_u32(env.state), want_state), what
                assert np.array_equal(env.target.cpu().numpy(), want_target), what
                assert np.array_equal(env.flags.cpu().numpy(), flags), what
                hit = (real & RESET) != 0
                assert len(picks) == int(hit.sum()) and (kind != "none" or not picks) and (kind != "every" or hit[:n].all())
                if copy is not None:
                    assert np.array_equal(copy.cpu().numpy(), np.where(hit, want_target, COPY_CANARY)), what
                # the canaries: envs that did not reset, and everything past num_envs
                assert np.array_equal(want_state[:, ~hit], state0[:, ~hit]) and (want_target[~hit] == TARGET_CANARY).all()
                seen |= {(s, t) for _, s, t, _ in picks}
                if name in ("pbn7", "multi"):   # a start state inside a multi-state attractor, not its first only
                    starts = [int(a) for a in spec.arrays["attractor_start"]]
                    seen |= {("row", row - starts[s]) for _, s, _, row in picks}
        env.close()
    if n >= 33:
        assert len({p for p in seen if p[0] != "row"}) >= min(A * (A - 1), 20) // 2
    if name in ("pbn7", "multi") and n >= 33:
        assert {p[1] for p in seen if p[0] == "row"} >= {0, 1, 2}


def test_it_is_a_curriculum():
    """A table with nearly all its weight on (2, 0): one redraw of 4,096 resetting envs sends the
    reference's number of envs there -- nearly all of them -- and the same envs."""
    spec, n = _spec("pbn7"), 4096
    env = VectorPBNEnv(spec, n, seed=31)
    env.reset()
    stats = EpisodeStats(env)
    cur = Curriculum(env, stats)
    uniform = cur.weights()
    off = ~np.eye(4, dtype=bool)
    assert np.allclose(uniform[off], 1 / 12) and (np.diag(uniform) == 0).all()
    pairs = C.dense_pairs(4, [(2, 0, 0, 60000)])
    stats.pairs_t.copy_(torch.from_numpy(pairs))
    cur.refresh(force=True)
    ref_table = C.build_table(pairs, 4, refreshes=2)
    _assert_table(cur.table(), ref_table, "skewed")
    assert np.array_equal(cur.weights(), C.weights(ref_table)) and cur.weights()[2, 0] > 0.99
    env.flags.fill_(RESET)
    cur.redraw(step=9)
    torch.cuda.synchronize()
    want_state, want_target, picks = C.redraw(ref_table, spec, env.seed, 0, 9, np.full(n, RESET, dtype=np.uint8),
                                              _u32(env.state), env.target.cpu().numpy())
    there = np.array([s == 2 and t == 0 for _, s, t, _ in picks])
    lookup = C.E.spec_attractor_id(spec)
    state, target = _u32(env.state), env.target.cpu().numpy()
    got = np.array([lookup(state[:, i]) == 2 and target[i] == 0 for i in range(n)])
    assert np.array_equal(got, there) and int(got.sum()) == int(there.sum()) > 4000
    assert np.array_equal(state, want_state) and np.array_equal(target, want_target)
    # the four states of attractor 2 are all used
    assert {row for _, s, _, row in picks if s == 2} == set(range(2, 6))


# ---------------------------------------------------------------- refresh
def _refresh(pairs_t, totals_t, A, H, every, table_t):
    L = _lib.load()
    _lib.check(L.pbn_curriculum_refresh(totals_t.data_ptr() if totals_t is not None else None, pairs_t.data_ptr(), A, H,
                                        every, table_t.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "pbn_curriculum_refresh")
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", sorted(C.PAIR_CASES))
def test_refresh_builds_the_reference_table(name):
    A, H, entries = C.PAIR_CASES[name]
    pairs = C.dense_pairs(A, entries)
    pairs[..., 1], pairs[..., 3] = 3, -5                      # missed and ret_sum are not the rule's
    dev = torch.device("cuda")
    lay = table_layout(A)
    assert _lib.load().pbn_curriculum_table_bytes(A) == lay["bytes"]
    pairs_t = torch.from_numpy(pairs).to(dev)
    totals_t = torch.zeros(8, dtype=torch.int64, device=dev)
    fill = 0x0123456789ABCDEF
    table_t = torch.full((lay["bytes"] // 8 + 1,), fill, dtype=torch.int64, device=dev)   # one canary word behind
    table_t[lay["refreshes"] // 8] = 7
    before = table_t.clone()
    # not due: frames 4 of every 3; never due: every 0
    totals_t[0] = 4
    _refresh(pairs_t, totals_t, A, H, 3, table_t)
    _refresh(pairs_t, totals_t, A, H, 0, table_t)
    assert torch.equal(table_t, before)
    # due
    totals_t[0] = 6
    _refresh(pairs_t, totals_t, A, H, 3, table_t)
    ref = C.build_table(pairs, H, refreshes=8)
    _assert_table(read_table(table_t, A), ref, (name, "due"))
    assert int(table_t[-1]) == fill
    pad = 4 * A * A % 8
    if pad:     # the four bytes between cdf and total stay as they were
        raw = table_t.cpu().numpy().view(np.uint32)
        assert raw[(lay["cdf"] + 4 * A * A) // 4] == np.array([fill], dtype=np.int64).view(np.uint32)[(A * A) % 2]
    # forced, on other statistics, with no totals at all; every frame: due whatever the count
    pairs2 = _seeded_pairs(A, 3)
    pairs_t.copy_(torch.from_numpy(pairs2))
    _refresh(pairs_t, None, A, H, -1, table_t)
    _assert_table(read_table(table_t, A), C.build_table(pairs2, H, refreshes=9), (name, "forced"))
    totals_t[0] = 5
    _refresh(pairs_t, totals_t, A, H, 1, table_t)
    assert read_table(table_t, A)["refreshes"] == 10 and int(table_t[-1]) == fill


# ---------------------------------------------------------------- the learners
N_ENVS, FRAMES, LOG, EVERY, CAPACITY = 300, 12, 3, 3, 4096


def _ddqn(settle):
    def make(graphable, curriculum=True, stats=True):
        from pbn_rl_amd.ddqn import DQN, DDQNLearner
        env = VectorPBNEnv(_pbn7(settle=settle), N_ENVS, seed=23)
        torch.manual_seed(11)
        lr = DDQNLearner(env, DQN(7, 8, [(16, 16)]), net_arch=[(16, 16)], total_frames=16, capacity=CAPACITY,
                         batch_size=16, target_update=4, exploration_fraction=0.5, beta_fraction=0.75, prioritised=True,
                         fused=True, seed=5, graphable=graphable, episode_stats=stats, stats_log_every=LOG,
                         curriculum=curriculum, curriculum_refresh=EVERY)
        env.reset()
        if stats:
            lr.stats.begin()                  # (the env was reset after the learner was built)
        return lr
    return make


def _bdq(graphable, curriculum=True, stats=True):
    from pbn_rl_amd.agent import BranchingQNetwork
    from pbn_rl_amd.replay import BDQLearner
    env = VectorPBNEnv(_pbn7(), N_ENVS, seed=23)
    torch.manual_seed(4)
    lr = BDQLearner(env, BranchingQNetwork((7, 7), 8, 3), capacity=CAPACITY, learning_starts=N_ENVS, batch_size=16,
                    target_update=4, epsilon_start=1.0, epsilon_final=0.5, epsilon_decay=8, seed=11, graphable=graphable,
                    fused=True, episode_stats=stats, stats_log_every=LOG, curriculum=curriculum, curriculum_refresh=EVERY)
    env.reset()
    if stats:
        lr.stats.begin()
    return lr


def _fields(lr):
    env, rp, fu, st = lr.env, lr.replay, lr.fused, lr.stats
    out = {"env.state": env.state, "env.target": env.target, "env.t": env.t, "env.flags": env.flags,
           "env.reward": env.reward, "ring.state": rp.state, "ring.next_state": rp.next_state, "ring.target": rp.target,
           "ring.action": rp.action, "ring.reward": rp.reward, "ring.done": rp.done,
           "loss": lr.last_loss.reshape(1) if lr.last_loss is not None else fu.loss.new_zeros(0),
           "q_flat": fu.q_flat, "t_flat": fu.t_flat, "adam.m": fu.m, "adam.v": fu.v}
    if st is not None:
        out.update({"stats.totals": st.totals_t, "stats.pairs": st.pairs_t, "stats.hist": st.hist_t,
                    "stats.series": st.series_t, "stats.ret": st.ret, "stats.len": st.len, "stats.src": st.src,
                    "stats.tgt": st.tgt})
    if lr.curriculum is not None:
        out["table"] = lr.curriculum.table_t
    return out


def _snapshot(lr):
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in _fields(lr).items()}


def _assert_fields(lr, want, what):
    torch.cuda.synchronize()
    for k, v in _fields(lr).items():
        assert torch.equal(v, want[k]), (what, k)


def _eager_against_the_reference(make):
    """FRAMES eager frames, each compared with the reference fed with the GPU's flags and rewards;
    returns the fields after the last one."""
    lr = make(False)
    env, rp, n = lr.env, lr.replay, N_ENVS
    spec = env.spec
    assert lr.curriculum is not None and lr.curriculum.refresh_every == EVERY and lr.curriculum.stats is lr.stats
    traj = C.Trajectory(spec, env.seed, env.env_offset, _u32(env.state[:, :n]), env.target[:n].cpu().numpy(), EVERY,
                        log_every=LOG)
    _assert_table(lr.curriculum.table(), traj.table, "constructed")
    resets = 0
    for f in range(FRAMES):
        rows = (rp.pos + np.arange(n)) % rp.capacity
        lr.frame()
        torch.cuda.synchronize()
        # what this frame stored as (state, target) is what the frame before left: the redrawn restart
        assert np.array_equal(_u32(rp.state)[:, rows], traj.state), (f, "ring.state")
        assert np.array_equal(rp.target.cpu().numpy()[rows], traj.target), (f, "ring.target")
        flags = env.flags[:n].cpu().numpy()
        traj.frame(env.step_index - 1, env.reward[:n].cpu().numpy(), flags, _u32(env.state[:, :n]))
        resets += len(traj.picks[-1])
        assert len(traj.picks[-1]) == int(((flags & RESET) != 0).sum())
        assert np.array_equal(_u32(env.state[:, :n]), traj.state), (f, "env.state")
        assert np.array_equal(env.target[:n].cpu().numpy(), traj.target), (f, "env.target")
        st, ref = lr.stats, traj.stats
        assert np.array_equal(st.pairs_t.cpu().numpy(), ref["pairs"]), (f, "pairs")
        assert np.array_equal(st.totals_t.cpu().numpy(), ref["totals"]), (f, "totals")
        assert np.array_equal(st.src[:n].cpu().numpy(), ref["src"]) and np.array_equal(st.tgt[:n].cpu().numpy(), ref["tgt"])
        assert np.array_equal(_u32(st.len[:n]), ref["len"]) and np.array_equal(st.series_t.cpu().numpy(), ref["series"])
        # the episode the statistics opened is the redrawn one
        picked = {i: (s, t) for i, s, t, _ in traj.picks[-1]}
        assert all((ref["src"][i], ref["tgt"][i]) == p for i, p in picked.items())
        _assert_table(lr.curriculum.table(), traj.table, (f, "table"))
    assert resets > n and traj.table["refreshes"] == 1 + FRAMES // EVERY
    w = traj.table["w"][~np.eye(4, dtype=bool)]
    assert len(set(w.tolist())) > 1                            # the statistics moved the weights
    assert int(traj.stats["totals"][7]) == 0                   # every episode started on an attractor: all paired
    # the padding envs keep the step law's restart: their targets are attractor ids all the same
    assert bool((env.target[n:] < 4).all())
    return _snapshot(lr)


@pytest.mark.parametrize("settle", [0, 3], ids=["one-update", "settle3"])
def test_ddqn_frames_eager_captured_and_run(settle):
    make = _ddqn(settle)
    want = _eager_against_the_reference(make)
    one, many = make(True), make(True)
    one.capture()
    many.capture()
    assert (one._tgt_prev is not None) == (settle >= 2)
    k = FRAMES - one.frames
    assert k >= 8 and many.frames == one.frames
    for _ in range(k):
        one.frame()
    many.run(k)
    _assert_fields(one, want, "captured, frame()")
    _assert_fields(many, want, "captured, run(k)")
    if settle >= 2:        # the carried targets are the redrawn ones
        assert torch.equal(one._tgt_prev, one.env.target) and torch.equal(many._tgt_prev, many.env.target)
    assert one.curriculum.table()["refreshes"] == 1 + FRAMES // EVERY


def test_bdq_frames_eager_and_captured():
    want = _eager_against_the_reference(_bdq)
    cap = _bdq(True)
    cap.capture()
    k = FRAMES - cap.frames
    assert k >= 6
    for _ in range(k):
        cap.frame()
    _assert_fields(cap, want, "captured")


def test_off_means_off(monkeypatch):
    """curriculum=False: no Curriculum, and no frame, eager or captured, reaches the library's
    curriculum entry points; the frames are those of a learner with the statistics alone."""
    L = _lib.load()

    def refuse(*a):
        raise AssertionError("a curriculum launch with curriculum=False")

    make = _ddqn(0)
    on = make(True, curriculum=False)
    eager = make(False, curriculum=False)
    assert on.curriculum is None and eager.curriculum is None
    monkeypatch.setattr(L, "pbn_curriculum_redraw", refuse)
    monkeypatch.setattr(L, "pbn_curriculum_refresh", refuse)
    for _ in range(6):
        eager.frame()
    on.capture()
    on.run(6 - on.frames)
    _assert_fields(on, _snapshot(eager), "captured against eager, curriculum off")
    with pytest.raises(AssertionError, match="curriculum launch"):
        L.pbn_curriculum_refresh()
    monkeypatch.undo()
    # the curriculum changes the trajectory (so the comparisons above compare something)
    with_c = make(False)
    for _ in range(6):
        with_c.frame()
    torch.cuda.synchronize()
    assert not torch.equal(with_c.env.target, eager.env.target)


def test_constructor_refusals():
    from pbn_rl_amd.ddqn import DQN, DDQNLearner
    env = VectorPBNEnv(_pbn7(), 64, seed=1)
    with pytest.raises(ValueError, match="curriculum=True needs episode_stats=True"):
        DDQNLearner(env, DQN(7, 8, [(16, 16)]), net_arch=[(16, 16)], total_frames=16, capacity=256, batch_size=16,
                    curriculum=True)
    one = VectorPBNEnv(_pbn7(1), 64, seed=1)
    with pytest.raises(ValueError, match="at least two attractors, the env's spec has 1"):
        Curriculum(one, EpisodeStats(one))
    with pytest.raises(ValueError, match="built for another env or spec"):
        Curriculum(env, EpisodeStats(one))
    other = VectorPBNEnv(_pbn7(), 64, seed=2)
    with pytest.raises(ValueError, match="built for another env or spec"):
        Curriculum(env, EpisodeStats(other))
    with pytest.raises(ValueError, match="refresh_every must be >= 0"):
        Curriculum(env, EpisodeStats(env), refresh_every=-1)
    cur = Curriculum(env, EpisodeStats(env))
    with pytest.raises(ValueError, match="step_t must be a one-element int64 tensor"):
        cur.redraw(step_t=torch.zeros(1, dtype=torch.int32, device=env.device))
    with pytest.raises(ValueError, match="target_copy must be a uint8 tensor of n_alloc elements"):
        cur.redraw(target_copy=torch.zeros(32, dtype=torch.uint8, device=env.device))
    env.set_spec(_pbn7(3))
    with pytest.raises(ValueError, match="3 attractors, this curriculum was built for 4"):
        cur.redraw()
    with pytest.raises(ValueError, match="3 attractors, this curriculum was built for 4"):
        cur.refresh()


# ---------------------------------------------------------------- the entry points' rejections
def test_rejections():
    env = VectorPBNEnv(_pbn7(), 64, seed=1)
    env.reset()
    st = EpisodeStats(env)
    cur = Curriculum(env, st)
    one = VectorPBNEnv(_pbn7(1), 64, seed=1)
    L = _lib.load()
    stream = env._stream()
    p = lambda t: t.data_ptr()  # noqa: E731
    step_t = torch.zeros(2, dtype=torch.int64, device=env.device)
    redraw = dict(net=env.net.handle, seed=1, step=1, d_step=None, env_offset=0, n_alloc=64, n_real=64,
                  d_flags=p(env.flags), d_state=p(env.state), d_target=p(env.target), d_target_copy=None,
                  d_table=p(cur.table_t), stream=stream)
    refresh = dict(d_totals=p(st.totals_t), d_pairs=p(st.pairs_t), n_attr=4, horizon=4, refresh_every=1,
                   d_table=p(cur.table_t), stream=stream)

    def rejected(fn, base, message, **change):
        args = {**base, **change}
        rc = getattr(L, fn)(*[args[k] for k in _lib.declared()[fn].params])
        assert rc == -22, (fn, change, rc)
        assert L.pbn_last_error().decode() == message, (fn, change, L.pbn_last_error().decode())

    env.flags.fill_(RESET)
    state, target, table = env.state.clone(), env.target.clone(), cur.table_t.clone()
    attr = "n_attr must be in 2..254"
    for A in (-1, 0, 1, 255):
        assert L.pbn_curriculum_table_bytes(A) == -22 and L.pbn_last_error().decode() == attr
    assert L.pbn_curriculum_table_bytes(2) == 16 + 16 + 16 and L.pbn_curriculum_table_bytes(3) == 24 + 40 + 16

    group = "n_alloc must be a positive multiple of 32 below 2^31"
    fn = "pbn_curriculum_redraw"
    rejected(fn, redraw, "null net", net=None)
    rejected(fn, redraw, "the curriculum needs a net with at least two attractors", net=one.net.handle)
    rejected(fn, redraw, "the curriculum needs a net with at least two attractors", net=one.net.handle, n_alloc=0)
    rejected(fn, redraw, group, n_alloc=0)
    rejected(fn, redraw, group, n_alloc=48)
    rejected(fn, redraw, group, n_alloc=1 << 31)
    rejected(fn, redraw, group, n_alloc=0, d_flags=None)                     # the sizes before the buffers
    rejected(fn, redraw, "n_real must be in 1..n_alloc", n_real=0)
    rejected(fn, redraw, "n_real must be in 1..n_alloc", n_real=65)
    for k in ("d_flags", "d_state", "d_target", "d_table"):
        rejected(fn, redraw, "null buffer", **{k: None})
    rejected(fn, redraw, "null buffer", d_flags=None, d_state=redraw["d_state"] + 2)   # null before misaligned
    rejected(fn, redraw, "d_state must be 4-byte aligned", d_state=redraw["d_state"] + 2)
    rejected(fn, redraw, "d_state must be 4-byte aligned", d_state=redraw["d_state"] + 2, d_table=redraw["d_table"] + 4)
    rejected(fn, redraw, "d_table must be 8-byte aligned", d_table=redraw["d_table"] + 4)
    rejected(fn, redraw, "d_table must be 8-byte aligned", d_table=redraw["d_table"] + 4, d_step=p(step_t) + 4)
    rejected(fn, redraw, "d_step must be 8-byte aligned", d_step=p(step_t) + 4)

    fn = "pbn_curriculum_refresh"
    for A in (1, 255):
        rejected(fn, refresh, attr, n_attr=A)
    rejected(fn, refresh, attr, n_attr=1, horizon=0)                         # the attractors before the horizon
    for H in (0, -3, 65536):
        rejected(fn, refresh, "horizon must be in 1..65535", horizon=H)
    rejected(fn, refresh, "horizon must be in 1..65535", horizon=0, refresh_every=-2)
    rejected(fn, refresh, "refresh_every must be >= -1", refresh_every=-2)
    rejected(fn, refresh, "refresh_every must be >= -1", refresh_every=-2, d_pairs=None)
    for k in ("d_pairs", "d_table"):
        rejected(fn, refresh, "null buffer", **{k: None})
    rejected(fn, refresh, "d_totals may be null only when refresh_every is -1 or 0", d_totals=None)
    for k in ("d_totals", "d_pairs", "d_table"):
        rejected(fn, refresh, "d_totals, d_pairs and d_table must be 8-byte aligned", **{k: refresh[k] + 4})
    torch.cuda.synchronize()
    # a rejected call launches nothing
    assert torch.equal(env.state, state) and torch.equal(env.target, target) and torch.equal(cur.table_t, table)
    # what is allowed: no totals when forced or never due, the step through a tensor, a target copy
    ok = {**refresh, "d_totals": None, "refresh_every": -1}
    assert L.pbn_curriculum_refresh(*[ok[k] for k in _lib.declared()[fn].params]) == 0
    ok["refresh_every"] = 0
    assert L.pbn_curriculum_refresh(*[ok[k] for k in _lib.declared()[fn].params]) == 0
    copy = torch.zeros(64, dtype=torch.uint8, device=env.device)
    ok = {**redraw, "d_step": p(step_t), "d_target_copy": p(copy)}
    assert L.pbn_curriculum_redraw(*[ok[k] for k in _lib.declared()["pbn_curriculum_redraw"].params]) == 0
    torch.cuda.synchronize()
    assert cur.table()["refreshes"] == 2 and torch.equal(copy, env.target)
