"""What tests/test_gpu_checkpoint.py and tests/test_gpu_bdq_run.py share: the learners of the issue's
shapes, every field a frame writes, the host mirrors, and the exact comparisons.

Shapes (all cases): 90 envs (``n_alloc`` 96: the padding envs are stored and restored too), a 256-row
ring (it wraps before and after the checkpoint), horizon 6, perturbation 0.01."""
import copy
import functools

import numpy as np
import torch

from pbn_rl_amd.attractors import load_attractors
from pbn_rl_amd.ddqn import DQN, DDQNLearner
from pbn_rl_amd.network import load_network
from pbn_rl_amd.replay import BDQLearner
from pbn_rl_amd.spec import EnvSpec
from pbn_rl_amd.vector_env import VectorPBNEnv

N_ENVS, CAP = 90, 256
ENV_SEED, WEIGHTS_SEED = 23, 11            # learner A's
OTHER_ENV_SEED, OTHER_WEIGHTS_SEED = 99, 77     # learner B's, so that anything load forgets shows up


@functools.lru_cache(maxsize=None)
def spec_of(net, settle=0):
    return EnvSpec(load_network(net), load_attractors(net), perturbation=0.01, horizon=6, settle=settle)


def _stats_kw(stats):
    return dict(episode_stats=True, stats_log_every=2, curriculum=True, curriculum_refresh=3) if stats else {}


def _reset(lr, other):
    """A's env resets once under its own seed.  B's resets under another seed (``load`` puts A's back)
    unless it is to be captured before the load: a captured frame holds the env's seed and the base
    of its step index as launch arguments, so such a B keeps both and differs by the frames it runs."""
    lr.env.reset(seed=OTHER_ENV_SEED) if other else lr.env.reset()
    if lr.stats is not None:
        lr.stats.begin()
    return lr


def ddqn_learner(net, arch, B, settle, graphable, *, other=False, other_env=None, stats=False, n_envs=N_ENVS, **kw):
    env = VectorPBNEnv(spec_of(net, settle), n_envs, seed=ENV_SEED)
    n = spec_of(net, settle).n
    torch.manual_seed(OTHER_WEIGHTS_SEED if other else WEIGHTS_SEED)
    args = dict(net_arch=[tuple(a) for a in arch], total_frames=16, capacity=CAP, batch_size=B, target_update=4,
                exploration_fraction=0.5, beta_fraction=0.75, prioritised=True, fused=True, seed=5,
                graphable=graphable, **_stats_kw(stats))
    args.update(kw)
    lr = DDQNLearner(env, DQN(n, n + 1, args["net_arch"]), **args)
    return _reset(lr, other if other_env is None else other_env)


def bdq_learner(graphable, *, fused=True, prioritised=False, other=False, other_env=None, stats=False, **kw):
    env = VectorPBNEnv(spec_of("pbn28"), N_ENVS, seed=ENV_SEED)
    torch.manual_seed(OTHER_WEIGHTS_SEED if other else WEIGHTS_SEED)
    args = dict(capacity=CAP, batch_size=16 if fused else 32, learning_starts=16, updates_per_frame=2, target_update=6,
                epsilon_decay=10, seed=5, graphable=graphable, fused=fused, prioritised=prioritised,
                per_beta_steps=16, **_stats_kw(stats))
    args.update(kw)
    lr = BDQLearner(env, **args)
    return _reset(lr, other if other_env is None else other_env)


# ------------------------------------------------------------------------------------ what is compared
def fields(lr):
    """Every device tensor a frame writes: tests/test_gpu_ddqn_graph.py's ``_fields`` (the images and
    ``last_loss`` among them), the env's ``t`` and ``final_state``, the PyTorch update's parameters and
    Adam state, the episode statistics and the curriculum table.  Not ``beta_t`` and not the
    pre-drawn rows: an eager and a captured learner hold them a frame apart (``check_counters``)."""
    env, rp, fu = lr.env, lr.replay, lr.fused
    d = {"env.state": env.state, "env.target": env.target, "env.t": env.t, "env.flags": env.flags,
         "env.reward": env.reward, "env.flipmask": env.flipmask, "env.final_state": env.final_state,
         "actions": lr.agent.actions,
         "ring.state": rp.state, "ring.next_state": rp.next_state, "ring.target": rp.target,
         "ring.action": rp.action, "ring.reward": rp.reward, "ring.done": rp.done,
         "last_loss": lr.last_loss.reshape(1) if lr.last_loss is not None else torch.zeros(0, device=env.device)}
    if lr.prioritised:
        d.update({"sum_tree": rp.sum_tree, "min_tree": rp.min_tree, "max_priority": rp.max_priority,
                  "counter_t": rp.counter_t, "prio": lr._prio})
    if fu is not None:
        d.update({"q_flat": fu.q_flat, "t_flat": fu.t_flat, "q_image": fu.q_image, "t_image": fu.t_image,
                  "adam.m": fu.m, "adam.v": fu.v, "adam.step": fu.step, "loss": fu.loss})
        if hasattr(fu, "grad_norm"):
            d["grad_norm"] = fu.grad_norm
    else:
        for prefix, net in (("q", lr.q), ("target", lr.target)):
            for k, v in net.state_dict().items():
                d[f"{prefix}.{k}"] = v
        for name, p in lr.q.named_parameters():
            for k, v in lr.opt.state[p].items():
                d[f"adam.{k}.{name}"] = torch.as_tensor(v).reshape(-1)
    if lr.stats is not None:
        for k in lr.stats._STATE_TENSORS:
            d["stats." + k] = getattr(lr.stats, k)
    if lr.curriculum is not None:
        d["curriculum.table_t"] = lr.curriculum.table_t
    return d


def mirrors(lr):
    """Every host mirror."""
    rp, env = lr.replay, lr.env
    names = ("frames", "updates", "epsilon") + (("beta", "last_beta", "syncs") if isinstance(lr, DDQNLearner) else ())
    m = {k: copy.copy(getattr(lr, k)) for k in names}
    m.update({"replay.pos": rp.pos, "replay.size": rp.size, "env.step_index": env.step_index, "env.seed": env.seed,
              "env.env_offset": env.env_offset})
    if lr.prioritised:
        m["replay.beta"] = rp.beta
    if isinstance(lr, BDQLearner) and lr._predraws():
        m["draws"] = lr.draws
    if lr.stats is not None:
        m["stats.last_totals"] = dict(lr.stats._last_totals)
        m["stats.last_missed"] = lr.stats._last_missed.tolist()
    return m


def snapshot(lr):
    torch.cuda.synchronize()
    return {"fields": {k: v.clone() for k, v in fields(lr).items()}, "mirrors": mirrors(lr)}


def assert_same(lr, want, what, skip=()):
    """``lr`` against a snapshot, exactly (but the fields named in ``skip``)."""
    torch.cuda.synchronize()
    got = fields(lr)
    assert got.keys() == want["fields"].keys(), what
    for k, v in got.items():
        w = want["fields"][k]
        if k in skip:
            continue
        assert v.dtype == w.dtype and v.shape == w.shape and torch.equal(v, w), (what, k)
    have = mirrors(lr)
    for k, w in want["mirrors"].items():
        assert have[k] == w, (what, k, have[k], w)


def check_counters(lr, what):
    """The device counters against the host mirrors, by the learner's mode."""
    torch.cuda.synchronize()
    rp, env = lr.replay, lr.env
    captured = lr._graph is not None
    if getattr(lr, "_pos_t", None) is not None:
        assert int(lr._pos_t) == rp.pos and int(lr._size_t) == rp.size, what
    if captured:
        assert int(lr._step_t) == env.step_index, what
        assert float(lr._eps64) == lr.epsilon, (what, float(lr._eps64), lr.epsilon)
        assert float(lr._eps32) == torch.tensor(lr.epsilon, dtype=torch.float32).item(), what
        if lr._tgt_prev is not None:
            assert torch.equal(lr._tgt_prev, env.target), what
    if lr.fused is not None:
        assert float(lr.fused.step) == lr.updates, what
    if isinstance(lr, DDQNLearner):
        assert int(rp.counter_t) == lr.updates, what
        # beta_t across the frame boundary: the next frame's beta when captured, the last frame's when eager
        assert rp.beta_t.dtype == torch.float64
        assert float(rp.beta_t) == (lr.beta if captured else lr.last_beta), (what, float(rp.beta_t), lr.beta, lr.last_beta)
        assert rp.beta == lr.last_beta, what
    else:
        if lr.prioritised:
            assert float(rp.beta_t) == rp.beta and int(rp.counter_t) == lr.updates, what
        if lr._predraws():      # a captured frame has drawn the next frame's rows already
            assert int(lr._draw_t) == lr.draws + (1 if captured else 0), (what, int(lr._draw_t), lr.draws)


def pointers(lr):
    """The addresses a captured graph, RingStore and FrameAdvance hold."""
    extra = [getattr(lr, k) for k in ("_pos_t", "_size_t", "_step_t", "_eps64", "_eps32", "_draw_t", "_idx", "_tgt_prev")
             if getattr(lr, k, None) is not None]
    return [v.data_ptr() for k, v in fields(lr).items() if v.numel() and k != "last_loss"] + [t.data_ptr() for t in extra] + \
           [p.data_ptr() for p in lr.q.parameters()] + [lr.replay.beta_t.data_ptr() if lr.prioritised else 0]


def same_value(a, b):
    """Equality of the statistics' readings: dicts, lists, numpy arrays, floats (nan equals nan)."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_value(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_value(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))
    if isinstance(a, float) and a != a:
        return isinstance(b, float) and b != b
    return a == b
