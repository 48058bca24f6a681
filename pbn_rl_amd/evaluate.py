"""Source -> target control evaluation of a trained agent, batched on the GPU.

The reference scores every trained agent with the loop of model_tester.py:587-658: for each
ordered pair of attractors (``itertools.product``, :598) and each run, the env starts in the
source attractor's first state ('*' -> 0, :609), the agent acts greedily towards the target
attractor's first state (:600-603,622), and the ``env.step`` calls are counted until the state
lies in the target attractor (:616); a run that is still outside after ``max_steps`` = 100 steps
fails and is recorded as 101 (:628-636).  The result is the per-pair sum of lengths
(``save_matrix``) and the length histogram (``data``), pickled as ``data/results/pbn_*.pkl``.

Here every (pair, run) is one env of a ``VectorPBNEnv``: env ``i = pair_index * runs + run``,
padded to a multiple of 32, env ids from 0.  ``reset()`` takes step index 0 and protocol step
``k`` uses step index ``k``, so a CPU replay over the oracle at the same (seed, env id, step) is
bit-identical.  One protocol step is act -> ``pbn_step_dev`` -> ``pbn_eval_track`` -> step index
+ 1 on one stream, captured once as a hipGraph and replayed; the host reads the number of open
runs every ``poll`` steps instead of synchronising every step.  Runs that have ended keep
stepping (no compaction: env ids, and with them the draws of the open runs, never move) and
``pbn_eval_track`` ignores them.

The pair plan, the summary and the writers below are plain numpy (no GPU needed);
``evaluate_control`` imports torch and the HIP library when it is called.
"""
from __future__ import annotations

import copy
import itertools
import json
import pickle
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .attractors import clean_state
from .spec import EnvSpec

__all__ = ["evaluate_control", "ControlEvaluation", "EvalPlan", "plan_pairs", "summarize", "pooled_mean"]

MAX_STEPS_CAP = 254      # the step kernels' per-episode step counter is uint8


def _round32(n: int) -> int:
    return (n + 31) // 32 * 32


def _pack_words(bits: np.ndarray) -> np.ndarray:
    """(n, N) 0/1 -> (W, n) uint32 words (bit i of word w = node 32 w + i)."""
    n, N = bits.shape
    W = (N + 31) // 32
    pad = np.zeros((n, 32 * W), np.uint64)
    pad[:, :N] = bits
    words = (pad.reshape(n, W, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2)
    return np.ascontiguousarray(words.T.astype(np.uint32))


@dataclass
class EvalPlan:
    """Which env runs what.  Arrays have ``n_alloc`` rows; rows past ``n_real`` are padding
    (source and target = attractor 0, closed)."""
    pairs: List[Tuple[int, int]]
    runs: int
    n_attractors: int
    n_real: int
    n_alloc: int
    start_bits: np.ndarray        # (n_alloc, N) uint8
    target_bits: np.ndarray       # (n_alloc, N) uint8: the target attractor's first state
    target_id: np.ndarray         # (n_alloc,) uint8
    count0: np.ndarray            # (n_alloc,) int32, 0
    open0: np.ndarray             # (n_alloc,) uint8: 0 where the start state lies in the target (:616)

    @property
    def start_words(self) -> np.ndarray:
        return _pack_words(self.start_bits)


def plan_pairs(attractors, pairs: Optional[Sequence[Tuple[int, int]]] = None, runs: int = 10) -> EvalPlan:
    """The env layout of one evaluation: env ``pair_index * runs + run`` starts in
    ``attractors[source][0]`` and aims at attractor ``target``.  ``pairs`` defaults to
    ``itertools.product(range(A), repeat=2)`` in that order (model_tester.py:598).  A run whose
    start state already lies in its target attractor has length 0 and is closed from the start
    (the ``while not env.in_target(state)`` of :616 never enters)."""
    atts = [[clean_state(s) for s in a] for a in attractors]
    A = len(atts)
    if A == 0 or any(len(a) == 0 for a in atts):
        raise ValueError("the evaluation needs at least one attractor, none of them empty")
    if runs < 1:
        raise ValueError("runs must be at least 1")
    pairs = list(itertools.product(range(A), repeat=2)) if pairs is None else [(int(a), int(t)) for a, t in pairs]
    if not pairs:
        raise ValueError("no pairs to evaluate")
    for a, t in pairs:
        if not (0 <= a < A and 0 <= t < A):
            raise ValueError(f"pair {(a, t)} outside the {A} attractors")
    N = len(atts[0][0])
    n_real = len(pairs) * runs
    n_alloc = _round32(n_real)
    first = np.array([a[0] for a in atts], dtype=np.uint8).reshape(A, N)
    sets = [set(a) for a in atts]
    src = np.zeros(n_alloc, np.int64)
    tgt = np.zeros(n_alloc, np.int64)
    src[:n_real] = np.repeat([a for a, _ in pairs], runs)
    tgt[:n_real] = np.repeat([t for _, t in pairs], runs)
    inside = np.array([atts[a][0] in sets[t] for a, t in pairs], dtype=bool)
    open0 = np.zeros(n_alloc, np.uint8)
    open0[:n_real] = np.repeat(~inside, runs)
    return EvalPlan(pairs=pairs, runs=int(runs), n_attractors=A, n_real=n_real, n_alloc=n_alloc,
                    start_bits=first[src], target_bits=first[tgt], target_id=tgt.astype(np.uint8),
                    count0=np.zeros(n_alloc, np.int32), open0=open0)


def pooled_mean(data: Dict[int, int], max_steps: int = 100) -> float:
    """model_tester.py:713-727: the mean length over the runs that took 1..max_steps steps
    (lengths 0 and failures left out); nan when there is none."""
    s = div = 0
    for k, v in data.items():
        if k == 0 or k > max_steps:
            continue
        s += k * v
        div += v
    return s / div if div else float("nan")


@dataclass
class ControlEvaluation:
    """The result of ``evaluate_control``.

    counts      (n_pairs, runs) int32: env.step calls until the target; max_steps + 1 = failure
    matrix      (A, A) float64: per-pair sums of the counts, a failure adding max_steps + 1 -- the
                reference's ``save_matrix`` (``matrix / runs`` is the heat map it plots)
    data        {length: runs}, always with the failure key max_steps + 1 (the reference's ``data``)
    open_after  (max_steps + 1,) runs still open after protocol step k (index 0: at the start)
    hit_states  (n_pairs, runs, W) uint32 state words in which the run ended: the start state for
                length 0, the state that hit the target otherwise; zeros for failures
    strategies  (n, max_steps, K) int16 actions of run n = pair * runs + run, -1 where no step
                was taken; None unless recorded
    """
    counts: np.ndarray
    matrix: np.ndarray
    data: Dict[int, int]
    pairs: List[Tuple[int, int]]
    runs: int
    max_steps: int
    pair_fail: Optional[np.ndarray] = None
    open_after: Optional[np.ndarray] = None
    hit_states: Optional[np.ndarray] = None
    strategies: Optional[np.ndarray] = None
    settings: dict = field(default_factory=dict)

    @property
    def failed(self) -> int:
        return int(self.data.get(self.max_steps + 1, 0))

    @property
    def total(self) -> int:
        return int(self.counts.size)

    def mean_length(self) -> float:
        return pooled_mean(self.data, self.max_steps)

    def as_dict(self) -> dict:
        return {"save_matrix": self.matrix.tolist(), "data": {str(k): int(v) for k, v in self.data.items()},
                "counts": self.counts.tolist(), "pairs": [list(p) for p in self.pairs], "runs": self.runs,
                "max_steps": self.max_steps, "failed": self.failed, "mean_length": self.mean_length(),
                "settings": self.settings}

    def save(self, path: str) -> None:
        """``.pkl``: the reference's ``pkl.dump((save_matrix, data), f)`` (model_tester.py:656-658),
        a float64 array and a plain dict; ``.json``: the same with the counts and the settings."""
        if path.endswith(".pkl"):
            with open(path, "wb") as f:
                pickle.dump((np.array(self.matrix, dtype=np.float64), {int(k): int(v) for k, v in self.data.items()}),
                            f)
        elif path.endswith(".json"):
            with open(path, "w") as f:
                json.dump(self.as_dict(), f)
        else:
            raise ValueError("save() writes .pkl or .json")


def summarize(counts: np.ndarray, pairs: Sequence[Tuple[int, int]], n_attractors: int, max_steps: int = 100, *,
              pair_sum: Optional[np.ndarray] = None, pair_fail: Optional[np.ndarray] = None,
              hist: Optional[np.ndarray] = None, **extra) -> ControlEvaluation:
    """(n_pairs, runs) counts -> ControlEvaluation.  ``pair_sum`` / ``pair_fail`` / ``hist`` are
    ``pbn_eval_reduce``'s outputs when the counts come from the GPU; without them the same sums
    are taken here."""
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    if counts.ndim != 2 or counts.shape[0] != len(pairs):
        raise ValueError("counts must have shape (n_pairs, runs)")
    if counts.min(initial=0) < 0 or counts.max(initial=0) > max_steps + 1:
        raise ValueError(f"counts must lie in 0..{max_steps + 1}")
    if pair_sum is None:
        pair_sum = counts.sum(axis=1, dtype=np.int64)
    if pair_fail is None:
        pair_fail = (counts == max_steps + 1).sum(axis=1).astype(np.int32)
    if hist is None:
        hist = np.bincount(counts.ravel(), minlength=max_steps + 2)
    matrix = np.zeros((n_attractors, n_attractors), dtype=np.float64)
    np.add.at(matrix, (np.array([a for a, _ in pairs]), np.array([t for _, t in pairs])),
              np.asarray(pair_sum, dtype=np.float64))
    data = {int(k): int(v) for k, v in enumerate(np.asarray(hist)) if v}
    data.setdefault(max_steps + 1, 0)
    return ControlEvaluation(counts=counts, matrix=matrix, data=data, pairs=[tuple(p) for p in pairs],
                             runs=int(counts.shape[1]), max_steps=int(max_steps),
                             pair_fail=np.asarray(pair_fail, dtype=np.int32), **extra)


def evaluate_control(env_or_spec, model, *, attractors=None, pairs=None, runs: int = 10, max_steps: int = 100,
                     seed: int = 0, device=None, graph: bool = True, poll: int = 8, record_actions: bool = False,
                     fused: bool = True) -> ControlEvaluation:
    """model_tester.py:587-658 for every (pair, run) at once on one GPU.

    ``env_or_spec``: a PBNEnv, a VectorPBNEnv or an EnvSpec; its network, step law (``settle``),
    perturbation and rewards are kept, the evaluation runs without horizon and autoreset.
    ``attractors`` (default: the spec's) are the evaluation's attractor set, in the order the
    result matrix is indexed; ``pairs`` as ``plan_pairs``.
    ``model``: a BranchingQNetwork, acting greedily through ``BatchedBDQ.act_q`` (one fused launch;
    ``fused=False``: the torch module on the unpacked observation), a DQN (ddqn.py; one branch,
    greedy through ``BatchedDDQN.act_q``), or a policy
    ``(state_bits (n, N) uint8, target_bits (n, N) uint8) -> (n, k)`` actions in [0, N] on the GPU.
    ``graph``: capture one protocol step after a first eager one and replay it (a policy that
    synchronises cannot be captured: pass ``graph=False``).  ``poll``: the number of open runs is
    read every ``poll`` steps, and the loop ends when it is 0.  Neither changes the result.
    ``record_actions``: keep every run's actions (``strategies``).
    """
    import torch

    from . import _lib
    from .agent import BatchedBDQ, BranchingQNetwork
    from .ddqn import DQN, BatchedDDQN
    from .ssd import _spec_of
    from .vector_env import VectorPBNEnv, actions_to_flipmask, unpack_states

    if not 1 <= max_steps <= MAX_STEPS_CAP:
        raise ValueError(f"max_steps must be in 1..{MAX_STEPS_CAP}")
    if poll < 1:
        raise ValueError("poll must be at least 1")
    base = _spec_of(env_or_spec)
    atts = base.attractors if attractors is None else attractors
    spec = EnvSpec(base.network, atts, perturbation=base.perturbation, prob_bits=base.prob_bits, horizon=0,
                   success_reward=base.success_reward, wrong_attractor_cost=base.wrong_attractor_cost,
                   action_cost=base.action_cost, step_cost=base.step_cost, settle=base.settle)
    plan = plan_pairs(spec.attractors, pairs, runs)
    N, W, n, n_real = spec.n, spec.words, plan.n_alloc, plan.n_real
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    L = _lib.load()
    if not hasattr(L, "pbn_eval_track"):
        raise _lib.PbnError("libpbn_env.so predates pbn_eval_track: rebuild it")

    def to_dev(a: np.ndarray, dtype) -> "torch.Tensor":
        return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)

    venv = VectorPBNEnv(spec, n_real, seed=seed, device=dev, autoreset=False, keep_final_state=False)
    with torch.cuda.device(dev), torch.no_grad():
        venv.reset()                                     # step index 0; the padding envs keep its state
        start_words = plan.start_words.view(np.int32)
        venv.set_state(to_dev(start_words[:, :n_real], torch.int32), target=to_dev(plan.target_id[:n_real], torch.uint8),
                       t=torch.zeros(n_real, dtype=torch.uint8, device=dev))
        venv.flipmask.zero_()
        step0 = venv.step_index                          # 1: protocol step k runs at step index k
        step_t = torch.full((1,), step0, dtype=torch.int64, device=dev)
        count = to_dev(plan.count0, torch.int32)
        open_ = to_dev(plan.open0, torch.uint8)
        closed0 = plan.open0 == 0
        closed0[n_real:] = False
        hit = to_dev(np.where(closed0[None, :], start_words, 0), torch.int32)
        open_after = torch.zeros(max_steps + 1, dtype=torch.int32, device=dev)
        n_open = int(plan.open0.sum())
        open_after[0] = n_open
        buf = {"actions": None, "strategy": None}

        if isinstance(model, BranchingQNetwork):
            K = int(model.n)
            bdq = BatchedBDQ(venv, copy.deepcopy(model), branches=K, epsilon=0.0, fused_tail=True)
            buf["actions"] = bdq.actions

            def act(check: bool) -> None:
                if fused:
                    bdq.act_q(epsilon=0.0, step_t=step_t)
                else:
                    bdq.act_dev(bdq.q(bdq.observe()), step_t, epsilon=0.0)
        elif isinstance(model, DQN):
            # one branch, greedy (DDQN.predict(deterministic=True), ddqn_per/__init__.py:155-179)
            ddqn = BatchedDDQN(venv, copy.deepcopy(model), epsilon=0.0)
            buf["actions"] = ddqn.actions.view(n, 1)

            def act(check: bool) -> None:
                ddqn.act_q(epsilon=0.0, step_t=step_t)
        elif callable(model):
            tbits = to_dev(plan.target_bits[:n_real], torch.uint8)

            def act(check: bool) -> None:
                a = model(unpack_states(venv.state[:, :n_real], N), tbits).to(dev)
                if a.dim() == 1:
                    a = a[:, None]
                venv.flipmask[:, :n_real].copy_(actions_to_flipmask(a, N, check=check))
                if buf["actions"] is None:
                    buf["actions"] = torch.zeros(n, a.shape[1], dtype=torch.int32, device=dev)
                buf["actions"][:n_real].copy_(a)
        else:
            raise TypeError("model must be a BranchingQNetwork, a DQN or a callable policy")

        def track() -> None:
            actions = buf["actions"]
            if record_actions and buf["strategy"] is None:
                buf["strategy"] = torch.full((max_steps, n, actions.shape[1]), -1, dtype=torch.int16, device=dev)
            strategy = buf["strategy"]
            _lib.check(L.pbn_eval_track(n, n_real, W, actions.shape[1], max_steps, step_t.data_ptr(), step0,
                                        venv.flags.data_ptr(), actions.data_ptr(), venv.state.data_ptr(),
                                        count.data_ptr(), open_.data_ptr(), hit.data_ptr(),
                                        strategy.data_ptr() if strategy is not None else None,
                                        open_after.data_ptr(), venv._stream()), "pbn_eval_track")

        def protocol_step(check: bool) -> None:
            act(check)
            venv.step_flipmask_dev(step_t)
            track()
            step_t.add_(1)

        pinned = torch.zeros(1, dtype=torch.int32).pin_memory()
        k, g = 0, None
        while n_open > 0 and k < max_steps:
            if not graph or k == 0:
                protocol_step(check=True)                # eager: the first step validates the actions
            else:
                if g is None:                            # (capturing records the step, it does not run it)
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        protocol_step(check=False)
                g.replay()
            k += 1
            if k % poll == 0 and k < max_steps:          # (after max_steps steps every run is closed)
                pinned.copy_(open_after[k:k + 1], non_blocking=True)
                torch.cuda.current_stream(dev).synchronize()
                n_open = int(pinned[0])
        venv.step_index = step0 + k

        n_pairs = len(plan.pairs)
        pair_sum = torch.empty(n_pairs, dtype=torch.int64, device=dev)
        pair_fail = torch.empty(n_pairs, dtype=torch.int32, device=dev)
        hist = torch.zeros(max_steps + 2, dtype=torch.int64, device=dev)
        _lib.check(L.pbn_eval_reduce(count.data_ptr(), n_pairs, plan.runs, max_steps, pair_sum.data_ptr(),
                                     pair_fail.data_ptr(), hist.data_ptr(), venv._stream()), "pbn_eval_reduce")
        counts = count[:n_real].view(n_pairs, plan.runs).cpu().numpy()
        hit_states = hit[:, :n_real].t().contiguous().cpu().numpy().view(np.uint32).reshape(n_pairs, plan.runs, W)
        strategies = None
        if record_actions:
            if buf["strategy"] is None:                  # no step was taken
                strategies = np.full((n_real, max_steps, 0), -1, dtype=np.int16)
            else:
                strategies = buf["strategy"][:, :n_real].transpose(0, 1).contiguous().cpu().numpy()
        res = summarize(counts, plan.pairs, plan.n_attractors, max_steps, pair_sum=pair_sum.cpu().numpy(),
                        pair_fail=pair_fail.cpu().numpy(), hist=hist.cpu().numpy(),
                        open_after=open_after.cpu().numpy(), hit_states=hit_states, strategies=strategies,
                        settings={"network": spec.network.name, "n_attractors": plan.n_attractors,
                                  "settle": spec.settle, "perturbation": spec.perturbation, "seed": int(seed),
                                  "runs": plan.runs, "max_steps": int(max_steps)})
    venv.close()
    return res
