"""Steady-state distribution (SSD) of a PBN, batched on the GPU.

The reference evaluates every trained agent with ``gym_PBN.utils.eval.compute_ssd_hist(env,
model, resets=300, iters=100_000, multiprocess=True)`` (train_pbn_28.py:257,
train_pbn_10.py:257, train_ddqn.py:156): independent chains of the (optionally controlled)
PBN are run from resets and the visited states are counted.  gym_PBN is not available
(SURVEY.md 8(c)), so the estimator is restated here and its result is parity-unpinned:

* ``resets`` chains, one env each, started by ``pbn_reset`` (a random attractor state);
* no autoreset and no horizon: each chain runs ``burn_in + iters`` steps of the frozen step
  semantics with perturbation; the interventions are the policy's (``model``),
  or none;
* every state s' after step ``burn_in + 1 .. burn_in + iters`` of every chain is counted
  (``pbn_state_histogram`` on the rollout's ``final_state``), and the counts are normalised.

The dense histogram's bins are full states, so networks with at most 32 nodes (2^N bins in HBM:
1 GiB of 32-bit counters for Bittner-28).  ``sparse=True`` counts the visited states in a device
hash table instead (state_table.py): any network the env runs, 64-bit counts, no 2^N array.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib
from .spec import EnvSpec
from .state_table import SparseSSD, StateTable
from .vector_env import VectorPBNEnv, actions_to_flipmask, unpack_states

__all__ = ["compute_ssd_hist", "state_histogram", "SparseSSD"]


def state_histogram(states: torch.Tensor, n_cols: int, n_bits: int, hist: torch.Tensor) -> None:
    """hist[states[r, c] & (2^n_bits - 1)] += 1 for every row r and column c < n_cols
    (states: int32 [rows, row_stride] on the GPU, hist: int32 [2^n_bits])."""
    if states.dim() != 2 or not states.is_contiguous():
        raise ValueError("states must be a contiguous [rows, row_stride] tensor")
    L = _lib.load()
    with torch.cuda.device(states.device):
        _lib.check(L.pbn_state_histogram(states.data_ptr(), states.shape[0], n_cols, states.shape[1], n_bits,
                                         hist.data_ptr(), torch.cuda.current_stream(states.device).cuda_stream),
                   "pbn_state_histogram")


def _spec_of(env) -> EnvSpec:
    if isinstance(env, EnvSpec):
        return env
    for obj in (env, getattr(env, "env", None), getattr(getattr(env, "env", None), "env", None)):
        if obj is not None and isinstance(getattr(obj, "spec", None), EnvSpec):
            return obj.spec
    raise TypeError("compute_ssd_hist needs an EnvSpec, a VectorPBNEnv or a PBNEnv")


def compute_ssd_hist(env, model: Optional[Callable] = None, resets: int = 300, iters: int = 100_000,
                     multiprocess: bool = False, *, burn_in: int = 0, seed: int = 0, chunk: int = 200,
                     device=None, graph: bool = True, fused: Optional[bool] = None, sparse: bool = False,
                     capacity: int = 1 << 16,
                     stats: Optional[dict] = None) -> Tuple[Union[np.ndarray, SparseSSD], None]:
    """Returns (ssd, plot): ssd[s] = fraction of counted steps spent in state s (float64,
    2^N entries, state s = bit i for node i); plot is None (no plotting backend here).

    ``model``: None (no interventions); a ``DQN``, or a ``BatchedDDQN`` whose network is taken
    (the reference's trained DDQN agent, train_ddqn.py:156), acting greedily (epsilon 0) on each
    chain's state and the target its reset drew; or a policy mapping the (resets, N) uint8 state
    bits on the GPU to (resets, k) actions in [0, N] (0 = no-op), called every step.
    ``multiprocess`` is accepted for signature compatibility; chains already run in parallel.
    ``fused`` (a ``DQN`` only; default: whenever the step kernel takes the network, see
    ``BatchedDDQN``): the chains run as ``BatchedDDQN.rollout`` launches of ``chunk`` steps, the
    network evaluated inside the step kernel, exactly as the chains without a model do;
    ``fused=False`` runs one ``act_q`` + ``pbn_step_dev`` + histogram per step.  Both give the same
    histogram.
    ``graph``: with a per-step model, capture one policy step (state unpack, model, flip masks,
    pbn_step_dev, histogram) in a hipGraph after a first eager step has validated the
    actions, and replay it; a model that cannot be captured (host syncs) raises, and
    ``graph=False`` runs every step eagerly.  Both give the same histogram.
    ``sparse``: count the visited states in a ``StateTable`` of initially ``capacity`` slots
    instead of 2^N bins, and return (``SparseSSD``, None): any N the env supports, no limit on
    resets * iters.  The chains are the dense call's (same envs, seeds and step indices), so for
    N <= 32 ``SparseSSD.to_dense()`` equals the dense result exactly.  With a per-step model the
    captured step stages its ``final_state`` into a (chunk, W, n) buffer at a device-held row, and
    the host inserts the staged rows every ``chunk`` steps (the insert's epoch is a launch
    argument and growth reallocates the table, so it stays out of the graph).  ``stats`` (a dict)
    receives the table's final ``capacity``, ``n_growths`` and ``n_states``.
    """
    spec = _spec_of(env)
    N = spec.n
    if N > 32 and not sparse:
        raise ValueError("the SSD histogram has 2^N bins: networks with at most 32 nodes "
                         "(sparse=True counts the visited states of any network)")
    if resets * iters >= 1 << 32 and not sparse:
        # the histogram's bins are 32-bit counters: a fixed-point attractor could take every count
        raise ValueError(f"resets * iters = {resets * iters} counted steps overflow the 32-bit bins (< 2^32; "
                         "sparse=True counts in 64 bits)")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    venv = VectorPBNEnv(spec, resets, seed=seed, device=dev, autoreset=False, keep_final_state=True)
    venv.reset()
    n = venv.n_alloc
    if sparse:
        table = StateTable(N, dev, capacity=capacity)

        def count_rows(fs: torch.Tensor) -> None:     # fs: (k, W, n) final states of k steps
            table.add(fs, resets)
    else:
        hist = torch.zeros(1 << N, dtype=torch.int32, device=dev)

        def count_rows(fs: torch.Tensor) -> None:
            state_histogram(fs.view(fs.shape[0], n), resets, N, hist)
    from .ddqn import DQN, BatchedDDQN      # (ddqn.py imports this package's env modules)
    agent = None
    if isinstance(model, (DQN, BatchedDDQN)):
        agent = BatchedDDQN(venv, model.q if isinstance(model, BatchedDDQN) else model, epsilon=0.0)
    if fused is None:
        fused = agent is not None and agent.kernel
    if fused and agent is None:
        raise ValueError("fused=True needs a DQN (or a BatchedDDQN): the step kernel evaluates no other model")

    def run_chunks(roll) -> None:
        """burn-in, then the counted steps, as launches of ``chunk`` steps: roll(k, keep_final, out)"""
        left = burn_in
        while left > 0:
            k = min(chunk, left)
            roll(k, False, None)
            left -= k
        left, buf = iters, None
        while left > 0:
            k = min(chunk, left)
            buf = roll(k, True, buf if buf is not None and buf["_n_steps"] == k else None)
            count_rows(buf["final_state"])
            left -= k

    with torch.cuda.device(dev):
        if model is None:
            run_chunks(lambda k, keep, out: venv.rollout(k, random_actions=False, keep_final=keep, out=out))
        elif fused:
            run_chunks(lambda k, keep, out: agent.rollout(k, 0.0, keep_final=keep, out=out))
        else:
            step_t = torch.full((1,), venv.step_index, dtype=torch.int64, device=dev)
            if sparse:   # the counted steps' final states, staged on the device for the host's inserts
                stage = torch.empty(max(1, min(chunk, iters)), venv.words, n, dtype=torch.int32, device=dev)
                stage_row = torch.zeros(1, dtype=torch.int64, device=dev)
            staged = 0

            def flush_stage() -> None:
                nonlocal staged
                if staged:
                    count_rows(stage[:staged])
                    stage_row.zero_()
                    staged = 0

            def policy_step(count: bool, check: bool) -> None:
                if agent is not None:
                    agent.act_q(0.0, step_t)
                else:
                    bits = unpack_states(venv.state[:, :resets], N)
                    fm = actions_to_flipmask(model(bits).to(dev), N, check=check)
                    venv.flipmask[:, :resets].copy_(fm)
                venv.step_flipmask_dev(step_t)
                step_t.add_(1)
                if count and sparse:
                    stage.index_copy_(0, stage_row, venv.final_state.unsqueeze(0))
                    stage_row.add_(1)
                elif count:
                    count_rows(venv.final_state.unsqueeze(0))

            venv.flipmask.zero_()      # padding envs (n_alloc > resets) are never intervened on
            total = burn_in + iters
            it = 0
            graphs = {}
            while it < total:
                count = it >= burn_in
                if not graph or it == 0:
                    policy_step(count, check=True)      # eager: the first step validates the actions
                else:
                    g = graphs.get(count)
                    if g is None:
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g):
                            policy_step(count, check=False)
                        graphs[count] = g
                    g.replay()
                it += 1
                if sparse and count:
                    staged += 1
                    if staged == stage.shape[0]:
                        flush_stage()
            flush_stage()
        if sparse:
            words, cnt = table.items()
            if stats is not None:
                stats.update(capacity=table.capacity, n_growths=table.n_growths, n_states=len(cnt))
            venv.close()
            return SparseSSD(words, cnt, N), None
        counts = hist.cpu().numpy().view(np.uint32)
    total = int(counts.sum(dtype=np.uint64))     # the bins are unsigned 32-bit counts
    venv.close()
    # one host pass over the 2^N bins (float64 out), not astype + divide
    ssd = np.empty(counts.shape, dtype=np.float64)
    if total > 0:
        np.divide(counts, total, out=ssd)
    else:
        ssd[:] = 0.0
    return ssd, None
