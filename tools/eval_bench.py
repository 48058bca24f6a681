"""Time one control evaluation two ways on one GPU (model_tester.py:587-658, batched).

    python tools/eval_bench.py [--network pbn28] [--runs 256] [--reps 5] [--out profiles/eval_pbn28_256.json]

Shape: Bittner-28, its 14 bundled attractors (196 ordered pairs), 256 runs per pair = 50,176 envs,
p = 0.01, a seeded random-init BranchingQNetwork, under the settle law (settle = 64) and the
one-update law.  An untrained agent reaches few targets, so both loops run close to all 100 steps.

  parent_loop   the loop a user assembles from VectorPBNEnv alone: module forward on the unpacked
                states, actions_to_flipmask, step_flipmask, count / done kept with torch ops, and
                bool(done.all()) after every step (one host synchronisation per step)
  evaluate      pbn_rl_amd.evaluate.evaluate_control(graph=True): fused acting launch, pbn_step_dev,
                pbn_eval_track and the step counter as one replayed hipGraph, the open runs read
                every 8 steps, pbn_eval_reduce at the end

Each time is a host clock around the whole call, which ends in a device synchronisation (both
include building the envs and copying the counts back); after one warm-up of each the two are run
alternately ``reps`` times and the median is reported with every sample.  ``per_step`` counts what
one protocol step issues: for the parent loop the aten operators torch dispatches (views left
out; each is at least one kernel launch) plus the library's launch, for the new loop the launches
captured in its graph.  Prints one JSON line.
"""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pbn_rl_amd.agent import BranchingQNetwork  # noqa: E402
from pbn_rl_amd.attractors import load_attractors  # noqa: E402
from pbn_rl_amd.evaluate import evaluate_control  # noqa: E402
from pbn_rl_amd.network import load_network  # noqa: E402
from pbn_rl_amd.spec import EnvSpec  # noqa: E402
from pbn_rl_amd.vector_env import VectorPBNEnv, actions_to_flipmask, pack_states, unpack_states  # noqa: E402

VIEW_OPS = ("view", "reshape", "t.", "transpose", "slice", "select", "unsqueeze", "squeeze", "expand", "alias",
            "detach", "as_strided", "permute", "unbind", "_unsafe_view")


class OpCounter(TorchDispatchMode):
    """Counts the aten operators dispatched while active, view-like ones (no launch) left out."""

    def __init__(self):
        super().__init__()
        self.ops = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func).replace("aten.", "")
        if not name.startswith(VIEW_OPS):
            self.ops += 1
        return func(*args, **(kwargs or {}))


def parent_loop(spec, q, runs, seed, max_steps=100, count_ops_at=None):
    """The evaluation assembled from the API without pbn_rl_amd.evaluate.  Returns (counts,
    steps run, aten operators of step ``count_ops_at`` or None)."""
    atts = spec.attractors
    A, N = len(atts), spec.n
    pairs = list(itertools.product(range(A), repeat=2))
    n = len(pairs) * runs
    dev = torch.device("cuda", torch.cuda.current_device())
    env = VectorPBNEnv(spec, n, seed=seed, device=dev, autoreset=False, keep_final_state=False)
    env.reset()
    first = np.array([a[0] for a in atts], dtype=np.int64)
    src = np.repeat([a for a, _ in pairs], runs)
    tgt = np.repeat([t for _, t in pairs], runs)
    env.set_state(pack_states(torch.from_numpy(first[src]).to(dev), N),
                  target=torch.from_numpy(tgt.astype(np.uint8)).to(dev),
                  t=torch.zeros(n, dtype=torch.uint8, device=dev))
    tgt_bits = torch.from_numpy(first[tgt].astype(np.float32)).to(dev)
    count = torch.full((n,), max_steps + 1, dtype=torch.int64, device=dev)
    done = torch.from_numpy(src == tgt).to(dev)
    count[done] = 0
    ops, k = None, 0
    with torch.no_grad():
        for k in range(1, max_steps + 1):
            counter = OpCounter() if k == count_ops_at else None
            if counter is not None:
                counter.__enter__()
            s = unpack_states(env.state[:, :n], N).to(torch.float32)
            acts = q(torch.stack([s, tgt_bits])).argmax(dim=2)
            _, _, flags = env.step_flipmask(actions_to_flipmask(acts, N, check=False))
            hit = (flags & 1).bool() & ~done
            count[hit] = k
            done |= hit
            stop = bool(done.all())
            if counter is not None:
                counter.__exit__(None, None, None)
                ops = counter.ops
            if stop:
                break
    torch.cuda.synchronize()
    out = count.view(len(pairs), runs).cpu().numpy()
    env.close()
    return out, k, ops


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def bench_law(net, atts, settle, args):
    spec = EnvSpec(net, atts, perturbation=args.perturbation, horizon=0, settle=settle)
    torch.manual_seed(args.seed)
    q = BranchingQNetwork((net.n, net.n), net.n + 1, 3).eval()
    q_dev = BranchingQNetwork((net.n, net.n), net.n + 1, 3)
    q_dev.load_state_dict(q.state_dict())
    q_dev = q_dev.to("cuda").eval()
    old = lambda ops_at=None: parent_loop(spec, q_dev, args.runs, args.seed, count_ops_at=ops_at)  # noqa: E731
    new = lambda: evaluate_control(spec, q, runs=args.runs, seed=args.seed, graph=True)  # noqa: E731
    _, (counts_old, steps_old, ops) = timed(lambda: old(2))          # warm-up of both (code objects, allocator)
    _, ev = timed(new)
    t_old, t_new = [], []
    for _ in range(args.reps):                                       # alternating, same seeded inputs
        t_old.append(timed(old)[0])
        t_new.append(timed(new)[0])
    n = counts_old.size
    return {"settle": settle,
            "parent_loop_s": statistics.median(t_old), "evaluate_s": statistics.median(t_new),
            "parent_loop_samples_s": t_old, "evaluate_samples_s": t_new,
            "speedup": statistics.median(t_old) / statistics.median(t_new),
            "steps_run_parent_loop": steps_old,
            "per_step": {"parent_loop": {"aten_ops": ops, "library_launches": 1, "host_syncs": 1},
                         # act_q, pbn_step_dev, the state copy-back, pbn_eval_track, the step counter's add
                         "evaluate": {"graph_replays": 1, "kernels_in_graph": 5, "host_syncs": 1 / 8}},
            # the two loops act with different kernels (module vs the fused network, equal to 1e-5 on
            # the heads), so a random-init network's near-ties may split single runs
            "runs_with_equal_count": int((counts_old == ev.counts).sum()), "runs": int(n),
            "failed_parent_loop": int((counts_old == 101).sum()), "failed_evaluate": ev.failed,
            "mean_length_evaluate": ev.mean_length()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--network", default="pbn28")
    ap.add_argument("--runs", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--perturbation", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs a GPU: there is no CPU timing of this loop")
    net = load_network(args.network)
    atts = load_attractors(args.network)
    res = {"what": f"control evaluation, {args.network}, {len(atts)} attractors, {len(atts) ** 2} pairs x {args.runs} "
                   f"runs = {len(atts) ** 2 * args.runs} envs, p={args.perturbation}, random-init BDQ (seed {args.seed}), "
                   f"max 100 steps; whole-call host time ending in a device sync, median of {args.reps} alternating runs",
           "device": torch.cuda.get_device_name(0),
           "laws": [bench_law(net, atts, settle, args) for settle in (64, 0)]}
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
