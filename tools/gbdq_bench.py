"""The GBDQ graph agent at pbn28, 32,768 envs, 5 bins (pbn_rl_amd/gbdq.py; DESIGN.md "GBDQ"), in
tools/ddqn_bench.py's manner: HIP events, alternating blocks, median (min-max), one process.

  python tools/gbdq_bench.py [--out profiles/gbdq_pbn28.json]
      front   pbn_gbdq_front (one launch) beside the ``per_env=True`` PyTorch forward of the same
              commit on the same observations; the PyTorch forward forms one row per (env, edge) and
              is run over chunks of ``--chunk`` envs (its intermediates at 32,768 envs would be
              gigabytes), the observation unpack outside the timed region for both
      trunk   the trunk and heads GEMMs on the front's output (GraphBranchingQNetwork.heads_raw)
      act     one whole BatchedGBDQ.act: front + trunk and heads + pbn_heads_to_flipmask
      frame   one whole GBDQLearner.frame(): whole-run host time ending in a device synchronise, before
              learning starts (act, step, split store) and with the PyTorch update in every frame
The result is one JSON line (and ``--out``)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from pbn_rl_amd.attractors import load_attractors  # noqa: E402
from pbn_rl_amd.gbdq import BatchedGBDQ, GBDQLearner, GraphBranchingQNetwork  # noqa: E402
from pbn_rl_amd.network import load_network  # noqa: E402
from pbn_rl_amd.spec import EnvSpec  # noqa: E402
from pbn_rl_amd.vector_env import VectorPBNEnv  # noqa: E402

BINS = 5


def event_times(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def summary(us):
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us), "n": len(us)}


def alternate(legs, reps, rounds=4):
    """Every leg warmed up, then ``reps`` event-timed calls each in ``rounds`` alternating blocks."""
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            times[k] += event_times(fn, max(1, reps // rounds))
    return {k: summary(v) for k, v in times.items()}


def spec28():
    return EnvSpec(load_network("pbn28"), load_attractors("pbn28"), perturbation=0.01)


def bench_act(args):
    env = VectorPBNEnv(spec28(), args.envs, seed=3)
    env.reset()
    torch.manual_seed(0)
    agent = BatchedGBDQ(env, GraphBranchingQNetwork(28, 29, BINS), branches=BINS)
    x = agent.observe()
    q, edges = agent.q, agent.edges

    @torch.no_grad()
    def torch_front():
        return torch.cat([q.front(x[i:i + args.chunk], edges, per_env=True) for i in range(0, x.shape[0], args.chunk)])

    front = agent.front()
    diff = float((torch_front() - front).abs().max())

    @torch.no_grad()
    def trunk():
        return q.heads_raw(front)

    res = alternate({"front hip (1 launch)": agent.front, f"front pytorch per_env (chunks of {args.chunk})": torch_front,
                     "trunk and heads (torch GEMMs)": trunk, "act (front + trunk + heads_to_flipmask)": lambda: agent.act(0.1)},
                    args.reps)
    res["front_max_abs_diff_hip_vs_pytorch"] = diff
    res["trunk_share_of_act"] = res["trunk and heads (torch GEMMs)"]["median_us"] / \
        res["act (front + trunk + heads_to_flipmask)"]["median_us"]
    return res


def run_frames(lr, frames):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        lr.frame()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / frames * 1e6


def bench_frames(args):
    env = VectorPBNEnv(spec28(), args.envs, seed=3)
    env.reset()
    torch.manual_seed(0)
    lr = GBDQLearner(env, GraphBranchingQNetwork(28, 29, BINS), capacity=max(10 ** 4, args.envs), learning_starts=0, seed=5)
    run_frames(lr, 8)
    acting = [run_frames(lr, args.frames) for _ in range(args.reps_frames)]
    while lr.frames <= lr.batch_size + 4:      # update_policy runs from frame batch_size + 1 on
        lr.frame()
    learning = [run_frames(lr, args.frames) for _ in range(args.reps_frames)]
    fmt = lambda v: {"median_us_per_frame": statistics.median(v), "min_us": min(v), "max_us": max(v), "samples_us": v}  # noqa: E731
    return {"before learning (act, step, split store)": fmt(acting), "learning (+ gbdq_update, 2 x 512 rows)": fmt(learning),
            "updates": lr.updates, "loss": float(lr.last_loss)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=32768)
    ap.add_argument("--chunk", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--reps-frames", type=int, default=5)
    ap.add_argument("--frames-per-run", dest="frames", type=int, default=20)
    ap.add_argument("--no-frames", action="store_true", help="the acting legs only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gbdq_bench needs a GPU")
    res = {"what": f"GBDQ, pbn28, GraphBranchingQNetwork(28, 29, {BINS}), {args.envs} envs",
           "device": torch.cuda.get_device_name(0)}
    res["act_hip_events"] = bench_act(args)
    if not args.no_frames:
        res["learner_frame"] = bench_frames(args)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
