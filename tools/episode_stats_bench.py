"""What ``episode_stats=True`` costs the captured DDQN-PER frame at train_ddqn.py's shape: pbn28,
32,768 envs, DQN(28, 29, [(50, 50)]), batch 64.

  python tools/episode_stats_bench.py [--out profiles/episode_stats_pbn28.json]
      Three captured learners in one process -- stats off, stats on with log_every 0, stats on with
      log_every 100 -- timed in alternating blocks: ``--reps-frames`` runs of ``--frames-per-run``
      frames each, whole-run host time ending in a device synchronise, once with one replay per
      frame() and once through run(k).  The median with min-max per variant, and each stats variant's
      difference to stats off (median to median).
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/episode_stats_bench.py --captured-frames 200
      then ``--trace DIR`` on a later run adds the two kernels' own times from the trace.

The result is one JSON line (and ``--out``)."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from pbn_rl_amd.attractors import load_attractors  # noqa: E402
from pbn_rl_amd.ddqn import DQN, DDQNLearner  # noqa: E402
from pbn_rl_amd.network import load_network  # noqa: E402
from pbn_rl_amd.spec import EnvSpec  # noqa: E402
from pbn_rl_amd.vector_env import VectorPBNEnv  # noqa: E402

KERNELS = ["episode_track_kernel", "episode_series_kernel"]
ARCH = [(50, 50)]
VARIANTS = {"stats off": None, "stats on, log_every 0": 0, "stats on, log_every 100": 100}


def learner(args, log_every):
    spec = EnvSpec(load_network("pbn28"), load_attractors("pbn28"), perturbation=0.01)
    env = VectorPBNEnv(spec, args.envs, seed=3)
    torch.manual_seed(0)
    lr = DDQNLearner(env, DQN(28, 29, ARCH), total_frames=10 ** 6, capacity=args.capacity, batch_size=args.batch,
                     prioritised=True, fused=True, seed=5, graphable=True, episode_stats=log_every is not None,
                     stats_log_every=log_every or 0)
    env.reset()
    if lr.stats is not None:
        lr.stats.begin()
    lr.capture()
    return lr


def run_frames(lr, frames, run_k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if run_k:
        lr.run(frames)
    else:
        for _ in range(frames):
            lr.frame()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / frames * 1e6


def bench(args):
    lrs = {name: learner(args, log_every) for name, log_every in VARIANTS.items()}
    out = {}
    for mode, run_k in (("captured, one replay per frame()", False), ("captured, run(k)", True)):
        for lr in lrs.values():
            run_frames(lr, 8, run_k)
        samples = {k: [] for k in lrs}
        for _ in range(args.reps_frames):              # alternating blocks
            for k, lr in lrs.items():
                samples[k].append(run_frames(lr, args.frames, run_k))
        res = {k: {"median_us_per_frame": statistics.median(v), "min_us": min(v), "max_us": max(v), "samples_us": v}
               for k, v in samples.items()}
        off = res["stats off"]["median_us_per_frame"]
        for k in res:
            if k != "stats off":
                res[k]["minus_stats_off_us"] = res[k]["median_us_per_frame"] - off
        out[mode] = res
    on = lrs["stats on, log_every 100"].stats
    out["stats_after"] = {k: v for k, v in on.totals().items()}
    out["series_windows"] = len(on.series()["windows"])
    return out


def trace_times(trace_dir):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {trace_dir}")
    acc = {}
    for path in files:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                for key in KERNELS:
                    if key in row["Kernel_Name"]:
                        acc.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: {"avg_us": sum(v) / len(v), "median_us": statistics.median(v), "min_us": min(v), "max_us": max(v),
                "dispatches": len(v)} for k, v in acc.items()}


def captured_frames_only(args):
    """The process to put under rocprofv3 --kernel-trace: the log_every 100 learner, captured, then
    ``--captured-frames`` replays through run(k), and nothing else."""
    lr = learner(args, 100)
    lr.run(args.captured_frames)
    torch.cuda.synchronize()
    print(json.dumps({"captured_frames": args.captured_frames, "frames": lr.frames,
                      "episodes": lr.stats.totals()["episodes"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captured-frames", type=int, default=0,
                    help="only capture the frame with stats on and replay it this many times (for rocprofv3)")
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace run of --captured-frames")
    ap.add_argument("--envs", type=int, default=32768)
    ap.add_argument("--capacity", type=int, default=1 << 20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps-frames", type=int, default=7)
    ap.add_argument("--frames-per-run", dest="frames", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("episode_stats_bench needs a GPU")
    if args.captured_frames:
        return captured_frames_only(args)
    res = {"what": f"captured DDQN-PER frame with and without episode statistics, pbn28, DQN(28, 29, {ARCH}), "
                   f"{args.envs} envs, capacity {args.capacity}, batch {args.batch}; {args.reps_frames} alternating "
                   f"runs of {args.frames} frames per variant", "device": torch.cuda.get_device_name(0)}
    if args.trace:
        res["kernel_trace"] = trace_times(args.trace)
    res["frame"] = bench(args)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
