"""What ``curriculum=True`` costs the captured DDQN-PER frame at train_ddqn.py's shape: pbn28,
32,768 envs, DQN(28, 29, [(50, 50)]), batch 64.  The yardstick is the stats-on frame of the same
process (tools/episode_stats_bench.py measures that one against stats off).

  python tools/curriculum_bench.py [--out profiles/curriculum_pbn28.json]
      Three captured learners in one process -- stats on, stats + curriculum with refresh_every 1000,
      stats + curriculum with refresh_every 1 -- timed in alternating blocks: ``--reps-frames`` runs of
      ``--frames-per-run`` frames each, whole-run host time ending in a device synchronise, once with
      one replay per frame() and once through run(k).  The median with min-max per variant, and each
      curriculum variant's difference to stats on (median to median).
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/curriculum_bench.py --captured-frames 200 --refresh 1
      then ``--trace DIR`` on a later run adds the two kernels' own times from the trace.
  python tools/curriculum_bench.py --off-frames 300 [--root OTHER_TREE]
      One process, curriculum off (the learner's defaults): one run(k) of that many replays after
      capture, µs per frame.  Run alternately on two trees to compare builds.

The result is one JSON line (and ``--out``)."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

KERNELS = ["curriculum_redraw_kernel", "curriculum_refresh_kernel", "episode_track_kernel", "episode_series_kernel"]
ARCH = [(50, 50)]
# name -> (curriculum, refresh_every)
VARIANTS = {"stats on": (False, 0), "stats + curriculum, refresh 1000": (True, 1000),
            "stats + curriculum, refresh 1": (True, 1)}
BASE = "stats on"


def learner(args, stats, curriculum, refresh):
    import torch

    from pbn_rl_amd.attractors import load_attractors
    from pbn_rl_amd.ddqn import DQN, DDQNLearner
    from pbn_rl_amd.network import load_network
    from pbn_rl_amd.spec import EnvSpec
    from pbn_rl_amd.vector_env import VectorPBNEnv
    spec = EnvSpec(load_network("pbn28"), load_attractors("pbn28"), perturbation=0.01)
    env = VectorPBNEnv(spec, args.envs, seed=3)
    torch.manual_seed(0)
    extra = {"episode_stats": True, "stats_log_every": 100} if stats else {}
    if curriculum:       # (absent otherwise: an older tree's learner does not know the arguments)
        extra.update(curriculum=True, curriculum_refresh=refresh)
    lr = DDQNLearner(env, DQN(28, 29, ARCH), total_frames=10 ** 6, capacity=args.capacity, batch_size=args.batch,
                     prioritised=True, fused=True, seed=5, graphable=True, **extra)
    env.reset()
    if lr.stats is not None:
        lr.stats.begin()
    lr.capture()
    return lr


def run_frames(lr, frames, run_k):
    import torch
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
    lrs = {name: learner(args, True, c, r) for name, (c, r) in VARIANTS.items()}
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
        base = res[BASE]["median_us_per_frame"]
        for k in res:
            if k != BASE:
                res[k]["minus_stats_on_us"] = res[k]["median_us_per_frame"] - base
        out[mode] = res
    after = {}
    for k, lr in lrs.items():
        t = lr.stats.totals()
        after[k] = {"frames": t["frames"], "episodes": t["episodes"], "ep_len_mean": t["ep_len_mean"],
                    "success_rate": t["success_rate"],
                    "resets_per_frame": t["episodes"] / max(t["frames"], 1),
                    "refreshes": lr.curriculum.table()["refreshes"] if lr.curriculum is not None else None}
    out["after"] = after
    w = lrs["stats + curriculum, refresh 1"].curriculum.weights()
    out["weights_refresh_1"] = {"max": float(w.max()), "min_off_diagonal": float(w[w > 0].min()),
                                "uniform": 1.0 / (w.shape[0] * (w.shape[0] - 1))}
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
    """The process to put under rocprofv3 --kernel-trace: the curriculum learner with ``--refresh``,
    captured, then ``--captured-frames`` replays through run(k), and nothing else."""
    import torch
    lr = learner(args, True, True, args.refresh)
    lr.run(args.captured_frames)
    torch.cuda.synchronize()
    print(json.dumps({"captured_frames": args.captured_frames, "frames": lr.frames, "refresh_every": args.refresh,
                      "episodes": lr.stats.totals()["episodes"], "refreshes": lr.curriculum.table()["refreshes"]}),
          flush=True)


def off_frames_only(args):
    import torch
    lr = learner(args, False, False, 0)
    run_frames(lr, 8, True)
    us = run_frames(lr, args.off_frames, True)
    print(json.dumps({"root": os.path.abspath(args.root), "off_frames": args.off_frames, "us_per_frame": us,
                      "device": torch.cuda.get_device_name(0)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captured-frames", type=int, default=0,
                    help="only capture the frame with the curriculum on and replay it this many times (for rocprofv3)")
    ap.add_argument("--refresh", type=int, default=1, help="refresh_every of --captured-frames")
    ap.add_argument("--off-frames", type=int, default=0,
                    help="only capture the frame with curriculum and statistics off and time this many replays")
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."),
                    help="the tree whose pbn_rl_amd is measured (default: this one)")
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace run of --captured-frames")
    ap.add_argument("--envs", type=int, default=32768)
    ap.add_argument("--capacity", type=int, default=1 << 20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps-frames", type=int, default=7)
    ap.add_argument("--frames-per-run", dest="frames", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("curriculum_bench needs a GPU")
    if args.captured_frames:
        return captured_frames_only(args)
    if args.off_frames:
        return off_frames_only(args)
    res = {"what": f"captured DDQN-PER frame with episode statistics, with and without the curriculum, pbn28, "
                   f"DQN(28, 29, {ARCH}), {args.envs} envs, capacity {args.capacity}, batch {args.batch}; "
                   f"{args.reps_frames} alternating runs of {args.frames} frames per variant",
           "device": torch.cuda.get_device_name(0)}
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
