"""Prioritised replay at the learner's benched shape: pbn28, 32,768 envs, a 2^20-row ring, batch 256.

  python tools/per_bench.py --launches [--out profiles/per_pbn28.json]
      HIP-event time of each new launch (pbn_per_store's two, pbn_per_sample, pbn_per_update,
      pbn_bdq_td_loss_per's row pass and sum): ``reps`` launches timed one by one between a pair of
      events, the median and the spread reported.  Run the same command under
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/per_bench.py --launches
      and pass ``--trace DIR`` to a later run to add the trace's per-kernel averages.
  python tools/per_bench.py --frames
      The learner frame under BDQLearner(fused=False) with uniform and with prioritised replay,
      eager and graph-captured: ``reps`` alternating runs of ``frames`` frames each, whole-run host
      time ending in a device sync; the median per frame with every sample.
  python tools/per_bench.py --fused
      The fused update with prioritised replay (pbn_bdq_learn_per).  The captured frame of three
      learners -- fused uniform, fused prioritised, fused=False prioritised -- in ``reps-frames``
      alternating runs; and the HIP-event time of one pbn_bdq_learn beside one pbn_bdq_learn_per
      (three launches each) on the same ring rows, in alternating blocks.  Under rocprofv3 (above),
      ``--trace DIR`` adds learn_bwd_kernel<false> and <true> and the PER launches.  With a library
      that predates pbn_bdq_learn_per (PBN_LIB) only the unweighted legs run;
      ``--fused-update-only`` leaves the frames out, ``--unweighted-only`` the weighted legs (like
      for like against such a library).

All can be given at once; the result is one JSON line (and ``--out``; ``--merge`` keeps the other
entries of an existing ``--out`` file)."""
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

from pbn_rl_amd.agent import BranchingQNetwork  # noqa: E402
from pbn_rl_amd.attractors import load_attractors  # noqa: E402
from pbn_rl_amd.network import load_network  # noqa: E402
from pbn_rl_amd import _lib  # noqa: E402
from pbn_rl_amd.replay import BDQLearner, DeviceReplay, FusedBDQUpdate, PrioritisedDeviceReplay, _TDLossPER  # noqa: E402
from pbn_rl_amd.spec import EnvSpec  # noqa: E402
from pbn_rl_amd.vector_env import VectorPBNEnv  # noqa: E402

KERNELS = {"per_store_chunks_kernel": "store_chunks", "per_store_top_kernel": "store_top",
           "per_sample_kernel": "sample", "per_update_kernel": "update", "td_loss_kernel<true>": "td_loss_per_rows",
           "learn_bwd_kernel<false>": "learn_bwd<false>", "learn_bwd_kernel<true>": "learn_bwd<true>",
           "learn_bwd_kernel(": "learn_bwd (a build before the template)", "learn_fwd_kernel": "learn_fwd",
           "learn_apply_kernel": "learn_apply"}


def event_times(fn, reps):
    """Each of ``reps`` calls between its own pair of events, in microseconds."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
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


def bench_launches(args):
    dev = torch.device("cuda")
    cap, n, B = args.capacity, args.envs, args.batch
    rp = PrioritisedDeviceReplay(cap, 1, 3, dev, alpha=0.6, beta=0.4, beta_step=1e-4, seed=1)
    pos_t = torch.tensor([cap - n // 2], dtype=torch.int64, device=dev)     # a frame that wraps
    rp.store_priorities(cap, torch.zeros(1, dtype=torch.int64, device=dev))
    rp.size = cap
    size_t = torch.tensor([cap], dtype=torch.int64, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    idx = torch.randint(0, cap, (B,), device=dev, generator=g)
    prio = torch.rand(B, device=dev, generator=g) * 4 + 1e-3
    for _ in range(64):    # varied priorities all over the ring
        rp.update_priorities(torch.randint(0, cap, (1024,), device=dev, generator=g),
                             torch.rand(1024, device=dev, generator=g) * 4 + 1e-3)
    K, A = 3, 29
    heads = torch.randn(K + 1, 2 * B, A, device=dev, generator=g)
    t_heads = torch.randn(K + 1, B, A, device=dev, generator=g)
    acts = torch.randint(0, A, (B, K), device=dev, generator=g)
    rew, msk = torch.randn(B, device=dev, generator=g), torch.ones(B, device=dev)
    w, pr = torch.rand(B, device=dev, generator=g), torch.empty(B, device=dev)
    res = {
        "store (2 launches)": summary(event_times(lambda: rp.store_priorities(n, pos_t), args.reps)),
        "sample": summary(event_times(lambda: rp.sample(B, size_t), args.reps)),
        "update": summary(event_times(lambda: rp.update_priorities(idx, prio, size_t), args.reps)),
        "td_loss_per (2 launches)": summary(event_times(
            lambda: _TDLossPER.apply(heads, t_heads, acts, rew, msk, w, 0.999, 1e-5, pr), args.reps)),
    }
    return res


def trace_averages(trace_dir):
    """Per-kernel average (us) and dispatch count from a rocprofv3 --kernel-trace csv."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {trace_dir}")
    acc = {}
    for path in files:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                for key, label in KERNELS.items():
                    if key in row["Kernel_Name"]:
                        acc.setdefault(label, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: {"avg_us": sum(v) / len(v), "median_us": statistics.median(v), "dispatches": len(v)}
            for k, v in acc.items()}


def make_learner(args, prioritised, graph, fused=False):
    spec = EnvSpec(load_network("pbn28"), load_attractors("pbn28"), perturbation=0.01)
    env = VectorPBNEnv(spec, args.envs, seed=3)
    torch.manual_seed(0)
    lr = BDQLearner(env, BranchingQNetwork((28, 28), 29, 3), capacity=args.capacity, batch_size=args.batch,
                    learning_starts=args.envs, fused=fused, graphable=graph, prioritised=prioritised, seed=5)
    env.reset()
    if graph:
        lr.capture()
    else:
        for _ in range(4):
            lr.frame()
    return lr


def run_frames(lr, frames):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        lr.frame()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / frames * 1e6


def bench_frames(args):
    out = {}
    for graph in (False, True):
        uni, per = make_learner(args, False, graph), make_learner(args, True, graph)
        run_frames(uni, 5)
        run_frames(per, 5)
        t_u, t_p = [], []
        for _ in range(args.reps_frames):          # alternating
            t_u.append(run_frames(uni, args.frames))
            t_p.append(run_frames(per, args.frames))
        out["captured" if graph else "eager"] = {
            "uniform_us_per_frame": statistics.median(t_u), "prioritised_us_per_frame": statistics.median(t_p),
            "uniform_samples_us": t_u, "prioritised_samples_us": t_p,
            "added_us_per_frame": statistics.median(t_p) - statistics.median(t_u)}
    return out


def bench_fused(args):
    """The captured frames and the two fused entries, legs alternated (see the module docstring)."""
    dev = torch.device("cuda")
    has_per = hasattr(_lib.load(), "pbn_bdq_learn_per") and not args.unweighted_only
    out = {"library": os.environ.get("PBN_LIB", "in-tree")}
    # one update: the same nets, ring rows and batch through both entries, in alternating blocks
    spec = EnvSpec(load_network("pbn28"), load_attractors("pbn28"), perturbation=0.01)
    env = VectorPBNEnv(spec, 64, seed=3)
    cap, B, K = args.capacity, args.batch, 3
    g = torch.Generator(device=dev).manual_seed(0)
    R = DeviceReplay(cap, spec.words, K, dev)
    R.state.copy_(torch.randint(0, 1 << 28, (spec.words, cap), device=dev, generator=g, dtype=torch.int32))
    R.next_state.copy_(torch.randint(0, 1 << 28, (spec.words, cap), device=dev, generator=g, dtype=torch.int32))
    R.target.copy_(torch.randint(0, len(spec.attractors), (cap,), device=dev, generator=g).to(torch.uint8))
    R.action.copy_(torch.randint(0, 29, (cap, K), device=dev, generator=g, dtype=torch.int32))
    R.reward.copy_(torch.randn(cap, device=dev, generator=g))
    R.done.copy_(torch.randint(0, 2, (cap,), device=dev, generator=g).to(torch.uint8))
    R.size = cap
    idx = torch.randint(0, cap, (B,), device=dev, generator=g)
    w, pr = torch.rand(B, device=dev, generator=g) + 0.05, torch.empty(B, device=dev)
    torch.manual_seed(0)
    legs = {}
    for name in ("pbn_bdq_learn",) + (("pbn_bdq_learn_per",) if has_per else ()):
        q, t = BranchingQNetwork((28, 28), 29, K).to(dev), BranchingQNetwork((28, 28), 29, K).to(dev)
        fu = FusedBDQUpdate(q, t, env.net, K, batch_size=B)
        legs[name] = ((lambda fu=fu: fu.update(R, idx)) if name == "pbn_bdq_learn" else
                      (lambda fu=fu: fu.update(R, idx, weights=w, priorities_out=pr)))
    times = {k: [] for k in legs}
    rounds = 8
    for _ in range(rounds):
        for k, fn in legs.items():
            times[k] += event_times(fn, max(1, args.reps // rounds))
    out["hip_events (3 launches)"] = {k: summary(v) for k, v in times.items()}
    if args.fused_update_only:
        return out
    # the captured frames
    make = {"fused uniform": lambda: make_learner(args, False, True, fused=True),
            "fused=False prioritised": lambda: make_learner(args, True, True, fused=False)}
    if has_per:
        make["fused prioritised"] = lambda: make_learner(args, True, True, fused=True)
    lrs = {k: f() for k, f in make.items()}
    for lr in lrs.values():
        run_frames(lr, 5)
    samples = {k: [] for k in lrs}
    for _ in range(args.reps_frames):              # alternating
        for k, lr in lrs.items():
            samples[k].append(run_frames(lr, args.frames))
    fr = {k: {"median_us_per_frame": statistics.median(v), "min_us": min(v), "max_us": max(v), "samples_us": v}
          for k, v in samples.items()}
    if has_per:
        fr["fused prioritised - fused uniform (us)"] = (fr["fused prioritised"]["median_us_per_frame"]
                                                        - fr["fused uniform"]["median_us_per_frame"])
    out["captured_frame"] = fr
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--frames-bench", "--frames", dest="frames_bench", action="store_true")
    ap.add_argument("--fused", action="store_true", help="the fused update with prioritised replay")
    ap.add_argument("--fused-update-only", action="store_true", help="--fused without the captured frames")
    ap.add_argument("--unweighted-only", action="store_true",
                    help="--fused without the pbn_bdq_learn_per legs (what a library without the entry runs: "
                         "like for like against such a build)")
    ap.add_argument("--merge", action="store_true", help="keep the other entries of an existing --out file")
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace run of --launches")
    ap.add_argument("--envs", type=int, default=32768)
    ap.add_argument("--capacity", type=int, default=1 << 20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--reps-frames", type=int, default=5)
    ap.add_argument("--frames-per-run", dest="frames", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"what": f"prioritised replay, pbn28, {args.envs} envs, capacity {args.capacity}, batch {args.batch}"}
    if args.trace:
        res["kernel_trace"] = trace_averages(args.trace)
    if args.launches or args.frames_bench or args.fused or args.fused_update_only:
        if not torch.cuda.is_available():
            raise SystemExit("per_bench needs a GPU")
        res["device"] = torch.cuda.get_device_name(0)
    if args.launches:
        res["hip_events"] = bench_launches(args)
    if args.frames_bench:
        res["learner_frame"] = bench_frames(args)
    args.fused = args.fused or args.fused_update_only
    if args.fused:
        res["fused_update"] = bench_fused(args)
        if args.trace:      # (a trace of a --fused run: its kernels belong with the fused entries)
            res["fused_update"]["kernel_trace"] = res.pop("kernel_trace")
    if args.out and args.merge and os.path.exists(args.out):
        with open(args.out) as f:
            old = json.loads(f.read())
        old.update({k: v for k, v in res.items() if k not in ("what", "device") or k not in old})
        res = old
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
