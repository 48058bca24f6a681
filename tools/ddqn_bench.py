"""The DDQN / DDQNPER agent at train_ddqn.py's shape: pbn28, 32,768 envs, DQN(28, 29, [(50, 50)]),
batch 64, a 2^20-row ring.  The HIP path of pbn_rl_amd/ddqn.py beside the PyTorch path of the same
commit (``fused=False``: acting through DQN.forward on pbn_obs_unpack's observation and
pbn_q_to_flipmask, the update through ddqn_update + torch.optim.Adam).

  python tools/ddqn_bench.py [--out profiles/ddqn_pbn28.json]
      act     HIP-event time of one acting call (BatchedDDQN.act_q), both paths
      update  HIP-event time of one update on the same ring rows: FusedDDQNUpdate.update (4 launches)
              beside gather + ddqn_update, each unweighted and with importance weights
      frame   one whole DDQNLearner.frame(), prioritised and uniform, both paths: alternating runs of
              ``--frames-per-run`` frames, whole-run host time ending in a device synchronise; and the
              prioritised HIP frame captured in one hipGraph (DDQNLearner.capture), timed the same
              way: "captured" replays once per frame(), "captured run" is one run(k) per run
    ``reps`` calls are timed one by one between a pair of events after a warm-up, the legs in
    alternating blocks; the median and the spread are reported.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/ddqn_bench.py --no-frames
      then ``--trace DIR`` on a later run adds the trace's per-kernel times of the new kernels.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR2 -o run -- python tools/ddqn_bench.py --captured-frames 200
      then ``--frame-trace DIR2`` adds the captured frame's launch list with each kernel's median
      time and their sum over one frame.

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
from pbn_rl_amd.ddqn import DQN, BatchedDDQN, DDQNLearner, FusedDDQNUpdate, ddqn_update  # noqa: E402
from pbn_rl_amd.network import load_network  # noqa: E402
from pbn_rl_amd.replay import DeviceReplay  # noqa: E402
from pbn_rl_amd.spec import EnvSpec  # noqa: E402
from pbn_rl_amd.vector_env import VectorPBNEnv  # noqa: E402

KERNELS = ["dqn_act_kernel", "ddqn_fb_kernel", "ddqn_grad_kernel", "ddqn_adam_kernel", "dqn_pack_kernel"]
ARCH = [(50, 50)]


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


def alternate(legs, reps, rounds=8):
    """Every leg warmed up, then ``reps`` event-timed calls each in ``rounds`` alternating blocks."""
    for fn in legs.values():
        for _ in range(5):
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
    spec = spec28()
    torch.manual_seed(0)
    q = DQN(28, 29, ARCH).cuda()
    legs = {}
    for name, kernel in (("hip (1 launch)", True), ("pytorch", False)):
        env = VectorPBNEnv(spec, args.envs, seed=3)
        env.reset()
        agent = BatchedDDQN(env, q, kernel=kernel)
        legs[name] = lambda agent=agent: agent.act_q(0.1)
    return alternate(legs, args.reps)


def filled_ring(spec, cap, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    R = DeviceReplay(cap, spec.words, 1, dev)
    R.state.copy_(torch.randint(0, 1 << 28, (spec.words, cap), device=dev, generator=g, dtype=torch.int32))
    R.next_state.copy_(torch.randint(0, 1 << 28, (spec.words, cap), device=dev, generator=g, dtype=torch.int32))
    R.target.copy_(torch.randint(0, len(spec.attractors), (cap,), device=dev, generator=g).to(torch.uint8))
    R.action.copy_(torch.randint(0, 29, (cap, 1), device=dev, generator=g, dtype=torch.int32))
    R.reward.copy_(torch.randn(cap, device=dev, generator=g))
    R.done.copy_(torch.randint(0, 2, (cap,), device=dev, generator=g).to(torch.uint8))
    R.size = cap
    return R, g


def bench_update(args):
    dev = torch.device("cuda")
    spec = spec28()
    env = VectorPBNEnv(spec, 64, seed=3)
    B = args.batch
    R, g = filled_ring(spec, args.capacity, dev)
    idx = torch.randint(0, args.capacity, (B,), device=dev, generator=g)
    w, pr = torch.rand(B, device=dev, generator=g) + 0.05, torch.empty(B, device=dev)
    torch.manual_seed(0)
    legs = {}
    for weighted in (False, True):
        q, t = DQN(28, 29, ARCH).to(dev), DQN(28, 29, ARCH).to(dev)
        fu = FusedDDQNUpdate(q, t, env.net, batch_size=B)
        kw = dict(weights=w, priorities_out=pr) if weighted else {}
        legs["hip (4 launches)" + (" weighted" if weighted else "")] = lambda fu=fu, kw=kw: fu.update(R, idx, **kw)
        q2, t2 = DQN(28, 29, ARCH).to(dev), DQN(28, 29, ARCH).to(dev)
        opt = torch.optim.Adam(q2.parameters(), lr=1e-4)

        def torch_update(q2=q2, t2=t2, opt=opt, kw=kw):
            b = R.gather(idx, env.net)
            x = b["x"]
            batch = {"state": x[0, :B], "target": x[1, :B], "next_state": x[0, B:], "action": b["actions"].view(B, 1),
                     "reward": b["rewards"], "done": b["masks"]}
            ddqn_update(q2, t2, opt, batch, 0.95, 10.0, **kw)
        legs["pytorch" + (" weighted" if weighted else "")] = torch_update
    return alternate(legs, args.reps)


def run_frames(lr, frames, run_k=False):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if run_k:
        lr.run(frames)
    else:
        for _ in range(frames):
            lr.frame()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / frames * 1e6


CAPTURED, CAPTURED_RUN = "prioritised hip captured", "prioritised hip captured run"


def bench_frames(args):
    lrs = {}

    def learner(prioritised, fused, **kw):
        env = VectorPBNEnv(spec28(), args.envs, seed=3)
        torch.manual_seed(0)
        lr = DDQNLearner(env, DQN(28, 29, ARCH), total_frames=10 ** 6, capacity=args.capacity,
                         batch_size=args.batch, prioritised=prioritised, fused=fused, seed=5, **kw)
        env.reset()
        return lr

    for prioritised in (True, False):
        for fused in (True, False):
            lr = learner(prioritised, fused)
            run_frames(lr, 8)
            lrs[("prioritised" if prioritised else "uniform") + (" hip" if fused else " pytorch")] = lr
    # the same frame captured in one hipGraph: one replay per frame(), and run(k)'s back-to-back replays
    for name in (CAPTURED, CAPTURED_RUN):
        lr = learner(True, True, graphable=True)
        lr.capture()
        run_frames(lr, 8, run_k=name == CAPTURED_RUN)
        lrs[name] = lr
    samples = {k: [] for k in lrs}
    for _ in range(args.reps_frames):              # alternating
        for k, lr in lrs.items():
            samples[k].append(run_frames(lr, args.frames, run_k=k == CAPTURED_RUN))
    out = {k: {"median_us_per_frame": statistics.median(v), "min_us": min(v), "max_us": max(v), "samples_us": v}
           for k, v in samples.items()}
    eager = out["prioritised hip"]["median_us_per_frame"]
    for name in (CAPTURED, CAPTURED_RUN):
        out[name]["ratio_to_prioritised_hip"] = out[name]["median_us_per_frame"] / eager
    return out


def trace_averages(trace_dir):
    """Per-kernel average and median (us) and dispatch count from a rocprofv3 --kernel-trace csv."""
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
    return {k: {"avg_us": sum(v) / len(v), "median_us": statistics.median(v), "dispatches": len(v)}
            for k, v in acc.items()}


def captured_frames_only(args):
    """The process to put under rocprofv3 --kernel-trace for the captured frame: capture, then
    ``--captured-frames`` replays through run(k), and nothing else."""
    env = VectorPBNEnv(spec28(), args.envs, seed=3)
    torch.manual_seed(0)
    lr = DDQNLearner(env, DQN(28, 29, ARCH), total_frames=10 ** 6, capacity=args.capacity, batch_size=args.batch,
                     prioritised=True, fused=True, seed=5, graphable=True)
    env.reset()
    lr.capture()
    lr.run(args.captured_frames)
    torch.cuda.synchronize()
    print(json.dumps({"captured_frames": args.captured_frames, "frames": lr.frames, "updates": lr.updates}), flush=True)


def frame_trace(trace_dir, frames):
    """The captured frame's kernels from the kernel-trace csv of a ``--captured-frames frames`` run:
    every kernel dispatched at least once per replayed frame (the few eager frames before the
    capture and the set-up dispatch the rest), its dispatches per frame, its median time, and the sum
    over one frame."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {trace_dir}")
    acc = {}
    for path in files:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].strip()
                acc.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    kernels = {k: {"per_frame": len(v) // frames, "median_us": statistics.median(v), "dispatches": len(v)}
               for k, v in acc.items() if len(v) >= frames}
    return {"frames": frames, "kernels": kernels,
            "launches_per_frame": sum(k["per_frame"] for k in kernels.values()),
            "sum_us_per_frame": sum(k["per_frame"] * k["median_us"] for k in kernels.values())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captured-frames", type=int, default=0,
                    help="only capture the prioritised frame and replay it this many times (for rocprofv3)")
    ap.add_argument("--frame-trace", default=None,
                    help="directory of a rocprofv3 --kernel-trace run of --captured-frames (with --frame-trace-frames)")
    ap.add_argument("--frame-trace-frames", type=int, default=200)
    ap.add_argument("--no-frames", action="store_true", help="the acting and update legs only")
    ap.add_argument("--trace", default=None, help="directory of a rocprofv3 --kernel-trace run")
    ap.add_argument("--envs", type=int, default=32768)
    ap.add_argument("--capacity", type=int, default=1 << 20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--reps-frames", type=int, default=5)
    ap.add_argument("--frames-per-run", dest="frames", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ddqn_bench needs a GPU")
    if args.captured_frames:
        return captured_frames_only(args)
    res = {"what": f"DDQN / DDQNPER, pbn28, DQN(28, 29, {ARCH}), {args.envs} envs, capacity {args.capacity}, "
                   f"batch {args.batch}", "device": torch.cuda.get_device_name(0)}
    if args.trace:
        res["kernel_trace"] = trace_averages(args.trace)
    if args.frame_trace:
        res["captured_frame_kernel_trace"] = frame_trace(args.frame_trace, args.frame_trace_frames)
    res["act_hip_events"] = bench_act(args)
    res["update_hip_events"] = bench_update(args)
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
