"""The ControlGBDQ agent at pbn28 with 8 control nodes and pbn7 with 3, 32,768 envs
(pbn_rl_amd/cgbdq.py; DESIGN.md "ControlGBDQ"), in tools/gbdq_bench.py's manner: HIP events, warmed,
4 alternating blocks of 10 calls, median (min-max), one process.

  python tools/cgbdq_bench.py [--out profiles/cgbdq_pbn28.json]
      tail hip      pbn_cgbdq_flipmask on the front's output (one launch: the tail, the combination,
                    the argmax, epsilon-greedy, the flip mask)
      tail pytorch  the same from this commit's PyTorch pieces: heads_raw, the stated combination,
                    argmax, control_to_flipmask
      front         pbn_gbdq_front
      act           one whole BatchedControlGBDQ.act (front + the fused tail)
      frame         one whole ControlGBDQLearner.frame(): whole-run host time ending in a device
                    synchronise, before learning starts (act, step, store) and with the PyTorch
                    update in every frame
The tail is 2 (256 N N + 2 256^2 + 256 (1 + 2 C)) FLOP per env; the kernel's share of the fp32 matrix
peak (157.3 TFLOP/s) is reported.  The result is one JSON line (and ``--out``)."""
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
from pbn_rl_amd.cgbdq import (BatchedControlGBDQ, ControlGBDQLearner, ControlGraphBranchingQNetwork,  # noqa: E402
                              combine_heads, stacked_heads)
from pbn_rl_amd.network import load_network  # noqa: E402
from pbn_rl_amd.spec import EnvSpec  # noqa: E402
from pbn_rl_amd.vector_env import VectorPBNEnv, control_to_flipmask  # noqa: E402
from tools.gbdq_bench import alternate  # noqa: E402

FP32_MATRIX_PEAK = 157.3e12
SHAPES = {"pbn28": [2, 5, 9, 13, 17, 20, 23, 27], "pbn7": [1, 3, 5]}


def spec_of(name):
    return EnvSpec(load_network(name), load_attractors(name), perturbation=0.01)


def bench_act(name, ctrl, args):
    spec = spec_of(name)
    N, C = spec.n, len(ctrl)
    env = VectorPBNEnv(spec, args.envs, seed=3)
    env.reset()
    torch.manual_seed(0)
    agent = BatchedControlGBDQ(env, ControlGraphBranchingQNetwork(N, 2, C), ctrl, "uniform")
    front = agent.front()
    q = agent.q

    @torch.no_grad()
    def torch_tail():
        acts = torch.argmax(combine_heads(stacked_heads(q.heads_raw(front))), dim=2)
        return control_to_flipmask(env.state, acts, ctrl, N)

    def hip_tail():
        agent_front = agent.front
        agent.front = lambda: front        # the tail alone: the front's output is already there
        try:
            agent.act(0.0)
        finally:
            agent.front = agent_front

    hip_tail()
    same = bool(torch.equal(env.flipmask, torch_tail()))
    res = alternate({"tail hip (1 launch)": hip_tail, "tail pytorch (heads_raw, combination, argmax, control_to_flipmask)": torch_tail,
                     "front hip (1 launch)": agent.front, "act (front + fused tail)": lambda: agent.act(0.1)}, args.reps)
    flop = 2.0 * (256 * N * N + 2 * 256 * 256 + 256 * (1 + 2 * C)) * env.n_alloc
    t = res["tail hip (1 launch)"]["median_us"] * 1e-6
    res["tail_flop"] = flop
    res["tail_hip_tflops"] = flop / t / 1e12
    res["tail_hip_share_of_fp32_matrix_peak"] = flop / t / FP32_MATRIX_PEAK
    res["tail_speedup_hip_vs_pytorch"] = res["tail pytorch (heads_raw, combination, argmax, control_to_flipmask)"]["median_us"] / \
        res["tail hip (1 launch)"]["median_us"]
    res["front_share_of_act"] = res["front hip (1 launch)"]["median_us"] / res["act (front + fused tail)"]["median_us"]
    res["greedy_masks_equal_hip_vs_pytorch"] = same
    env.close()
    return res


def run_frames(lr, frames):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        lr.frame()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / frames * 1e6


def bench_frames(name, ctrl, args):
    spec = spec_of(name)
    env = VectorPBNEnv(spec, args.envs, seed=3)
    env.reset()
    torch.manual_seed(0)
    lr = ControlGBDQLearner(env, ControlGraphBranchingQNetwork(spec.n, 2, len(ctrl)), control_nodes=ctrl,
                            capacity=max(10 ** 5, args.envs), learning_starts=0, seed=5)
    run_frames(lr, 8)
    acting = [run_frames(lr, args.frames) for _ in range(args.reps_frames)]
    while lr.frames <= lr.batch_size + 4:      # update_policy runs from frame batch_size + 1 on
        lr.frame()
    learning = [run_frames(lr, args.frames) for _ in range(args.reps_frames)]
    fmt = lambda v: {"median_us_per_frame": statistics.median(v), "min_us": min(v), "max_us": max(v), "samples_us": v}  # noqa: E731
    out = {"before learning (act, step, store)": fmt(acting), "learning (+ cgbdq_update, 256 rows)": fmt(learning),
           "updates": lr.updates, "loss": float(lr.last_loss)}
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--reps-frames", type=int, default=5)
    ap.add_argument("--frames-per-run", dest="frames", type=int, default=20)
    ap.add_argument("--no-frames", action="store_true", help="the acting legs only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cgbdq_bench needs a GPU")
    res = {"what": f"ControlGBDQ, {args.envs} envs", "device": torch.cuda.get_device_name(0)}
    for name, ctrl in SHAPES.items():
        res[name] = {"control_nodes": ctrl, "act_hip_events": bench_act(name, ctrl, args)}
        if not args.no_frames and name == "pbn28":
            res[name]["learner_frame"] = bench_frames(name, ctrl, args)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
