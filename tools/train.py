"""Train, checkpoint and resume: the reference's entry scripts (train_BDQ.py, train_ddqn.py /
train_pbn_28.py) over the batched learners.

  python tools/train.py --agent ddqn --network pbn28 --envs 32768 --frames 2000 --chunk 500 --checkpoint-dir D
  python tools/train.py --agent ddqn --network pbn28 --envs 32768 --frames 4000 --chunk 500 --checkpoint-dir D --resume

The second command loads the latest ``ckpt_<frames>.npz`` of D (by frame number) and goes on to frame
4,000, ending in the state of an uninterrupted 4,000-frame run, bit for bit (DESIGN.md "Checkpoint and
resume").  A resumed run takes the flags of the run it continues: the file holds the run's state, not
its hyper-parameters, and refuses a learner of another shape.  ``--schedule-frames`` (the DDQN
schedules' length, ``total_frames``) is a flag of its own, so that ``--frames`` only says where to stop.

The frame is captured in one hipGraph and replayed ``--chunk`` frames per ``run()`` (``--no-capture``:
eager frames).  After every chunk the reference's line is printed from ``stats.window()``; a checkpoint
is written every ``--checkpoint-every`` frames and at the end, with the wall time of the save.
``--save-reference`` also writes the reference's own files (``bdq_<frame>.pt`` / ``bdq_final.pt``,
``ddqn_<num_timesteps>.pt``).  One process, no child, no environment variable.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from pbn_rl_amd import checkpoint  # noqa: E402
from pbn_rl_amd.attractors import load_attractors  # noqa: E402
from pbn_rl_amd.ddqn import DDQNLearner  # noqa: E402
from pbn_rl_amd.evaluate import evaluate_control  # noqa: E402
from pbn_rl_amd.network import load_network  # noqa: E402
from pbn_rl_amd.replay import BDQLearner  # noqa: E402
from pbn_rl_amd.spec import EnvSpec  # noqa: E402
from pbn_rl_amd.vector_env import VectorPBNEnv  # noqa: E402

# a save then costs under 1 % of the run at train_ddqn.py's shape (DESIGN.md "Checkpoint and resume", "Measured")
DEFAULT_CHECKPOINT_EVERY = 50_000


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--agent", choices=("bdq", "ddqn"), default="ddqn")
    ap.add_argument("--network", default="pbn28")
    ap.add_argument("--envs", type=int, default=32768)
    ap.add_argument("--frames", type=int, required=True, help="stop when the run has this many frames")
    ap.add_argument("--chunk", type=int, default=1000, help="frames per run() and per printed line")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--settle", type=int, default=0, help="the step law: 0 one update per step, K >= 2 settle")
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--perturbation", type=float, default=0.01)
    # the hyper-parameters the two reference scripts set
    ap.add_argument("--batch-size", type=int, default=None, help="default: 64 (ddqn), 256 (bdq)")
    ap.add_argument("--capacity", type=int, default=1 << 20)
    ap.add_argument("--learning-rate", type=float, default=1e-4)
    ap.add_argument("--gamma", type=float, default=None, help="default: 0.95 (ddqn), 0.999 (bdq)")
    ap.add_argument("--target-update", type=int, default=None, help="default: 512 frames (ddqn), 10,000 updates (bdq)")
    ap.add_argument("--learning-starts", type=int, default=None)
    ap.add_argument("--schedule-frames", type=int, default=100_000,
                    help="ddqn: total_frames of the epsilon / beta schedules; bdq: epsilon_decay")
    ap.add_argument("--exploration-fraction", type=float, default=0.1)
    ap.add_argument("--min-epsilon", type=float, default=0.05)
    ap.add_argument("--net-arch", default="50,50", help="ddqn: the hidden Linear's widths")
    ap.add_argument("--uniform", action="store_true", help="uniform replay instead of prioritised")
    ap.add_argument("--curriculum", action="store_true", help="the reference's rework_probas restarts")
    ap.add_argument("--stats-log-every", type=int, default=0)
    ap.add_argument("--checkpoint-dir", default=None)
    ap.add_argument("--checkpoint-every", type=int, default=DEFAULT_CHECKPOINT_EVERY)
    ap.add_argument("--resume", action="store_true", help="continue the latest checkpoint of --checkpoint-dir")
    ap.add_argument("--no-capture", action="store_true", help="eager frames instead of the captured one")
    ap.add_argument("--eval-runs", type=int, default=0, help="evaluate_control with this many runs at the end")
    ap.add_argument("--save-reference", action="store_true", help="also write the reference's own .pt files")
    args = ap.parse_args(argv)
    if args.frames < 1 or args.chunk < 1 or args.checkpoint_every < 1:
        ap.error("--frames, --chunk and --checkpoint-every must be >= 1")
    if (args.resume or args.save_reference) and not args.checkpoint_dir:
        ap.error("--resume and --save-reference need --checkpoint-dir")
    return args


def build_learner(args):
    spec = EnvSpec(load_network(args.network), load_attractors(args.network), perturbation=args.perturbation,
                   horizon=args.horizon, settle=args.settle)
    env = VectorPBNEnv(spec, args.envs, seed=args.seed)
    torch.manual_seed(args.seed)
    common = dict(capacity=args.capacity, learning_rate=args.learning_rate, seed=args.seed,
                  graphable=not args.no_capture, episode_stats=True, stats_log_every=args.stats_log_every,
                  curriculum=args.curriculum)
    opt = {k: v for k, v in (("gamma", args.gamma), ("target_update", args.target_update),
                             ("learning_starts", args.learning_starts)) if v is not None}
    if args.agent == "ddqn":
        arch = [tuple(int(x) for x in args.net_arch.split(","))]
        learner = DDQNLearner(env, net_arch=arch, total_frames=args.schedule_frames, batch_size=args.batch_size or 64,
                              exploration_fraction=args.exploration_fraction, min_epsilon=args.min_epsilon,
                              prioritised=not args.uniform, **common, **opt)
    else:
        learner = BDQLearner(env, batch_size=args.batch_size or 256, epsilon_decay=args.schedule_frames,
                             prioritised=not args.uniform, fused=True, **common, **opt)
    env.reset()
    learner.stats.begin()
    return learner


def report(args, learner):
    w = learner.stats.window()
    if args.agent == "bdq":
        print(f"frame {learner.frames}  Average episode reward: {w['ep_last_reward_mean']:.4f}  "
              f"Avg len: {w['ep_len_mean']:.3f}  Missed paths: {w['missed_pairs']}  "
              f"(episodes {w['episodes']}, epsilon {learner.epsilon:.4f})", flush=True)
    else:
        print(f"frame {learner.frames}  rollout/ep_rew_mean {w['ep_rew_mean']:.4f}  "
              f"rollout/ep_len_mean {w['ep_len_mean']:.3f}  (episodes {w['episodes']}, epsilon {learner.epsilon:.4f}, "
              f"beta {learner.beta:.4f})", flush=True)


def save(args, learner, final=False):
    d = args.checkpoint_dir
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, checkpoint.checkpoint_name(learner.frames))
    t0 = time.perf_counter()
    learner.save(path)
    dt = time.perf_counter() - t0
    print(f"saved {path} in {dt:.3f} s ({os.path.getsize(path)} bytes)", flush=True)
    if args.save_reference:
        if args.agent == "bdq":
            checkpoint.save_reference_bdq(learner, os.path.join(d, f"bdq_{learner.frames}.pt"))
            if final:
                checkpoint.save_reference_bdq(learner, os.path.join(d, "bdq_final.pt"))
        else:
            checkpoint.save_reference_ddqn(learner, d, exploration_fraction=args.exploration_fraction)


def main(argv=None):
    args = parse(argv)
    if not torch.cuda.is_available():
        raise SystemExit("train.py needs a GPU")
    learner = build_learner(args)
    if args.resume:
        path = checkpoint.latest(args.checkpoint_dir)
        if path is None:
            print(f"no checkpoint in {args.checkpoint_dir}: starting from frame 0", flush=True)
        else:
            t0 = time.perf_counter()
            learner.load(path)
            torch.cuda.synchronize()
            print(f"loaded {path} in {time.perf_counter() - t0:.3f} s: frame {learner.frames}", flush=True)
    captured = False
    t_start, f_start = time.perf_counter(), learner.frames
    saved_at = learner.frames if args.resume else -1
    while learner.frames < args.frames:
        if not args.no_capture and not captured:
            learner.capture()       # (eager frames first where the run has not learned yet; none after a resume that has)
            captured = True
        every = args.checkpoint_every
        # (chunks and checkpoints fall on multiples of --chunk and --checkpoint-every, whatever capture() ran first)
        n = min(args.chunk - learner.frames % args.chunk, args.frames - learner.frames, every - learner.frames % every)
        if n > 0:
            if captured:
                learner.run(n)
            else:
                for _ in range(n):
                    learner.frame()
        report(args, learner)
        if args.checkpoint_dir and learner.frames % every == 0:
            save(args, learner, final=learner.frames >= args.frames)
            saved_at = learner.frames
    torch.cuda.synchronize()
    dt = time.perf_counter() - t_start
    done = learner.frames - f_start
    if done:
        print(f"{done} frames in {dt:.2f} s ({dt / done * 1e6:.1f} us per frame, saves included)", flush=True)
    if args.checkpoint_dir and saved_at != learner.frames:
        save(args, learner, final=True)
    if args.eval_runs:
        ev = evaluate_control(learner.env, learner.q, runs=args.eval_runs)
        print(f"evaluate_control: mean length {ev.mean_length():.3f}, failed {ev.failed} of {ev.total}", flush=True)


if __name__ == "__main__":
    main()
