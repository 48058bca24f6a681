"""Source -> target control evaluation of a trained agent (model_tester.py:587-658) on one GPU.

    python tools/evaluate.py --network bb33 --checkpoint tests/golden/bb33_bdq_final.npz \
        --attractor-order 0,2,1 --settle 64 --perturbation 0 [--runs 10] [--out results/pbn_33_3.pkl]

--network      a bundled name (pbn7, pbn10, pbn28, pbn70, bb33, m47) or an .ispl / .bnet file
--checkpoint   a reference bdq_final.pt (load_bdq_checkpoint) or an exported .npz (tools/export_agent.py)
--attractors   evaluate the first N attractors (model_tester.py's --attractors); the set is the bundled
               one, or --attractor-file (a networks/*_attractors.json-style file, e.g. tools/discover.py's)
--attractor-order  indices into that set, in the order of the result matrix
--out          .pkl: the reference's (save_matrix, data) tuple; .json: the same with the settings

Prints the per-run matrix (save_matrix / runs, what the reference prints and plots), the failure
share and the pooled mean length, then one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from pbn_rl_amd.agent import BranchingQNetwork, load_bdq_checkpoint  # noqa: E402
from pbn_rl_amd.attractors import clean_state, load_attractors  # noqa: E402
from pbn_rl_amd.bnet import parse_bnet_file  # noqa: E402
from pbn_rl_amd.evaluate import evaluate_control  # noqa: E402
from pbn_rl_amd.network import Network, load_network  # noqa: E402
from pbn_rl_amd.spec import EnvSpec  # noqa: E402


def read_network(arg: str):
    """(network, bundled name or None)."""
    if arg.endswith(".ispl"):
        return Network.from_ispl(arg), None
    if arg.endswith(".bnet"):
        return parse_bnet_file(arg, name=os.path.splitext(os.path.basename(arg))[0]), None
    return load_network(arg), arg


def read_agent(path: str, n_nodes: int) -> BranchingQNetwork:
    q = BranchingQNetwork((n_nodes, n_nodes), n_nodes + 1, 3)      # three branches (train_BDQ.py:83)
    if path.endswith(".npz"):
        from tests.golden_parts import load_parts      # an export may come in parts below 1 MiB
        q.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in load_parts(path).items()})
    else:
        load_bdq_checkpoint(q, path)
    return q.eval()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--network", required=True)
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--attractors", type=int, default=None, help="use the first N attractors")
    ap.add_argument("--attractor-file", default=None)
    ap.add_argument("--attractor-order", default=None, help="comma-separated indices, e.g. 0,2,1")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--max-steps", type=int, default=100)
    ap.add_argument("--settle", type=int, default=64)
    ap.add_argument("--perturbation", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    net, bundled = read_network(args.network)
    if args.attractor_file:
        with open(args.attractor_file) as f:
            atts = [[clean_state(s) for s in a] for a in json.load(f)["attractors"]]
    elif bundled:
        atts = load_attractors(bundled)
    else:
        ap.error("a network file needs --attractor-file")
    if args.attractor_order:
        atts = [atts[int(i)] for i in args.attractor_order.split(",")]
    if args.attractors is not None:
        atts = atts[:args.attractors]
    spec = EnvSpec(net, atts, perturbation=args.perturbation, horizon=0, settle=args.settle)
    agent = read_agent(args.checkpoint, net.n)

    t0 = time.perf_counter()
    ev = evaluate_control(spec, agent, runs=args.runs, max_steps=args.max_steps, seed=args.seed)
    seconds = time.perf_counter() - t0
    np.set_printoptions(linewidth=200, precision=3, suppress=True)
    print(ev.matrix / args.runs)
    print(f"{ev.failed} state pairs failed out of {ev.total}, {ev.failed * 100 / ev.total}%")
    print(f"average is {ev.mean_length()}")
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        ev.save(args.out)
    print(json.dumps({"network": net.name, "n_attractors": len(atts), "runs": args.runs, "max_steps": args.max_steps,
                      "settle": args.settle, "perturbation": args.perturbation, "seed": args.seed,
                      "failed": ev.failed, "total": ev.total, "mean_length": ev.mean_length(),
                      "data": {str(k): v for k, v in sorted(ev.data.items())}, "seconds": seconds,
                      "out": args.out}), flush=True)


if __name__ == "__main__":
    main()
