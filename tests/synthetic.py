"""Seeded random PBNs for tests: the paths the kaban networks never take.

Every kaban network has 2-3 functions per node with weights 1 (a few merged duplicates).
These networks add nodes with up to 6 distinct functions (the > kNodeRecs chain tail),
arbitrary relative weights (per-node thresholds), constant (arity 0) functions, node counts
that give 1..4 state words, and (max_arity > 4) wide functions that need gates.
"""
from fractions import Fraction

import numpy as np

from pbn_rl_amd.attractors import random_state_targets
from pbn_rl_amd.network import Network, NodeFunction, _reduce
from pbn_rl_amd.spec import EnvSpec


def random_network(n_nodes: int, seed: int, max_funcs: int = 6, max_arity: int = 4) -> Network:
    rng = np.random.default_rng(seed)
    nodes = []
    for i in range(n_nodes):
        nf = int(rng.integers(1, max_funcs + 1))
        funcs, seen = [], set()
        while len(funcs) < nf:
            k = int(rng.integers(0, min(max_arity, n_nodes) + 1))
            ins = [int(x) for x in rng.choice(n_nodes, size=k, replace=False)]
            if (1 << k) <= 32:
                table = int(rng.integers(0, 1 << (1 << k)))
            else:   # wide functions (k >= 6): a random 2^k-bit table
                table = int.from_bytes(rng.bytes((1 << k) // 8), "little")
            key = _reduce(ins, table)
            if key in seen:
                continue
            seen.add(key)
            funcs.append(NodeFunction(key[0], key[1], Fraction(int(rng.integers(1, 10))), []))
        nodes.append(funcs)
    return Network([f"g{i}" for i in range(n_nodes)], nodes, name=f"rand{n_nodes}_{seed}")


def random_spec(n_nodes: int, seed: int, n_targets: int = 8, max_funcs: int = 6, **kw) -> EnvSpec:
    net = random_network(n_nodes, seed, max_funcs=max_funcs)
    return EnvSpec(net, random_state_targets(n_nodes, n_targets, seed + 1), **kw)


def multi_state_spec(**kw) -> EnvSpec:
    """A 40-node network (two state words) whose four 'attractors' hold 3, 1, 5 and 2 seeded random
    states: the start-state draw within an attractor, which no bundled fixture takes."""
    net = random_network(40, 31, max_funcs=3)
    rng = np.random.default_rng(32)
    states = set()
    while len(states) < 11:
        states.add(tuple(int(b) for b in rng.integers(0, 2, size=40)))
    states = sorted(states)
    return EnvSpec(net, [states[0:3], states[3:4], states[4:9], states[9:11]], **kw)


def law_branch_specs(**kw) -> dict:
    """Specs that take the branches of the per-env law (csrc/step_law.h) the bundled fixtures at
    their usual settings do not: one attractor (start 0, target 0, no pair draw), none,
    multi-state attractors, the gap methods other than the bucket table (p = 0.3: the log
    estimate; p = 0.6: the binary search), and the tail of further gaps taken by most envs, on the
    general env loops (the three above) and on the fast ones (bucket table, single-state
    attractors: pbn28 at p = 0.12, pbn70 at p = 0.05)."""
    from pbn_rl_amd.attractors import load_attractors
    from pbn_rl_amd.network import load_network
    p28, a28 = load_network("pbn28"), load_attractors("pbn28")
    return {
        "one_attractor": EnvSpec(p28, a28[:1], **{"perturbation": 0.05, **kw}),
        "no_attractors": EnvSpec(p28, [], **{"perturbation": 0.05, **kw}),
        "multi_state": multi_state_spec(**{"perturbation": 0.05, **kw}),
        "gap_estimate_tail": EnvSpec(p28, a28, **{"perturbation": 0.3, **kw}),
        "gap_search_tail": EnvSpec(load_network("pbn7"), load_attractors("pbn7"), **{"perturbation": 0.6, **kw}),
        "fast_tail_pbn28": EnvSpec(p28, a28, **{"perturbation": 0.12, **kw}),
        "fast_tail_pbn70": EnvSpec(load_network("pbn70"), load_attractors("pbn70"), **{"perturbation": 0.05, **kw}),
    }


LAW_BRANCHES = ["one_attractor", "no_attractors", "multi_state", "gap_estimate_tail", "gap_search_tail",
                "fast_tail_pbn28", "fast_tail_pbn70"]
