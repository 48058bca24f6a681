"""Seeded random PBNs for tests: the paths the kaban networks never take.

Every kaban network has 2-3 functions per node with weights 1 (a few merged duplicates).
These networks add nodes with up to 6 distinct functions (the > kNodeRecs chain tail),
arbitrary relative weights (per-node thresholds), constant (arity 0) functions, node counts
that give 1..4 state words, and (max_arity > 4) wide functions that need gates.  Further down:
specs at the limits of the network descriptor (attractor hashes that no multiplier makes collision
free, lowered gates that fill every plane a byte addresses).
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


# ------------------------------------------------ the attractor hash beyond one probe
def hold_network(n_nodes: int) -> Network:
    """Every node keeps its value (one function, the identity on itself): without perturbation
    the next state is state ^ flipmask, so a test puts every env on a state of its choice."""
    nodes = [[NodeFunction((i,), 0b10, Fraction(1), [])] for i in range(n_nodes)]
    return Network([f"g{i}" for i in range(n_nodes)], nodes, name=f"hold{n_nodes}")


def random_states(n_nodes: int, count: int, rng, avoid=()) -> list:
    """count distinct seeded random states (bit tuples) outside avoid, in the order drawn."""
    seen, out = set(avoid), []
    while len(out) < count:
        s = tuple(int(b) for b in rng.integers(0, 2, size=n_nodes))
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out


def many_attractor_spec(n_nodes: int, n_states: int, groups=None, seed: int = 0, **kw) -> EnvSpec:
    """n_states seeded random attractor states on hold_network: single-state attractors, or
    (groups: a list of sizes that sum to n_states) multi-state ones.  From 128 or so random
    states on no LDS hash is collision free: the kernels' lookups probe more than one slot."""
    states = random_states(n_nodes, n_states, np.random.default_rng(seed))
    groups = [1] * n_states if groups is None else list(groups)
    assert sum(groups) == n_states
    ends = np.cumsum(groups)
    return EnvSpec(hold_network(n_nodes), [states[e - g:e] for g, e in zip(groups, ends)], **kw)


def collapse_spec(n_nodes: int, seed: int, free: int = 8, n_random: int = 127, **kw) -> EnvSpec:
    """Attractor hits under random actions: `free` randomly placed nodes keep their value and every
    other node is a constant, so after one update a state is the constants with some pattern
    of the free bits.  254 single-state attractors: n_random random states first (they take their
    home slots of the hash and displace what collides with them; the pattern family alone usually
    hashes collision free), then 254 - n_random of the 2^free patterns."""
    rng = np.random.default_rng(seed)
    held = sorted(int(i) for i in rng.choice(n_nodes, size=free, replace=False))
    const = [int(b) for b in rng.integers(0, 2, size=n_nodes)]
    nodes = [[NodeFunction((i,), 0b10, Fraction(1), [])] if i in held else [NodeFunction((), const[i], Fraction(1), [])]
             for i in range(n_nodes)]
    net = Network([f"g{i}" for i in range(n_nodes)], nodes, name=f"collapse{n_nodes}_{seed}")
    patterns = []
    for m in (int(m) for m in rng.permutation(1 << free)[:254 - n_random]):
        s = list(const)
        for j, i in enumerate(held):
            s[i] = (m >> j) & 1
        patterns.append(tuple(s))
    states = random_states(n_nodes, n_random, rng, avoid=patterns) + patterns
    return EnvSpec(net, [[s] for s in states], **kw)


# ------------------------------------------------ gate planes up to the last addressable one
# N -> (seed of random_network(N, seed, max_funcs=3), arities of the wide functions appended to the
# first nodes): 32 W + n_gates == 256 (a function of 5, 6, 7, 8 inputs lowers to 2, 6, 14, 30 gates)
GATE_LIMIT = {32: (41, [8] * 7 + [7]), 64: (42, [8] * 6 + [6] * 2), 70: (43, [8] * 5 + [5] * 5),
              96: (44, [8] * 5 + [5] * 5), 97: (45, [8] * 4 + [5] * 4), 128: (46, [8] * 4 + [5] * 4)}


def add_wide_functions(net: Network, arities, seed: int, weight=None) -> Network:
    """Appends a seeded random function of arities[i] inputs (a table only: Shannon-lowered) to
    node i, with the given weight or a random one in 1..9."""
    rng = np.random.default_rng(seed)
    for i, k in enumerate(arities):
        ins = [int(x) for x in rng.choice(net.n, size=k, replace=False)]
        ins, table = _reduce(ins, int.from_bytes(rng.bytes(max((1 << k) // 8, 1)), "little") & ((1 << (1 << k)) - 1))
        assert len(ins) == k
        net.nodes[i].append(NodeFunction(ins, table, Fraction(weight or int(rng.integers(1, 10))), []))
    return net


def gate_limit_network(n_nodes: int, extra=()) -> Network:
    seed, arities = GATE_LIMIT[n_nodes]
    net = add_wide_functions(random_network(n_nodes, seed, max_funcs=3), list(arities) + list(extra), seed + 1000)
    net.name = f"gates{n_nodes}_limit"
    return net


def gate_hold_mix_spec(**kw) -> EnvSpec:
    """Gates and a many-probe hash in one image, as bb33 has gates and attractors: 70 nodes that keep
    their value, the first ten of which take a wide function instead with probability 1 / 10
    (160 gates: planes 96..255), and 254 random single-state attractors.  An env that starts on an
    attractor state stays there with probability 0.6 or so and otherwise leaves it by what the
    gates computed."""
    net = hold_network(70)
    for fl in net.nodes:
        fl[0].weight = Fraction(9)
    add_wide_functions(net, GATE_LIMIT[70][1], 7070, weight=1)
    net.name = "gates70_a254"
    spec = EnvSpec(net, [[s] for s in random_states(70, 254, np.random.default_rng(7071))], **kw)
    assert 32 * spec.words + int(spec.arrays["n_gates"][0]) == 256
    return spec


def gate_limit_spec(n_nodes: int, attractors=None, **kw) -> EnvSpec:
    """A network whose lowered wide functions fill every plane a byte addresses: the last gate's
    output is plane 255.  attractors: a list, or (default) 8 random single-state targets."""
    net = gate_limit_network(n_nodes)
    atts = random_state_targets(n_nodes, 8, GATE_LIMIT[n_nodes][0] + 1) if attractors is None else attractors
    spec = EnvSpec(net, atts, **kw)
    assert 32 * spec.words + int(spec.arrays["n_gates"][0]) == 256
    return spec


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
