"""pbn_rollout's pipelined kernel where the env-draw wave's fast loop takes its rare fourth-flip
tail (csrc/rollout_pipe.h env_fast: PERT call 0 from a pinned Philox prefix, the fourth gap in
line unless its word falls in the bucket table's sentinel bucket, the further gaps behind a
second branch; csrc/step_law.h gap_tail_split) == the CPU oracle, bit for bit.

Every case runs pbn_rollout with in-kernel random actions, autoreset, and the per-step obs and
final states kept (run_launches of test_gpu_rollout_prefix.py: every output of every step, and
state, t and target after every launch).  Seed 4242, env offset 96, horizon 6 unless stated:

  1  pbn28, p = 0.17, 96 and 33 envs, launches [7, 2]: the highest round rate at which N = 28 still
     gets the gap bucket table (the fast loop's condition); a block with an invalid half, a ragged
     env count; perturbations of 8 and of 11 flips (PERT calls 1 and 2)
  2  pbn28, p = 0.02, 160 envs, [8], seed 4243 (4242 draws no fourth flip in these 1,280
     env-steps): the product's sparse regime: waves with no lane in the tail, with one, with several
  3  pbn10, p = 0.45, 96 envs, [7]
  4  pbn7, p = 0.4, 96 envs, [7]
     The bundled attractors of pbn10 and pbn7 hold several states each, which sends the env draws
     to the general loop: cases 3 and 4 run these networks with single-state targets instead
     (random_state_targets; three and four of them, the bundled counts), and 3b, 4b with the
     bundled attractors, which check the general loop's tail and assert that they do not take
     the fast one
  5  a 31-node synthetic network, p = 0.14, 96 envs, [5, 2]: the bit-31 clamp of first_gaps_mask31
  6  pbn28, p = 0.17, 96 envs, [6] from step 2^32: the step's low word is 0 where the tail's call
     takes the running word minus one
  7  the same from step 2^32 - 9: the last steps below the wrap that the fast loops take
  8  the same with env offset 2^32 + 192: the id's high half in counter word 3 of the PERT prefix

Every case asserts, from the host-side net image, that it meets the fast loop's conditions, and,
from the oracle alone, that the events it exists for occurred: the perturbation mask of an
env-step is final_state ^ obs ^ flipmask where FLAG_PERTURBED is set.
"""
import numpy as np
import pytest

from oracle import oracle
from pbn_rl_amd.attractors import load_attractors, random_state_targets
from pbn_rl_amd.network import load_network
from pbn_rl_amd.spec import EnvSpec

from .synthetic import random_spec
from .test_gpu_rollout_prefix import MODE, run_launches
from .test_net_image import build_shim, compile_raw

pytestmark = pytest.mark.gpu

SEED = 4242
FLAG_PERTURBED = 8


def bundled(name, p):
    return EnvSpec(load_network(name), load_attractors(name), perturbation=p, horizon=6)


def single_state(name, n_targets, p):
    net = load_network(name)
    return EnvSpec(net, random_state_targets(len(net.nodes), n_targets, 7), perturbation=p, horizon=6)


CASES = {
    "1_pbn28_p17": dict(spec=lambda: bundled("pbn28", 0.17), envs=(96, 33), launches=[7, 2]),
    "2_pbn28_sparse": dict(spec=lambda: bundled("pbn28", 0.02), envs=(160,), launches=[8], seed=4243),
    "3_pbn10": dict(spec=lambda: single_state("pbn10", 3, 0.45), envs=(96,), launches=[7]),
    "3b_pbn10_bundled": dict(spec=lambda: bundled("pbn10", 0.45), envs=(96,), launches=[7], fast=False),
    "4_pbn7": dict(spec=lambda: single_state("pbn7", 4, 0.4), envs=(96,), launches=[7]),
    "4b_pbn7_bundled": dict(spec=lambda: bundled("pbn7", 0.4), envs=(96,), launches=[7], fast=False),
    "5_rand31": dict(spec=lambda: random_spec(31, 22, max_funcs=3, perturbation=0.14, horizon=6), envs=(96,),
                     launches=[5, 2]),
    "6_step_2p32": dict(spec=lambda: bundled("pbn28", 0.17), envs=(96,), launches=[6], first_step=2 ** 32),
    "7_step_below_wrap": dict(spec=lambda: bundled("pbn28", 0.17), envs=(96,), launches=[6], first_step=2 ** 32 - 9),
    "8_env_offset_2p32": dict(spec=lambda: bundled("pbn28", 0.17), envs=(96,), launches=[6], env_offset=2 ** 32 + 192),
}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("gap_tail_image"))


def assert_fast_loop(shim, spec, launches, first_step, fast=True):
    """The conditions of env_fast, so that the case tests it and not the general env loop."""
    rc, err, sc, _ = compile_raw(shim, spec)
    assert rc == 0, err
    assert sc["gap_exact"] == 2 and sc["n_attr"] >= 2 and sc["att_single"] == (1 if fast else 0)
    assert sc["W"] == 1 and sc["n_nodes"] <= 31
    step = 1 if first_step is None else first_step   # (the reset is step 0)
    for T in launches:   # the step's high word does not change within a launch, its one-ahead call included
        assert step >> 32 == (step + T) >> 32
        step += T


def perturbation_masks(spec, n, launches, env_offset, first_step, seed=SEED):
    """[steps, n_alloc] perturbation masks of the oracle's steps (single-word states)."""
    n = -(-n // 32) * 32
    st, tg, t = oracle.reset(spec, seed, 0, env_offset, n)
    step = 1 if first_step is None else first_step
    flip = np.zeros((1, n), np.uint32)
    rows = []
    for _ in range(sum(launches)):
        ref = oracle.step(spec, seed, step, env_offset, st, flip, tg, t, MODE)
        pert = (ref["flags"] & FLAG_PERTURBED) != 0
        rows.append(np.where(pert, ref["final_state"][0] ^ st[0] ^ ref["flipmask"][0], 0).astype(np.uint32))
        st, tg, t = ref["state_out"], ref["target"], ref["t"]
        step += 1
    return np.stack(rows)


def popcount(m):
    return np.unpackbits(m.view(np.uint8).reshape(m.shape + (4,)), axis=-1).sum(axis=-1)


def third_flip(m):
    """The node of the third flip (lowest first) of every mask with three or more; -1 elsewhere."""
    out = np.full(m.shape, -1)
    seen = np.zeros(m.shape, int)
    for b in range(32):
        on = ((m >> np.uint32(b)) & 1) == 1
        seen += on
        out[on & (seen == 3)] = b
    return out


def events(masks, N):
    pc, third = popcount(masks), third_flip(masks)
    steps, n = masks.shape
    waves = pc.reshape(steps, n // 32, 32)
    if (n // 32) % 2:   # (the last block's invalid half: no env)
        waves = np.concatenate([waves, np.zeros((steps, 1, 32), pc.dtype)], axis=1)
    three_up = (waves.reshape(steps, -1, 64) >= 3).sum(axis=-1)   # per wave-step: envs with three or more flips
    return {"max_flips": int(pc.max()),
            "four_or_more": int((pc >= 4).sum()),
            "three_last_at_end": int(((pc == 3) & (third == N - 1)).sum()),
            "three_tail_nothing_landed": int(((pc == 3) & (third >= 0) & (third <= N - 2)).sum()),
            "flip_at_last_node": int((((masks >> np.uint32(N - 1)) & 1) == 1).sum()),
            "waves_without_three": int((three_up == 0).sum()),
            "waves_with_one_three": int((three_up == 1).sum()),
            "waves_with_several_three": int((three_up >= 2).sum())}


def case_events(case):
    spec = case["spec"]()
    total = {}
    for n in case["envs"]:
        ev = events(perturbation_masks(spec, n, case["launches"], case.get("env_offset", 96), case.get("first_step"),
                                       case.get("seed", SEED)), spec.n)
        for k, v in ev.items():
            total[k] = max(total.get(k, 0), v) if k == "max_flips" else total.get(k, 0) + v
    return total


@pytest.fixture(autouse=True)
def pipelined(monkeypatch):
    monkeypatch.setenv("PBN_ROLL", "pipe")


@pytest.mark.parametrize("name", list(CASES))
def test_fourth_flip_tail_matches_oracle(shim, name):
    case = CASES[name]
    spec = case["spec"]()
    assert_fast_loop(shim, spec, case["launches"], case.get("first_step"), case.get("fast", True))
    ev = case_events(case)
    print(name, ev)
    assert ev["four_or_more"] > 0
    if name[0] in "12345":
        assert ev["three_last_at_end"] > 0 and ev["three_tail_nothing_landed"] > 0 and ev["flip_at_last_node"] > 0
    if name[0] == "1":
        assert ev["max_flips"] >= 11   # 8 and up: PERT call 1; 11 and up: call 2
    if name[0] == "2":
        assert ev["waves_without_three"] > 0 and ev["waves_with_one_three"] > 0
    for n in case["envs"]:
        seen = run_launches(spec, n, case["launches"], seed=case.get("seed", SEED), env_offset=case.get("env_offset", 96),
                            first_step=case.get("first_step"))
        assert seen & FLAG_PERTURBED
