"""The host side of pbn_rl_amd.evaluate (CPU): the pair plan, the summary and the writers.

model_tester.py:587-658 is the protocol; tests/protocol.py restates it in numpy over a step
function, and data/results/pbn_33_3.pkl (tests/golden/ref_fixtures.json) is the reference's own
recorded result for the bb33 agent.
"""
import itertools
import json
import pickle

import numpy as np
import pytest

from pbn_rl_amd.attractors import load_attractors
from pbn_rl_amd.evaluate import ControlEvaluation, plan_pairs, pooled_mean, summarize
from pbn_rl_amd.network import load_network
from pbn_rl_amd.spec import EnvSpec

from .protocol import load_agent, pack, replay
from .test_bn_pin import oracle_step_fn, reference_result
from .test_law_pin import ref_pbn7_attractors


def bb33_chosen():
    atts = load_attractors("bb33")
    return [atts[i] for i in (0, 2, 1)]


# ------------------------------------------------------------------------------ the plan
def test_plan_bb33_layout():
    atts = bb33_chosen()
    plan = plan_pairs(atts, runs=10)
    assert plan.pairs == list(itertools.product(range(3), repeat=2))
    assert (plan.n_real, plan.n_alloc, plan.runs, plan.n_attractors) == (90, 96, 10, 3)
    for i, (a, t) in enumerate(plan.pairs):
        rows = slice(10 * i, 10 * i + 10)                          # pair-major: env = pair * runs + run
        assert (plan.start_bits[rows] == np.array(atts[a][0], np.uint8)).all()
        assert (plan.target_bits[rows] == np.array(atts[t][0], np.uint8)).all()
        assert (plan.target_id[rows] == t).all()
        assert (plan.open0[rows] == (0 if a == t else 1)).all()    # the diagonal starts inside its target
    assert (plan.count0 == 0).all() and plan.count0.dtype == np.int32
    # padding: closed, attractor 0 as source and target
    assert (plan.open0[90:] == 0).all() and (plan.target_id[90:] == 0).all()
    assert (plan.start_bits[90:] == np.array(atts[0][0], np.uint8)).all()
    assert plan.start_words.shape == (2, 96) and plan.start_words.dtype == np.uint32
    assert np.array_equal(plan.start_words, pack(plan.start_bits.astype(np.int64)))


def test_plan_pbn7_multi_state_attractors():
    """pbn7's four reference attractors (one of them a '*' pattern of several states): the start
    is the attractor's first state, and only the diagonal lies inside its target."""
    atts = ref_pbn7_attractors()
    assert len(atts) == 4 and max(len(a) for a in atts) > 1
    plan = plan_pairs(atts, runs=6)
    assert (plan.n_real, plan.n_alloc) == (96, 96)                 # no padding at a multiple of 32
    assert plan.pairs == list(itertools.product(range(4), repeat=2))
    for i, (a, t) in enumerate(plan.pairs):
        assert (plan.start_bits[6 * i:6 * i + 6] == np.array(atts[a][0], np.uint8)).all()
        assert (plan.target_id[6 * i:6 * i + 6] == t).all()
        assert (plan.open0[6 * i:6 * i + 6] == (a != t)).all()


def test_plan_start_inside_another_target_and_custom_pairs():
    """A run is closed whenever its start state is a state of the target attractor, not only on
    the diagonal (model_tester.py:616 tests membership); `pairs` selects and orders the runs."""
    atts = [[(0, 0, 1)], [(1, 1, 0), (0, 0, 1)], [("*", 1, 1)]]
    plan = plan_pairs(atts, pairs=[(0, 1), (1, 0), (2, 2), (1, 2)], runs=3)
    assert plan.pairs == [(0, 1), (1, 0), (2, 2), (1, 2)]
    assert plan.open0[:12].tolist() == [0] * 3 + [1] * 3 + [0] * 3 + [1] * 3
    assert plan.start_bits[6].tolist() == [0, 1, 1]                # '*' -> 0 (:609)
    assert (plan.n_real, plan.n_alloc) == (12, 32)
    with pytest.raises(ValueError):
        plan_pairs(atts, pairs=[(0, 3)])
    with pytest.raises(ValueError):
        plan_pairs(atts, runs=0)


# --------------------------------------------------------------------------- the summary
def test_summary_of_bb33_replay_equals_reference_pickle():
    """The CPU replay's counts (settle law, p = 0, 10 runs) through the product's summary are the
    reference's recorded (save_matrix, data)."""
    chosen = bb33_chosen()
    spec = EnvSpec(load_network("bb33"), chosen, perturbation=0.0, horizon=0, settle=64)
    res = replay(oracle_step_fn(spec), load_agent("bb33", 33), chosen, n_runs=10)
    plan = plan_pairs(chosen, runs=10)
    counts = np.stack([res[p] for p in plan.pairs])
    ev = summarize(counts, plan.pairs, plan.n_attractors, 100)
    ref, ref_data = reference_result()
    assert np.array_equal(ev.matrix / 10, ref)
    assert {k: v for k, v in ev.data.items() if v} == ref_data
    assert ev.data[101] == 0 and ev.failed == 0                    # the failure key is always there
    assert ev.counts.shape == (9, 10) and ev.counts.dtype == np.int32
    assert ev.pair_fail.tolist() == [0] * 9
    assert ev.mean_length() == (40 * 1 + 20 * 2) / 60


def test_summary_counts_failures_as_max_steps_plus_one():
    counts = np.array([[0, 0], [3, 6], [6, 2], [6, 6]])
    ev = summarize(counts, [(0, 0), (0, 1), (1, 0), (1, 1)], 2, max_steps=5)
    assert ev.matrix.tolist() == [[0.0, 9.0], [8.0, 12.0]] and ev.matrix.dtype == np.float64
    assert ev.data == {0: 2, 2: 1, 3: 1, 6: 4}
    assert ev.failed == 4 and ev.pair_fail.tolist() == [0, 1, 1, 2] and ev.total == 8
    assert ev.mean_length() == 2.5
    with pytest.raises(ValueError):
        summarize(np.array([[7]]), [(0, 0)], 1, max_steps=5)


# ----------------------------------------------------------------------------- the writers
def hand_made():
    counts = np.array([[0, 0, 0], [1, 4, 101], [2, 2, 2], [0, 0, 0]])
    return summarize(counts, [(0, 0), (0, 1), (1, 0), (1, 1)], 2, 100, settings={"network": "toy", "seed": 3})


def test_save_pkl_is_the_reference_tuple(tmp_path):
    ev = hand_made()
    path = str(tmp_path / "pbn_2_2.pkl")
    ev.save(path)
    with open(path, "rb") as f:
        mat, data = pickle.load(f)
    assert type(mat) is np.ndarray and mat.shape == (2, 2) and mat.dtype == np.float64
    assert type(data) is dict and all(type(k) is int and type(v) is int for k, v in data.items())
    assert np.array_equal(mat, ev.matrix) and mat.tolist() == [[0.0, 106.0], [6.0, 0.0]]
    assert data == ev.data == {0: 6, 1: 1, 2: 3, 4: 1, 101: 1}


def test_save_json_round_trips(tmp_path):
    ev = hand_made()
    path = str(tmp_path / "eval.json")
    ev.save(path)
    with open(path) as f:
        obj = json.load(f)
    assert obj["save_matrix"] == ev.matrix.tolist()
    assert {int(k): v for k, v in obj["data"].items()} == ev.data
    assert obj["counts"] == ev.counts.tolist() and obj["pairs"] == [list(p) for p in ev.pairs]
    assert obj["settings"] == {"network": "toy", "seed": 3}
    assert (obj["runs"], obj["max_steps"], obj["failed"]) == (3, 100, 1)
    back = summarize(np.array(obj["counts"]), [tuple(p) for p in obj["pairs"]], 2, obj["max_steps"])
    assert np.array_equal(back.matrix, ev.matrix) and back.data == ev.data
    with pytest.raises(ValueError):
        ev.save(str(tmp_path / "eval.txt"))


# ------------------------------------------------------------------------- the pooled mean
def test_pooled_mean_restates_model_tester():
    """model_tester.py:713-727: s += k * v and div += v for every key but 0 and those past 100."""
    data = {0: 30, 1: 40, 2: 20, 7: 3, 100: 1, 101: 5}
    s = div = 0
    for k in data:
        v = data[k]
        if k == 0 or k > 100:
            continue
        s += k * v
        div += v
    assert pooled_mean(data) == s / div == (40 + 40 + 21 + 100) / 64
    ev = ControlEvaluation(counts=np.zeros((1, 1), np.int32), matrix=np.zeros((1, 1)), data=data, pairs=[(0, 0)],
                           runs=1, max_steps=100)
    assert ev.mean_length() == s / div and ev.failed == 5
    assert np.isnan(pooled_mean({0: 4, 101: 2}))
