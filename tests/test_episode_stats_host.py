"""Episode statistics without a GPU: the numpy restatement (tests/episode_stats_reference.py) on
hand-written sequences with known answers, the header's declarations, and -- from the C oracle
alone -- that every seeded case the GPU tests compare on contains the events they rely on."""
import os

import numpy as np
import pytest

from pbn_rl_amd import _lib
from tests import episode_stats_reference as R

T, U = R.TERMINATED, R.TRUNCATED
F = R.FIXED_ONE
ATTRACTORS = {5: 0, 9: 1}          # one state word: state 5 is attractor 0, state 9 attractor 1


def att(words):
    return ATTRACTORS.get(int(words[0]), -1)


def frame(reward, flags, state, target):
    return (np.asarray(reward, dtype=np.float32), np.asarray(flags, dtype=np.uint8),
            np.asarray([state], dtype=np.uint32), np.asarray(target, dtype=np.uint8))


def totals(ref):
    return dict(zip(R.TOTALS, (int(x) for x in ref["totals"])))


def test_hand_sequence_known_answers():
    """Four envs, three frames.  env 0: closes on the first frame with both flags (a success, not
    missed), then runs on; env 1: starts outside every attractor, truncates in frame 2 (unpaired);
    env 2: target NO_TARGET, truncates in frame 3 (unpaired); env 3: pair (1, 0), terminates in frame 2
    and again in frame 3 from its autoreset start (0, 1)."""
    state0, target0 = np.asarray([[5, 7, 9, 9]], dtype=np.uint32), np.asarray([1, 0, R.NO_TARGET, 0], dtype=np.uint8)
    frames = [
        frame([2.5, -1.0, -1.0, -2.0], [T | U, 0, 0, 0], [9, 7, 9, 3], [0, 0, R.NO_TARGET, 0]),
        frame([-1.0, -3.0, 0.25, 5.0], [0, U, 0, T], [9, 5, 9, 5], [0, 1, R.NO_TARGET, 1]),
        frame([-1.0, -1.0, -0.5, 4.0], [0, 0, U, T], [9, 5, 5, 9], [0, 1, 1, 0]),
    ]
    ref = R.episode_stats(frames, state0, target0, att, 2, log_every=1, series_rows=2)
    assert totals(ref) == {"frames": 3, "episodes": 5, "successes": 3, "missed": 2, "len_sum": 1 + 2 + 3 + 2 + 1,
                           "ret_sum": int((2.5 - 4.0 - 1.25 + 3.0 + 4.0) * F),
                           "last_reward_sum": int((2.5 - 3.0 - 0.5 + 5.0 + 4.0) * F), "unpaired": 2}
    # pairs[src][tgt] = episodes, missed, len_sum, ret_sum
    assert ref["pairs"][0, 1].tolist() == [2, 0, 2, int(6.5 * F)]      # env 0's first, env 3's second
    assert ref["pairs"][1, 0].tolist() == [1, 0, 2, int(3.0 * F)]      # env 3's first
    assert ref["pairs"].sum(axis=(0, 1))[0] == 3
    assert ref["hist"][1] == 2 and ref["hist"][2] == 2 and ref["hist"][3] == 1 and ref["hist"].sum() == 5
    # the open episodes: env 0 reopened at (1, 0) after frame 1 and has two steps since
    assert ref["src"].tolist() == [1, 0, 0, 1] and ref["tgt"].tolist() == [0, 1, 1, 0]
    assert ref["len"].tolist() == [2, 1, 0, 0] and ref["ret"].tolist() == [-2.0, -1.0, 0.0, 0.0]
    # log_every 1, two rows: frames 2 and 3 are kept, frame 3 in row 0
    assert ref["series"][1].tolist()[:3] == [2, 3, 2] and ref["series"][0].tolist() == ref["totals"].tolist()
    assert [len(c) for c in ref["closes"]] == [1, 2, 2]


def test_done_mask_and_length_cap():
    """A 300-step episode lands in bin 255 with its whole length in len_sum; with done_mask =
    TERMINATED alone a truncation closes nothing."""
    state0, target0 = np.asarray([[5]], dtype=np.uint32), np.asarray([1], dtype=np.uint8)
    frames = [frame([-0.125], [0], [7], [1]) for _ in range(299)] + [frame([-0.125], [U], [9], [0])]
    ref = R.episode_stats(frames, state0, target0, att, 2)
    assert totals(ref) == {"frames": 300, "episodes": 1, "successes": 0, "missed": 1, "len_sum": 300,
                           "ret_sum": int(-0.125 * 300 * F), "last_reward_sum": int(-0.125 * F), "unpaired": 0}
    assert ref["hist"][255] == 1 and ref["hist"].sum() == 1
    assert ref["pairs"][0, 1].tolist() == [1, 1, 300, int(-37.5 * F)]
    assert (ref["src"][0], ref["tgt"][0]) == (1, 0)
    open_ = R.episode_stats(frames, state0, target0, att, 2, done_mask=T)
    assert totals(open_)["episodes"] == 0 and open_["len"][0] == 300 and open_["ret"][0] == np.float32(-37.5)


def test_fixed_point_is_round_to_nearest_of_the_float32_return():
    assert R.to_fixed(np.float32(0.1)) == int(np.rint(np.float64(np.float32(0.1)) * 2 ** 20))
    assert R.to_fixed(-2.0) == -2 * F and R.to_fixed(2 ** -21) == 0 and R.to_fixed(3 * 2 ** -21) == 2


def test_spec_attractor_id_answers_as_envspec():
    spec = R.case_spec("pbn7_70")
    lookup = R.spec_attractor_id(spec)
    rng = np.random.default_rng(0)
    states = [s for a in spec.attractors for s in a] + [tuple(int(b) for b in rng.integers(0, 2, spec.n))
                                                         for _ in range(64)]
    for s in states:
        assert lookup(spec.network.pack(s)) == spec.attractor_id(s)


def test_header_declares_the_exports():
    decl = _lib.declared()
    assert _lib.ABI_VERSION == 11
    assert "pbn_episode.hip" in _lib.SOURCES
    assert os.path.exists(os.path.join(_lib.SRC_DIR, "pbn_episode.hip"))
    begin, track = decl["pbn_episode_begin"], decl["pbn_episode_track"]
    assert begin.params == ("net", "n_alloc", "n_real", "d_state", "d_target", "d_ret", "d_len", "d_src", "d_tgt",
                            "stream")
    assert track.params == ("net", "n_alloc", "n_real", "done_mask", "d_reward", "d_flags", "d_state", "d_target",
                            "d_ret", "d_len", "d_src", "d_tgt", "d_totals", "d_pairs", "d_hist", "log_every",
                            "series_rows", "d_series", "stream")
    assert track.ctext[3] == "uint32_t done_mask" and track.ctext[15] == "int64_t log_every"
    assert track.ctext[12] == "int64_t* d_totals" and begin.ctext[5] == "float* d_ret"


def test_python_names_match_the_contract():
    from pbn_rl_amd import episode_stats as E
    assert E.TOTALS == R.TOTALS and E.FIXED_ONE == R.FIXED_ONE and E.HIST_BINS == 256


@pytest.mark.parametrize("name", list(R.CASES))
def test_oracle_trajectory_contains_what_the_gpu_cases_rely_on(name):
    """From the C oracle alone: the case's trajectory closes episodes in the ways its GPU comparison
    is meant to cover (a terminated and a truncated episode, two closers of one 64-env wave with the
    same pair and with different pairs, an autoreset that changes an env's target)."""
    required = R.CASES[name][4]
    _, target0, frames, ref = R.case_oracle(name)
    got = R.events(ref, target0, frames)
    assert set(required) <= got, (name, sorted(set(required) - got))
    assert ref["totals"][1] > 0 and ref["totals"][0] == R.CASES[name][2]
    if name == "a254":       # whole waves of closers whose keys are all distinct
        assert any(len({(s, t) for _, s, t, _ in c}) >= 60 for c in ref["closes"])
    if name == "one_attractor":    # every close has key (0, 0)
        assert {(s, t) for c in ref["closes"] for _, s, t, _ in c} == {(0, 0)}
    if name == "no_attractors":
        assert ref["totals"][7] == ref["totals"][1]
