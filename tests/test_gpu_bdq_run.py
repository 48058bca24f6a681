"""``BDQLearner.run(k)``: ``k`` captured frames back to back, against ``k`` calls of ``frame()`` on a twin
captured learner.  Every comparison is exact.

tests/checkpoint_cases.py's shapes: pbn28, 90 envs, a 256-row ring, ``updates_per_frame`` 2 and
``target_update`` 6.  Both learners capture after two eager frames (4 updates); ``run(7)`` then takes the
updates from 4 to 18, so soft updates fall due after its first, fourth and seventh frame: two inside
the run and one at its end, and ``run`` replays 1 + 3 + 3 frames.  ``stats_log_every`` 2: the windows
that end at frames 4, 6 and 8 elapse inside the run."""
import pytest
import torch

from tests.checkpoint_cases import assert_same, bdq_learner, check_counters, same_value, snapshot

pytestmark = pytest.mark.gpu

KINDS = {"fused-uniform": dict(), "fused-prioritised": dict(prioritised=True), "pytorch": dict(fused=False)}


def _twin(kind):
    lr = bdq_learner(True, episode_stats=True, stats_log_every=2, **KINDS[kind])
    lr.capture()
    assert lr.frames == 2 and lr.updates == 4
    return lr


@pytest.mark.parametrize("kind", list(KINDS))
def test_run_k_equals_k_frames(kind):
    one, many = _twin(kind), _twin(kind)
    t0 = many.fused.t_flat.clone() if many.fused is not None else None
    out_many = many.run(7)
    for _ in range(7):
        out_one = one.frame()
    torch.cuda.synchronize()
    assert torch.equal(out_many[0], out_one[0]) and torch.equal(out_many[1], out_one[1])
    assert out_many[1].dtype == torch.bool
    assert_same(many, snapshot(one), "run(7) against 7 frames")
    check_counters(many, "run(7)")
    check_counters(one, "7 frames")
    assert many.frames == 9 and many.updates == 18 and many.epsilon == one.epsilon < 1.0
    if t0 is not None:
        assert not torch.equal(many.fused.t_flat, t0)                        # the soft updates ran
    series = many.stats.series()
    assert same_value(series, one.stats.series())
    assert [w["frames"] for w in series["windows"]] == [2, 4, 6, 8] and series["lost"] == 0
    # and the two go on alike from there, through run(1) and frame()
    out_many, out_one = many.run(1), one.frame()
    torch.cuda.synchronize()
    assert torch.equal(out_many[0], out_one[0]) and torch.equal(out_many[1], out_one[1])
    assert_same(many, snapshot(one), "the frame after")


def test_run_refuses_what_it_cannot_do():
    lr = bdq_learner(True)
    with pytest.raises(ValueError, match="call capture\\(\\) first"):
        lr.run(3)
    lr.capture()
    with pytest.raises(ValueError, match="k must be >= 1"):
        lr.run(0)
    assert lr.frames == 2
