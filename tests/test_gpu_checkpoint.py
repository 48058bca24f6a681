"""Checkpoint and resume of a training run on the GPU (``learner.save`` / ``learner.load``,
pbn_rl_amd/checkpoint.py; DESIGN.md "Checkpoint and resume").

The protocol of every case: learner A runs F1 frames, saves, runs F2 more and is snapshot.  Learner B
is built from scratch -- a new env, new learner objects, other initial weights, the env reset under
another seed -- loads, runs F2 frames and must equal A in every field a frame writes (images and
``last_loss`` included), the trees, the statistics and the curriculum table, the ``(reward, done)`` of
each of the F2 frames, every host mirror, and in its device counters against those mirrors.  Every
comparison is exact.

A is saved from an eager or a captured learner; B resumes eager, captured after the load
(``capture()`` then runs no eager frame), or "inplace": B is captured and has run frames of its own
before it loads, and is not captured again.  A captured frame holds the env's seed and the base of its
step index as launch arguments, so an inplace B is built with A's seed and one reset (it then differs
from A in its weights and in the five frames it has run), and the refusal of another seed is a case
of its own.

DDQN-PER: total_frames 16, exploration_fraction 0.5, beta_fraction 0.75, target_update 4, F1 = 6,
F2 = 10: target copies after frames 3 | 7, 11, 15, epsilon still moving at the checkpoint, beta
reaching 1 after it.  BDQ: pbn28, batch 16, learning_starts 16, updates_per_frame 2, target_update 6,
F1 = 5, F2 = 7: soft updates at updates 6 | 12, 18, 24.  The PyTorch-update BDQ case has batch 32
(``pbn_replay_batch`` gathers multiples of 32)."""
import functools
import os
import tempfile

import pytest
import torch

from pbn_rl_amd import checkpoint
from tests.checkpoint_cases import (CAP, assert_same, bdq_learner, check_counters, ddqn_learner, pointers, same_value,
                                    snapshot)

pytestmark = pytest.mark.gpu

DDQN_SHAPES = {"pbn28": ("pbn28", ((50, 50),), 64, 0), "pbn28-settle64": ("pbn28", ((50, 50),), 64, 64),
               "pbn70": ("pbn70", ((64, 64),), 16, 0)}
BDQ_KINDS = {"uniform": dict(), "per": dict(prioritised=True), "pytorch": dict(fused=False)}
PAIRS = [("eager", "eager"), ("eager", "captured"), ("captured", "captured"), ("captured", "inplace"),
         ("captured", "eager"), ("eager", "inplace")]

_DIR = tempfile.TemporaryDirectory(prefix="pbn_ckpt_")


def _make(agent, kind, graphable, stats=False, **kw):
    if agent == "ddqn":
        return ddqn_learner(*DDQN_SHAPES[kind], graphable, stats=stats, **kw), 6, 10
    return bdq_learner(graphable, stats=stats, **BDQ_KINDS[kind], **kw), 5, 7


def _readings(lr):
    if lr.stats is None:
        return None
    out = {"series": lr.stats.series(), "pairs": lr.stats.pairs(), "window": lr.stats.window()}
    if lr.curriculum is not None:
        out["weights"] = lr.curriculum.weights()
    return out


@functools.lru_cache(maxsize=None)
def _run_a(agent, kind, captured, stats=False):
    """Learner A, once per configuration: the checkpoint's path, the F2 frames' outputs, the end."""
    lr, f1, f2 = _make(agent, kind, captured, stats)
    if captured:
        lr.capture()
        assert lr.frames == 2
    while lr.frames < f1:
        lr.frame()
        if stats and lr.frames == 3:
            lr.stats.window()                      # once before the save: the baseline is part of the run
    path = os.path.join(_DIR.name, f"{agent}-{kind}-{captured}-{stats}.npz")
    lr.save(path)
    at_save = snapshot(lr)
    outs = []
    for _ in range(f2):
        r, d = lr.frame()
        outs.append((r.clone(), d.clone()))
    return {"path": path, "outs": outs, "end": snapshot(lr), "at_save": at_save, "readings": _readings(lr),
            "idx": lr._idx.clone() if agent == "bdq" and lr._predraws() else None}


def _resume(agent, kind, src, dst, stats=False):
    a = _run_a(agent, kind, src == "captured", stats)
    inplace = dst == "inplace"
    b, f1, f2 = _make(agent, kind, dst != "eager", stats, other=True, other_env=not inplace)
    if inplace:
        b.capture()
        for _ in range(3):
            b.frame()
        graph, ptrs = b._graph, pointers(b)
    else:
        b.frame()                                  # (a frame of its own: Adam state, a loss, a ring row)
    b.load(a["path"])
    assert_same(b, a["at_save"], "after load", skip=("actions", "prio"))   # (outputs the next frame rewrites)
    if inplace:
        assert b._graph is graph and pointers(b) == ptrs          # not captured again, nothing rebound
    elif dst == "captured":
        frames = b.frames
        b.capture()
        assert b.frames == frames == f1 and b._graph is not None  # zero warm-up frames
    check_counters(b, "after load")
    for f, (r, d) in enumerate(a["outs"]):
        rb, db = b.frame()
        torch.cuda.synchronize()
        assert rb.dtype == r.dtype and db.dtype == torch.bool
        assert torch.equal(rb, r) and torch.equal(db, d), (f, "reward, done")
    assert_same(b, a["end"], "the end")
    check_counters(b, "the end")
    if a["idx"] is not None and (src == "captured") == (dst != "eager"):
        assert torch.equal(b._idx, a["idx"])                      # the pre-drawn rows, where both hold the same frame's
    return a, b


@pytest.mark.parametrize("src,dst", PAIRS, ids=[f"{s}-{d}" for s, d in PAIRS])
def test_ddqn_resumes_bit_equal(src, dst):
    a, b = _resume("ddqn", "pbn28", src, dst)
    m = a["end"]["mirrors"]
    assert m["syncs"] == [3, 7, 11, 15] and m["beta"] == 1 and m["replay.size"] == CAP
    s = a["at_save"]["mirrors"]
    assert s["syncs"] == [3] and s["epsilon"] > 0.05 and s["beta"] < 1 and s["replay.pos"] < 96    # (the ring wrapped)


@pytest.mark.parametrize("kind", ["pbn28-settle64", "pbn70"])
@pytest.mark.parametrize("src,dst", [("eager", "captured"), ("captured", "inplace")])
def test_ddqn_other_shapes_resume_bit_equal(kind, src, dst):
    _, b = _resume("ddqn", kind, src, dst)
    assert (b._tgt_prev is not None) == (kind == "pbn28-settle64")          # the store_at path and its carried targets


@pytest.mark.parametrize("src,dst", PAIRS, ids=[f"{s}-{d}" for s, d in PAIRS])
def test_bdq_fused_uniform_resumes_bit_equal(src, dst):
    a, b = _resume("bdq", "uniform", src, dst)
    assert a["at_save"]["mirrors"]["updates"] == 10 and a["end"]["mirrors"]["updates"] == 24
    assert a["at_save"]["mirrors"]["draws"] == 5 and 0 < a["at_save"]["mirrors"]["epsilon"] < 1


@pytest.mark.parametrize("kind,src,dst", [("per", "eager", "captured"), ("per", "captured", "inplace"),
                                          ("pytorch", "eager", "eager"), ("pytorch", "captured", "inplace")])
def test_bdq_prioritised_and_pytorch_update_resume_bit_equal(kind, src, dst):
    a, b = _resume("bdq", kind, src, dst)
    assert (b.opt is not None) == (kind == "pytorch")
    if kind == "per":
        assert 0.4 < a["at_save"]["mirrors"]["replay.beta"] < a["end"]["mirrors"]["replay.beta"] == 1.0


def test_pytorch_update_warms_up_again_before_a_capture():
    """The PyTorch update's capture needs this process's autograd and BLAS workspaces initialised:
    after a load, capture() runs its ``min_updates`` of eager frames all the same, and the run goes on.
    (No field is compared here: the PyTorch update's eager and captured frames differ by GEMM rounding,
    with or without a checkpoint -- tests/test_gpu_per.py -- so its bit-equal cases above stay in one mode.)"""
    a = _run_a("bdq", "pytorch", False)
    b, f1, f2 = _make("bdq", "pytorch", True, other=True)
    b.load(a["path"])
    b.capture()
    assert b.frames == f1 + 2 and b.updates == 2 * (f1 + 2) and b._graph is not None
    b.frame()
    check_counters(b, "a replayed frame")
    assert b.frames == f1 + 3 and bool(torch.isfinite(b.last_loss))


@pytest.mark.parametrize("agent,kind,src,dst", [("ddqn", "pbn28", "eager", "captured"),
                                                ("bdq", "uniform", "captured", "inplace")])
def test_statistics_and_curriculum_resume(agent, kind, src, dst):
    a, b = _resume(agent, kind, src, dst, stats=True)
    got = _readings(b)
    for k, want in a["readings"].items():
        assert same_value(got[k], want), k
    # window() reports what happened after the checkpoint's own last window() (frame 3), not since B was built
    assert a["readings"]["window"]["frames"] == a["end"]["mirrors"]["frames"] - 3
    assert a["readings"]["window"]["episodes"] > 0 and len(a["readings"]["series"]["windows"]) == a["end"]["mirrors"]["frames"] // 2
    assert a["end"]["fields"]["curriculum.table_t"].ne(a["at_save"]["fields"]["curriculum.table_t"]).any()


# ------------------------------------------------------------------------------------ refusals
def _state(lr):
    torch.cuda.synchronize()
    return lr.state_dict()


def _assert_untouched(lr, before):
    after = _state(lr)
    assert before.keys() == after.keys()
    for k, v in before.items():
        assert torch.equal(v, after[k]) if isinstance(v, torch.Tensor) else v == after[k], k


REFUSALS = {
    "network": (lambda: ddqn_learner("pbn70", ((64, 64),), 16, 0, False, other=True), r"network \(file 'pbn28', learner 'pbn70'\)"),
    "n_alloc": (lambda: ddqn_learner(*DDQN_SHAPES["pbn28"], False, other=True, n_envs=64), r"n_alloc \(file 96, learner 64\)"),
    "capacity": (lambda: ddqn_learner(*DDQN_SHAPES["pbn28"], False, other=True, capacity=512), r"capacity \(file 256, learner 512\)"),
    "net_arch": (lambda: ddqn_learner("pbn28", ((32, 32),), 64, 0, False, other=True), r"net_arch \(file \[\[50, 50\]\], learner \[\[32, 32\]\]\)"),
    "agent": (lambda: bdq_learner(False, other=True), r"agent \(the file was written by a 'ddqn' learner, this one is 'bdq'\)"),
    "prioritised": (lambda: ddqn_learner(*DDQN_SHAPES["pbn28"], False, other=True, prioritised=False), r"prioritised \(file True, learner False\)"),
}


@pytest.mark.parametrize("field", list(REFUSALS))
def test_load_refuses_a_mismatch_and_writes_nothing(field):
    a = _run_a("ddqn", "pbn28", False)
    make, message = REFUSALS[field]
    b = make()
    b.frame()
    before = _state(b)
    with pytest.raises(ValueError, match="checkpoint mismatch: .*" + message):
        b.load(a["path"])
    _assert_untouched(b, before)


def test_load_refuses_a_truncated_file_and_a_captured_frame_of_another_seed():
    a = _run_a("ddqn", "pbn28", False)
    header = checkpoint.read_header(a["path"])
    assert header["fingerprint"]["network"] == "pbn28" and header["fingerprint"]["n_alloc"] == 96
    assert header["host"]["learner.frames"] == 6 and header["host"]["learner.captured"] is False
    whole = open(a["path"], "rb").read()
    torn = os.path.join(_DIR.name, "torn.npz")
    with open(torn, "wb") as f:
        f.write(whole[: len(whole) * 3 // 4])
    b = ddqn_learner(*DDQN_SHAPES["pbn28"], True, other=True)          # (its env reset under another seed)
    b.capture()
    b.frame()
    before = _state(b)
    with pytest.raises(ValueError, match="unreadable checkpoint"):
        b.load(torn)
    _assert_untouched(b, before)
    with pytest.raises(ValueError, match=r"checkpoint mismatch: env.seed \(file 23, learner 99\).*launch argument"):
        b.load(a["path"])
    _assert_untouched(b, before)
    # and a checkpoint from before every frame learns does not go into a captured frame
    early = ddqn_learner(*DDQN_SHAPES["pbn28"], False)         # (no frame yet: frame 0 does not learn)
    path = os.path.join(_DIR.name, "early.npz")
    early.save(path)
    c = ddqn_learner(*DDQN_SHAPES["pbn28"], True, other=True, other_env=False)
    c.capture()
    before = _state(c)
    with pytest.raises(ValueError, match="before every frame learns"):
        c.load(path)
    _assert_untouched(c, before)
