"""Checkpoints without a GPU (pbn_rl_amd/checkpoint.py): the file (dtypes, ``allow_pickle=False``, the
atomic write), the header and every refusal's message, ``DeviceReplay``'s in-place round trip, a whole
DDQNLearner resumed on a CPU stub env, and the two reference-format writers' key sets.

Every comparison is exact: a resumed run computes what the uninterrupted one computes."""
import copy
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from pbn_rl_amd import checkpoint
from pbn_rl_amd.agent import BranchingQNetwork, load_bdq_checkpoint
from pbn_rl_amd.ddqn import DQN, DDQNLearner
from pbn_rl_amd.replay import DeviceReplay

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

ARRAYS = {"tree": np.array([0.1, float("inf"), 2.0 ** -60], dtype=np.float64),
          "counter": np.array([2 ** 40 + 3], dtype=np.int64),
          "flags": np.array([0, 1, 255], dtype=np.uint8),
          "words": np.array([[-1, 2 ** 31 - 1]], dtype=np.int32),
          "reward": np.array([np.float32(0.1), -np.float32(5)], dtype=np.float32)}
HEADER = {"format": checkpoint.FORMAT, "version": checkpoint.FORMAT_VERSION, "fingerprint": {"agent": "ddqn"},
          "host": {"learner.epsilon": 0.1 + 0.2, "learner.frames": 7, "learner.syncs": [3, 7], "learner.last_beta": None,
                   "env.seed": 2 ** 64 - 1}}


# ------------------------------------------------------------------------------------ the file
def test_file_round_trip_keeps_dtypes_and_needs_no_pickle(tmp_path):
    path = tmp_path / "ckpt.npz"
    checkpoint.write_checkpoint(str(path), HEADER, ARRAYS)
    assert os.listdir(tmp_path) == ["ckpt.npz"]                       # the temporary file is gone
    with np.load(path, allow_pickle=False) as z:                      # plain numpy reads it, nothing executed
        assert sorted(z.files) == sorted(list(ARRAYS) + ["header"])
        for k, a in ARRAYS.items():
            assert z[k].dtype == a.dtype and z[k].shape == a.shape and np.array_equal(z[k], a), k
    import zipfile
    with zipfile.ZipFile(path) as z:                                  # uncompressed
        assert all(i.compress_type == zipfile.ZIP_STORED for i in z.infolist())
    header, arrays = checkpoint.read_checkpoint(str(path))
    assert header == HEADER                                           # floats and big ints exactly, None kept
    assert header["host"]["learner.epsilon"] == 0.1 + 0.2 and header["host"]["env.seed"] == 2 ** 64 - 1
    assert set(arrays) == set(ARRAYS)
    assert checkpoint.read_header(str(path)) == HEADER


def test_write_is_atomic(tmp_path, monkeypatch):
    path = tmp_path / "ckpt.npz"
    checkpoint.write_checkpoint(str(path), HEADER, ARRAYS)
    before = path.read_bytes()
    real = np.savez

    def torn(f, **arrays):
        real(f, **{k: arrays[k] for k in list(arrays)[:2]})           # part of the file is on disk
        raise RuntimeError("killed mid-write")

    monkeypatch.setattr(np, "savez", torn)
    with pytest.raises(RuntimeError, match="killed mid-write"):
        checkpoint.write_checkpoint(str(path), HEADER, {**ARRAYS, "more": np.zeros(4)})
    assert path.read_bytes() == before                                # the existing checkpoint survives
    assert os.listdir(tmp_path) == ["ckpt.npz"]                       # and nothing else is left
    with pytest.raises(ValueError, match="may not be named 'header'"):
        checkpoint.write_checkpoint(str(path), HEADER, {"header": np.zeros(1)})


def test_read_refuses_what_is_not_a_checkpoint(tmp_path):
    path = tmp_path / "ckpt.npz"
    checkpoint.write_checkpoint(str(path), HEADER, ARRAYS)
    whole = path.read_bytes()
    torn = tmp_path / "torn.npz"
    torn.write_bytes(whole[: len(whole) // 2])
    for read in (checkpoint.read_header, checkpoint.read_checkpoint):
        with pytest.raises(ValueError, match="unreadable checkpoint"):
            read(str(torn))
    other = tmp_path / "other.npz"
    np.savez(other, a=np.zeros(3))
    with pytest.raises(ValueError, match="no 'header' array"):
        checkpoint.read_header(str(other))
    checkpoint.write_checkpoint(str(other), {**HEADER, "version": 99}, ARRAYS)
    with pytest.raises(ValueError, match="format version 99"):
        checkpoint.read_header(str(other))
    checkpoint.write_checkpoint(str(other), {**HEADER, "format": "something"}, ARRAYS)
    with pytest.raises(ValueError, match="format 'something'"):
        checkpoint.read_checkpoint(str(other))


def test_latest_goes_by_frame_number(tmp_path):
    assert checkpoint.latest(str(tmp_path)) is None and checkpoint.latest(str(tmp_path / "absent")) is None
    for f in (900, 12000, 5):
        (tmp_path / checkpoint.checkpoint_name(f)).write_bytes(b"")
    (tmp_path / "ckpt_final.npz").write_bytes(b"")
    assert checkpoint.latest(str(tmp_path)) == str(tmp_path / checkpoint.checkpoint_name(12000))


# ------------------------------------------------------------------------------------ the fingerprint
def test_fingerprint_mismatch_names_every_field():
    own = {k: 1 for k in checkpoint.FIELDS}
    own.update(agent="ddqn", network="pbn28", net_arch=[[50, 50]], fused=True, prioritised=True, episode_stats=False,
               curriculum=False)
    checkpoint.check_fingerprint(dict(own), own)
    for field, other in (("network", "pbn70"), ("table_hash", "x"), ("n_attractors", 3), ("num_envs", 64),
                         ("n_alloc", 64), ("words", 3), ("capacity", 512), ("batch_size", 16), ("branches", 3),
                         ("net_arch", [[32, 32]]), ("fused", False), ("prioritised", False), ("episode_stats", True),
                         ("curriculum", True), ("settle", 64), ("seed", 9), ("abi_version", 0)):
        with pytest.raises(ValueError, match=rf"checkpoint mismatch: {field} \(file .*, learner .*\)"):
            checkpoint.check_fingerprint({**own, field: other}, own)
    with pytest.raises(ValueError, match=r"num_envs \(file 64, learner 1\); n_alloc \(file 64, learner 1\)"):
        checkpoint.check_fingerprint({**own, "num_envs": 64, "n_alloc": 64}, own)
    with pytest.raises(ValueError, match="checkpoint mismatch: agent .*'bdq' learner, this one is 'ddqn'"):
        checkpoint.check_fingerprint({**own, "agent": "bdq", "branches": 3}, own)


# ------------------------------------------------------------------------------------ DeviceReplay
def test_device_replay_round_trip_is_in_place():
    g = torch.Generator().manual_seed(1)
    a, b = DeviceReplay(64, 2, 3, "cpu"), DeviceReplay(64, 2, 3, "cpu")
    for _ in range(3):      # 72 rows: the ring wraps
        n = 24
        a.store(torch.randint(-2 ** 31, 2 ** 31 - 1, (2, n), generator=g, dtype=torch.int32),
                torch.randint(0, 4, (n,), generator=g), torch.randint(0, 9, (n, 3), generator=g),
                torch.randn(n, generator=g), torch.randint(0, 99, (2, n), generator=g, dtype=torch.int32),
                torch.randint(0, 2, (n,), generator=g))
    sd = a.state_dict()
    assert sd["pos"] == 8 and sd["size"] == 64
    assert {k: v.dtype for k, v in sd.items() if isinstance(v, torch.Tensor)} == {
        "state": torch.int32, "next_state": torch.int32, "target": torch.uint8, "action": torch.int32,
        "reward": torch.float32, "done": torch.uint8}
    assert all(sd[k].data_ptr() != getattr(a, k).data_ptr() for k in DeviceReplay._STATE_TENSORS)   # copies
    ptrs = {k: getattr(b, k).data_ptr() for k in DeviceReplay._STATE_TENSORS}
    b.load_state_dict(sd)
    assert {k: getattr(b, k).data_ptr() for k in DeviceReplay._STATE_TENSORS} == ptrs                # in place
    assert (b.pos, b.size) == (8, 64)
    for k in DeviceReplay._STATE_TENSORS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k


# ------------------------------------------------------------------------------------ a whole learner
class StubEnv:
    """What DDQNLearner and a checkpoint read of a VectorPBNEnv, on the CPU: 32 envs of 7 nodes whose
    step flips the masked bits, terminates every fifth env and truncates every seventh."""

    def __init__(self, start=0):
        self.device = torch.device("cpu")
        self.n_nodes, self.words, self.num_envs, self.n_alloc = 7, 1, 32, 32
        self.keep_final_state = True
        self.spec = types.SimpleNamespace(n=7, attractors=[[(1, 0, 1, 0, 1, 0, 1)], [(0, 0, 0, 0, 0, 0, 0)]])
        self.state = (torch.arange(32, dtype=torch.int32).reshape(1, 32) + start) % 128
        self.flipmask = torch.zeros(1, 32, dtype=torch.int32)
        self.final_state = torch.zeros(1, 32, dtype=torch.int32)
        self.target = ((torch.arange(32) + start) % 2).to(torch.uint8)
        self.reward = torch.zeros(32)
        self.flags = torch.zeros(32, dtype=torch.uint8)
        self.step_index = start

    def step_flipmask(self, use_current=False):
        assert use_current
        self.state = self.state ^ self.flipmask
        self.final_state = self.state.clone()
        self.step_index += 1
        k = torch.arange(32) + self.step_index
        self.reward = -(k % 3).to(torch.float32)
        self.flags = (k % 5 == 0).to(torch.uint8) * 1 + (k % 7 == 0).to(torch.uint8) * 2
        return self.state, self.reward, self.flags

    _TENSORS = ("state", "flipmask", "final_state", "target", "reward", "flags")

    def state_dict(self):
        return {**{k: getattr(self, k).clone() for k in self._TENSORS}, "step_index": self.step_index}

    def load_state_dict(self, sd):
        for k in self._TENSORS:
            setattr(self, k, sd[k].clone())
        self.step_index = int(sd["step_index"])


def _stub_learner(weights_seed, start=0, **kw):
    torch.manual_seed(weights_seed)
    args = dict(net_arch=[(8, 8)], total_frames=40, capacity=256, batch_size=16, target_update=8,
                exploration_fraction=0.5, beta_fraction=0.75, prioritised=False, fused=False, seed=3)
    args.update(kw)
    return DDQNLearner(StubEnv(start), **args)


def _assert_same_run(a, b):
    for (k, p), (_, r) in zip(a.q.state_dict().items(), b.q.state_dict().items()):
        assert torch.equal(p, r), ("q", k)
    for (k, p), (_, r) in zip(a.target.state_dict().items(), b.target.state_dict().items()):
        assert torch.equal(p, r), ("target", k)
    for (name, p), (_, r) in zip(a.q.named_parameters(), b.q.named_parameters()):
        sa, sb = a.opt.state[p], b.opt.state[r]
        for k in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(sa[k], sb[k]), ("adam", k, name)
    for k in DeviceReplay._STATE_TENSORS:
        assert torch.equal(getattr(a.replay, k), getattr(b.replay, k)), ("ring", k)
    for k in StubEnv._TENSORS:
        assert torch.equal(getattr(a.env, k), getattr(b.env, k)), ("env", k)
    for k in ("frames", "updates", "epsilon", "beta", "last_beta", "syncs"):
        assert getattr(a, k) == getattr(b, k), k
    assert (a.replay.pos, a.replay.size, a.env.step_index) == (b.replay.pos, b.replay.size, b.env.step_index)
    assert int(b._pos_t) == b.replay.pos and int(b._size_t) == b.replay.size
    assert torch.equal(a.gen.get_state(), b.gen.get_state())
    assert torch.equal(a.last_loss, b.last_loss)


def test_ddqn_learner_resumes_on_a_stub_env(tmp_path):
    path = str(tmp_path / "stub.npz")
    a = _stub_learner(0)
    for _ in range(9):
        a.frame()
    a.save(path)
    header = checkpoint.read_header(path)
    assert header["fingerprint"]["agent"] == "ddqn" and header["fingerprint"]["net_arch"] == [[8, 8]]
    assert header["host"]["learner.frames"] == 9 and header["host"]["learner.syncs"] == [7]
    outs_a = [a.frame() for _ in range(11)]
    # the twin: other weights, an env that starts elsewhere, frames of its own behind it
    b = _stub_learner(1, start=5)
    for _ in range(3):
        b.frame()
    ptrs = [p.data_ptr() for p in b.q.parameters()] + [b.replay.state.data_ptr(), b._pos_t.data_ptr()]
    b.load(path)
    assert ptrs == [p.data_ptr() for p in b.q.parameters()] + [b.replay.state.data_ptr(), b._pos_t.data_ptr()]
    assert b.frames == 9 and b.syncs == [7] and b.updates == 8 and b.epsilon == header["host"]["learner.epsilon"]
    for (ra, da) in outs_a:
        rb, db = b.frame()
        assert torch.equal(ra, rb) and torch.equal(da, db)
    _assert_same_run(a, b)
    assert a.syncs == [7, 15] and a.frames == 20 and a.epsilon < 1.0 and 0.4 < a.beta < 1.0
    # saved before the first update (Adam has no state yet), loaded into a learner that has one
    c = _stub_learner(2)
    c.frame()
    assert c.updates == 0
    c.save(path)
    b.load(path)
    for _ in range(4):
        c.frame(), b.frame()
    _assert_same_run(c, b)


def test_ddqn_learner_refuses_before_it_writes(tmp_path):
    path = str(tmp_path / "stub.npz")
    a = _stub_learner(0)
    for _ in range(3):
        a.frame()
    a.save(path)
    for field, kw in (("capacity", dict(capacity=128)), ("batch_size", dict(batch_size=32)),
                      ("net_arch", dict(net_arch=[(8, 12)])), ("seed", dict(seed=4))):
        b = _stub_learner(1, **kw)
        b.frame()
        before = copy.deepcopy(b.state_dict())
        with pytest.raises(ValueError, match=f"checkpoint mismatch: {field} "):
            b.load(path)
        after = b.state_dict()
        assert before.keys() == after.keys()
        for k, v in before.items():
            assert torch.equal(v, after[k]) if isinstance(v, torch.Tensor) else v == after[k], (field, k)
    whole = open(path, "rb").read()
    with open(path, "wb") as f:
        f.write(whole[: len(whole) * 2 // 3])
    b = _stub_learner(1)
    before = copy.deepcopy(b.state_dict())
    with pytest.raises(ValueError, match="unreadable checkpoint"):
        b.load(path)
    after = b.state_dict()
    for k, v in before.items():
        assert torch.equal(v, after[k]) if isinstance(v, torch.Tensor) else v == after[k], k


# ------------------------------------------------------------------------------------ the reference's files
# DDQN._make_save_dict's keys and BranchingDQN.state_dict()'s (q / target: a BranchingQNetwork each), as data
DDQN_SAVE_KEYS = ["params", "policy_kwargs", "input_size", "output_size", "buffer_size", "batch_size", "epsilon",
                  "target_update", "gamma", "max_epsilon", "min_epsilon", "exploration_fraction", "learning_rate",
                  "max_grad_norm", "train_steps", "num_timesteps"]
DQN_PARAMS = ["input.weight", "input.bias", "linears.0.weight", "linears.0.bias", "output.weight", "output.bias"]
BDQ_NET_KEYS = (["model.0.bilinear.weight", "model.0.bilinear.bias"]
                + [f"model.{i}.{p}" for i in (2, 4, 6) for p in ("weight", "bias")]
                + [f"value_head.{i}.{p}" for i in (0, 2) for p in ("weight", "bias")]
                + [f"adv_heads.{h}.{i}.{p}" for h in range(3) for i in (0, 2) for p in ("weight", "bias")])


def test_save_reference_ddqn_has_the_reference_keys(tmp_path):
    assert len(DDQN_SAVE_KEYS) == 16 and list(checkpoint.REFERENCE_DDQN_KEYS) == DDQN_SAVE_KEYS
    lr = _stub_learner(0)
    for _ in range(5):
        lr.frame()
    out = checkpoint.save_reference_ddqn(lr, str(tmp_path))
    assert out == str(tmp_path / "ddqn_5.pt") and os.listdir(tmp_path) == ["ddqn_5.pt"]
    sd = torch.load(out, map_location="cpu", weights_only=True)
    assert list(sd) == DDQN_SAVE_KEYS and list(sd["params"]) == DQN_PARAMS
    assert sd["policy_kwargs"] == {"net_arch": [(8, 8)]} and (sd["input_size"], sd["output_size"]) == (7, 8)
    assert (sd["buffer_size"], sd["batch_size"], sd["target_update"]) == (256, 16, 8)
    assert (sd["num_timesteps"], sd["train_steps"], sd["epsilon"]) == (5, 4, lr.epsilon)
    assert sd["exploration_fraction"] == pytest.approx(0.5, rel=1e-12) and sd["learning_rate"] == 1e-4
    q = DQN(sd["input_size"], sd["output_size"], **sd["policy_kwargs"])
    q.load_state_dict(sd["params"])
    for k, v in lr.q.state_dict().items():
        assert torch.equal(v, q.state_dict()[k]), k


def test_save_reference_bdq_has_the_reference_keys(tmp_path):
    torch.manual_seed(0)
    q, t = BranchingQNetwork((7, 7), 8, 3), BranchingQNetwork((7, 7), 8, 3)
    out = str(tmp_path / "sub" / "bdq_final.pt")
    checkpoint.save_reference_bdq(types.SimpleNamespace(q=q, target=t), out)
    sd = torch.load(out, map_location="cpu", weights_only=True)
    assert list(sd) == ["q." + k for k in BDQ_NET_KEYS] + ["target." + k for k in BDQ_NET_KEYS]
    for prefix, net in (("q.", q), ("target.", t)):
        got = load_bdq_checkpoint(BranchingQNetwork((7, 7), 8, 3), out, prefix=prefix)
        for k, v in net.state_dict().items():
            assert torch.equal(v, got.state_dict()[k]), (prefix, k)


def test_train_tool_is_lint_clean_and_states_its_flags():
    tool = os.path.join(ROOT, "tools", "train.py")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lint_names.py"), tool], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    text = open(tool).read()
    for flag in ("--agent", "--network", "--envs", "--frames", "--chunk", "--seed", "--settle", "--checkpoint-dir",
                 "--checkpoint-every", "--resume", "--no-capture", "--eval-runs", "--save-reference"):
        assert f'"{flag}"' in text, flag
