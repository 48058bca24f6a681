"""The DDQN / DDQNPER agent without a GPU: the DQN module and ``ddqn_update`` against the reference's
own update (tests/golden/ddqn_update.npz, tools/gen_ddqn_golden.py), the learner's schedules on a
stub env, ``ddqn_fused_supported``, and the new entry points' argument checks."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from pbn_rl_amd import _lib
from pbn_rl_amd.ddqn import DQN, DDQNLearner, ddqn_fused_supported, ddqn_update, dqn_layout, load_ddqn_checkpoint
from tests.golden_parts import load_parts

GOLD = os.path.join(os.path.dirname(__file__), "golden", "ddqn_update.npz")
SHAPES = [("s7", 7, 16), ("s28", 28, 64)]


@pytest.fixture(scope="module")
def gold():
    return load_parts(GOLD)


def nets_from(d, prefix, N):
    arch = [tuple(int(x) for x in a) for a in d[prefix + ".arch"]]
    names = [str(n) for n in d[prefix + ".names"]]
    q, t = DQN(N, N + 1, arch), DQN(N, N + 1, arch)
    q.load_state_dict({n: torch.from_numpy(d[f"{prefix}.q0.{n}"]) for n in names})
    t.load_state_dict({n: torch.from_numpy(d[f"{prefix}.t0.{n}"]) for n in names})
    return q, t, names


def batch_of(d, prefix):
    p = prefix + ".b."
    f32 = lambda k: torch.from_numpy(d[p + k].astype(np.float32))  # noqa: E731
    return {"state": f32("states"), "target": f32("targets"), "next_state": f32("next_states"),
            "action": torch.from_numpy(d[p + "actions"]).long().reshape(-1, 1), "reward": f32("rewards").reshape(-1, 1),
            "done": f32("done").reshape(-1, 1)}


def test_fixture_is_the_reference_methods(gold):
    assert tuple(gold["lines.DDQN._get_loss"]) == (218, 256)
    assert tuple(gold["lines.DDQN._back_propagate"]) == (258, 270)
    assert tuple(gold["lines.DDQNPER._learn_step"]) == (468, 486)
    for prefix, _, B in SHAPES:   # both sides of the clip are in the fixture
        for tag in ("ddqn", "per"):
            assert float(gold[f"{prefix}.{tag}_a.norm"]) < float(gold[f"{prefix}.{tag}_a.max_grad_norm"])
            assert float(gold[f"{prefix}.{tag}_b.norm"]) > float(gold[f"{prefix}.{tag}_b.max_grad_norm"])


@pytest.mark.parametrize("prefix,N,B", SHAPES)
def test_dqn_matches_the_reference_module(gold, prefix, N, B):
    q, _, names = nets_from(gold, prefix, N)
    assert list(q.state_dict().keys()) == names
    for n, p in q.state_dict().items():
        assert tuple(p.shape) == gold[f"{prefix}.q0.{n}"].shape
    b = batch_of(gold, prefix)
    with torch.no_grad():
        out = q(b["state"], b["target"]).numpy()
    np.testing.assert_allclose(out, gold[prefix + ".forward"], rtol=1e-6, atol=0)
    # one (state, target) pair, as DDQN._get_learned_action calls it: torch sums a single row in
    # another order than a batch's, so outputs of O(0.1) terms agree to a few fp32 ulps of those terms
    with torch.no_grad():
        one = q(b["state"][0], b["target"][0]).numpy()
    np.testing.assert_allclose(one, gold[prefix + ".forward"][0], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("call", ["ddqn_a", "ddqn_b", "per_a", "per_b"])
@pytest.mark.parametrize("prefix,N,B", SHAPES)
def test_ddqn_update_matches_the_reference_learn_step(gold, prefix, N, B, call):
    d = gold
    q, t, _ = nets_from(d, prefix, N)
    opt = torch.optim.Adam(q.parameters(), lr=float(d["lr"]))
    key = f"{prefix}.{call}"
    per = call.startswith("per")
    w = torch.from_numpy(d[prefix + ".b.weights"]) if per else None
    prio = torch.empty(B) if per else None
    loss, norm = ddqn_update(q, t, opt, batch_of(d, prefix), float(d["gamma"]), float(d[key + ".max_grad_norm"]),
                             weights=w, priorities_out=prio, replay_constant=float(d["replay_constant"]))
    assert abs(float(loss) - float(d[key + ".loss"])) <= 1e-5 * abs(float(d[key + ".loss"]))
    assert abs(float(norm) - float(d[key + ".norm"])) <= 1e-5 * float(d[key + ".norm"])
    if per:
        np.testing.assert_allclose(prio.numpy(), d[key + ".priorities"], rtol=1e-5, atol=0)
    rtol, atol = (1e-5, 1e-7) if N == 7 else (1e-4, 1e-6)
    for n, p in q.named_parameters():
        g = torch.from_numpy(d[f"{key}.g.{n}"])
        assert torch.allclose(p.grad, g, rtol=rtol, atol=atol), (n, (p.grad - g).abs().max().item())
        after = torch.from_numpy(d[f"{key}.q1.{n}"])
        assert torch.allclose(p.detach(), after, rtol=0, atol=1e-5), (n, (p.detach() - after).abs().max().item())


def test_ddqn_update_rejects_priorities_without_weights(gold):
    q, t, _ = nets_from(gold, "s7", 7)
    with pytest.raises(ValueError, match="priorities_out needs weights"):
        ddqn_update(q, t, torch.optim.Adam(q.parameters()), batch_of(gold, "s7"), 0.9, 10.0, priorities_out=torch.empty(16))


class StubEnv:
    """What DDQNLearner reads of a VectorPBNEnv, on the CPU: 32 envs of 7 nodes whose step flips the
    masked bits and terminates every fifth env."""

    def __init__(self):
        self.device = torch.device("cpu")
        self.n_nodes, self.words, self.num_envs, self.n_alloc = 7, 1, 32, 32
        self.keep_final_state = True
        self.spec = types.SimpleNamespace(n=7, attractors=[[(1, 0, 1, 0, 1, 0, 1)], [(0, 0, 0, 0, 0, 0, 0)]])
        self.state = torch.arange(32, dtype=torch.int32).reshape(1, 32)
        self.flipmask = torch.zeros(1, 32, dtype=torch.int32)
        self.final_state = torch.zeros(1, 32, dtype=torch.int32)
        self.target = (torch.arange(32) % 2).to(torch.uint8)
        self.reward = torch.zeros(32)
        self.flags = torch.zeros(32, dtype=torch.uint8)
        self.steps = 0

    def step_flipmask(self, use_current=False):
        assert use_current
        self.state = self.state ^ self.flipmask
        self.final_state = self.state.clone()
        self.steps += 1
        self.reward = -torch.ones(32)
        self.flags = ((torch.arange(32) + self.steps) % 5 == 0).to(torch.uint8) * 1 + \
                     ((torch.arange(32) + self.steps) % 7 == 0).to(torch.uint8) * 2
        return self.state, self.reward, self.flags


def test_learner_schedules_follow_the_closed_forms():
    """epsilon, beta and the target-sync frames of _schedule_step for total_frames 40, target_update 8,
    exploration_fraction 0.5, beta_fraction 0.75, on a stub env."""
    env = StubEnv()
    torch.manual_seed(0)
    lr = DDQNLearner(env, net_arch=[(8, 8)], total_frames=40, capacity=256, batch_size=16, target_update=8,
                     exploration_fraction=0.5, beta_fraction=0.75, prioritised=False, fused=False, seed=3)
    assert lr.fused is None and lr.epsilon == 1.0 and lr.beta == 0.4
    eps, beta = 1.0, 0.4
    for f in range(40):
        assert lr.epsilon == pytest.approx(max(0.05, 1.0 - f * 0.95 / 20.0), abs=1e-12)
        assert lr.beta == pytest.approx(min(1.0, 0.4 + f * 0.6 / 30.0), abs=1e-12)
        assert lr.epsilon == eps and lr.beta == beta
        stored_done = None
        pos = lr.replay.pos
        lr.frame()
        # done = TERMINATED only
        stored_done = lr.replay.done[pos:pos + 32]
        assert torch.equal(stored_done, (env.flags & 1))
        same = all(torch.equal(a, b) for a, b in zip(lr.target.state_dict().values(), lr.q.state_dict().values()))
        assert same == ((f + 1) % 8 == 0 or lr.updates == 0), f
        eps = max(0.05, eps - 0.95 / (0.5 * 40))
        beta = min(beta + 0.6 / (0.75 * 40), 1)
    assert lr.syncs == [7, 15, 23, 31, 39]
    assert lr.epsilon == 0.05 and lr.beta == 1
    assert lr.frames == 40 and lr.updates == 39      # frames 1..39: num_timesteps > learning_starts = 0
    assert lr.replay.size == 256 and torch.isfinite(lr.last_loss)


def test_learner_refuses_what_cannot_work():
    env = StubEnv()
    with pytest.raises(ValueError, match="prioritised replay runs on the GPU"):
        DDQNLearner(env, net_arch=[(8, 8)], total_frames=10, capacity=64, prioritised=True)
    with pytest.raises(ValueError, match="fused update"):
        DDQNLearner(env, net_arch=[(8, 8)], total_frames=10, capacity=64, prioritised=False, fused=True)


def test_fused_supported():
    assert ddqn_fused_supported(28, [(50, 50)], 64)
    assert ddqn_fused_supported(7, [(8, 8)], 16)
    assert ddqn_fused_supported(7, [(20, 40)], 16)
    assert ddqn_fused_supported(127, [(64, 64)], 1024)
    assert not ddqn_fused_supported(28, [(50, 50), (50, 50)], 64)     # two hidden Linears
    assert not ddqn_fused_supported(28, [(65, 50)], 64)
    assert not ddqn_fused_supported(28, [(50, 65)], 64)
    assert not ddqn_fused_supported(128, [(50, 50)], 64)              # N + 1 = 129 actions
    assert not ddqn_fused_supported(28, [(50, 50)], 24)               # not a multiple of 16
    assert not ddqn_fused_supported(28, [(50, 50)], 1040)


def test_layout_is_aligned_and_ordered():
    off = dqn_layout(28, 50, 50)
    sizes = [50 * 28 * 28, 50, 50 * 50, 50, 29 * 50, 29]
    assert off[0] == 0 and all(o % 16 == 0 for o in off)
    for s in range(6):
        assert off[s + 1] == off[s] + (sizes[s] + 15) // 16 * 16


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _err(lib):
    return lib.pbn_last_error().decode()


def test_entry_points_reject_bad_arguments_before_the_device(lib):
    off = (ctypes.c_int64 * 7)()
    n = ctypes.c_int64()
    assert lib.pbn_dqn_layout(128, 50, 50, off) == -22 and "n_nodes must be 1..127" in _err(lib)
    assert lib.pbn_dqn_layout(28, 65, 50, off) == -22 and "hidden widths must be 1..64" in _err(lib)
    assert lib.pbn_dqn_layout(28, 50, 50, None) == -22 and "null offsets" in _err(lib)
    assert lib.pbn_ddqn_learn_workspace(28, 50, 50, 24, ctypes.byref(n)) == -22
    assert "batch must be a multiple of 16 in 16..1024" in _err(lib)
    assert lib.pbn_ddqn_learn_workspace(28, 50, 0, 64, ctypes.byref(n)) == -22 and "hidden widths" in _err(lib)
    assert lib.pbn_ddqn_learn_workspace(28, 50, 50, 64, ctypes.byref(n)) == 0 and n.value > 0
    # a null net
    assert lib.pbn_dqn_image_floats(None, 50, 50, ctypes.byref(n)) == -22
    assert lib.pbn_dqn_pack(None, 50, 50, None, None, None) == -22
    assert lib.pbn_dqn_flipmask_from_state(None, 0, 0, None, 0, 32, None, None, 50, 50, None, 0.0, None, None, None,
                                           None, None) == -22
    assert lib.pbn_dqn_flipmask_from_state(None, 0, 0, None, 0, 48, None, None, 50, 50, None, 0.0, None, None, None,
                                           None, None) == -22
    assert "multiples of 32" in _err(lib)
    assert lib.pbn_dqn_flipmask_from_state(None, 0, 0, None, 0, 32, None, None, 50, 50, None, 1.5, None, None, None,
                                           None, None) == -22
    assert "epsilon must be in [0, 1]" in _err(lib)
    learn = lambda batch, w, p: lib.pbn_ddqn_learn(  # noqa: E731
        None, 50, 50, batch, None, 1024, None, None, None, None, None, None, None, None, None, None, None, None,
        1e-4, 0.9, 0.999, 1e-8, 0.95, 10.0, None, 0, None, None, None, w, 1e-5, p, None)
    assert learn(64, None, None) == -22                                  # (the null net)
    assert learn(24, None, None) == -22 and "batch must be a multiple of 16" in _err(lib)
    assert learn(64, 64, None) == -22 and "d_weights and d_priority come together" in _err(lib)
    assert learn(64, None, 64) == -22 and "d_weights and d_priority come together" in _err(lib)
    assert learn(64, 66, 64) == -22 and "4-byte aligned" in _err(lib)


def test_load_ddqn_checkpoint_reads_an_export(tmp_path, gold):
    q, _, names = nets_from(gold, "s7", 7)
    path = tmp_path / "ddqn_7.npz"
    np.savez(path, net_arch=np.array([(8, 8)]), input_size=np.int64(7), output_size=np.int64(8),
             **{"params." + n: p.numpy() for n, p in q.state_dict().items()})
    got = load_ddqn_checkpoint(str(path))
    assert list(got.state_dict().keys()) == names
    for n, p in got.state_dict().items():
        assert torch.equal(p, q.state_dict()[n])
