"""The DDQN-PER learning frame captured in one hipGraph (DDQNLearner.capture / frame / run,
pbn_ddqn_schedule) against the eager frame it replaces.

Every comparison is exact (``torch.equal``, ``==``): the captured frame issues the eager frame's
launches on the same inputs, and csrc/pbn_ddqn.hip reduces in a fixed order without atomics, so any
difference is a bug in the capture.  Settings (all shapes): 96 envs, a 256-row ring (it wraps in
frame 2), total_frames 16 with exploration_fraction 0.5 and beta_fraction 0.75 -- epsilon still moves
when the replays start (frame 2) and reaches its floor in frame 8, beta reaches 1.0 in frame 12 --
and target_update 4: copies fall due after frames 3, 7, 11 and 15.  The envs perturb and truncate
(horizon 6), so the returned ``done`` differs from the stored one.

One field is compared across a frame boundary rather than at equal times.  The eager frame writes
``replay.beta_t`` just before it samples and leaves it there, so after frame f it holds frame f's
beta; the captured frame's schedule launch moves ``beta_t`` on at the end of the frame (that is what
lets replays follow each other without the host), so after frame f it holds frame f + 1's.  Hence:
the captured ``beta_t`` equals the eager learner's host ``beta`` (the value the eager frame f + 1
will write), and the eager ``beta_t`` equals the captured learner's ``last_beta`` -- both exactly."""
import copy
import functools

import pytest
import torch

from pbn_rl_amd.attractors import load_attractors
from pbn_rl_amd.ddqn import DQN, DDQNLearner
from pbn_rl_amd.network import load_network
from pbn_rl_amd.spec import EnvSpec
from pbn_rl_amd.vector_env import VectorPBNEnv

pytestmark = pytest.mark.gpu

N_ENVS, CAP, TOTAL = 96, 256, 16
# (network, net_arch, batch, settle): train_ddqn.py's; the settle law's store_at path; W = 3 state words
SHAPES = [("pbn28", ((50, 50),), 64, 0), ("pbn28", ((50, 50),), 64, 64), ("pbn70", ((64, 64),), 16, 0)]
IDS = ["pbn28", "pbn28-settle64", "pbn70"]
MIRRORS = ("epsilon", "beta", "last_beta", "frames", "updates", "syncs")


@functools.lru_cache(maxsize=None)
def _spec(net, settle):
    return EnvSpec(load_network(net), load_attractors(net), perturbation=0.01, horizon=6, settle=settle)


@functools.lru_cache(maxsize=None)
def _q0(net, arch):
    torch.manual_seed(11)
    n = _spec(net, 0).n
    return DQN(n, n + 1, [tuple(a) for a in arch])


def _learner(net, arch, B, settle, graphable, **kw):
    env = VectorPBNEnv(_spec(net, settle), N_ENVS, seed=23)
    args = dict(net_arch=[tuple(a) for a in arch], total_frames=TOTAL, capacity=CAP, batch_size=B, target_update=4,
                exploration_fraction=0.5, beta_fraction=0.75, prioritised=True, fused=True, seed=5,
                graphable=graphable)
    args.update(kw)
    lr = DDQNLearner(env, copy.deepcopy(_q0(net, arch)), **args)
    env.reset()
    return lr


def _fields(lr):
    """Every device field a frame writes, but ``beta_t`` (the module docstring)."""
    env, rp, fu = lr.env, lr.replay, lr.fused
    return {"env.state": env.state, "env.target": env.target, "env.t": env.t, "env.flags": env.flags,
            "env.reward": env.reward, "env.flipmask": env.flipmask, "actions": lr.agent.actions,
            "ring.state": rp.state, "ring.next_state": rp.next_state, "ring.target": rp.target,
            "ring.action": rp.action, "ring.reward": rp.reward, "ring.done": rp.done,
            "sum_tree": rp.sum_tree, "min_tree": rp.min_tree, "max_priority": rp.max_priority,
            "counter_t": rp.counter_t, "q_flat": fu.q_flat, "t_flat": fu.t_flat, "q_image": fu.q_image,
            "t_image": fu.t_image, "adam.m": fu.m, "adam.v": fu.v, "adam.step": fu.step,
            "last_loss": lr.last_loss.reshape(1) if lr.last_loss is not None else fu.loss.new_zeros(0),
            "prio": lr._prio}


def _snapshot(lr, out):
    torch.cuda.synchronize()
    snap = {k: v.clone() for k, v in _fields(lr).items()}
    snap["beta_t"] = lr.replay.beta_t.clone()
    snap["reward"], snap["done"] = out[0].clone(), out[1].clone()
    snap["host"] = {k: copy.copy(getattr(lr, k)) for k in MIRRORS}
    snap["host"].update({"replay.beta": lr.replay.beta, "replay.pos": lr.replay.pos, "replay.size": lr.replay.size,
                         "env.step_index": lr.env.step_index})
    return snap


@functools.lru_cache(maxsize=None)
def _eager(net, arch, B, settle):
    """The eager learner's state after each of the 16 frames: computed once per shape, then only read."""
    lr = _learner(net, arch, B, settle, graphable=False)
    return [_snapshot(lr, lr.frame()) for _ in range(TOTAL)]


def _assert_equal(lr, out, want, what):
    """A captured learner after a frame against the eager snapshot of the same frame."""
    torch.cuda.synchronize()
    assert out[0].dtype == want["reward"].dtype and out[1].dtype == torch.bool
    assert torch.equal(out[0], want["reward"]), (what, "reward")
    assert torch.equal(out[1], want["done"]), (what, "done")
    for k, v in _fields(lr).items():
        assert torch.equal(v, want[k]), (what, k)
    host = want["host"]
    for k in MIRRORS:
        assert getattr(lr, k) == host[k], (what, k, getattr(lr, k), host[k])
    rp, env = lr.replay, lr.env
    assert (rp.beta, rp.pos, rp.size, env.step_index) == (host["replay.beta"], host["replay.pos"], host["replay.size"],
                                                          host["env.step_index"]), what
    # beta across the frame boundary (the module docstring), exactly
    assert rp.beta_t.dtype == torch.float64
    assert float(rp.beta_t) == float(host["beta"]) == float(lr.beta), (what, "beta_t", float(rp.beta_t), host["beta"])
    assert float(want["beta_t"]) == float(lr.last_beta), (what, "eager beta_t", float(want["beta_t"]), lr.last_beta)
    # the host's mirrors against the device's own values
    assert int(lr._step_t) == env.step_index and int(lr._pos_t) == rp.pos and int(lr._size_t) == rp.size, what
    assert float(lr._eps64) == lr.epsilon, (what, float(lr._eps64), lr.epsilon)
    assert float(lr._eps32) == torch.tensor(lr.epsilon, dtype=torch.float32).item(), what
    assert float(lr.fused.step) == lr.updates and int(rp.counter_t) == lr.updates, what


@pytest.mark.parametrize("net,arch,B,settle", SHAPES, ids=IDS)
def test_captured_frames_equal_eager_frames(net, arch, B, settle):
    eager = _eager(net, arch, B, settle)
    lr = _learner(net, arch, B, settle, graphable=True)
    lr.capture()
    first = lr.frames
    assert first == 2 and lr.updates == 1 and lr._graph is not None      # frames 0, 1 ran eagerly; frame 1 learned
    assert eager[first]["host"]["epsilon"] > 0.05 and eager[first - 1]["host"]["beta"] < 1.0
    assert (lr._ring is None) == (settle >= 2)                            # which store path was captured
    for f in range(first, TOTAL):
        out = lr.frame()
        _assert_equal(lr, out, eager[f], f"frame {f}")
    assert lr.syncs == [3, 7, 11, 15] and lr.epsilon == 0.05 and lr.beta == 1 and lr.updates == TOTAL - 1
    assert lr.replay.size == CAP and bool(torch.isfinite(lr.last_loss))
    # the run exercised what it claims to: the returned done is not the stored one, and ring rows wrapped
    assert any(bool(s["done"].any()) for s in eager[first:])
    assert any(s["host"]["replay.pos"] < N_ENVS for s in eager[first:])


def test_run_k_equals_k_frames():
    shape = SHAPES[0]
    eager = _eager(*shape)
    one, many = _learner(*shape, graphable=True), _learner(*shape, graphable=True)
    one.capture()
    many.capture()
    assert one.frames == many.frames == 2
    out_many = many.run(12)
    for _ in range(12):
        out_one = one.frame()
    _assert_equal(many, out_many, eager[13], "run(12)")
    _assert_equal(one, out_one, eager[13], "12 frames")
    assert one.syncs == many.syncs == eager[13]["host"]["syncs"] == [3, 7, 11]
    # and the two go on alike from there
    _assert_equal(many, many.frame(), eager[14], "the frame after run(12)")
    with pytest.raises(ValueError, match="k must be >= 1"):
        many.run(0)


def test_target_copy_only_on_due_frames():
    lr = _learner(*SHAPES[0], graphable=True, target_update=3)
    lr.capture()
    fu = lr.fused
    assert lr.frames == 2
    versions = [p._version for p in lr.target.parameters()]
    for f in range(2, 9):
        lr.frame()
        torch.cuda.synchronize()
        due = (f + 1) % 3 == 0
        assert torch.equal(fu.t_flat, fu.q_flat) == due, f
        assert torch.equal(fu.t_image, fu.q_image) == due, f
        same = all(torch.equal(a, b) for a, b in zip(lr.target.state_dict().values(), lr.q.state_dict().values()))
        assert same == due, f
        now = [p._version for p in lr.target.parameters()]
        assert all(n > v for n, v in zip(now, versions)) == due, f           # the target's versions move with it
        versions = now
    assert lr.syncs == [2, 5, 8]


def test_weights_loaded_between_replays_are_used():
    net, arch, B, settle = SHAPES[0]
    lr = _learner(net, arch, B, settle, graphable=True, max_epsilon=0.0, min_epsilon=0.0)
    lr.capture()
    lr.frame()
    torch.manual_seed(99)
    new = DQN(28, 29, [(50, 50)]).cuda()
    s, g = lr.agent.observe()
    with torch.no_grad():
        q_old, q_new = lr.q(s, g), new(s, g)
    lr.q.load_state_dict(new.state_dict())
    lr.frame()
    torch.cuda.synchronize()
    acts = lr.agent.actions.long()
    # envs whose two best Q values are further apart than ten times the 1e-5 to which the kernel's Q
    # equals the module's (test_gpu_ddqn.py): their argmax is the same on both
    top2 = q_new.topk(2, dim=1)[0]
    clear = (top2[:, 0] - top2[:, 1]) > 1e-4
    assert int(clear.sum()) >= N_ENVS // 2
    assert torch.equal(acts[clear], q_new.argmax(1)[clear])
    assert int((q_new.argmax(1) != q_old.argmax(1))[clear].sum()) > 0       # (the old weights choose otherwise)
    assert lr.epsilon == 0.0 and float(lr._eps32) == 0.0


def test_capture_twice_is_refused():
    lr = _learner(*SHAPES[0], graphable=True)
    lr.capture()
    with pytest.raises(ValueError, match="already captured"):
        lr.capture()
    _assert_equal(lr, lr.frame(), _eager(*SHAPES[0])[2], "the frame after the refusal")
