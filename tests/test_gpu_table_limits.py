"""The step kernels at two documented limits of the network descriptor no bundled network comes
near, bit for bit against oracle/pbn_oracle.c (whose attractor_of is a linear scan and whose
eval_gates walks the gates in order: independent of both mechanisms under test).

Attractor hashes that need 2 and 4 probes (254 attractors; four attractors of 1,000 states): the
hash_more_probes arm of attractor_lookup and the env_fast loops' copy of it, the (h + p) & mask
wrap, ids up to 253 against targets up to 255, in images of up to 150 KB (every launch above
64 KB depends on raise_lds_limits).  Gate planes at three and four state words up to plane 255,
the last one a byte addresses.  tests/test_table_limits_host.py checks on the CPU that the chains
used here visit every attractor state, the displaced ones included."""
import numpy as np
import pytest
import torch

from oracle import agent_oracle
from pbn_rl_amd import _lib
from pbn_rl_amd.agent import BatchedBDQ, BranchingQNetwork
from pbn_rl_amd.vector_env import VectorPBNEnv

from . import table_limits as tl
from . import test_gpu_policy_rollout as policy
from .test_gpu_parity import run_pair, run_rollout_pair, u32

pytestmark = pytest.mark.gpu

PERTURBATIONS = [0.0, 0.02]


def start_env(chain):
    """A VectorPBNEnv on the chain's reset state and targets."""
    spec = chain["spec"]
    st, tg, t = chain["init"]
    env = VectorPBNEnv(spec, tl.GIVEN_N, seed=tl.GIVEN_SEED, env_offset=tl.GIVEN_OFFSET,
                       autoreset=bool(chain["mode"] & 1))
    env.reset()
    assert np.array_equal(u32(env.state), st), "reset state"
    assert np.array_equal(env.t.cpu().numpy(), t)
    env.set_state(env.state.clone(), torch.from_numpy(tg).to(env.device))
    return env


def check_steps(chain):
    """pbn_step on the chain's flip masks: every output of every step."""
    env = start_env(chain)
    for k, (flip, ref) in enumerate(zip(chain["flips"], chain["refs"])):
        state, reward, flags = env.step_flipmask(torch.from_numpy(flip.view(np.int32)).to(env.device))
        tag = f"step {k}"
        assert np.array_equal(u32(env.final_state), ref["final_state"]), tag + " final_state"
        assert np.array_equal(flags.cpu().numpy(), ref["flags"]), tag + " flags"
        assert np.array_equal(u32(reward), ref["reward"].view(np.uint32)), tag + " reward"
        assert np.array_equal(u32(state), ref["state_out"]), tag + " state_out"
        assert np.array_equal(env.target.cpu().numpy(), ref["target"]), tag + " target"
        assert np.array_equal(env.t.cpu().numpy(), ref["t"]), tag + " t"
    env.close()


def check_rollout(chain):
    """pbn_rollout on the chain's flip masks, one launch: every output of every step."""
    env = start_env(chain)
    flips = np.stack(chain["flips"])
    out = env.rollout(len(flips), flipmasks=torch.from_numpy(flips.view(np.int32)).to(env.device),
                      random_actions=False, keep_obs=True, keep_updates=True)
    st = chain["init"][0]
    for k, ref in enumerate(chain["refs"]):
        tag = f"step {k}"
        assert np.array_equal(u32(out["obs"][k]), st), tag + " obs"
        assert np.array_equal(u32(out["final_state"][k]), ref["final_state"]), tag + " final_state"
        assert np.array_equal(out["flags"][k].cpu().numpy(), ref["flags"]), tag + " flags"
        assert np.array_equal(u32(out["reward"][k]), ref["reward"].view(np.uint32)), tag + " reward"
        assert np.array_equal(out["updates"][k].cpu().numpy().view(np.uint16), ref["updates"]), tag + " updates"
        assert np.array_equal(u32(out["flipmask"][k]), chain["flips"][k]), tag + " flipmask"
        st = ref["state_out"]
    last = chain["refs"][-1]
    assert np.array_equal(u32(env.state), last["state_out"])
    assert np.array_equal(env.target.cpu().numpy(), last["target"])
    assert np.array_equal(env.t.cpu().numpy(), last["t"])
    env.close()


# ------------------------------------------------ hashes of 2 and 4 probes, given masks
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("p", PERTURBATIONS)
@pytest.mark.parametrize("name", tl.HASH_CASES)
def test_hash_given_masks_step(name, p, mode, monkeypatch):
    """pbn_step (the wave kernel's one-step variant), without and with autoreset."""
    monkeypatch.delenv("PBN_ROLL", raising=False)
    check_steps(tl.given_chain(name, p, 0, mode))


@pytest.mark.parametrize("variant", ["lean", "pipe"])
@pytest.mark.parametrize("p", PERTURBATIONS)
@pytest.mark.parametrize("name", tl.HASH_CASES)
def test_hash_given_masks_rollout(name, p, variant, monkeypatch):
    """pbn_rollout through the wave kernel's lean variant and the pipelined kernel's general env
    loop (given masks); lds_pipe fits a CU's LDS for every case (hold100_a254: 154 KB)."""
    monkeypatch.setenv("PBN_ROLL", variant)
    check_rollout(tl.given_chain(name, p, 0, 1))
    check_rollout(tl.given_chain(name, p, 0, 0))


@pytest.mark.parametrize("p", PERTURBATIONS)
@pytest.mark.parametrize("name", tl.HASH_CASES)
def test_hash_given_masks_settle_step(name, p, monkeypatch):
    """pbn_step under the settle law (settle = 8: a lookup per update; a near miss runs to the cap
    and is flagged unsettled).  lds_settle is above 64 KB in every case: the wave kernel."""
    monkeypatch.delenv("PBN_ROLL", raising=False)
    check_steps(tl.given_chain(name, p, 8, 1))
    check_steps(tl.given_chain(name, p, 8, 0))


@pytest.mark.parametrize("name,variant", [(c, "lean") for c in tl.HASH_CASES] + [(c, "pipe") for c in tl.SETTLE_PIPE_CASES])
@pytest.mark.parametrize("p", PERTURBATIONS)
def test_hash_given_masks_settle_rollout(name, variant, p, monkeypatch):
    """pbn_rollout under the settle law: the wave kernel's variant 4 and pbn_rollout_settle (not for
    hold100_a254, whose pipelined settle kernel would need more LDS than a CU has)."""
    monkeypatch.setenv("PBN_ROLL", variant)
    check_rollout(tl.given_chain(name, p, 8, 1))
    check_rollout(tl.given_chain(name, p, 8, 0))


# ------------------------------------------------ hashes of 2 probes, random actions (env_fast)
@pytest.mark.parametrize("mode", [3, 2])
@pytest.mark.parametrize("name", tl.COLLAPSE_CASES)
def test_collapse_random_actions_step(name, mode):
    run = tl.COLLAPSE_STEP
    assert (run["seed"], run["env_offset"]) == (12345, 0)      # run_pair's defaults: the chain the host test walked
    run_pair(tl.limit_spec(name, **tl.collapse_kw()), run["n"], run["steps"], mode=mode)


@pytest.mark.parametrize("kernel", ["lean", "pipe", "settle_lean", "settle_pipe"])
@pytest.mark.parametrize("mode", [3, 2])
@pytest.mark.parametrize("name", tl.COLLAPSE_CASES)
def test_collapse_random_actions_rollout(name, mode, kernel, monkeypatch):
    """Half of the env-steps end in one of 254 attractors, some on states displaced from their home
    slot: the pipelined kernels take their env_fast loops (single-state attractors, the gap bucket
    table, random actions), which carry their own copy of the further probes."""
    run = tl.COLLAPSE_ROLLOUT
    assert (run["seed"], run["env_offset"]) == (4242, 2048)    # run_rollout_pair's defaults
    monkeypatch.setenv("PBN_ROLL", kernel.split("_")[-1])
    spec = tl.limit_spec(name, **tl.collapse_kw(8 if kernel.startswith("settle") else 0))
    ref = run_rollout_pair(spec, run["n"], run["steps"], mode)
    assert (ref["flags"] & _lib.FLAG_IN_ATTRACTOR).any()


# ------------------------------------------------ gate planes up to plane 255
@pytest.mark.parametrize("n_nodes", tl.GATE_SIZES)
def test_gate_limit_step(n_nodes):
    spec = tl.limit_spec(f"gates{n_nodes}_limit", perturbation=0.01, horizon=6)
    run_pair(spec, 1024, 4, mode=3, start_random=True)
    run_pair(spec, 1024, 4, mode=0, start_random=True)


@pytest.mark.parametrize("n_nodes", tl.GATE_SIZES)
def test_gate_limit_rollout(n_nodes, monkeypatch):
    monkeypatch.setenv("PBN_ROLL", "lean")
    run_rollout_pair(tl.limit_spec(f"gates{n_nodes}_limit", perturbation=0.01, horizon=6), 1056, 6, 3)


@pytest.mark.parametrize("n_nodes", tl.GATE_SIZES)
def test_gate_limit_settle(n_nodes, monkeypatch):
    monkeypatch.delenv("PBN_ROLL", raising=False)
    spec = tl.limit_spec(f"gates{n_nodes}_limit", perturbation=0.01, horizon=6, settle=6)
    run_pair(spec, 1024, 4, mode=3, start_random=True)
    run_rollout_pair(spec, 1056, 5, 3)


@pytest.mark.parametrize("settle", [0, 6])
def test_gates_and_many_attractors(settle, monkeypatch):
    """Gates up to plane 255 and a two-probe hash in one image (three state words): envs start on
    attractor states and stay or leave by what the gates computed."""
    monkeypatch.delenv("PBN_ROLL", raising=False)
    spec = tl.limit_spec("gates70_a254", perturbation=0.002, horizon=6, settle=settle)
    ref = run_pair(spec, 1024, 2, mode=1, flip_density=0.0)
    hit = ((ref["flags"] & _lib.FLAG_IN_ATTRACTOR) != 0).mean()
    assert 0.05 < hit < 0.95, hit          # both outcomes, by the oracle
    run_pair(spec, 1024, 5, mode=0, flip_density=0.0)
    run_pair(spec, 1024, 4, mode=2)
    run_rollout_pair(spec, 1056, 6, 3)
    run_rollout_pair(spec, 1056, 6, 1)


# ------------------------------------------------ the kernels next to them
def test_obs_unpack_at_254_attractors():
    """pbn_obs_unpack's target half at the last attractor (253), past it (254) and without a target
    (255) against agent_oracle.obs_unpack."""
    spec = tl.limit_spec("hold28_a254")
    n = 2080
    env = VectorPBNEnv(spec, n, seed=5)
    rng = np.random.default_rng(1)
    st = rng.integers(0, 1 << 28, size=(1, n), dtype=np.uint64).astype(np.uint32)
    tg = rng.integers(0, 254, size=n).astype(np.uint8)
    for k, v in enumerate((0, 253, 254, 255)):
        tg[k::9] = v
    env.set_state(torch.from_numpy(st.view(np.int32)).cuda(), torch.from_numpy(tg).cuda())
    agent = BatchedBDQ(env, BranchingQNetwork((spec.n, spec.n), spec.n + 1, 3))
    obs = agent.observe()
    torch.cuda.synchronize()
    want = agent_oracle.obs_unpack(spec, st, tg)
    assert np.array_equal(obs.cpu().numpy(), want)
    assert not want[1][tg >= 254].any() and want[1][tg == 253].any()
    env.close()


@pytest.mark.parametrize("name,arch", [("hold28_a254", [(50, 50)]), ("gates97_limit", [(64, 64)])])
def test_policy_rollout_at_the_limits(name, arch):
    """pbn_rollout_dqn (the wave kernel with the Q-network in its loop) on a two-probe hash and on
    gates at four state words: the launch against act-then-step, and against the oracle."""
    spec = tl.limit_spec(name, perturbation=0.05, horizon=3)
    policy.run_pair(spec, arch, 96)
    policy.steps_are_the_oracles(spec, arch)
