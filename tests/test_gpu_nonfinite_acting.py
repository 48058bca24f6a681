"""NaN and infinite weights fed through the acting kernels' forwards (DESIGN.md "Non-finite values"):
BatchedDDQN.q_values / act_q / rollout (csrc/dqn_forward.h, pbn_ddqn.hip, step_wave.h) and
BatchedBDQ.q_values / act_q (pbn_qnet.hip), against the PyTorch module on the CPU.

Per case (tests/nonfinite_cases.py): Q has the fp32 module's pattern of NaN, +inf and -inf exactly;
its finite entries equal the float64 module's at rtol 1e-5 / atol 1e-5; the greedy actions are
torch.argmax's of the fp32 module's Q on every row that a NaN or a single +inf decides, and the
float64 module's on the finite rows whose top-2 gap exceeds 1e-4 (at least half of them, asserted on
the reference).  The references' own patterns are asserted equal first.

A NaN in a bilinear weight is the one intended difference: the DDQN kernels and pbn_bilinear_targets
add the table rows of the set bits only, where the dense product makes every row NaN.  Those cases
are held to a plain float64 restatement of the sparse sum.  (The fused BDQ forward multiplies the
table by the 0/1 bits on the MFMA, a dense product: it is held to the module.)"""
import copy

import pytest
import torch

from pbn_rl_amd.agent import BatchedBDQ
from pbn_rl_amd.ddqn import BatchedDDQN
from pbn_rl_amd.vector_env import VectorPBNEnv
from tests import nonfinite_cases as C
from tests.edge_shapes import edge_spec
from tests.test_gpu_policy_rollout import make_spec as rollout_spec
from tests.test_gpu_policy_rollout import run_pair

pytestmark = pytest.mark.gpu

_ENVS = {}


def the_env(shape):
    """One reset env per shape, NO_TARGET envs without a target; its observation is C.observation's."""
    if shape not in _ENVS:
        spec = C.the_spec(shape)
        env = VectorPBNEnv(spec, C.N_ENVS, seed=C.ENV_SEED)
        env.reset()
        for e in C.NO_TARGET:
            env.target[e] = 255
        assert env.n_alloc == C.N_ENVS
        s, g = C.observation(spec)
        so, go = BatchedDDQN(env, C.dqn_net(spec.n, (8, 8)).cuda()).observe()
        assert torch.equal(so.cpu(), s) and torch.equal(go.cpu(), g)
        _ENVS[shape] = (spec, env, s, g)
    return _ENVS[shape]


def check_actions(acts, q32, q64):
    """Greedy actions (rows,) against the references' Q (rows, A)."""
    special = C.special_rows(q32)
    want = q32.argmax(1)
    assert torch.equal(acts[special], want[special]), (acts[special] != want[special]).nonzero()[:8].tolist()
    clear, _ = C.finite_row_filter(q32, q64)
    assert torch.equal(acts[clear], q64.argmax(1)[clear])
    return int(special.sum()), int(clear.sum())


# ---- DDQN -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.DDQN_INJECTIONS))
@pytest.mark.parametrize("shape,arch", C.DDQN_ACT_SHAPES, ids=C.DDQN_ACT_IDS)
def test_ddqn_q_and_greedy_actions_are_the_modules(shape, arch, name):
    spec, env, s, g = the_env(shape)
    q = C.inject(C.dqn_net(spec.n, arch), *C.DDQN_INJECTIONS[name])
    q32, q64 = C.dqn_refs(q, s, g)
    agent = BatchedDDQN(env, copy.deepcopy(q).cuda())
    assert agent.kernel
    qk = agent.q_values().clone().cpu()
    agent.actions.fill_(-1)
    agent.act_q(0.0)
    acts = agent.actions.cpu().long()
    C.assert_same_pattern(qk, q32, name)
    n_fin = C.check_finite(qk, q64, 1e-5, 1e-5, name)
    n_special, n_clear = check_actions(acts, q32, q64)
    print(f"{shape} {arch} {name}: {n_fin} finite entries, {n_special} rows decided by a non-finite value, "
          f"{n_clear} finite rows compared")
    A = spec.n + 1
    if name in ("nan_out_bias", "pinf_out_bias"):
        assert bool((acts == A - 1).all())
    if name in ("nan_input_bias", "nan_l1_bias"):
        assert bool((acts == 0).all())                     # an all-NaN row: action 0


@pytest.mark.parametrize("shape,arch", C.DDQN_ACT_SHAPES, ids=C.DDQN_ACT_IDS)
def test_ddqn_bilinear_weight_nan_reaches_the_rows_that_select_it(shape, arch):
    spec, env, s, g = the_env(shape)
    q = C.dqn_net(spec.n, arch)
    i, j = C.bilinear_nan_pair(s, g)
    qn = C.inject(q, "input.weight", (-1, i, j), C.NAN)
    hit = torch.isnan(C.sparse_bilinear_features(qn, s, g)).any(1)
    assert torch.equal(hit, (s[:, i] > 0) & (g[:, j] > 0)) and 0 < int(hit.sum()) < C.N_ENVS
    zero = C.inject(q, "input.weight", (-1, i, j), 0.0)
    q32, q64 = C.dqn_refs(zero, s, g)
    q32[hit], q64[hit] = C.NAN, C.NAN                      # a NaN feature: the whole row of Q
    agent = BatchedDDQN(env, qn.cuda())
    qk = agent.q_values().clone().cpu()
    agent.act_q(0.0)
    C.assert_same_pattern(qk, q32)
    C.check_finite(qk, q64, 1e-5, 1e-5)
    check_actions(agent.actions.cpu().long(), q32, q64)


@pytest.mark.parametrize("name", C.ROLLOUT_INJECTIONS)
@pytest.mark.parametrize("shape,arch", C.DDQN_ACT_SHAPES, ids=C.DDQN_ACT_IDS)
def test_ddqn_rollout_equals_act_then_step(shape, arch, name):
    spec = rollout_spec(shape) if isinstance(shape, str) else edge_spec(shape, horizon=3)
    q = C.inject(C.dqn_net(spec.n, arch), *C.DDQN_INJECTIONS[name])
    run_pair(spec, [arch], C.N_ENVS, q=q.cuda())


# ---- BDQ --------------------------------------------------------------------------------------------
def bdq_refs(q, obs):
    """(Q fp32, Q float64) (n, K, A) of the module on the CPU; asserts the precondition."""
    with torch.no_grad():
        q32 = q(obs)
        q64 = copy.deepcopy(q).double()(obs.double())
    C.assert_same_pattern(q32, q64, "precondition: the fp32 and float64 modules")
    return q32, q64


@pytest.mark.parametrize("name", sorted(C.BDQ_INJECTIONS))
@pytest.mark.parametrize("shape,K", C.BDQ_SHAPES, ids=C.BDQ_IDS)
def test_bdq_q_and_greedy_actions_are_the_modules(shape, K, name):
    spec, env, s, g = the_env(shape)
    A = spec.n + 1
    q = C.inject(C.bdq_net(spec.n, K), *C.bdq_injection(name, K))
    q32, q64 = bdq_refs(q, torch.stack([s, g]))
    agent = BatchedBDQ(env, copy.deepcopy(q).cuda(), branches=K)
    assert agent.fused_tail
    with torch.no_grad():
        qk = agent.q_values().clone().cpu()
    agent.actions.fill_(-1)
    agent.act_q(0.0)
    acts = agent.actions.cpu().long()
    C.assert_same_pattern(qk, q32, name)
    C.check_finite(qk, q64, 1e-5, 1e-5, name)
    check_actions(acts.reshape(-1), q32.reshape(-1, A), q64.reshape(-1, A))
    if name.endswith("_adv_bias"):
        # one non-finite advantage entry reaches the branch's whole row through the dueling mean
        assert not bool(torch.isfinite(qk[:, K - 1]).any())
        assert bool(torch.isnan(qk[:, K - 1, A - 1]).all()) and bool((acts[:, K - 1] == (A - 1 if "nan" not in name else 0)).all())
        assert K == 1 or bool(torch.isfinite(qk[:, :K - 1]).all())


@pytest.mark.parametrize("shape,K", C.BDQ_SHAPES, ids=C.BDQ_IDS)
def test_bdq_bilinear_weight_nan(shape, K):
    """BatchedBDQ contracts the bilinear layer with every attractor's first state by a dense product
    (MyBilinear.target_table), so table row i of every target holds the NaN of W[o][i][j].
    pbn_bilinear_targets adds the table rows of the set state bits: feature o is NaN exactly in the
    rows that have a target and bit i set, and everything else is the module's with that weight 0.
    The fused forward (pbn_qnet_heads_from_state) multiplies the table by the 0/1 bits on the MFMA, a
    dense product as PyTorch's over the 16 rows of a wave and the targets present in it: every row
    is NaN, as the module's, the two rows without a target included (their zeros meet the NaN of
    their wave's targets; a wave of 16 rows that all lack a target would read no table)."""
    spec, env, s, g = the_env(shape)
    q = C.bdq_net(spec.n, K)
    i, j = C.bilinear_nan_pair(s, g)
    qn = C.inject(q, "model.0.bilinear.weight", (-1, i, j), C.NAN)
    has_target = g.abs().sum(1) > 0
    hit = (s[:, i] > 0) & has_target
    assert 0 < int(hit.sum()) < int(has_target.sum()) < C.N_ENVS
    zero = C.inject(q, "model.0.bilinear.weight", (-1, i, j), 0.0)
    obs = torch.stack([s, g])
    with torch.no_grad():
        y32 = zero.model[1](zero.model[0](obs))
        z64 = copy.deepcopy(zero).double()
        y64 = z64.model[1](z64.model[0](obs.double()))
        dense = qn(obs)
    y32[hit, -1], y64[hit, -1] = C.NAN, C.NAN
    assert bool(torch.isnan(dense).all())
    agent = BatchedBDQ(env, qn.cuda(), branches=K)
    with torch.no_grad():
        agent.bilinear()
        y = agent._y.clone().cpu()
        qk = agent.q_values().clone().cpu()
    C.assert_same_pattern(y, y32)
    C.check_finite(y, y64, 1e-5, 1e-5)
    C.assert_same_pattern(qk, dense)


@pytest.mark.parametrize("shape,K", C.BDQ_SHAPES, ids=C.BDQ_IDS)
def test_bdq_fused_forward_waves_without_a_target_read_no_table(shape, K):
    """The fused forward sorts a block's envs by target and gives each wave 16 of them.  With 32 of 96
    envs without a target, scattered, the 64 with one fill four waves and the 32 fill two of their
    own: those read no table row, so a NaN bilinear weight does not reach them and their Q is the
    module's with that weight 0 (the bias alone), where the module's dense product gives NaN.  The
    rows with a target are NaN, as the module's."""
    spec = C.the_spec(shape)
    env = VectorPBNEnv(spec, C.N_ENVS, seed=C.ENV_SEED)
    env.reset()
    none = torch.arange(0, C.N_ENVS, 3)
    env.target[none.cuda()] = 255
    s, g = C.observation(spec)
    g[none] = 0.0
    assert none.numel() == 32 and float(g[none].abs().sum()) == 0.0
    q = C.bdq_net(spec.n, K)
    i, j = C.bilinear_nan_pair(s, g)
    qn = C.inject(q, "model.0.bilinear.weight", (-1, i, j), C.NAN)
    obs = torch.stack([s, g])
    q32, q64 = bdq_refs(C.inject(q, "model.0.bilinear.weight", (-1, i, j), 0.0), obs)
    with torch.no_grad():
        assert bool(torch.isnan(qn(obs)).all())                       # the module: every row
    with_target = torch.ones(C.N_ENVS, dtype=torch.bool)
    with_target[none] = False
    q32[with_target], q64[with_target] = C.NAN, C.NAN
    agent = BatchedBDQ(env, qn.cuda(), branches=K)
    assert agent.fused_tail
    with torch.no_grad():
        qk = agent.q_values().clone().cpu()
    C.assert_same_pattern(qk, q32)
    assert C.check_finite(qk, q64, 1e-5, 1e-5) == 32 * K * (spec.n + 1)
    env.close()
