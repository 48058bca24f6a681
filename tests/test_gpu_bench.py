"""bench.py's plain run on the GPU, in process: --steps sets the timed steps, the result line
carries ms_per_step and none of --full's lines, and --dump-outputs writes what a caller stepping a
VectorPBNEnv through the same warmup and timed launches receives from the last step, whatever
the clock ramp replayed in between (1,000 envs: a ragged batch, padded to 1,024)."""
import json
import sys

import numpy as np
import pytest
import torch

import bench
from pbn_rl_amd.attractors import load_attractors
from pbn_rl_amd.network import load_network
from pbn_rl_amd.spec import EnvSpec
from pbn_rl_amd.vector_env import VectorPBNEnv

pytestmark = pytest.mark.gpu

ENVS, WARMUP, CHUNK, SEED = 1000, 5, 3, 3


def _run_bench(monkeypatch, capsys, out_dir, steps, extra, clock_warm):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--envs", str(ENVS), "--steps", str(steps),
                                      "--warmup", str(WARMUP), "--chunk", str(CHUNK), "--seed", str(SEED),
                                      "--clock-warm", str(clock_warm), "--dump-outputs", str(out_dir), *extra])
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), {p.stem: np.load(p) for p in out_dir.iterdir()}


def _direct(mode, n_steps, graph):
    """The same steps through VectorPBNEnv alone: the warmup, the untimed replays of the timed
    steps after which bench.py keeps the envs (MIX_STEPS steps' worth), then the timed steps; the
    last step's outputs, as bench.last_step_outputs.  A captured run replays the step indices
    (the RNG's time coordinate) it was captured with; eager launches go on counting."""
    spec = EnvSpec(load_network("pbn28"), load_attractors("pbn28"), perturbation=0.01, prob_bits=16, horizon=20)
    env = VectorPBNEnv(spec, ENVS, seed=SEED, device="cuda:0", keep_final_state=False)
    env.reset()
    bufs = {}

    def steps(plan):
        for k in plan:
            if mode == "rollout":
                bufs[k] = env.rollout(k, random_actions=True, keep_obs=True, keep_final=True, out=bufs.get(k))
            else:
                for _ in range(k):
                    env.step_flipmask(random_actions=True)

    steps(bench.launch_plan(WARMUP, CHUNK))
    first = env.step_index
    plan = bench.launch_plan(n_steps, CHUNK)
    for _ in range(-(-bench.MIX_STEPS // n_steps) + 1):
        if graph:
            env.step_index = first
        steps(plan)
    torch.cuda.synchronize()
    want = bench.last_step_outputs(env, rollout_out=bufs.get(plan[-1]))
    env.close()
    return want


@pytest.mark.parametrize("mode,steps,extra", [("rollout", 7, []), ("rollout", 7, ["--graph"]),
                                              ("step", 7, ["--mode", "step", "--no-graph"]),
                                              ("step", 8, ["--mode", "step"])],
                         ids=["rollout", "rollout-graph", "step", "step-graph"])
def test_plain_run_dumps_the_last_timed_step(mode, steps, extra, tmp_path, monkeypatch, capsys):
    """7 steps in launches of 3: a ragged plan; the captured step run takes 8 (an even count brings
    the env's two state buffers back to where the capture found them)."""
    graph = "--graph" in extra or (mode == "step" and "--no-graph" not in extra)
    line, got = _run_bench(monkeypatch, capsys, tmp_path / "a", steps, extra, 0.0)
    assert line["steps"] == steps and line["warmup"] == WARMUP and line["ms_per_step"] > 0
    assert line["config"]["launch"] == ("hipGraph" if graph else "eager")
    assert line["value"] == pytest.approx(ENVS * steps / (line["ms_per_step"] * steps * 1e-3))
    assert line["unit"] == "env-steps/s" and line["higher_is_better"] is True and line["dtype"] == "u32"
    for key in ("cpu_baseline", "settle_law", "gather", "value_with_gather", "config1"):
        assert key not in line                                    # --full's lines
    assert "default_events" not in line["timing"]
    want = _direct(mode, steps, graph)
    assert set(got) == set(want) and {"state", "target", "t", "flipmask", "reward", "flags"} <= set(got)
    for name, a in want.items():
        assert got[name].dtype in (np.float32, np.float64) and got[name].shape[-1] == ENVS
        assert np.array_equal(got[name], a), name
    # a longer clock ramp replays the run more often; the timed steps compute the same
    _, again = _run_bench(monkeypatch, capsys, tmp_path / "b", steps, extra, 0.05)
    for name, a in got.items():
        assert np.array_equal(again[name], a), name
