"""Time compute_ssd_hist at the reference's evaluation settings.

    python tools/ssd_bench.py [--network pbn28] [--resets 300] [--iters 100000]
    python tools/ssd_bench.py --sparse       # dense against sparse=True, and pbn70 (sparse only)

The reference calls compute_ssd_hist(env, model, resets=300, iters=100_000) after every
training run (train_pbn_28.py:257).  Prints one JSON line:
  gpu_chain_s   chains + histogram on the GPU (HIP events around the rollout/histogram loop)
  total_s       the whole call, including the 2^N-bin copy to the host and the normalisation
  cpu_*         the same env-steps priced at the CPU restatements' measured rates (bounded
                samples: the C oracle on host threads over the same number of chains, and
                the per-env pure-Python step), not run to completion
--sparse times the dense call and compute_ssd_hist(sparse=True) (the visited-state hash table,
state_table.py) in alternating blocks in one process, then one sparse call on pbn70, and writes
profiles/ssd_sparse_pbn28.json (``sparse_times``).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pbn_rl_amd.attractors import load_attractors  # noqa: E402
from pbn_rl_amd.network import load_network  # noqa: E402
from pbn_rl_amd.spec import EnvSpec  # noqa: E402
from pbn_rl_amd.ssd import compute_ssd_hist, state_histogram  # noqa: E402
from pbn_rl_amd.vector_env import VectorPBNEnv  # noqa: E402


def gpu_chain_time(spec, resets, iters, chunk=200):
    """The no-policy loop of compute_ssd_hist, timed with HIP events on the current stream."""
    venv = VectorPBNEnv(spec, resets, seed=0, autoreset=False, keep_final_state=True)
    venv.reset()
    hist = torch.zeros(1 << spec.n, dtype=torch.int32, device=venv.device)
    n = venv.n_alloc
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    left, buf = iters, None
    while left > 0:
        k = min(chunk, left)
        buf = venv.rollout(k, random_actions=False, keep_final=True,
                           out=buf if buf is not None and buf["_n_steps"] == k else None)
        state_histogram(buf["final_state"].view(k, n), resets, spec.n, hist)
        left -= k
    b.record()
    torch.cuda.synchronize()
    total = int(hist.sum().item())
    venv.close()
    return a.elapsed_time(b) / 1e3, total


def _spread(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs)), "runs": [float(x) for x in xs]}


def policy_times(spec, resets, iters, policy_iters, blocks, net_arch=((50, 50),), weight_seed=0):
    """compute_ssd_hist with a DQN policy, three ways, in alternating blocks of one call each at
    ``policy_iters`` counted steps (wall time of the whole call / policy_iters = seconds per step):

      fused      the network inside the step kernel (BatchedDDQN.rollout chunks)
      per_step   fused=False: act_q + pbn_step_dev + histogram, one captured graph per step
      closure    what a DQN policy cost before compute_ssd_hist took one: a closure calling the
                 same module in PyTorch on unpack_states' bits (graph=True).  A closure cannot see
                 the chains' targets, so it passes attractor 0's first state for every chain: its
                 time is comparable, its histogram is not.

    then one fused call at ``iters`` counted steps."""
    from pbn_rl_amd.ddqn import DQN

    torch.manual_seed(weight_seed)
    N = spec.n
    q = DQN(N, N + 1, list(net_arch)).cuda()
    goal = torch.tensor(list(spec.attractors[0][0]), dtype=torch.float32, device="cuda").unsqueeze(0)

    @torch.no_grad()
    def closure(bits):
        s = bits.to(torch.float32)
        return q(s, goal.expand(s.shape[0], -1)).argmax(1, keepdim=True)

    def timed(model, n_iters, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ssd, _ = compute_ssd_hist(spec, model, resets=resets, iters=n_iters, **kw)
        dt = time.perf_counter() - t0
        assert abs(float(ssd.sum()) - 1.0) < 1e-9
        return dt, ssd

    ways = {"fused": (q, {}), "per_step": (q, {"fused": False}), "closure": (closure, {})}
    for model, kw in ways.values():       # warm-up: code objects, allocator, the graphs' first capture
        timed(model, 200, **kw)
    runs = {k: [] for k in ways}
    calls = {k: [] for k in ways}
    ssds = {}
    short = 200
    for _ in range(blocks):
        for k, (model, kw) in ways.items():
            base, _ = timed(model, short, **kw)
            dt, ssds[k] = timed(model, policy_iters, **kw)
            runs[k].append((dt - base) / (policy_iters - short))
            calls[k].append(dt)
    assert np.array_equal(ssds["fused"], ssds["per_step"])
    whole_s, _ = timed(q, iters)
    res = {k: _spread(v) for k, v in runs.items()}
    return {"policy": f"DQN({N}, {N + 1}, {list(net_arch)}), torch.manual_seed({weight_seed}), greedy",
            "policy_iters": policy_iters, "blocks": blocks,
            "per_step_s": res,
            "per_step_note": f"(call at policy_iters - call at {short} counted steps, back to back) / the difference "
                             "in steps: the call's fixed cost (the 2^N-bin histogram's allocation, copy to the host "
                             "and normalisation, the reset, graph capture) cancels",
            "call_s": {k: _spread(v) for k, v in calls.items()},
            "fused_whole_call_s": whole_s, "fused_whole_call_iters": iters,
            "fused_vs_closure": res["closure"]["median"] / res["fused"]["median"],
            "fused_vs_per_step": res["per_step"]["median"] / res["fused"]["median"],
            "fused_below_closure_by_more_than_spread": bool(res["fused"]["max"] < res["closure"]["min"]),
            "fused_equals_per_step_histogram": True}


def gpu_sparse_chain_time(spec, resets, iters, capacity, chunk=200):
    """gpu_chain_time with the table insert in place of the histogram (growth included)."""
    from pbn_rl_amd.state_table import StateTable
    venv = VectorPBNEnv(spec, resets, seed=0, autoreset=False, keep_final_state=True)
    venv.reset()
    table = StateTable(spec.n, venv.device, capacity=capacity)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    left, buf = iters, None
    while left > 0:
        k = min(chunk, left)
        buf = venv.rollout(k, random_actions=False, keep_final=True,
                           out=buf if buf is not None and buf["_n_steps"] == k else None)
        table.add(buf["final_state"], resets)
        left -= k
    b.record()
    torch.cuda.synchronize()
    total, lost = table.total, table.n_lost
    venv.close()
    return a.elapsed_time(b) / 1e3, total, lost


def sparse_times(resets, iters, perturbation, blocks, out_path):
    """The dense call against compute_ssd_hist(sparse=True) on pbn28 at the reference's settings, in
    alternating blocks of one call each in this process: dense; sparse from the default capacity
    (the table grows during the call); sparse pre-sized to the capacity the first sparse call ended
    with (no growth).  Then the GPU time of the chunks alone (HIP events: rollout + histogram /
    rollout + insert), and one sparse call on pbn70, which the dense path cannot run."""
    spec = EnvSpec(load_network("pbn28"), load_attractors("pbn28"), perturbation=perturbation)
    spec70 = EnvSpec(load_network("pbn70"), load_attractors("pbn70"), perturbation=perturbation)

    def timed(sp, **kw):
        stats = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kw.get("sparse"):
            kw["stats"] = stats
        ssd, _ = compute_ssd_hist(sp, None, resets=resets, iters=iters, **kw)
        return time.perf_counter() - t0, ssd, stats

    # warm-up: code objects, allocator (a short call of each kind), and the capacity to pre-size to
    compute_ssd_hist(spec, None, resets=resets, iters=400)
    compute_ssd_hist(spec, None, resets=resets, iters=400, sparse=True)
    _, first, stats = timed(spec, sparse=True)
    cap = stats["capacity"]
    runs = {"dense": [], "sparse": [], "sparse_presized": []}
    dense = ssd = None
    for _ in range(blocks):
        dt, dense, _ = timed(spec)
        runs["dense"].append(dt)
        dt, ssd, grown = timed(spec, sparse=True)
        runs["sparse"].append(dt)
        dt, pre, sized = timed(spec, sparse=True, capacity=cap)
        runs["sparse_presized"].append(dt)
        assert sized["n_growths"] == 0
        assert np.array_equal(pre.counts, ssd.counts) and np.array_equal(pre.words, ssd.words)
    assert np.array_equal(ssd.to_dense(), dense)          # the same counts over the same total
    del dense
    gpu_chain_time(spec, resets, 1000)
    dense_chain_s, counted = gpu_chain_time(spec, resets, iters)
    assert counted == resets * iters
    gpu_sparse_chain_time(spec, resets, 1000, 1 << 16)
    grow_chain_s, total, lost = gpu_sparse_chain_time(spec, resets, iters, 1 << 16)
    assert total == resets * iters and lost == 0
    sized_chain_s, total, lost = gpu_sparse_chain_time(spec, resets, iters, cap)
    assert total == resets * iters and lost == 0
    compute_ssd_hist(spec70, None, resets=resets, iters=400, sparse=True)
    dt70, ssd70, stats70 = timed(spec70, sparse=True)
    assert ssd70.total == resets * iters
    chain70_s, _, lost70 = gpu_sparse_chain_time(spec70, resets, iters, 1 << 16)
    assert lost70 == 0
    res = {
        "what": f"compute_ssd_hist(pbn28, model=None, resets={resets}, iters={iters}), p={perturbation}: dense (2^28 "
                f"32-bit bins) against sparse=True (visited-state hash table), {blocks} alternating blocks in one "
                "process; wall time of each whole call, seconds",
        "env_steps": resets * iters, "blocks": blocks,
        "call_s": {k: _spread(v) for k, v in runs.items()},
        "sparse_vs_dense": float(np.median(runs["sparse"]) / np.median(runs["dense"])),
        "sparse_presized_vs_dense": float(np.median(runs["sparse_presized"]) / np.median(runs["dense"])),
        "gpu_chunks_s": {"dense": dense_chain_s, "sparse": grow_chain_s, "sparse_presized": sized_chain_s},
        "gpu_chunks_note": "HIP events around the rollout + histogram / rollout + insert launches of one run (the "
                           "sparse figure from the default capacity includes the table's growth and its "
                           "synchronisations)",
        "distinct_states": len(ssd), "final_capacity": grown["capacity"], "growths": grown["n_growths"],
        "presized_capacity": cap, "default_capacity": 1 << 16,
        "sparse_to_dense_equals_dense": True,
        "pbn70": {"what": f"compute_ssd_hist(pbn70, model=None, resets={resets}, iters={iters}, sparse=True), one call",
                  "call_s": dt70, "gpu_chunks_s": chain70_s, "distinct_states": len(ssd70),
                  "final_capacity": stats70["capacity"], "growths": stats70["n_growths"]},
        "host": {"cpu_count": os.cpu_count()}}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--network", default="pbn28")
    ap.add_argument("--resets", type=int, default=300)
    ap.add_argument("--iters", type=int, default=100_000)
    ap.add_argument("--perturbation", type=float, default=0.01)
    ap.add_argument("--cpu-seconds", type=float, default=5.0)
    ap.add_argument("--policy", choices=["none", "ddqn"], default="none",
                    help="ddqn: also time compute_ssd_hist with a DQN policy (fused, per-step, PyTorch closure)")
    ap.add_argument("--policy-iters", type=int, default=20_000, help="counted steps of each timed policy call")
    ap.add_argument("--blocks", type=int, default=5, help="alternating blocks of the policy timings")
    ap.add_argument("--sparse", action="store_true",
                    help="time dense against sparse=True on pbn28 (and sparse on pbn70); writes --sparse-out")
    ap.add_argument("--sparse-out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                         "ssd_sparse_pbn28.json"))
    args = ap.parse_args()
    if args.sparse:
        print(json.dumps(sparse_times(args.resets, args.iters, args.perturbation, args.blocks, args.sparse_out)),
              flush=True)
        return
    spec = EnvSpec(load_network(args.network), load_attractors(args.network), perturbation=args.perturbation)
    steps = args.resets * args.iters
    policy = None
    if args.policy == "ddqn":
        policy = policy_times(spec, args.resets, args.iters, args.policy_iters, args.blocks)

    gpu_chain_time(spec, args.resets, 1000)                      # warm-up (allocator, code objects)
    chain_s, counted = gpu_chain_time(spec, args.resets, args.iters)
    assert counted == steps, (counted, steps)
    t0 = time.perf_counter()
    ssd, _ = compute_ssd_hist(spec, None, resets=args.resets, iters=args.iters)
    total_s = time.perf_counter() - t0
    assert abs(float(ssd.sum()) - 1.0) < 1e-9

    from oracle import oracle, pyoracle
    threads = max(1, min(16, os.cpu_count() or 1))
    st, tg, t = oracle.reset(spec, 1, 0, 0, 320)
    zero = np.zeros_like(st)
    k, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < args.cpu_seconds:
        out = oracle.step(spec, 1, k + 1, 0, st, zero, tg, t, 0, want_final=False, n_threads=threads)
        st, tg, t = out["state_out"], out["target"], out["t"]
        k += 1
    c_rate = 320 * k / (time.perf_counter() - t0)
    py = pyoracle.PyPBN(spec)
    s, g, tt = py.reset(1, 0, 0)
    k, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < 2.0:
        r = py.step(1, k + 1, 0, s, [0] * spec.n, g, tt, 0)
        s, tt = r["final_state"], r["t"]
        k += 1
    py_rate = k / (time.perf_counter() - t0)
    if policy is not None:
        policy["fused_whole_call_vs_model_less"] = policy["fused_whole_call_s"] / total_s
    print(json.dumps({
        "what": f"compute_ssd_hist({args.network}, model=None, resets={args.resets}, iters={args.iters}), "
                f"p={args.perturbation}, 2^{spec.n} 32-bit bins in HBM",
        "env_steps": steps, "gpu_chain_s": chain_s, "gpu_env_steps_per_s": steps / chain_s,
        "total_s": total_s,
        **({"ddqn_policy": policy} if policy is not None else {}),
        "total_note": "includes the 2^N-bin device-to-host copy and float64 normalisation on the host",
        "cpu_c_oracle_env_steps_per_s": c_rate, "cpu_c_oracle_threads": threads,
        "cpu_c_oracle_est_s": steps / c_rate,
        "cpu_python_env_steps_per_s": py_rate, "cpu_python_est_s": steps / py_rate,
        "host": {"cpu_count": os.cpu_count()}}), flush=True)


if __name__ == "__main__":
    main()
