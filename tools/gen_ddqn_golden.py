"""Generate tests/golden/ddqn_update.npz: the reference's own DDQN / DDQNPER update
(ddqn_per/__init__.py: DDQN._get_loss, DDQN._back_propagate, DDQN._learn_step, DDQNPER._learn_step)
on fixed batches, the pin of pbn_rl_amd/ddqn.py's ``ddqn_update`` and of pbn_ddqn_learn.

  python tools/gen_ddqn_golden.py       (build container only: reads /root/reference)

The reference package cannot be imported (its __init__ imports the absent gym), so, as
tools/gen_update_golden.py does:
  * ``DQN`` is loaded from its own file, ddqn_per/network.py, by path;
  * the four methods are taken from ddqn_per/__init__.py with ``ast`` (their source text,
    unchanged) and executed on a stand-in ``self`` carrying what they read: ``controller``,
    ``target``, ``optimizer`` (Adam), ``gamma``, ``max_grad_norm``, ``REPLAY_CONSTANT``,
    ``log = False``, a ``replay_memory.update_priorities`` recorder and a ``_fetch_minibatch``
    returning the fixed batch.  torch.nn.utils.clip_grad_norm_ is wrapped for the call to record
    the total norm it returns (the reference discards it).

Two shapes: DQN(7, 8, [(8, 8)]) at B = 16 on pbn7's attractors (key prefix ``s7.``) and
DQN(28, 29, [(50, 50)]) at B = 64 on Bittner-28's (``s28.``, train_ddqn.py's).  Per shape: the batch
(0/1 states and next states, target ids -- two rows carry 255, no target --, actions in [0, N],
rewards, terminated flags, importance weights), the parameters before (q0.*, t0.*: seeded init, the
target a perturbed copy), and four calls, each from that same fresh state with a new Adam:
``ddqn_a`` / ``per_a`` at max_grad_norm = 10 and ``ddqn_b`` / ``per_b`` at half the measured norm, with
their loss, total norm, clipped gradients (g.*), parameters after (q1.*) and (per) priorities; the
reference DQN's state-dict keys and its forward on the batch.  Asserted here: the norm at
max_grad_norm = 10 is below 10 (no clip) and the other call clips; the reference's |delta| lies
below 1 and above 1 in at least a quarter of the rows each; every row's top-two gap of Q(s')
exceeds 1e-4 (no argmax tie).
"""
import ast
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from pbn_rl_amd.attractors import load_attractors  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "ddqn_update.npz")
LR, GAMMA, REPLAY_CONSTANT = 1e-3, 0.95, 1e-5
SHAPES = [("s7", "pbn7", 7, [(8, 8)], 16), ("s28", "pbn28", 28, [(50, 50)], 64)]


def ref_dqn_module():
    spec = importlib.util.spec_from_file_location("ref_ddqn_network", os.path.join(REF, "ddqn_per", "network.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def ref_methods():
    """{(class, method): function} for the four methods, compiled from the reference file."""
    path = os.path.join(REF, "ddqn_per", "__init__.py")
    tree = ast.parse(open(path).read(), filename=path)
    want = {"DDQN": ["_get_loss", "_back_propagate", "_learn_step"], "DDQNPER": ["_learn_step"]}
    out, lines = {}, {}
    for cls in (n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in want):
        for fn in (n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in want[cls.name]):
            ns = {"torch": torch, "np": np, "F": F}
            exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
            out[(cls.name, fn.name)] = ns[fn.name]
            lines[f"{cls.name}.{fn.name}"] = (fn.lineno, fn.end_lineno)
    assert len(out) == 4, sorted(out)
    return out, lines


def make_batch(rng, N, B, att_first):
    states = rng.integers(0, 2, size=(B, N), dtype=np.uint8)
    next_states = rng.integers(0, 2, size=(B, N), dtype=np.uint8)
    tid = rng.integers(0, len(att_first), size=B).astype(np.uint8)
    tid[[3, B - 2]] = 255                                   # rows without a target: zeros
    targets = np.where((tid == 255)[:, None], 0, att_first[np.minimum(tid, len(att_first) - 1)]).astype(np.uint8)
    actions = rng.integers(0, N + 1, size=B).astype(np.int64)
    wide = rng.random(B) < 0.55                             # rewards over about +-6, the rest near 0
    rewards = np.where(wide, rng.uniform(-6, 6, B), rng.uniform(-0.8, 0.8, B)).astype(np.float32)
    done = (rng.random(B) < 0.3).astype(np.uint8)
    weights = rng.uniform(0.2, 1.0, B).astype(np.float32)
    weights[0] = 1.0
    return dict(states=states, next_states=next_states, target_ids=tid, targets=targets, actions=actions,
                rewards=rewards, done=done, weights=weights)


def main():
    net_mod = ref_dqn_module()
    methods, lines = ref_methods()
    Agent = type("Agent", (), {"_get_loss": methods[("DDQN", "_get_loss")],
                               "_back_propagate": methods[("DDQN", "_back_propagate")]})
    out = {"lr": np.float32(LR), "gamma": np.float32(GAMMA), "replay_constant": np.float32(REPLAY_CONSTANT)}
    for k, v in lines.items():
        out["lines." + k] = np.array(v)
    for prefix, network, N, arch, B in SHAPES:
        att_first = np.array([list(a[0]) for a in load_attractors(network)], dtype=np.uint8)
        rng = np.random.default_rng(20261019 + N)
        torch.manual_seed(11 + N)
        q = net_mod.DQN(N, N + 1, arch)
        target = net_mod.DQN(N, N + 1, arch)
        with torch.no_grad():
            for pt, pq in zip(target.parameters(), q.parameters()):
                pt.copy_(pq + 0.05 * torch.randn_like(pq))
        q0 = {n: p.detach().clone() for n, p in q.state_dict().items()}
        b = make_batch(rng, N, B, att_first)
        for k, v in b.items():
            out[f"{prefix}.b.{k}"] = v
        out[f"{prefix}.names"] = np.array(list(q.state_dict().keys()))
        out[f"{prefix}.arch"] = np.array(arch, dtype=np.int64)
        for n, p in q.state_dict().items():
            out[f"{prefix}.q0.{n}"] = p.detach().numpy().copy()
        for n, p in target.state_dict().items():
            out[f"{prefix}.t0.{n}"] = p.detach().numpy().copy()
        f32 = lambda a: torch.tensor(np.asarray(a)).float()   # noqa: E731
        experiences = (f32(b["states"]), f32(b["targets"]), torch.tensor(b["actions"]).long().unsqueeze(1),
                       f32(b["rewards"]).unsqueeze(1), f32(b["next_states"]), f32(b["done"]).unsqueeze(1))
        with torch.no_grad():
            out[f"{prefix}.forward"] = q(experiences[0], experiences[1]).numpy().copy()
            qn = q(experiences[4], experiences[1])
            top2 = qn.topk(2, dim=1)[0]
            assert float((top2[:, 0] - top2[:, 1]).min()) > 1e-4, "argmax tie in Q(s'): change the seed"
            ap = qn.max(dim=1)[1].unsqueeze(1)
            y = experiences[3] + (1 - experiences[5]) * GAMMA * target(experiences[4], experiences[1]).gather(1, ap)
            delta = (q(experiences[0], experiences[1]).gather(1, experiences[2]) - y).abs().squeeze(1)
        small, large = float((delta < 1).float().mean()), float((delta > 1).float().mean())
        assert small >= 0.25 and large >= 0.25, (small, large)
        per_batch = {"experiences": experiences,
                     "per_data": (list(range(B)), f32(b["weights"]).unsqueeze(1))}

        def run(call, per, max_norm):
            q.load_state_dict(q0)
            prio, norms = [], []
            this = Agent()
            this.controller, this.target, this.gamma, this.max_grad_norm = q, target, GAMMA, max_norm
            this.optimizer = torch.optim.Adam(q.parameters(), lr=LR)
            this.REPLAY_CONSTANT, this.log, this.num_timesteps, this.LOG_INTERVAL = REPLAY_CONSTANT, False, 0, 100
            this.replay_memory = types.SimpleNamespace(update_priorities=lambda idx, p: prio.append(list(p)))
            this._fetch_minibatch = (lambda: per_batch) if per else (lambda: experiences)
            losses = []
            back = Agent._back_propagate
            this._back_propagate = lambda loss: (losses.append(float(loss.detach())), back(this, loss))
            clip = torch.nn.utils.clip_grad_norm_
            torch.nn.utils.clip_grad_norm_ = lambda *a, **k: (norms.append(clip(*a, **k)), norms[-1])[1]
            try:
                methods[("DDQNPER" if per else "DDQN", "_learn_step")](this)
            finally:
                torch.nn.utils.clip_grad_norm_ = clip
            key = f"{prefix}.{call}"
            out[key + ".loss"] = np.float32(losses[0])
            out[key + ".norm"] = np.float32(float(norms[0]))
            out[key + ".max_grad_norm"] = np.float32(max_norm)
            if per:
                out[key + ".priorities"] = np.array(prio[0], dtype=np.float32)
            for n, p in q.named_parameters():
                out[f"{key}.g.{n}"] = p.grad.detach().numpy().copy()
                out[f"{key}.q1.{n}"] = p.detach().numpy().copy()
            return float(norms[0])

        for tag, per in (("ddqn", False), ("per", True)):
            norm = run(tag + "_a", per, 10.0)
            assert norm < 10.0, f"{prefix}.{tag}: the norm {norm} clips at 10"
            clipped = run(tag + "_b", per, 0.5 * norm)
            assert abs(clipped - norm) <= 1e-6 * norm and clipped > 0.5 * norm, (clipped, norm)
            print(prefix, tag, "norm", norm, "|delta| < 1:", small, "> 1:", large)
    from tests.golden_parts import save_parts
    written = save_parts(OUT, out)
    print("wrote", written, "lines", lines, "bytes", [os.path.getsize(p) for p in written])


if __name__ == "__main__":
    main()
