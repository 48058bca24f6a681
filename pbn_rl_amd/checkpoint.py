"""Checkpoint and resume of a training run (DESIGN.md "Checkpoint and resume").

A run's state is the learner's ``state_dict()``: a flat ``{name: CPU tensor | int | float | list}`` put
together from the ``state_dict()`` of every stateful piece (the env, the ring and its priority trees,
the update's flat buffers and Adam state, the episode statistics, the curriculum table, the learner's
own counters).  ``save`` writes it as one uncompressed ``.npz``: every tensor an array under its name,
dtype kept, and one more array, ``header``, the UTF-8 bytes of a JSON object with the format version,
the fingerprint of the learner that wrote the file and the host values.  The file is read with
``allow_pickle=False``: nothing in it is executed.  It is written under a temporary name in the same
directory and moved into place with ``os.replace``, so a killed job leaves the last good file.

``load`` is for a learner built with the arguments of the one that saved: the env, its spec and the
hyper-parameters are not in the file.  It reads the whole file, compares the fingerprint, the names,
shapes and dtypes, and the learner's own conditions (``_check_loadable``) before it writes anything,
and then writes in place (``copy_`` / ``fill_``): a captured hipGraph holds raw pointers.

``save_reference_bdq`` / ``save_reference_ddqn`` write the reference's own files beside ours
(bdq_model/__init__.py:237-244: ``torch.save`` of the ``q.*`` / ``target.*`` state dict;
ddqn_per/__init__.py:130-153: ``_make_save_dict``'s 16 keys).
"""
from __future__ import annotations

import hashlib
import json
import os
from typing import Dict, Tuple

import numpy as np
import torch

from . import _lib

__all__ = ["FORMAT", "FORMAT_VERSION", "REFERENCE_DDQN_KEYS", "cpu_copy", "fingerprint", "check_fingerprint",
           "write_checkpoint", "read_checkpoint", "read_header", "save", "load", "latest", "checkpoint_name",
           "save_reference_bdq", "save_reference_ddqn"]

FORMAT = "pbn_rl_amd.checkpoint"
FORMAT_VERSION = 1
HEADER = "header"

# DDQN._make_save_dict's keys, in its order
REFERENCE_DDQN_KEYS = ("params", "policy_kwargs", "input_size", "output_size", "buffer_size", "batch_size", "epsilon",
                       "target_update", "gamma", "max_epsilon", "min_epsilon", "exploration_fraction", "learning_rate",
                       "max_grad_norm", "train_steps", "num_timesteps")

# the fingerprint's fields in the order a mismatch is looked for
FIELDS = ("agent", "network", "table_hash", "n_attractors", "num_envs", "n_alloc", "words", "capacity", "batch_size",
          "branches", "net_arch", "fused", "prioritised", "episode_stats", "curriculum", "settle", "seed",
          "abi_version")


def cpu_copy(t: torch.Tensor) -> torch.Tensor:
    """A CPU copy that shares nothing with ``t`` (what every ``state_dict()`` here returns)."""
    return t.detach().to("cpu", copy=True)


# ------------------------------------------------------------------------------------ fingerprint
def table_hash(spec) -> str:
    """sha256 over the spec's compiled arrays (what ``pbn_net_create`` is given), names and dtypes
    included; a spec without them (a test stub) hashes its attractors."""
    h = hashlib.sha256()
    arrays = getattr(spec, "arrays", None)
    if arrays is None:
        h.update(repr(getattr(spec, "attractors", None)).encode())
        return h.hexdigest()
    for k in sorted(arrays):
        a = np.ascontiguousarray(arrays[k])
        h.update(f"{k}:{a.dtype.str}:{a.shape};".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def fingerprint(learner) -> dict:
    """What a checkpoint must share with the learner it is loaded into."""
    env, rp = learner.env, learner.replay
    spec = env.spec
    fp = {"agent": learner.agent_kind,
          "network": str(getattr(getattr(spec, "network", None), "name", "")),
          "table_hash": table_hash(spec),
          "n_attractors": len(spec.attractors),
          "num_envs": int(env.num_envs), "n_alloc": int(env.n_alloc), "words": int(env.words),
          "capacity": int(rp.capacity), "batch_size": int(learner.batch_size),
          "branches": int(rp.action.shape[1]),
          "net_arch": [list(a) for a in getattr(learner.q, "net_arch", [])],
          "fused": learner.fused is not None, "prioritised": bool(learner.prioritised),
          "episode_stats": learner.stats is not None, "curriculum": learner.curriculum is not None,
          "settle": int(getattr(spec, "settle", 0)), "seed": int(learner.seed),
          "abi_version": int(_lib.ABI_VERSION)}
    return fp


def check_fingerprint(saved: dict, own: dict) -> None:
    """ValueError naming every field in which the file and the learner differ (the agent alone when
    that differs: the other fields then describe different things)."""
    if saved.get("agent") != own.get("agent"):
        raise ValueError(f"checkpoint mismatch: agent (the file was written by a {saved.get('agent')!r} learner, this "
                         f"one is {own.get('agent')!r})")
    wrong = [f"{k} (file {saved.get(k)!r}, learner {own.get(k)!r})" for k in FIELDS if saved.get(k) != own.get(k)]
    if wrong:
        raise ValueError("checkpoint mismatch: " + "; ".join(wrong))


# ------------------------------------------------------------------------------------ the file
def write_checkpoint(path: str, header: dict, arrays: Dict[str, np.ndarray]) -> None:
    """One uncompressed ``.npz``: ``arrays`` plus ``header`` (the JSON bytes).  Written under a
    temporary name in ``path``'s directory, flushed to disk, then moved over ``path``."""
    if HEADER in arrays:
        raise ValueError(f"an array may not be named {HEADER!r}")
    path = os.fspath(path)
    blob = np.frombuffer(json.dumps(header, sort_keys=True).encode("utf-8"), dtype=np.uint8)
    tmp = f"{path}.{os.getpid()}.tmp"
    try:
        with open(tmp, "wb") as f:
            np.savez(f, **{HEADER: blob}, **arrays)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def _header_of(z, path) -> dict:
    if HEADER not in z.files:
        raise ValueError(f"{path}: no {HEADER!r} array: not a {FORMAT} file")
    header = json.loads(np.asarray(z[HEADER]).tobytes().decode("utf-8"))
    if header.get("format") != FORMAT:
        raise ValueError(f"{path}: format {header.get('format')!r}, expected {FORMAT!r}")
    if header.get("version") != FORMAT_VERSION:
        raise ValueError(f"{path}: format version {header.get('version')!r}, this code reads {FORMAT_VERSION}")
    return header


def read_header(path: str) -> dict:
    """The header alone (format, version, fingerprint, host values); no GPU is touched."""
    try:
        with np.load(path, allow_pickle=False) as z:
            return _header_of(z, path)
    except ValueError:
        raise
    except Exception as e:   # a torn zip: BadZipFile, EOFError, OSError, KeyError ...
        raise ValueError(f"{path}: unreadable checkpoint ({type(e).__name__}: {e})") from e


def read_checkpoint(path: str) -> Tuple[dict, Dict[str, np.ndarray]]:
    """(header, arrays), every array read into memory; ValueError if any of it cannot be read."""
    try:
        with np.load(path, allow_pickle=False) as z:
            header = _header_of(z, path)
            arrays = {k: np.asarray(z[k]) for k in z.files if k != HEADER}
    except ValueError as e:
        if str(e).startswith(os.fspath(path)):
            raise
        raise ValueError(f"{path}: unreadable checkpoint ({type(e).__name__}: {e})") from e
    except Exception as e:
        raise ValueError(f"{path}: unreadable checkpoint ({type(e).__name__}: {e})") from e
    return header, arrays


# ------------------------------------------------------------------------------------ save / load
def _split(state: dict) -> Tuple[Dict[str, np.ndarray], dict]:
    arrays, host = {}, {}
    for k, v in state.items():
        if isinstance(v, torch.Tensor):
            arrays[k] = v.numpy()
        else:
            host[k] = v
    return arrays, host


def save(learner, path: str) -> None:
    """``learner.save``: the stream's work is finished first, then the state is copied out and written."""
    dev = torch.device(learner.env.device)
    if dev.type == "cuda":
        torch.cuda.current_stream(dev).synchronize()
    arrays, host = _split(learner.state_dict())
    header = {"format": FORMAT, "version": FORMAT_VERSION, "fingerprint": fingerprint(learner), "host": host}
    write_checkpoint(path, header, arrays)


def load(learner, path: str) -> dict:
    """``learner.load``: every refusal comes before the first write.  Returns the header."""
    header, arrays = read_checkpoint(path)
    check_fingerprint(header["fingerprint"], fingerprint(learner))
    own_arrays, own_host = _split(learner.state_dict())
    host = header["host"]
    for what, have, want in (("array", arrays, own_arrays), ("host value", host, own_host)):
        missing, extra = sorted(set(want) - set(have)), sorted(set(have) - set(want))
        if missing or extra:
            raise ValueError(f"{path}: checkpoint mismatch: {what}s missing {missing}, unexpected {extra}")
    for k, a in own_arrays.items():
        b = arrays[k]
        if a.shape != b.shape or a.dtype != b.dtype:
            raise ValueError(f"{path}: checkpoint mismatch: {k} is {b.dtype}{list(b.shape)} in the file, "
                             f"{a.dtype}{list(a.shape)} in the learner")
    learner._check_loadable(host)
    state = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in arrays.items()}
    state.update(host)
    learner.load_state_dict(state)
    return header


def checkpoint_name(frames: int) -> str:
    return f"ckpt_{int(frames):010d}.npz"


def latest(directory: str):
    """The checkpoint of ``directory`` with the highest frame number in its name, or None."""
    best = None
    for name in os.listdir(directory) if os.path.isdir(directory) else []:
        if name.startswith("ckpt_") and name.endswith(".npz") and name[5:-4].isdigit():
            if best is None or int(name[5:-4]) > best[0]:
                best = (int(name[5:-4]), os.path.join(directory, name))
    return best[1] if best else None


# ------------------------------------------------------------------------------------ the reference's files
def _atomic_torch_save(obj, path: str) -> None:
    path = os.fspath(path)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    tmp = f"{path}.{os.getpid()}.tmp"
    try:
        torch.save(obj, tmp)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def save_reference_bdq(learner, path: str) -> None:
    """``BranchingDQN.save`` (bdq_model/__init__.py:240-244): ``torch.save`` of a dict of CPU tensors
    with the module's ``state_dict()`` keys, ``q.*`` then ``target.*``; ``load_bdq_checkpoint`` and
    the reference's ``load_state_dict`` read it."""
    sd = {}
    for prefix, net in (("q.", learner.q), ("target.", learner.target)):
        for k, v in net.state_dict().items():
            sd[prefix + k] = cpu_copy(v)
    _atomic_torch_save(sd, path)


def save_reference_ddqn(learner, directory: str, *, max_epsilon: float = 1.0, exploration_fraction: float = None,
                        learning_rate: float = None) -> str:
    """``DDQN.save`` (ddqn_per/__init__.py:130-153): ``ddqn_{num_timesteps}.pt`` in ``directory``, a
    dict with ``_make_save_dict``'s keys.  ``num_timesteps`` and ``train_steps`` are the learner's
    frames and updates (one frame is one global_step for every env).  Returns the path."""
    if exploration_fraction is None:    # (max - min) / (fraction * total_frames) is what the learner keeps
        exploration_fraction = (max_epsilon - learner.min_epsilon) / (learner.epsilon_decrement * learner.total_frames)
    if learning_rate is None:
        learning_rate = learner.fused.lr if learner.fused is not None else learner.opt.param_groups[0]["lr"]
    q = learner.q
    values = {"params": {k: cpu_copy(v) for k, v in q.state_dict().items()},
              "policy_kwargs": {"net_arch": [tuple(a) for a in q.net_arch]},
              "input_size": q.input_size, "output_size": q.output_size,
              "buffer_size": learner.replay.capacity, "batch_size": learner.batch_size,
              "epsilon": learner.epsilon, "target_update": learner.target_update, "gamma": learner.gamma,
              "max_epsilon": float(max_epsilon), "min_epsilon": learner.min_epsilon,
              "exploration_fraction": float(exploration_fraction), "learning_rate": float(learning_rate),
              "max_grad_norm": learner.max_grad_norm, "train_steps": learner.updates,
              "num_timesteps": learner.frames}
    out = os.path.join(os.fspath(directory), f"ddqn_{learner.frames}.pt")
    _atomic_torch_save({k: values[k] for k in REFERENCE_DDQN_KEYS}, out)
    return out
