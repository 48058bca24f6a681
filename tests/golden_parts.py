"""Golden archives stored in parts, each below the repository's 1 MiB limit per committed file.

``save_parts(path, arrays)`` writes ``name.npz``, ``name.part2.npz``, ... (np.savez_compressed);
an array above PIECE bytes is cut along its first axis into pieces ``key@0``, ``key@1``, ...
``load_parts(path)`` reads them back into one dict with the arrays whole again.
"""
import os

import numpy as np

PART = 900 * 1024    # raw bytes per part (float weights barely compress; the zip adds ~100 B per entry)
PIECE = 256 * 1024   # raw bytes per stored array


def _part_path(path: str, i: int) -> str:
    return path if i == 1 else f"{path[:-len('.npz')]}.part{i}.npz"


def save_parts(path: str, arrays: dict) -> list:
    assert path.endswith(".npz") and not any("@" in k for k in arrays)
    pieces = []
    for key, a in arrays.items():
        a = np.asarray(a)
        if a.nbytes <= PIECE or a.ndim == 0:
            pieces.append((key, a))
            continue
        rows = max(1, PIECE // (a.nbytes // a.shape[0]))
        for j, lo in enumerate(range(0, a.shape[0], rows)):
            pieces.append((f"{key}@{j}", a[lo:lo + rows]))
    parts, size = [{}], 0
    for key, a in pieces:
        if parts[-1] and size + a.nbytes > PART:
            parts.append({})
            size = 0
        parts[-1][key] = a
        size += a.nbytes
    i = len(parts) + 1
    while os.path.exists(_part_path(path, i)):    # parts of an earlier, larger archive
        os.remove(_part_path(path, i))
        i += 1
    written = []
    for i, part in enumerate(parts, 1):
        np.savez_compressed(_part_path(path, i), **part)
        written.append(_part_path(path, i))
    return written


def load_parts(path: str) -> dict:
    stored, i = {}, 1
    while os.path.exists(_part_path(path, i)):
        with np.load(_part_path(path, i)) as z:
            stored.update({k: z[k] for k in z.files})
        i += 1
    if not stored:
        raise FileNotFoundError(path)
    out, cut = {}, {}
    for key, a in stored.items():
        if "@" in key:
            name, j = key.rsplit("@", 1)
            cut.setdefault(name, {})[int(j)] = a
        else:
            out[key] = a
    for name, pieces in cut.items():
        out[name] = np.concatenate([pieces[j] for j in range(len(pieces))], axis=0)
    return out
