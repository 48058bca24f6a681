"""The fused BDQ update's layouts (csrc/bdq_layout.h) on the CPU: the flat parameter layout, the
network image, the workspace, the LDS carvings of learn_fwd and learn_bwd and learn_apply's tasks,
as the stand-alone program tests/bdq_layout_check.cpp prints them (built with the host sanitizers),
against this file's own statement of each.  The LDS totals and the task count are written out
here as the launcher stated them before the header existed: the duplication is deliberate, this
file is the second copy and the kernels no longer are."""
import json
import os
import subprocess

import pytest

from pbn_rl_amd.agent import BranchingQNetwork
from pbn_rl_amd.replay import _bdq_segments

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "pbn_rl_amd", "csrc")

SHAPES = [(1, 1), (15, 3), (16, 3), (28, 3), (31, 7), (95, 7), (96, 6), (96, 7), (127, 1), (127, 7)]
BATCHES = [16, 256]
N_ATTR = [0, 14]
LDS_LIMIT = 160 * 1024


def al16(x):
    return (x + 15) // 16 * 16


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """{(N, K, B, n_attr): the program's record}"""
    exe = tmp_path_factory.mktemp("bdq_layout") / "bdq_layout_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe),
                    os.path.join(HERE, "bdq_layout_check.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stderr == ""
    recs = [json.loads(line) for line in out.stdout.splitlines()]
    return {(r["N"], r["K"], r["B"], r["n_attr"]): r for r in recs}


def cases():
    return [(N, K, B, t) for N, K in SHAPES for B in BATCHES for t in N_ATTR]


def test_the_program_prints_exactly_the_sweep(dump):
    assert sorted(dump) == sorted(cases())
    for (N, K, B, t), r in dump.items():
        assert r["Apad"] == 16 * ((N + 1 + 15) // 16) and r["Apad"] >= N + 1 and r["Apad"] % 16 == 0
        assert r["W"] == (N + 31) // 32 and r["NT"] == (N + 15) // 16
    assert {r["Apad"] for r in dump.values()} == {16, 32, 96, 112, 128}       # both sides of 16, 32, 96, 112
    assert {r["W"] for r in dump.values()} == {1, 3, 4}
    assert {r["NT"] for r in dump.values()} == {1, 2, 6, 8}


@pytest.mark.parametrize("N,K", SHAPES)
def test_segment_offsets_are_the_modules_parameters(dump, N, K):
    """make_layout against a CPU BranchingQNetwork: the running 16-float-aligned sums of the
    segments' sizes, a segment being the parameters _bdq_segments puts into it, stacked at the
    offsets it gives them (a head every N + 1 rows of the second head layers: the value head's one
    row leaves the rest of its slot unused, so the segment is as long as K + 1 advantage heads)."""
    A = N + 1
    q = BranchingQNetwork((N, N), A, K)
    size = [0] * 12
    for p, seg, at in _bdq_segments(q):
        assert at >= size[seg], (seg, at)        # in order, none over another
        size[seg] = at + p.numel()
    assert size[10] == (K + 1) * A * 64 and size[11] == (K + 1) * A
    want, o = [], 0
    for s in size:
        want.append(o)
        o += al16(s)
    want.append(o)
    assert len(want) == 13
    for B in BATCHES:
        for t in N_ATTR:
            assert dump[(N, K, B, t)]["layout"] == want
    assert sum(p.numel() for p in q.parameters()) == sum(size) - (A - 1) * 65      # (the value head's slot)


@pytest.mark.parametrize("N,K,B,n_attr", cases())
def test_image_layout(dump, N, K, B, n_attr):
    r = dump[(N, K, B, n_attr)]
    H, Ap = K + 1, r["Apad"]
    shapes = [(128, 256), (64, 128), (32, 64), (H * 64, 32), (H * Ap, 64)]
    assert r["image_rows_cols"] == [x for rc in shapes for x in rc]
    assert r["image_total"] == n_attr * N * 256 + 2 * sum(R * C for R, C in shapes)
    o = n_attr * N * 256                      # the order _check_image (test_gpu_learn.py) walks
    for l, (R, C) in enumerate(shapes):
        assert r["image_fwd"][l] == o
        o += R * C
        assert r["image_bwd"][l] == o
        o += R * C
    assert o == r["image_total"]
    assert all(x % 4 == 0 for x in r["image_fwd"] + r["image_bwd"])      # float4 tiles


WORK_ORDER = ["heads", "y1", "h2", "h3", "h4", "hh", "dheads", "dhh", "dh4", "dh3", "dh2", "g1", "srow", "trow",
              "partial"]


@pytest.mark.parametrize("N,K,B,n_attr", cases())
def test_workspace(dump, N, K, B, n_attr):
    r = dump[(N, K, B, n_attr)]
    H, Ap, W = K + 1, r["Apad"], r["W"]
    need = {"heads": 3 * H * B * Ap, "y1": 256 * B, "h2": 128 * B, "h3": 64 * B, "h4": 32 * B, "hh": 64 * H * B,
            "dheads": H * Ap * B, "dhh": 64 * H * B, "dh4": 32 * B, "dh3": 64 * B, "dh2": 128 * B, "g1": 256 * B,
            "srow": W * B, "trow": W * B, "partial": B // 16}
    assert [name for name, _, _ in r["work"]] == WORK_ORDER
    ends = [at for _, at, _ in r["work"][1:]] + [r["work_total"]]
    for (name, at, elem), end in zip(r["work"], ends):
        assert at % 16 == 0, name
        assert elem == 4, name                         # floats and uint32 words alike
        assert end - at >= need[name], name            # ... which also keeps the regions apart
    assert r["work"][0][1] == 0
    assert r["work_total"] * 4 == sum(al16(n) for n in need.values()) * 4   # the byte count pbn_bdq_learn_workspace reports


def in_order(regions, sizes, end):
    """every region ends where the next one begins or before it; the last one by `end`"""
    assert [name for name, _ in regions] == list(sizes)
    assert regions[0][1] == 0
    starts = [at for _, at in regions]
    for (name, at), nxt in zip(regions, starts[1:] + [end]):
        assert at >= 0 and at + sizes[name] <= nxt, name


@pytest.mark.parametrize("N,K,B,n_attr", cases())
def test_fwd_lds(dump, N, K, B, n_attr):
    r = dump[(N, K, B, n_attr)]
    H, A = K + 1, N + 1
    f = r["fwd_lds"]
    nbias = 256 + 128 + 64 + 32 + 64 * H + H * A
    assert r["fwd_bias_floats"] == nbias
    sizes = {"y1": 256 * 16, "x2": 128 * 16, "x3": 64 * 16, "x4": 32 * 16, "xh": 64 * H * 16, "sw": 4 * 16,
             "stg": 16, "scnt": 16, "slist": 16 * 128 // 4, "sbias": nbias + 1}     # 4-byte words
    in_order(f["regions"], sizes, f["end"])
    at = dict(f["regions"])
    for name in ("y1", "x2", "x3", "x4", "xh"):         # read as float4
        assert at[name] * 4 % 16 == 0, name
    # learn_launch's lds_f before the header existed
    lds_f = ((256 + 128 + 64 + 32 + 64 * H) * 16 + 4 * 16 + 2 * 16) * 4 + 16 * 128 + (nbias + 1) * 4
    assert f["bytes"] == lds_f == f["end"] * 4
    assert f["bytes"] <= LDS_LIMIT                      # every accepted shape: no new refusal
    # the bias order, next to the carving: [bilinear | 128 | 64 | 32 | H x 64 | H x A] of the segments
    off = r["layout"]
    want = []
    for seg, n in ((1, 256), (3, 128), (5, 64), (7, 32), (9, 64 * H), (11, H * A)):
        want += [off[seg] + i for i in range(n)]
    assert r["fwd_bias_src"] == want


def test_fwd_lds_at_the_largest_shape(dump):
    assert 72 * 1024 < dump[(127, 7, 256, 14)]["fwd_lds"]["bytes"] < 76 * 1024      # "about 74 KB"


@pytest.mark.parametrize("N,K,B,n_attr", cases())
def test_bwd_lds(dump, N, K, B, n_attr):
    r = dump[(N, K, B, n_attr)]
    H, Ap = K + 1, r["Apad"]
    b = r["bwd_lds"]
    at = dict(b["regions"])
    # the delta planes and the split tiles, in order, up to planes_end ...
    planes = {"dh": H * Ap * 16, "dhh": 64 * H * 16, "dh4": 32 * 16, "dh3": 64 * 16, "dh2": 128 * 16,
              "part": 8 * 64 * 4}
    in_order(b["regions"][:6], planes, at["planes_end"])
    # ... the staged head rows over the same space ...
    sh, pitch, staged = r["bwd_staged"]
    assert sh == 0 and pitch == Ap + 4 and pitch % 4 == 0 and staged == 3 * H * 16 * pitch
    # ... and the TD values past both
    assert at["sg"] >= at["planes_end"] and at["sg"] >= staged
    in_order([["sg", 0], ["sd", at["sd"] - at["sg"]], ["sact", at["sact"] - at["sg"]]],
             {"sg": 16 * K, "sd": 16 * K, "sact": 16 * K}, b["end"] - at["sg"])
    for name in ("dh", "dhh", "dh4", "dh3", "dh2", "part"):     # read as float4 (the staged rows: pitch % 4)
        assert at[name] * 4 % 16 == 0, name
    # learn_bwd_lds before the header existed
    planes_f = (H * Ap + H * 64 + 32 + 64 + 128) * 16 + 8 * 64 * 4
    staged_f = 3 * H * 16 * (Ap + 4)
    lds_b = (max(planes_f, staged_f) + 3 * 16 * K) * 4
    assert b["bytes"] == lds_b == b["end"] * 4
    assert r["bwd_refused"] == (lds_b > LDS_LIMIT)


def test_bwd_lds_on_both_sides_of_the_refusal(dump):
    got = {(N, K): dump[(N, K, 16, 0)]["bwd_lds"]["bytes"] for N, K in SHAPES}
    assert got[(95, 7)] == 154944 <= LDS_LIMIT
    assert got[(96, 6)] == 157056 <= LDS_LIMIT
    assert got[(96, 7)] == 179520 > LDS_LIMIT
    assert [nk for nk in SHAPES if dump[nk + (16, 0)]["bwd_refused"]] == [(96, 7), (127, 7)]


@pytest.mark.parametrize("N,K", SHAPES)
def test_apply_tasks(dump, N, K):
    r = dump[(N, K, 16, 0)]
    H, Ap = K + 1, r["Apad"]
    # learn_launch's ntasks before the header existed
    ntasks = (16 * N + (128 // 16) * (256 // 16) + (64 // 16) * (128 // 16) + (32 // 16) * (64 // 16) +
              (H * 64 // 16) * (32 // 16) + H * (Ap // 16) * (64 // 16))
    assert r["apply_bil"] + sum(r["apply_tiles"]) == r["apply_tasks"] == ntasks
    assert r["apply_blocks"] == (ntasks + r["apply_waves"] - 1) // r["apply_waves"]
    for other in dump.values():
        if (other["N"], other["K"]) == (N, K):
            assert (other["apply_bil"], other["apply_tiles"], other["apply_tasks"]) == \
                   (r["apply_bil"], r["apply_tiles"], r["apply_tasks"])
    # every task lands in one tile of one layer, every tile is some task's
    rows_cols = {-1: (256, 16 * N)}                    # the bilinear layer: (output tile, input i)
    rows_cols.update({l: (r["image_rows_cols"][2 * l], r["image_rows_cols"][2 * l + 1]) for l in range(5)})
    seen = set()
    assert len(r["decode"]) == ntasks
    for lay, ot, kt in r["decode"]:
        R, C = rows_cols[lay]
        assert 0 <= ot and ot * 16 < R and 0 <= kt and kt * 16 < C, (lay, ot, kt)
        assert (lay, ot, kt) not in seen
        seen.add((lay, ot, kt))
    assert len(seen) == sum(R // 16 * (C // 16) for R, C in rows_cols.values())
    assert [lay for lay, _, _ in r["decode"]] == sorted(lay for lay, _, _ in r["decode"])   # layer by layer
    assert r["decode_past"] == 5                       # the last block's spare waves: no layer
