"""The descriptor compiler (csrc/net_image.h) on the CPU: every section of the table image and
every launch scalar against tests/golden/net_image.json, which was recorded from the
pbn_net_create that preceded the split (a dump added just before its first device call; the cases
at the descriptor's limits, added later, from the unchanged builder), and the stand-alone check
program (tests/net_image_check.cpp)."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from pbn_rl_amd.attractors import load_attractors, random_state_targets
from pbn_rl_amd.network import load_network
from pbn_rl_amd.spec import EnvSpec
from tests.synthetic import random_network, random_spec
from tests.table_limits import limit_spec

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "pbn_rl_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden", "net_image.json")

VECTORS = ["tab", "fcompact", "nrec", "sthr", "sthr_pk", "att_first", "uthr", "hash_mult"]
SCALARS = ["n_nodes", "W", "n_attr", "horizon", "cdf_len", "hash_bits", "hash_probes", "tab_words", "prob_bits",
           "n_funcs", "wave_words", "gap_exact", "gap_lut_off", "gap_shift", "gap_nb", "inv_log2q_bits", "n_states",
           "att_off", "sel_off", "nrec_off", "cm_off", "n_cls", "max_nf", "lq", "slot_words", "gate_off",
           "glayer_off", "n_glayers", "att_single", "n1_magic", "am1_magic", "x_mult", "settle_max", "settle_pk",
           "n_gates", "slot_words_settle", "lds_wave", "lds_pipe", "lds_settle"]


def cases():
    """(name, spec factory): the smallest specs that reach each path of the builder."""
    def bundled(name, **kw):
        return lambda: EnvSpec(load_network(name), load_attractors(name), **kw)

    def wide():
        net = random_network(12, 7, max_funcs=3, max_arity=7)
        return EnvSpec(net, random_state_targets(12, 4, 8))

    out = [(name, bundled(name)) for name in ("pbn7", "pbn10", "pbn28", "pbn70", "bb33", "m47")]
    out += [(f"pbn28_bits{b}", bundled("pbn28", prob_bits=b)) for b in (4, 8, 12, 16)]
    out += [(f"pbn28_p{p}", bundled("pbn28", perturbation=p)) for p in (0.0, 0.6, 0.01, 0.3)]
    out += [(f"pbn28_settle{k}", bundled("pbn28", settle=k)) for k in (0, 64)]
    out += [("pbn7_no_attractors", lambda: EnvSpec(load_network("pbn7"), None))]
    out += [(f"rand{n}", lambda n=n: random_spec(n, 100 + n, max_funcs=6)) for n in (5, 33, 70, 100)]
    out += [("wide12", wide)]
    # the descriptor's limits: hashes of 2 and 4 probes in 2^12 slots (the largest images: 150 KB of
    # LDS at four state words), and gates up to plane 255 at one, three and four state words
    out += [(name, lambda name=name: limit_spec(name)) for name in (
        "hold28_a254", "hold20_s1000", "hold100_a254", "collapse70", "gates32_limit", "gates70_limit",
        "gates128_limit")]
    return out


def sha(words) -> str:
    return hashlib.sha256(np.ascontiguousarray(words, dtype=np.uint32).tobytes()).hexdigest()


def summarise(scalars: dict, vectors: dict) -> dict:
    """The golden's record of one image: the scalars, and a SHA-256 of every vector and of every
    section of the table image (a section runs to the next one's offset, alignment included)."""
    sc, tab = scalars, np.asarray(vectors["tab"], dtype=np.uint32)
    assert tab.size == sc["tab_words"]
    starts = [("cdf", 0), ("reward_rows", sc["cdf_len"]), ("hash", sc["cdf_len"] + 4 * (sc["n_nodes"] + 1)),
              ("attractors", sc["att_off"]), ("selectors", sc["sel_off"]), ("node_records", sc["nrec_off"])]
    if sc["n_gates"]:
        starts += [("gates", sc["gate_off"]), ("gate_levels", sc["glayer_off"])]
    if sc["gap_nb"]:
        starts += [("gap_table", sc["gap_lut_off"])]
    if sc["W"] == 1:
        starts += [("digit_masks", sc["cm_off"])]
    offs = [o for _, o in starts] + [sc["tab_words"]]
    assert offs == sorted(offs), starts
    sections = {name: sha(tab[offs[i]:offs[i + 1]]) for i, (name, _) in enumerate(starts)}
    return {"scalars": {k: int(sc[k]) for k in SCALARS},
            "vectors": {k: sha(vectors[k]) for k in VECTORS},
            "sections": sections}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("net_image"))


def build_shim(folder):
    so = os.path.join(str(folder), "libnet_image.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", str(so),
                    os.path.join(HERE, "net_image_shim.cpp")], check=True)
    L = ctypes.CDLL(str(so))
    L.ni_compile.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_int]
    L.ni_compile.restype = ctypes.c_void_p
    L.ni_free.argtypes = [ctypes.c_void_p]
    L.ni_vector.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64)]
    L.ni_vector.restype = ctypes.POINTER(ctypes.c_uint32)
    L.ni_scalar.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)]
    L.ni_scalar.restype = ctypes.c_int
    return L


def compile_spec(L, spec):
    """(rc, error, summary or None) of compile_net on spec.desc."""
    rc, err, scalars, vectors = compile_raw(L, spec)
    return rc, err, (None if scalars is None else summarise(scalars, vectors))


def compile_raw(L, spec):
    """(rc, error, scalars, vectors) of compile_net on spec.desc; None twice where it refuses."""
    rc, err = ctypes.c_int(-1), ctypes.create_string_buffer(256)
    h = L.ni_compile(ctypes.addressof(spec.desc), ctypes.byref(rc), err, 256)
    if not h:
        return rc.value, err.value.decode(), None, None
    try:
        scalars, vectors = {}, {}
        for name in SCALARS:
            v = ctypes.c_uint64()
            assert L.ni_scalar(h, name.encode(), ctypes.byref(v)) == 1, name
            scalars[name] = v.value
        for name in VECTORS:
            n = ctypes.c_int64()
            p = L.ni_vector(h, name.encode(), ctypes.byref(n))
            assert n.value >= 0, name
            vectors[name] = np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, np.uint32)
        return rc.value, err.value.decode(), scalars, vectors
    finally:
        L.ni_free(h)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_lists_exactly_the_cases(golden):
    assert sorted(golden) == sorted(name for name, _ in cases())


@pytest.mark.parametrize("name,make", cases(), ids=[name for name, _ in cases()])
def test_image_matches_the_recorded_one(shim, golden, name, make):
    rc, err, got = compile_spec(shim, make())
    assert rc == 0, err
    want = golden[name]
    assert got["scalars"] == want["scalars"]
    assert got["sections"] == want["sections"]
    assert got["vectors"] == want["vectors"]


def test_cases_reach_every_builder_path(golden):
    sc = {name: g["scalars"] for name, g in golden.items()}
    assert {s["gap_exact"] for s in sc.values()} == {0, 1, 2}          # estimate, binary search, bucket table
    assert sc["pbn28_p0.0"]["gap_exact"] == 1 and sc["pbn28_p0.6"]["gap_exact"] == 1
    assert sc["pbn28_p0.01"]["gap_exact"] == 2
    assert {s["W"] for s in sc.values()} == {1, 2, 3, 4}
    assert {s["prob_bits"] for s in sc.values()} == {4, 8, 12, 16}
    assert any(s["max_nf"] > 4 for s in sc.values())                     # the MANY instances
    assert any(s["n_cls"] == 0 for s in sc.values()) and any(s["n_cls"] > 0 for s in sc.values())
    assert sc["pbn7_no_attractors"]["n_attr"] == 0 and sc["pbn7_no_attractors"]["hash_bits"] == 0
    assert sc["wide12"]["n_gates"] > 0 and sc["wide12"]["n_glayers"] >= 2
    assert sc["pbn28_settle64"]["settle_max"] == 64
    assert {s["hash_probes"] for s in sc.values()} == {0, 1, 2, 4}      # 0: no attractors
    assert sc["hold28_a254"]["hash_probes"] == 2 and sc["hold20_s1000"]["hash_probes"] == 4
    at_limit = [s for s in sc.values() if 32 * s["W"] + s["n_gates"] == 256]
    assert {s["W"] for s in at_limit} >= {1, 3, 4}                       # plane 255 is a gate's output
    assert all(s["wave_words"] == 256 and s["n_glayers"] == 4 for s in at_limit)
    assert {s["W"] for s in sc.values() if s["n_gates"]} == {1, 2, 3, 4}
    assert sc["hold100_a254"]["lds_settle"] > 160 * 1024 >= sc["hold100_a254"]["lds_pipe"] > 150 * 1024


def test_compile_reports_the_reason(shim):
    spec = EnvSpec(load_network("pbn7"), load_attractors("pbn7"))
    spec.arrays["perturb_cdf"][1] = 0   # found after the hash has been built
    rc, err, got = compile_spec(shim, spec)
    assert rc == -22 and "perturb_cdf must be non-decreasing" in err and got is None


def test_standalone_check_program(tmp_path):
    """Three hand-written descriptors through compile_net, and route_launch against the
    conditions of the launcher it replaced, in a program of its own (which is also what runs
    under the host sanitizers)."""
    exe = tmp_path / "net_image_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe),
                    os.path.join(HERE, "net_image_check.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "net_image_check: ok" in out.stdout
