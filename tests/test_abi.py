"""The C-ABI shared library: loads, exports every entry point of include/pbn_env.h,
and rejects bad descriptors / arguments before touching the device (no GPU needed)."""
import ctypes
import os
import re
import subprocess

import pytest

from pbn_rl_amd import _lib
from pbn_rl_amd.attractors import load_attractors
from pbn_rl_amd.network import load_network
from pbn_rl_amd.spec import EnvSpec, PbnNetDesc

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "pbn_env.h")


def declared_functions():
    text = open(HEADER).read()
    return sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(pbn_\w+)\s*\(", text, re.M)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_header_declares_the_abi():
    """The looser regex above finds what _lib.declared()'s parser finds: it drops no declaration."""
    assert declared_functions() == sorted(_lib.EXPORTS) == sorted(_lib.declared())


SYNTHETIC = """
/* a header in small: int pbn_in_a_comment(int x); */
#define PBN_ABI_VERSION 7
#define PBN_EINVAL (-22)
typedef struct pbn_pair { int64_t a, b; const float* p; } pbn_pair;
typedef struct pbn_net pbn_net;
int pbn_make(const pbn_pair* pair, pbn_net** out);
int pbn_many(pbn_net* net, uint64_t seed,   /* the key */
             int64_t n_envs,                // any count
             uint32_t mode, int32_t k, float slope, double beta,
             const uint8_t* d_flags, void* stream);
const char* pbn_why(void);
int pbn_version(void);
void pbn_quiet(int code);
"""


def test_parser_cases():
    """Comments between parameters, (void), a const char* return, a pointer to a pointer."""
    vp = ctypes.c_void_p
    fns, version = _lib.parse_header(SYNTHETIC)
    assert version == 7 and list(fns) == ["pbn_make", "pbn_many", "pbn_why", "pbn_version", "pbn_quiet"]
    assert fns["pbn_make"].argtypes == (vp, vp) and fns["pbn_make"].params == ("pair", "out")
    assert fns["pbn_make"].ctext == ("const pbn_pair* pair", "pbn_net** out")
    many = fns["pbn_many"]
    assert many.restype is ctypes.c_int
    assert many.argtypes == (vp, ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint32, ctypes.c_int32, ctypes.c_float,
                             ctypes.c_double, vp, vp)
    assert many.params == ("net", "seed", "n_envs", "mode", "k", "slope", "beta", "d_flags", "stream")
    assert fns["pbn_why"] == (ctypes.c_char_p, (), (), ())
    assert fns["pbn_version"] == (ctypes.c_int, (), (), ())
    assert fns["pbn_quiet"].restype is None and fns["pbn_quiet"].argtypes == (ctypes.c_int,)


def test_parser_names_an_unknown_type():
    with pytest.raises(_lib.PbnError, match=r"pbn_odd: parameter n .*'size_t"):
        _lib.parse_header(SYNTHETIC + "int pbn_odd(pbn_net* net, size_t n);\n")
    with pytest.raises(_lib.PbnError, match=r"pbn_odd: the return value"):
        _lib.parse_header(SYNTHETIC + "size_t pbn_odd(void);\n")
    with pytest.raises(_lib.PbnError, match="cannot parse"):      # not dropped: refused
        _lib.parse_header(SYNTHETIC + "int (*pbn_callback)(int);\n")


def test_every_declared_function_is_bound_as_declared(lib):
    assert _lib.ABI_VERSION == 11 and len(_lib.declared()) == len(declared_functions())
    for name, d in _lib.declared().items():
        assert len(d.argtypes) == len(d.params) == len(d.ctext), name
        assert d.restype is (ctypes.c_char_p if name == "pbn_last_error" else ctypes.c_int), name
        fn = getattr(lib, name)
        assert fn.restype is d.restype and tuple(fn.argtypes) == d.argtypes, name
        assert all(t is ctypes.c_void_p for t, c in zip(d.argtypes, d.ctext) if "*" in c), name


STALE = """
const char* pbn_last_error(void) { return "stale"; }
int pbn_abi_version(void) { return %d; }
"""


def _load_other(tmp_path, monkeypatch, version):
    """_lib.load() of a tiny library that reports `version` and exports nothing else."""
    src, so = tmp_path / f"v{version}.c", tmp_path / f"libv{version}.so"
    src.write_text(STALE % version)
    subprocess.run(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    monkeypatch.setenv("PBN_LIB", str(so))
    monkeypatch.setattr(_lib, "_lib", None)      # restored, with the real library, at teardown
    return _lib.load()


def test_load_refuses_a_stale_library(tmp_path, monkeypatch):
    with pytest.raises(_lib.PbnError) as e:
        _load_other(tmp_path, monkeypatch, 10)
    assert "ABI version 10" in str(e.value) and "declares 11" in str(e.value) and "g.build()" in str(e.value)
    assert _lib._lib is None


def test_load_leaves_missing_symbols_unbound(tmp_path, monkeypatch):
    L = _load_other(tmp_path, monkeypatch, 11)
    assert L.pbn_abi_version() == 11 and L.pbn_last_error() == b"stale"
    assert not hasattr(L, "pbn_step")


def test_library_exports_every_symbol(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (\w+)$", out, re.M))
    for name in declared_functions():
        assert name in exported, name
        assert hasattr(lib, name)


def test_abi_version(lib):
    assert lib.pbn_abi_version() == 11


def test_descriptor_layout_matches_header(tmp_path):
    """ctypes' mirrors of the three structs == the C compiler's (sizeof and every offsetof, from the
    header); a field a mirror lacks would move sizeof, one it adds does not compile."""
    inc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")
    for c_name, mirror, n_fields in [("pbn_net_desc", PbnNetDesc, 20), ("pbn_ring_store", _lib.RingStore, 12),
                                     ("pbn_frame_advance", _lib.FrameAdvance, 13)]:
        fields = [f for f, _ in mirror._fields_]
        assert len(fields) == n_fields, c_name
        src = tmp_path / f"{c_name}.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pbn_env.h"\nint main(void) {\n'
                       f'  printf("%zu\\n", sizeof({c_name}));\n' +
                       "".join(f'  printf("%zu\\n", offsetof({c_name}, {f}));\n' for f in fields) +
                       "  return 0;\n}\n")
        exe = tmp_path / c_name
        subprocess.run(["gcc", "-I", inc, "-o", str(exe), str(src)], check=True)
        got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
        assert got[0] == ctypes.sizeof(mirror), c_name
        assert got[1:] == [getattr(mirror, f).offset for f in fields], c_name


def _create(lib, spec):
    h = ctypes.c_void_p()
    rc = lib.pbn_net_create(ctypes.addressof(spec.desc), ctypes.byref(h))
    return rc, lib.pbn_last_error().decode()


@pytest.mark.parametrize("field,value,msg", [
    ("prob_bits", 5, "prob_bits"),
    ("horizon", 300, "horizon"),
    ("settle_max", 5000, "settle_max"),
    ("n_nodes", 0, "n_nodes"),
    ("n_attractors", 255, "n_attractors"),
])
def test_create_rejects_bad_descriptor(lib, field, value, msg):
    spec = EnvSpec(load_network("pbn28"), load_attractors("pbn28"))
    setattr(spec.desc, field, value)
    rc, err = _create(lib, spec)
    assert rc == -22 and msg in err


def test_create_rejects_bad_thresholds(lib):
    spec = EnvSpec(load_network("pbn7"), load_attractors("pbn7"))
    last = spec.arrays["node_func_start"][1] - 1
    spec.arrays["func_threshold"][last] = 1  # last threshold of node 0 must be 2^prob_bits
    rc, err = _create(lib, spec)
    assert rc == -22 and "threshold" in err


def _first_func(spec, min_funcs=1, min_arity=0):
    """(node, first function index) of the first node with at least min_funcs functions whose
    first function has at least min_arity inputs."""
    start, arity = spec.arrays["node_func_start"], spec.arrays["func_arity"]
    for i in range(spec.n):
        if start[i + 1] - start[i] >= min_funcs and arity[start[i]] >= min_arity:
            return i, int(start[i])
    raise AssertionError("no such node")


def _gate_arity(spec):
    spec.arrays["gate_arity"][0] = 5


def _gate_table_bits(spec):
    spec.arrays["gate_table"][0] |= 1 << 16


def _gate_input_order(spec):
    g = int((spec.arrays["gate_arity"] >= 1).argmax())
    spec.arrays["gate_inputs"][4 * g] = spec.n + g   # itself


def _func_start_span(spec):
    spec.arrays["node_func_start"][0] = 1


def _func_count(spec):
    spec.arrays["node_func_start"][1] = 0


def _func_arity(spec):
    spec.arrays["func_arity"][0] = 5


def _thresholds_decrease(spec):
    _, f0 = _first_func(spec, min_funcs=3)
    spec.arrays["func_threshold"][f0] = spec.arrays["func_threshold"][f0 + 1] + 1


def _input_range(spec):
    _, f0 = _first_func(spec, min_arity=1)
    spec.arrays["func_inputs"][4 * f0] = spec.n + int(spec.arrays["n_gates"][0])


def _table_bits(spec):
    spec.arrays["func_table"][0] |= 1 << 16


def _null_attractors(spec):
    spec.desc.attractor_start = None


def _attractor_start(spec):
    spec.arrays["attractor_start"][0] = 1


def _empty_attractor(spec):
    assert len(spec.attractors) >= 2
    spec.arrays["attractor_start"][1] = 0


def _cdf_decreases(spec):
    spec.arrays["perturb_cdf"][1] = 0


def _too_many_gates(spec):
    spec.desc.n_gates = 300


def _negative_gates(spec):
    spec.desc.n_gates = -1


N_GATES_MSG = "n_gates out of range (32 * W + n_gates must be <= 256)"


@pytest.mark.parametrize("network,mutate,msg", [
    ("bb33", _gate_arity, "gate arity must be 0..4"),
    ("bb33", _gate_table_bits, "gate truth table has bits beyond 2^arity"),
    ("bb33", _gate_input_order, "gate input must be a node or an earlier gate"),
    ("pbn7", _func_start_span, "node_func_start must span 0..n_funcs"),
    ("pbn7", _func_count, "node 0 needs 1..16 functions"),
    ("pbn7", _func_arity, "function arity must be 0..4"),
    ("pbn7", _thresholds_decrease, "thresholds must be non-decreasing and <= 2^prob_bits"),
    ("bb33", _input_range, "function input reference out of range"),
    ("pbn7", _table_bits, "truth table has bits beyond 2^arity"),
    ("pbn7", _null_attractors, "null attractor tables"),
    ("pbn7", _attractor_start, "bad attractor_start"),
    ("pbn28", _empty_attractor, "empty attractor"),
    ("pbn7", _cdf_decreases, "perturb_cdf must be non-decreasing"),
    ("pbn7", _too_many_gates, N_GATES_MSG),
    ("pbn7", _negative_gates, N_GATES_MSG),
], ids=lambda v: getattr(v, "__name__", None))
def test_create_rejects_with_the_reason(lib, network, mutate, msg):
    """Every rejection of the descriptor compiler through the real library (all of them come
    before the first device call), with the message pbn_last_error reports."""
    spec = EnvSpec(load_network(network), load_attractors(network))
    mutate(spec)
    rc, err = _create(lib, spec)
    assert rc == -22 and err == msg


def test_step_rejects_null_net(lib):
    rc = lib.pbn_step(None, 0, 0, 0, 32, 3, None, None, None, None, None, None, None, None, None)
    assert rc == -22
    assert lib.pbn_reset(None, 0, 0, 0, 32, None, None, None, None) == -22
