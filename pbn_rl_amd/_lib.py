"""ctypes binding of libpbn_env.so, derived from include/pbn_env.h: the header's prototypes are
the one description of the ABI (declared()), and load() binds from them.

The HIP library is the only compute path: if it is missing or fails to load,
every entry point raises -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import functools
import os
import re
import subprocess
from typing import Dict, NamedTuple, Optional, Tuple

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libpbn_env.so")
SRC_DIR = os.path.join(HERE, "csrc")
INCLUDE_DIR = os.path.join(HERE, "..", "include")

MODE_AUTORESET = 1
MODE_RANDOM_ACTIONS = 2
FLAG_TERMINATED = 1
FLAG_TRUNCATED = 2
FLAG_IN_ATTRACTOR = 4
FLAG_PERTURBED = 8
FLAG_RESET = 16
FLAG_UNSETTLED = 32

SOURCES = ["pbn_env.hip", "pbn_settle.hip", "pbn_agent.hip", "pbn_qnet.hip", "pbn_learn.hip", "pbn_eval.hip",
           "pbn_per.hip", "pbn_ddqn.hip", "pbn_table.hip", "pbn_episode.hip", "pbn_curriculum.hip", "pbn_gbdq.hip",
           "pbn_cgbdq.hip"]

_lib: Optional[ctypes.CDLL] = None


class PbnError(RuntimeError):
    pass


class RingStore(ctypes.Structure):
    """pbn_ring_store (include/pbn_env.h, ABI 11): the replay ring pbn_step_dev_store writes the
    step's transitions into (pbn_replay_store's layout)."""
    _fields_ = [("capacity", ctypes.c_int64), ("d_pos", ctypes.c_void_p), ("d_state", ctypes.c_void_p),
                ("d_next_state", ctypes.c_void_p), ("d_target", ctypes.c_void_p), ("d_action", ctypes.c_void_p),
                ("d_reward", ctypes.c_void_p), ("d_done", ctypes.c_void_p), ("d_actions_in", ctypes.c_void_p),
                ("n_branches", ctypes.c_int32), ("done_mask", ctypes.c_uint32), ("d_done_out", ctypes.c_void_p)]


class FrameAdvance(ctypes.Structure):
    """pbn_frame_advance (include/pbn_env.h, ABI 9): the counters a captured learning frame's fused
    update advances in its last launch, and the next frame's replay rows it draws."""
    _fields_ = [("n_store", ctypes.c_int64), ("capacity", ctypes.c_int64), ("d_pos", ctypes.c_void_p),
                ("d_size", ctypes.c_void_p), ("d_step", ctypes.c_void_p), ("d_eps64", ctypes.c_void_p),
                ("d_eps32", ctypes.c_void_p), ("eps_final", ctypes.c_double), ("eps_step", ctypes.c_double),
                ("n_idx", ctypes.c_int64), ("seed", ctypes.c_uint64), ("d_counter", ctypes.c_void_p),
                ("d_idx", ctypes.c_void_p)]


def build(verbose: bool = False, out: str = LIB_PATH, defines=()) -> str:
    """Compile csrc/*.hip for gfx950 into pbn_rl_amd/libpbn_env.so (in-tree): one object per
    source, compiled in parallel, then one link.  ``defines`` builds a diagnostic variant (e.g.
    PBN_STAMPS) into another path."""
    import tempfile
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result",
             *[f"-D{d}" for d in defines]]
    with tempfile.TemporaryDirectory(prefix="pbn_build_") as tmp:
        objs, procs = [], []
        for f in SOURCES:
            obj = os.path.join(tmp, f.replace(".hip", ".o"))
            cmd = ["hipcc", *flags, "-c", "-o", obj, os.path.join(SRC_DIR, f)]
            if verbose:
                print(" ".join(cmd))
            procs.append((subprocess.Popen(cmd), cmd))
            objs.append(obj)
        rcs = [(p.wait(), cmd) for p, cmd in procs]   # all of them, before the directory goes
        for rc, cmd in rcs:
            if rc != 0:
                raise subprocess.CalledProcessError(rc, cmd)
        cmd = ["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out + ".tmp", *objs]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
    os.replace(out + ".tmp", out)
    return out


class Decl(NamedTuple):
    """One entry point as include/pbn_env.h declares it."""
    restype: object     # a ctypes type, or None for void
    argtypes: tuple     # one ctypes type per parameter
    params: tuple       # the parameters' names
    ctext: tuple        # the parameters as the header spells them, e.g. "const uint64_t* d_step"


_SCALARS = {"int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "int32_t": ctypes.c_int32,
            "uint32_t": ctypes.c_uint32, "float": ctypes.c_float, "double": ctypes.c_double, "int": ctypes.c_int}


def _ctype(ctext: str, what: str, returns: bool = False):
    """The binding's rule: any pointer is a c_void_p (a returned const char* a c_char_p), a scalar
    its ctypes twin; anything else is an error that names ``what``."""
    words = [w for w in ctext.replace("*", " * ").split() if w != "const"]
    if "*" in words:
        return ctypes.c_char_p if returns and words == ["char", "*"] else ctypes.c_void_p
    if returns and words == ["void"]:
        return None
    if len(words) != 1 or words[0] not in _SCALARS:
        raise PbnError(f"pbn_env.h: {what} has a type the binding does not know: '{ctext}'")
    return _SCALARS[words[0]]


def parse_header(text: str) -> Tuple[Dict[str, Decl], int]:
    """({function: Decl}, PBN_ABI_VERSION) of a header's text.  Every statement with a parameter
    list must parse as a prototype: a declaration is never dropped silently."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    version = re.search(r"^[ \t]*#[ \t]*define[ \t]+PBN_ABI_VERSION[ \t]+(\d+)", text, re.M)
    if not version:
        raise PbnError("pbn_env.h: PBN_ABI_VERSION is not defined")
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)    # preprocessor lines
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    text = re.sub(r"\{[^{}]*\}", " ", text)                    # struct bodies
    out: Dict[str, Decl] = {}
    for stmt in text.split(";"):
        if "(" not in stmt:
            continue
        m = re.fullmatch(r"\s*([\w\s*]+?)\s*\b(\w+)\s*\(([^()]*)\)\s*", stmt)
        if not m:
            raise PbnError(f"pbn_env.h: cannot parse '{' '.join(stmt.split())}'")
        ret, name, plist = m.groups()
        ctext = tuple(" ".join(p.split()) for p in plist.split(","))
        if ctext in (("void",), ("",)):
            ctext = ()
        names, argtypes = [], []
        for p in ctext:
            pm = re.fullmatch(r"(.*?)\b(\w+)", p)
            if not pm or not pm.group(1).strip():
                raise PbnError(f"pbn_env.h: {name}: cannot parse parameter '{p}'")
            names.append(pm.group(2))
            argtypes.append(_ctype(pm.group(1), f"{name}: parameter {pm.group(2)}"))
        out[name] = Decl(_ctype(ret, f"{name}: the return value", returns=True), tuple(argtypes), tuple(names), ctext)
    return out, int(version.group(1))


@functools.lru_cache(maxsize=None)
def _header() -> Tuple[Dict[str, Decl], int]:
    with open(os.path.join(INCLUDE_DIR, "pbn_env.h")) as f:
        return parse_header(f.read())


def declared() -> Dict[str, Decl]:
    """The C ABI, {function: Decl}, read once from include/pbn_env.h: the one description that
    load() binds from."""
    return _header()[0]


EXPORTS = list(declared())
ABI_VERSION = _header()[1]     # PBN_ABI_VERSION of the header


def load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("PBN_LIB", LIB_PATH)  # diagnostic builds only
    if not os.path.exists(path):
        raise PbnError(f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = ctypes.CDLL(path)
    for name, d in declared().items():
        if hasattr(L, name):   # (a diagnostic build of an older revision lacks the later exports)
            fn = getattr(L, name)
            fn.restype, fn.argtypes = d.restype, list(d.argtypes)
    want, got = ABI_VERSION, L.pbn_abi_version() if hasattr(L, "pbn_abi_version") else None
    if got != want:
        raise PbnError(f"{path} has ABI version {got}, include/pbn_env.h declares {want}: rebuild with "
                       "`python -c 'import __graft_entry__ as g; g.build()'`")
    _lib = L
    return L


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().pbn_last_error().decode(errors="replace")
        raise PbnError(f"{what} failed ({rc}): {msg}")


class NetHandle:
    """Owns one pbn_net (device tables) on the current device."""

    def __init__(self, spec):
        L = load()
        self.spec = spec
        h = ctypes.c_void_p()
        check(L.pbn_net_create(ctypes.addressof(spec.desc), ctypes.byref(h)), "pbn_net_create")
        self.handle = h
        self.words = L.pbn_net_words(h)

    def close(self) -> None:
        if getattr(self, "handle", None) is not None and self.handle.value:
            load().pbn_net_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
