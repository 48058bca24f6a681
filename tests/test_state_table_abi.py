"""pbn_table_insert in the C-ABI (no GPU needed): the symbol is exported under an unchanged ABI
version, and every argument error is rejected with its reason before any device call (all device
pointers are null here), while an empty input is accepted."""
import ctypes
import os
import re
import subprocess

import pytest

from pbn_rl_amd import _lib


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def call(lib, **over):
    a = dict(states=None, n_rows=3, n_cols=40, col_stride=64, n_words=2, n_bits=40, row_counts=None, capacity=1024,
             owner=None, keys=None, counts=None, used=None, lost=None, epoch=1, stream=None)
    a.update(over)
    return lib.pbn_table_insert(*a.values()), lib.pbn_last_error().decode()


def test_table_insert_is_exported_and_the_abi_version_stays(lib):
    assert "pbn_table_insert" in _lib.EXPORTS and "pbn_table.hip" in _lib.SOURCES
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert "pbn_table_insert" in set(re.findall(r" T (\w+)$", out, re.M))
    assert hasattr(lib, "pbn_table_insert") and lib.pbn_table_insert.argtypes is not None
    assert lib.pbn_abi_version() == 11
    decl = _lib.declared()["pbn_table_insert"]
    assert decl.restype is ctypes.c_int and tuple(lib.pbn_table_insert.argtypes) == decl.argtypes
    assert len(decl.params) == 15 and _lib.ABI_VERSION == 11


@pytest.mark.parametrize("over,msg", [
    (dict(n_words=0), "n_words must be 1..4"),
    (dict(n_words=5, n_bits=130), "n_words must be 1..4"),
    (dict(n_bits=32), "n_bits must be in 32 (n_words - 1) + 1 .. 32 n_words"),
    (dict(n_bits=65), "n_bits must be in 32 (n_words - 1) + 1 .. 32 n_words"),
    (dict(n_words=1, n_bits=0), "n_bits must be in 32 (n_words - 1) + 1 .. 32 n_words"),
    (dict(capacity=1000), "capacity must be a power of two, at least 64"),
    (dict(capacity=32), "capacity must be a power of two, at least 64"),
    (dict(capacity=0), "capacity must be a power of two, at least 64"),
    (dict(capacity=-64), "capacity must be a power of two, at least 64"),
    (dict(epoch=0), "epochs start at 1"),
    (dict(n_rows=1 << 16, n_cols=1 << 16, col_stride=1 << 16), "n_rows * n_cols must be below 2^32 - 1"),
    (dict(n_rows=1, n_cols=(1 << 32) - 1, col_stride=1 << 32), "n_rows * n_cols must be below 2^32 - 1"),
    (dict(n_rows=1 << 40, n_cols=1 << 40, col_stride=1 << 40), "n_rows * n_cols must be below 2^32 - 1"),
    (dict(col_stride=39), "col_stride < n_cols"),
    (dict(n_rows=-1), "n_rows < 0 or n_cols < 0"),
    (dict(n_cols=-1), "n_rows < 0 or n_cols < 0"),
    (dict(), "null buffer"),
], ids=lambda v: None if isinstance(v, str) else ("-".join(f"{k}={x}" for k, x in v.items()) or "null-buffers"))
def test_table_insert_rejects_with_the_reason(lib, over, msg):
    rc, err = call(lib, **over)
    assert rc == -22 and msg in err, (rc, err)


@pytest.mark.parametrize("over", [dict(n_rows=0), dict(n_cols=0), dict(n_rows=0, n_cols=0, col_stride=0)])
def test_table_insert_accepts_an_empty_input_without_a_launch(lib, over):
    rc, _ = call(lib, **over)      # (null buffers: a launch would have been rejected)
    assert rc == 0


def test_largest_row_count_passes_the_row_check(lib):
    """2^32 - 2 rows are allowed: the call gets as far as the buffers."""
    rc, err = call(lib, n_rows=2, n_cols=(1 << 31) - 1, col_stride=1 << 31)
    assert rc == -22 and err == "null buffer"
