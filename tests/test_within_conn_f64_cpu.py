"""The f64 `within` set, SearchConnectivity and unwrap_connectivity entries as far as they can be checked without a GPU:
the four symbols in the loader's table, the built library and the header, the Python methods, the argument checks that
come before any device call, and the Rust bindings."""
import ctypes as C
import os
import re

import numpy as np

from molar_amd import _lib
from molar_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("molar_hip_within_count_f64", "molar_hip_within_fill_f64", "molar_hip_search_connectivity_f64",
         "molar_hip_unwrap_connectivity_f64")
ERR_INVALID_ARGUMENT = 50


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "molar_hip.h")).read()
    lib = _lib.load()                                    # binds every symbol of SYMBOLS: raises if one is not exported
    for name in NAMES:
        assert name in _lib.SYMBOLS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert getattr(lib, name) is not None
    # the CSR is uint64 in both precisions: one fill call, no f64 twin
    assert "molar_hip_search_connectivity_fill_f64" not in header


def test_python_methods_exist():
    for name in ("within_set_f64", "search_connectivity_f64"):
        assert callable(getattr(api.Engine, name)), name
    assert callable(api.MeasureF64.unwrap_connectivity)


def test_null_arguments_are_rejected_before_any_device_call():
    lib = _lib.load()
    d = _lib.SearchDescF64()
    cnt = C.c_uint64(7)
    assert lib.molar_hip_within_count_f64(None, C.byref(d), C.byref(cnt)) == ERR_INVALID_ARGUMENT
    assert "null" in _lib.last_error()
    rows, ent = C.c_uint64(0), C.c_uint64(0)
    assert lib.molar_hip_search_connectivity_f64(None, C.byref(d), C.byref(rows), C.byref(ent)) == ERR_INVALID_ARGUMENT
    assert "null" in _lib.last_error()
    xyz = np.zeros((4, 3)); box9 = np.eye(3).reshape(9) * 5.0
    ng = C.c_size_t(0)
    assert lib.molar_hip_unwrap_connectivity_f64(None, xyz.ctypes.data, 4, None, 0, box9.ctypes.data, 0.2, 7, None, None,
                                                 C.byref(ng)) == ERR_INVALID_ARGUMENT
    assert "null" in _lib.last_error()
    # a fill without a count (no context at all here) is "no search", not a crash
    ids = np.zeros(4, np.uint64)
    assert lib.molar_hip_within_fill_f64(None, ids.ctypes.data) != 0


def test_null_descriptor_is_rejected_before_any_device_call():
    """A context pointer that is never dereferenced: the NULL descriptor is refused first."""
    lib = _lib.load()
    fake = C.c_void_p(0x1000)
    cnt = C.c_uint64(0)
    assert lib.molar_hip_within_count_f64(fake, None, C.byref(cnt)) == ERR_INVALID_ARGUMENT
    assert "null" in _lib.last_error()
    rows, ent = C.c_uint64(0), C.c_uint64(0)
    assert lib.molar_hip_search_connectivity_f64(fake, None, C.byref(rows), C.byref(ent)) == ERR_INVALID_ARGUMENT
    assert "null" in _lib.last_error()
    ng = C.c_size_t(0)
    box9 = np.eye(3).reshape(9) * 5.0
    assert lib.molar_hip_unwrap_connectivity_f64(fake, None, 4, None, 0, box9.ctypes.data, 0.2, 7, None, None,
                                                 C.byref(ng)) == ERR_INVALID_ARGUMENT
    assert "null" in _lib.last_error()


def test_rust_bindings_name_the_entries():
    ffi = open(os.path.join(ROOT, "rust", "molar_hip", "src", "ffi.rs")).read()
    for name in NAMES:
        assert name in ffi, name
    lib_rs = open(os.path.join(ROOT, "rust", "molar_hip", "src", "lib.rs")).read()
    for name in ("within_set_f64", "search_connectivity_f64", "unwrap_connectivity_f64"):
        assert re.search(r"pub fn %s\b" % name, lib_rs), name
