"""The neighbour-shell options of the chained membrane frame (molar_hip_membrane_plan_set_shells) through every layer
that has no GPU in it: declared in the C header, exported by the library, bound in molar_amd._lib and in the generated
Rust table, and mirrored by the C++ and Rust MembraneFrames and the Python MembranePlan."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "molar_hip_membrane_plan_set_shells"


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_declared_with_the_documented_signature():
    text = re.sub(r"\s+", " ", read("include", "molar_hip.h"))
    assert f"int {NAME}(molar_hip_membrane_plan *plan, size_t n_shells_patch, size_t n_shells_smoothing);" in text


def test_exported_by_a_fresh_build_and_bound():
    from molar_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    assert hasattr(lib, NAME)
    restype, argtypes = _lib.SYMBOLS[NAME]
    assert restype is C.c_int and list(argtypes) == [C.c_void_p, C.c_size_t, C.c_size_t]
    # a null plan is refused without touching a device
    assert getattr(lib, NAME)(None, 1, 1) != 0


def test_in_the_generated_rust_table():
    ffi = read("rust", "molar_hip", "src", "ffi.rs")
    assert "pub membrane_plan_set_shells: unsafe extern \"C\" fn(*mut MolarHipMembranePlan, usize, usize) -> c_int," in ffi
    assert f'b"{NAME}\\0"' in ffi


def test_mirrors_have_set_shells():
    hpp = read("include", "molar_hip.hpp")
    assert re.search(r"void set_shells\(size_t n_shells_patch, size_t n_shells_smoothing\)\s*\{\s*check\(" + NAME, hpp)
    rs = read("rust", "molar_hip", "src", "lib.rs")
    assert re.search(r"pub fn set_shells\(&mut self, n_shells_patch: usize, n_shells_smoothing: usize\)", rs)
    assert "fns.membrane_plan_set_shells)(self.plan, n_shells_patch, n_shells_smoothing)" in rs
    from molar_amd import api
    assert callable(getattr(api.MembranePlan, "set_shells", None))


def test_shell_options_keep_the_chained_path():
    from molar_amd import membrane as mb
    m = mb.Membrane.__new__(mb.Membrane)
    for opts in (dict(n_shells_patch=3), dict(n_shells_smoothing=2), dict(n_shells_patch=4, n_shells_smoothing=3)):
        m.opt = mb.MembraneOptions(**opts)
        assert m.fusable(), opts
        m.opt = mb.MembraneOptions(fused=False, **opts)
        assert not m.fusable(), opts
