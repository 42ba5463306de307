"""The RMSD matrix without a GPU: the ABI of its three entries, the plan entry (a pure host function), the numpy reference
(tests/rmsd_matrix_ref.py) against answers known in closed form, and the acceptance bound of the GPU tests against the same
Gram route in numpy - so the reference and the route's own f64 rounding do not use the bound up."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rmsd_matrix_ref as rr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("molar_hip_rmsd_matrix_plan", "molar_hip_rmsd_matrix", "molar_hip_rmsd_matrix_f64")


def test_abi_of_the_three_entries():
    from molar_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "molar_hip.h")).read())
    ffi = open(os.path.join(ROOT, "rust", "molar_hip", "src", "ffi.rs")).read()
    for name in NAMES:
        assert f"int {name}(" in header, name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert f'b"{name}\\0"' in ffi, name
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_ffi as gen
    funcs = {name: params for name, _, params in gen.c_functions(open(gen.HEADER).read())}
    assert len(funcs["molar_hip_rmsd_matrix_plan"]) == len(_lib.SYMBOLS["molar_hip_rmsd_matrix_plan"][1]) == 5
    assert len(funcs["molar_hip_rmsd_matrix"]) == len(_lib.SYMBOLS["molar_hip_rmsd_matrix"][1]) == 14
    assert len(funcs["molar_hip_rmsd_matrix_f64"]) == len(_lib.SYMBOLS["molar_hip_rmsd_matrix_f64"][1]) == 14
    assert open(gen.OUT).read() == gen.render(gen.c_functions(open(gen.HEADER).read())), "run python tools/gen_rust_ffi.py"
    hpp = open(os.path.join(ROOT, "include", "molar_hip.hpp")).read()
    assert "rmsd_matrix(" in hpp and "molar_hip_rmsd_matrix(" in hpp and "molar_hip_rmsd_matrix_f64(" in hpp
    lib_rs = open(os.path.join(ROOT, "rust", "molar_hip", "src", "lib.rs")).read()
    assert "pub fn rmsd_matrix(" in lib_rs and "pub fn rmsd_matrix_plan(" in lib_rs
    assert "rmsd_matrix.hip" in build.SOURCES


def test_plan_needs_no_gpu_and_is_monotone():
    from molar_amd import api, build
    build.build_library()
    assert api.rmsd_matrix_plan(0, 0, 100) == (0, 1)
    sizes_f = [1, 2, 15, 16, 17, 33, 48, 200, 640, 700, 720, 736, 1024, 1500, 4096]
    sizes_n = [1, 3, 4, 5, 255, 256, 511, 512, 513, 1000, 3000, 20000, 100000]
    for n in sizes_n:
        last = 0
        for F in sizes_f:
            ws, ks = api.rmsd_matrix_plan(F, 0, n)
            assert ws >= last and ks >= 1, (F, n, ws, last)
            assert ws >= 3 * 8 * F * n                      # the packed operand alone
            last = ws
    for F in sizes_f:
        last = 0
        for n in sizes_n:
            ws, _ = api.rmsd_matrix_plan(F, 0, n)
            assert ws >= last, (F, n)
            last = ws
    # rectangular: monotone in each block, and never below the two operands
    for n in (5, 3000):
        for F1 in (1, 7, 256):
            last = 0
            for F2 in sizes_f:
                ws, _ = api.rmsd_matrix_plan(F1, F2, n)
                assert ws >= last and ws >= 3 * 8 * (F1 + F2) * n
                last = ws
        for F2 in (1, 19, 1024):
            last = 0
            for F1 in sizes_f:
                ws, _ = api.rmsd_matrix_plan(F1, F2, n)
                assert ws >= last
                last = ws
    # the two paths of the GPU tests: few tiles and many atoms split K, few atoms do not
    assert api.rmsd_matrix_plan(3, 0, 3000)[1] > 1
    assert api.rmsd_matrix_plan(40, 0, 100)[1] == 1
    assert api.rmsd_matrix_plan(4096, 0, 1000)[1] == 1


def test_reference_pure_translation_without_fit():
    fr = rr.random_frames(1, 37, 1)
    t = np.array([0.3, -1.2, 2.0])
    frames = np.concatenate([fr, (fr.astype(np.float64) + t).astype(np.float32)])
    mass = np.random.default_rng(2).uniform(1, 16, 37)
    ref, _, _ = rr.matrix(frames, mass=mass, fit=False)
    assert ref[0, 0] == 0 and ref[1, 1] == 0
    assert abs(ref[0, 1] - np.linalg.norm(t)) < 1e-6 and ref[0, 1] == ref[1, 0]      # f32 rounding of the shifted copy
    fitted, _, _ = rr.matrix(frames, mass=mass, fit=True)
    assert fitted[0, 1] < 1e-6


def test_reference_rigid_copies_give_zero():
    frames = rr.rigid_copies(5, 200, 3, offset=0.0, dtype=np.float64)
    ref, rg, _ = rr.matrix(frames)
    assert np.all(ref < 1e-13 * np.sqrt(rg.max()) * 10)
    mass = np.random.default_rng(4).uniform(0, 3, 200)
    refm, _, _ = rr.matrix(frames, mass=mass)
    assert np.all(refm < 1e-13)


def test_reference_two_atom_frames():
    rng = np.random.default_rng(5)
    frames = rng.normal(size=(6, 2, 3)) * 2
    ref, _, _ = rr.matrix(frames)
    d = np.linalg.norm(frames[:, 0] - frames[:, 1], axis=1)
    assert np.allclose(ref, np.abs(d[:, None] - d[None, :]) / 2, atol=1e-13)


def test_reference_mirror_image_is_not_zero():
    frames = rr.random_frames(1, 50, 6).astype(np.float64)
    mirror = frames * np.array([1.0, 1.0, -1.0])
    ref, rg, _ = rr.matrix(np.concatenate([frames, mirror]))
    assert ref[0, 1] > 0.1 * np.sqrt(rg[0])
    # a planar structure IS its own mirror image up to a rotation
    flat = frames.copy()
    flat[..., 2] = 0
    ref, _, _ = rr.matrix(np.concatenate([flat, flat * np.array([1.0, -1.0, 1.0])]))
    assert ref[0, 1] < 1e-13


@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 257, 5000])
def test_gram_route_in_numpy_stays_inside_the_bound(n):
    """The bound is derived, not measured; here the same route in numpy (eigvalsh for the eigenvalue) is held against it."""
    rng = np.random.default_rng(n)
    blocks = {
        "unrelated": rr.random_frames(5, n, 10 + n),
        "rigid at 50 nm": rr.rigid_copies(5, n, 20 + n),
        "perturbed": (rr.rigid_copies(1, n, 30 + n)[0][None] + rng.normal(size=(5, n, 3)) * 1e-3).astype(np.float32),
    }
    base = rr.random_frames(1, n, 40 + n)
    blocks["mirror"] = np.concatenate([base, base * np.array([1, 1, -1], np.float32)])
    for what, frames in blocks.items():
        for mass in (None, rng.uniform(0.5, 30, n)):
            for fit in (True, False):
                ref, rg1, rg2 = rr.matrix(frames, mass=mass, fit=fit)
                got = rr.gram_route(frames, mass=mass, fit=fit)
                assert rr.check(got, ref, rg1, rg2, n, rr.EPS64, f"{what} n={n} fit={fit}") <= 0.5
