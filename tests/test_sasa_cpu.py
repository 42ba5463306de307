"""Surface area without a GPU: the point table of molar_hip_sasa_points against the definition's formula, the numpy
restatement (tests/sasa_ref.py) on one sphere and against the analytic two-sphere cap, and the ABI of the five entries."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sasa_ref as sr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("molar_hip_sasa_points", "molar_hip_sasa_points_f64", "molar_hip_sasa", "molar_hip_sasa_f64", "molar_hip_sasa_frames")


@pytest.fixture(scope="module")
def api():
    from molar_amd import build
    build.build_library()
    import molar_amd.api as a
    return a


@pytest.mark.parametrize("npoints", [1, 2, 64, 96, 960, 4096])
def test_point_table_is_the_formula(api, npoints):
    want = sr.table_formula(npoints)
    t64 = api.sasa_points(npoints, np.float64)
    t32 = api.sasa_points(npoints, np.float32)
    assert t64.shape == t32.shape == (npoints, 3) and t64.dtype == np.float64 and t32.dtype == np.float32
    # the host's sin / cos may differ from numpy's in the last bit (each is good to an ulp of its result; z, r and phi are
    # plain IEEE operations and agree exactly): 4 ulp of every component
    assert np.all(np.abs(t64 - want) <= 4 * np.spacing(np.abs(want)))
    assert np.array_equal(t32, t64.astype(np.float32))              # the f32 table is the f64 one, rounded
    assert np.all(np.abs(np.linalg.norm(t64, axis=1) - 1.0) <= 4 * np.spacing(1.0))
    assert np.all(np.abs(np.linalg.norm(t32.astype(np.float64), axis=1) - 1.0) <= 2 * np.spacing(np.float32(1.0)))


@pytest.mark.parametrize("npoints", [0, 4097])
def test_point_table_rejects_bad_counts(api, npoints):
    for real in (np.float32, np.float64):
        with pytest.raises(api.MolarHipError) as e:
            api.sasa_points(npoints, real)
        assert e.value.code == 50 and "npoints" in str(e.value)


@pytest.mark.parametrize("real", [np.float32, np.float64])
def test_one_sphere_is_fully_exposed(api, real):
    for npoints in (1, 96, 960):
        ex, areas, total = sr.sasa_ref(np.array([[0.3, -1.0, 2.0]]), [0.17], 0.14, sr.points(npoints, real), real)
        assert ex.tolist() == [npoints]
        R = float(real(0.17) + real(0.14))
        assert abs(float(areas[0]) - 4 * np.pi * R * R) <= 4 * np.pi * R * R * 4 * float(np.finfo(real).eps)
        assert total == float(areas[0])


@pytest.mark.parametrize("Ra,Rb", [(0.31, 0.31), (0.26, 0.34), (0.34, 0.25)])
def test_two_spheres_against_the_analytic_cap(api, Ra, Rb):
    npoints = 960
    table = sr.points(npoints, np.float32)
    axis = np.array([0.3, 0.5, np.sqrt(0.66)])                      # unit length
    worst = 0.0
    for d in np.linspace(0.05, 0.7, 40):
        xyz = np.stack([np.zeros(3), d * axis])
        ex, _, _ = sr.sasa_ref(xyz, [Ra, Rb], 0.0, table, np.float32)
        dev = abs(float(ex[0]) - npoints * sr.cap_fraction(d, Ra, Rb))
        worst = max(worst, dev)
        assert dev <= 5.0, (d, Ra, Rb, int(ex[0]), npoints * sr.cap_fraction(d, Ra, Rb))
    print(f"two spheres R = ({Ra}, {Rb}): worst deviation from the analytic cap {worst:.2f} points of {npoints}")


def test_non_finite_atoms_take_no_part(api):
    table = sr.points(96, np.float32)
    xyz = np.array([[0, 0, 0], [0.2, 0, 0], [np.nan, 0, 0], [0.1, 0.1, 0], [0.1, 0, 0.1]], np.float32)
    vdw = np.array([0.15, 0.15, 0.15, np.nan, -0.14], np.float32)
    ex, areas, _ = sr.sasa_ref(xyz, vdw, 0.14, table)
    ex2, areas2, _ = sr.sasa_ref(xyz[:2], vdw[:2], 0.14, table)
    assert np.array_equal(ex[:2], ex2) and np.array_equal(areas[:2], areas2)
    assert ex[2:].tolist() == [0, 0, 0] and areas[2:].tolist() == [0, 0, 0]


def test_abi_of_the_five_entries(api):
    from molar_amd import _lib
    lib = _lib.load()
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "molar_hip.h")).read())
    ffi = open(os.path.join(ROOT, "rust", "molar_hip", "src", "ffi.rs")).read()
    for name in NAMES:
        assert f"int {name}(" in header, name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert f'b"{name}\\0"' in ffi, name
    assert len(_lib.SYMBOLS["molar_hip_sasa"][1]) == len(_lib.SYMBOLS["molar_hip_sasa_f64"][1]) == 11
    assert len(_lib.SYMBOLS["molar_hip_sasa_frames"][1]) == 12
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_ffi as gen
    assert open(gen.OUT).read() == gen.render(gen.c_functions(open(gen.HEADER).read())), "run python tools/gen_rust_ffi.py"
    hpp = open(os.path.join(ROOT, "include", "molar_hip.hpp")).read()
    assert "struct Sasa" in hpp and "molar_hip_sasa(" in hpp


def test_selection_without_radii_fails_like_the_vdw_search(api):
    top = api.Topology(np.ones(4, np.float32))
    sel = api.Sel(top, api.State(np.zeros((4, 3), np.float32)))
    with pytest.raises(TypeError):
        sel.sasa()
