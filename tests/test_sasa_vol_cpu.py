"""Per-atom volumes without a GPU: the ABI of the three molar_hip_sasa_vol entries and their mirrors, the numpy
restatement of the definition (tests/sasa_vol_ref.py) in double on a lone sphere, against the analytic two-sphere split at
the radical plane and against a Monte-Carlo union volume, and the argument checks that need no device."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sasa_ref as sr  # noqa: E402
import sasa_vol_ref as vr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("molar_hip_sasa_vol", "molar_hip_sasa_vol_f64", "molar_hip_sasa_vol_frames")


@pytest.fixture(scope="module")
def api():
    from molar_amd import build
    build.build_library()
    import molar_amd.api as a
    return a


def test_abi_of_the_three_entries(api):
    from molar_amd import _lib
    lib = _lib.load()
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "molar_hip.h")).read())
    ffi = open(os.path.join(ROOT, "rust", "molar_hip", "src", "ffi.rs")).read()
    for name in NAMES:
        assert f"int {name}(" in header, name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert f'b"{name}\\0"' in ffi, name
    # the arguments of the area calls plus volumes and total_volume
    for vol, area in (("molar_hip_sasa_vol", "molar_hip_sasa"), ("molar_hip_sasa_vol_f64", "molar_hip_sasa_f64"),
                      ("molar_hip_sasa_vol_frames", "molar_hip_sasa_frames")):
        assert _lib.SYMBOLS[vol][1][:-2] == _lib.SYMBOLS[area][1] and len(_lib.SYMBOLS[vol][1]) == len(_lib.SYMBOLS[area][1]) + 2
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_ffi as gen
    assert open(gen.OUT).read() == gen.render(gen.c_functions(open(gen.HEADER).read())), "run python tools/gen_rust_ffi.py"
    hpp = open(os.path.join(ROOT, "include", "molar_hip.hpp")).read()
    assert "Sasa sasa_vol(" in hpp and "molar_hip_sasa_vol(" in hpp and "total_volume" in hpp and "volumes" in hpp
    rs = open(os.path.join(ROOT, "rust", "molar_hip", "src", "lib.rs")).read()
    assert "pub fn sasa_vol(" in rs and "fns.sasa_vol)(" in rs
    # the definition is in the header
    for phrase in ("power cell", "t = c / a", "hi_k = max(hi_k, lo_k)", "each keep their full ball"):
        assert phrase in header, phrase


def test_python_mirrors(api):
    for owner, name in ((api.Engine, "sasa_vol"), (api.Engine, "sasa_vol_frames"), (api.MeasureF64, "sasa_vol"), (api.Sel, "sasa_vol")):
        assert callable(getattr(owner, name))
    plain = api.Sasa(np.zeros(1, np.float32), 0.0)
    assert plain.volumes is None and plain.total_volume is None and plain.exposed is None


@pytest.mark.parametrize("npoints", [1, 96, 960])
def test_lone_sphere_is_its_ball(npoints):
    v, total = vr.sasa_vol_ref(np.array([[0.3, -1.0, 2.0]]), [0.17], 0.14, sr.table_formula(npoints), np.float64)
    R = 0.17 + 0.14
    want = 4.0 * np.pi * R ** 3 / 3.0
    assert abs(v[0] - want) <= 1e-14 * want and total == float(v[0])


# Two overlapping balls against the analytic split at their radical plane, centres along (0.3, 0.5, sqrt 0.66).  Each bound is
# twice the relative deviation measured for the restatement alone (in double, table_formula), which is what the table holds.
TWO_ANALYTIC = {
    # name: (Ra, Rb, d, {npoints: (measured deviation of a, of b)})
    "overlap": (0.3, 0.2, 0.35, {960: (1.29e-5, 2.63e-5), 3840: (1.13e-5, 1.40e-6)}),
    # the small ball's centre lies beyond the radical plane: its rays start at lo_k > 0
    "swallowed centre": (0.4, 0.15, 0.3, {960: (6.25e-7, 9.65e-4), 3840: (1.22e-6, 1.60e-4)}),
}


@pytest.mark.parametrize("name", list(TWO_ANALYTIC))
@pytest.mark.parametrize("npoints", [960, 3840])
def test_two_spheres_against_the_radical_plane_split(name, npoints):
    Ra, Rb, d, per_points = TWO_ANALYTIC[name]
    bound = [2.0 * m for m in per_points[npoints]]
    axis = np.array([0.3, 0.5, np.sqrt(0.66)])
    v, total = vr.sasa_vol_ref(np.stack([np.zeros(3), d * axis]), [Ra, Rb], 0.0, sr.table_formula(npoints), np.float64)
    want = vr.two_sphere_split(d, Ra, Rb)
    dev = [abs(float(v[k]) / want[k] - 1.0) for k in (0, 1)]
    print(f"{name} at {npoints} points: relative deviation {dev[0]:.3e} / {dev[1]:.3e} of {want[0]:.6f} / {want[1]:.6f} nm^3")
    assert dev[0] <= bound[0] and dev[1] <= bound[1]
    if name == "swallowed centre":
        assert (d * d + Rb * Rb - Ra * Ra) / (2 * d) < 0 < want[1]


def test_blob_adds_up_to_the_union_of_the_balls():
    """300 atoms at 100 atoms / nm^3, probe 0.14 nm: the volumes add up to the union's volume, here against a seeded
    Monte-Carlo estimate from 1e6 samples within three of its standard errors.  At 960 points the table's own bias (the
    sum is 5.8205 nm^3 at 96 points, 5.8236 at 960, 5.8242 at 3840) is far below the estimate's standard error, so the
    bound judges the definition and not the point count.  Measured: 5.8236 against 5.8337 +- 0.0041 (2.4 standard errors;
    8e6 samples of another seed give 5.8237 +- 0.0015)."""
    rng = np.random.default_rng(31)
    n = 300
    xyz = rng.uniform(0, (n / 100.0) ** (1.0 / 3.0), (n, 3))
    vdw = np.array([0.12, 0.152, 0.155, 0.17, 0.18])[rng.integers(0, 5, n)]
    v, total = vr.sasa_vol_ref(xyz, vdw, 0.14, sr.table_formula(960), np.float64)
    mc, se = vr.union_volume_mc(xyz, vdw + 0.14, 1_000_000, 32)
    print(f"sum of the volumes {total:.4f} nm^3, Monte Carlo {mc:.4f} +- {se:.4f}; {int((v == 0).sum())} atoms with volume 0")
    assert abs(total - mc) <= 3.0 * se
    assert np.all(v >= 0) and np.any(v == 0)                            # hidden power cells
    R = vdw + 0.14
    assert np.all(v <= (4.0 * np.pi / 3.0) * R ** 3 * (1 + 1e-12))


def test_f32_restatement_stays_near_the_f64_one():
    """c = ((dd + R_i^2) - R_j^2) / 2 cancels, so float and double differ by far more than an ulp: up to about 2e-5 relative
    per atom on this blob.  That is why the f32 kernel is compared with the f32 restatement."""
    rng = np.random.default_rng(31)
    n = 300
    xyz = rng.uniform(0, (n / 100.0) ** (1.0 / 3.0), (n, 3)).astype(np.float32)
    vdw = np.array([0.12, 0.152, 0.155, 0.17, 0.18], np.float32)[rng.integers(0, 5, n)]
    t64 = sr.table_formula(96)
    v32, _ = vr.sasa_vol_ref(xyz, vdw, np.float32(0.14), t64.astype(np.float32), np.float32)
    v64, _ = vr.sasa_vol_ref(xyz.astype(np.float64), (vdw + np.float32(0.14)).astype(np.float64), 0.0, t64, np.float64)
    keep = v64 > 1e-4
    rel = np.abs(v32[keep].astype(np.float64) / v64[keep] - 1.0)
    print(f"f32 against f64 restatement: worst {rel.max():.2e}, median {np.median(rel):.2e}")
    assert rel.max() < 1e-3


def test_atoms_that_take_no_part_have_no_volume_and_cut_nobody():
    table = sr.table_formula(96)
    xyz = np.array([[0, 0, 0], [0.2, 0, 0], [np.nan, 0, 0], [0.1, 0.1, 0], [0.1, 0, 0.1]], np.float32)
    vdw = np.array([0.15, 0.15, 0.15, np.nan, -0.14], np.float32)
    v, _ = vr.sasa_vol_ref(xyz, vdw, 0.14, table)
    v2, _ = vr.sasa_vol_ref(xyz[:2], vdw[:2], 0.14, table)
    assert np.array_equal(v[:2], v2) and v[2:].tolist() == [0, 0, 0]


def test_coincident_equal_atoms_each_keep_their_ball():
    v, _ = vr.sasa_vol_ref(np.zeros((2, 3)), [0.25, 0.25], 0.0, sr.table_formula(96), np.float64)
    want = 4.0 * np.pi * 0.25 ** 3 / 3.0
    assert np.all(np.abs(v - want) <= 1e-14 * want)


# ---- argument checks that are made before anything touches a device
def test_selection_without_radii_fails_like_the_area_call(api):
    top = api.Topology(np.ones(4, np.float32))
    sel = api.Sel(top, api.State(np.zeros((4, 3), np.float32)))
    with pytest.raises(TypeError):
        sel.sasa_vol()


def test_null_context_is_refused(api):
    from molar_amd import _lib
    lib = _lib.load()
    x = np.zeros((3, 3), np.float32)
    v = np.full(3, 0.1, np.float32)
    rc = lib.molar_hip_sasa_vol(None, x.ctypes.data, 3, None, 3, v.ctypes.data, 0.14, 96, None, None, None, None, None)
    assert rc != 0
