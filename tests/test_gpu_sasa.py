"""The fused surface-area kernel (sasa.hip) against the numpy restatement of its definition (tests/sasa_ref.py): the
exposed-point counts must be EQUAL, the areas agree to 1e-6 (f32) / 1e-14 (f64) relative, the total with the double sum of
the returned areas to 1e-12.  The cases reach the lane / point mapping and its tail, the strict compares at the bit level,
several cells, selections, the refill of the LDS chunk, mixed radii, the cell-count cap, coordinates far from the origin,
non-finite input, the frames form, buffer reuse, device tensors and the argument checks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sasa_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

PROBE = 0.14
VDW_SET = np.array([0.12, 0.152, 0.155, 0.17, 0.18], np.float32)


@pytest.fixture(scope="module")
def api():
    from molar_amd import build
    build.build_library()
    import molar_amd.api as a
    return a


@pytest.fixture(scope="module")
def eng(api):
    return api.Engine(0)


@pytest.fixture(scope="module")
def m64(api, eng):
    return api.MeasureF64(eng)


_tables = {}


def table(npoints, real=np.float32):
    key = (npoints, np.dtype(real).name)
    if key not in _tables:
        _tables[key] = sr.points(npoints, real)
    return _tables[key]


def verify(res, xyz_sel, vdw, probe, npoints, real=np.float32, ref=None):
    """`res` (a Sasa with exposed) against the restatement over the selected atoms; returns the reference."""
    ex, ar, _ = ref if ref is not None else sr.sasa_ref(xyz_sel, vdw, probe, table(npoints, real), real)
    got_ex, got_ar = np.asarray(res.exposed), np.asarray(res.areas)
    assert got_ar.dtype == np.dtype(real) and got_ex.dtype == np.uint32
    bad = np.nonzero(got_ex != ex)[0]
    assert len(bad) == 0, (len(bad), bad[:5], got_ex[bad[:5]], ex[bad[:5]])
    rtol = 1e-6 if np.dtype(real) == np.float32 else 1e-14
    assert np.all(np.abs(got_ar.astype(np.float64) - ar.astype(np.float64)) <= rtol * np.abs(ar.astype(np.float64)))
    s = float(np.sum(got_ar.astype(np.float64)))
    assert abs(res.total_area - s) <= 1e-12 * abs(s)
    return ex, ar, _


def blob(n, density, seed):
    rng = np.random.default_rng(seed)
    edge = (n / density) ** (1.0 / 3.0)
    xyz = rng.uniform(0, edge, (n, 3)).astype(np.float32)
    vdw = VDW_SET[rng.integers(0, len(VDW_SET), n)]
    return xyz, vdw


@pytest.fixture(scope="module")
def case_c():
    """2000 atoms at 100 atoms / nm^3 (edge 2.7 nm) and the restatement's results at 96 and 192 points"""
    xyz, vdw = blob(2000, 100.0, 11)
    refs = {p: sr.sasa_ref(xyz, vdw, PROBE, table(p)) for p in (96, 192)}
    return xyz, vdw, refs


# ---- a: one atom, the lane / point mapping and its tail
@pytest.mark.parametrize("npoints", [1, 63, 64, 65, 96, 960, 4096])
def test_one_atom(eng, npoints):
    xyz = np.array([[0.3, -1.0, 2.0]], np.float32)
    res = eng.sasa(xyz, [0.17], probe=PROBE, npoints=npoints, want_exposed=True)
    assert res.exposed.tolist() == [npoints]
    verify(res, xyz, [0.17], PROBE, npoints)


# ---- b: two atoms at the boundaries of both compares
TWO = {
    "coincident": ([[0, 0, 0], [0, 0, 0]], [0.25, 0.25]),
    "tangent": ([[0, 0, 0], [0.5, 0, 0]], [0.25, 0.25]),         # representable: d2 == lim^2, the compare is strict
    "inside": ([[0, 0, 0], [0.05, 0.02, 0]], [0.4, 0.1]),
    "half": ([[0, 0, 0], [0.25, 0, 0]], [0.25, 0.25]),
}


@pytest.mark.parametrize("name", list(TWO))
@pytest.mark.parametrize("real", [np.float32, np.float64])
def test_two_atoms(eng, m64, name, real):
    xyz, R = TWO[name]
    xyz, R = np.array(xyz, real), np.array(R, real)
    call = eng.sasa if real == np.float32 else m64.sasa
    for npoints in (96, 960):
        res = call(xyz, R, probe=0.0, npoints=npoints, want_exposed=True)
        ex, _, _ = verify(res, xyz, R, 0.0, npoints, real)
        if name == "tangent":
            assert ex.tolist() == [npoints, npoints]
        if name == "inside":
            assert ex[0] == npoints and ex[1] == 0


# ---- c: several cells, most atoms buried
@pytest.mark.parametrize("npoints", [96, 192])
def test_blob(eng, case_c, npoints):
    xyz, vdw, refs = case_c
    res = eng.sasa(xyz, vdw, probe=PROBE, npoints=npoints, want_exposed=True)
    ex, _, _ = verify(res, xyz, vdw, PROBE, npoints, ref=refs[npoints])
    assert 0.5 < np.mean(ex == 0) < 0.95 and np.any((ex > 0) & (ex < npoints))


def test_blob_960_points(eng, case_c):
    xyz, vdw, _ = case_c
    res = eng.sasa(xyz[:600], vdw[:600], probe=PROBE, npoints=960, want_exposed=True)
    verify(res, xyz[:600], vdw[:600], PROBE, 960)


# ---- d: a selection of a larger frame
def test_selection(eng):
    xyz, vdw_all = blob(5000, 100.0, 12)
    rng = np.random.default_rng(13)
    idx = np.sort(rng.choice(5000, 2000, replace=False)).astype(np.uint64)
    vdw = vdw_all[idx.astype(np.int64)]
    res = eng.sasa(xyz, vdw, idx=idx, probe=PROBE, npoints=96, want_exposed=True)
    assert res.areas.shape == (2000,)
    verify(res, xyz[idx.astype(np.int64)], vdw, PROBE, 96)
    # selection order is the order of idx, sorted or not
    perm = rng.permutation(2000)
    res2 = eng.sasa(xyz, vdw[perm], idx=idx[perm], probe=PROBE, npoints=96, want_exposed=True)
    assert np.array_equal(res2.exposed, res.exposed[perm]) and np.array_equal(res2.areas, res.areas[perm])


# ---- e: one crowded cell, the LDS chunk refills with the masks carried over
@pytest.fixture(scope="module")
def case_e():
    rng = np.random.default_rng(14)
    xyz = rng.uniform(0, 0.8, (700, 3)).astype(np.float32)
    R = rng.uniform(0.45, 0.55, 700).astype(np.float32)
    return xyz, R


def test_crowded(eng, case_e):
    xyz, R = case_e
    res = eng.sasa(xyz, R, probe=0.0, npoints=192, want_exposed=True)
    verify(res, xyz, R, 0.0, 192)


# ---- f: mixed radii
def test_mixed_radii(eng):
    rng = np.random.default_rng(15)
    xyz = rng.uniform(0, 5.0, (1500, 3)).astype(np.float32)
    R = np.array([0.05, 0.3, 1.0], np.float32)[rng.integers(0, 3, 1500)]
    res = eng.sasa(xyz, R, probe=0.0, npoints=96, want_exposed=True)
    ex, _, _ = verify(res, xyz, R, 0.0, 96)
    assert np.any(ex[R == np.float32(0.05)] == 0) and np.any(ex > 0)


# ---- g: sparse sets and the cap on the number of cells
def test_sparse(eng):
    rng = np.random.default_rng(16)
    xyz = rng.uniform(0, 50.0, (300, 3)).astype(np.float32)
    vdw = VDW_SET[rng.integers(0, 5, 300)]
    res = eng.sasa(xyz, vdw, probe=PROBE, npoints=96, want_exposed=True)
    ex, _, _ = verify(res, xyz, vdw, PROBE, 96)
    assert np.mean(ex == 96) > 0.9


def test_two_atoms_far_apart(eng):
    xyz = np.array([[0, 0, 0], [1.0e4, 0, 0]], np.float32)
    res = eng.sasa(xyz, [0.17, 0.17], probe=PROBE, npoints=96, want_exposed=True)
    assert res.exposed.tolist() == [96, 96]
    verify(res, xyz, [0.17, 0.17], PROBE, 96)


# ---- h: the strict < at the bit level
def lattice(spacing, real):
    g = np.arange(6, dtype=real) * real(spacing)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(real)


@pytest.mark.parametrize("real", [np.float32, np.float64])
@pytest.mark.parametrize("shrink", [False, True])
def test_lattice(eng, m64, real, shrink):
    R = 0.25                                                          # vdw 0.125 + probe 0.125, exact in both precisions
    spacing = 2 * R * (1 - 2.0 ** -20) if shrink else 2 * R
    xyz = lattice(spacing, real)
    vdw = np.full(216, 0.125, real)
    call = eng.sasa if real == np.float32 else m64.sasa
    res = call(xyz, vdw, probe=0.125, npoints=192, want_exposed=True)
    ex, _, _ = verify(res, xyz, vdw, 0.125, 192, real)
    if not shrink:
        assert np.all(ex == 192)                                     # d2 == (2R)^2: nobody is anybody's neighbour


# ---- i: far from the origin, d is taken from the stored coordinates
def test_far_origin(eng, case_c):
    xyz, vdw, _ = case_c
    far = (xyz + np.array([1000.0, -2000.0, 3000.0], np.float32)).astype(np.float32)
    res = eng.sasa(far, vdw, probe=PROBE, npoints=96, want_exposed=True)
    verify(res, far, vdw, PROBE, 96)


# ---- j: atoms that take no part
def test_non_finite(eng):
    xyz, vdw = blob(200, 100.0, 17)
    xyz, vdw = xyz.copy(), vdw.copy()
    xyz[17, 1] = np.nan
    vdw[60] = np.nan
    vdw[133] = np.float32(-PROBE)
    res = eng.sasa(xyz, vdw, probe=PROBE, npoints=96, want_exposed=True)
    verify(res, xyz, vdw, PROBE, 96)
    keep = np.setdiff1d(np.arange(200), [17, 60, 133])
    ex, ar, _ = sr.sasa_ref(xyz[keep], vdw[keep], PROBE, table(96))
    assert np.array_equal(res.exposed[keep], ex) and res.exposed[[17, 60, 133]].tolist() == [0, 0, 0]
    assert res.areas[[17, 60, 133]].tolist() == [0, 0, 0]


# ---- k: double precision (two atoms and the lattice: above)
def test_blob_f64(m64, case_c):
    xyz, vdw, _ = case_c
    x64, v64 = xyz.astype(np.float64) + 1e-9, vdw.astype(np.float64)
    res = m64.sasa(x64, v64, probe=PROBE, npoints=192, want_exposed=True)
    verify(res, x64, v64, PROBE, 192, np.float64)


def test_crowded_f64(m64, case_e):
    xyz, R = case_e
    x64, r64 = xyz.astype(np.float64) * (1 + 1e-12), R.astype(np.float64)
    res = m64.sasa(x64, r64, probe=0.0, npoints=192, want_exposed=True)
    verify(res, x64, r64, 0.0, 192, np.float64)


# ---- l: frames
def test_frames_equal_single_calls(eng, case_c):
    xyz, vdw, _ = case_c
    rng = np.random.default_rng(18)
    natoms, F, stride = 2000, 5, 3 * 2000 + 7
    buf = np.full(F * stride, np.nan, np.float32)                    # the padding is never read
    frames = []
    for f in range(F):
        fr = (xyz + rng.normal(0, 0.02, xyz.shape).astype(np.float32)).astype(np.float32)
        frames.append(fr)
        buf[f * stride:f * stride + 3 * natoms] = fr.reshape(-1)
    areas = np.zeros((F, natoms), np.float32)
    totals = np.zeros(F, np.float64)
    from molar_amd._lib import check
    check(eng.lib.molar_hip_sasa_frames(eng.ctx, buf.ctypes.data, F, stride, natoms, None, natoms, vdw.ctypes.data,
                                        C.c_float(PROBE), 96, areas.ctypes.data, totals.ctypes.data))
    singles = [eng.sasa(fr, vdw, probe=PROBE, npoints=96) for fr in frames]
    for f in range(F):
        assert np.array_equal(areas[f], singles[f].areas) and totals[f] == singles[f].total_area
    assert len(set(totals.tolist())) == F
    a2, t2 = eng.sasa_frames(np.stack(frames), vdw, probe=PROBE, npoints=96)
    assert np.array_equal(a2, areas) and np.array_equal(t2, totals)
    # totals alone
    t3 = np.zeros(F, np.float64)
    check(eng.lib.molar_hip_sasa_frames(eng.ctx, buf.ctypes.data, F, stride, natoms, None, natoms, vdw.ctypes.data,
                                        C.c_float(PROBE), 96, None, t3.ctypes.data))
    assert np.array_equal(t3, totals)


# ---- m: reuse of the state
def test_reuse_across_shapes_and_precisions(api, case_c):
    xyz, vdw, refs = case_c
    eng = api.Engine(0)
    m64 = api.MeasureF64(eng)
    small, vs = xyz[:37], vdw[:37]
    ref_small = {(p, r): sr.sasa_ref(small, vs, PROBE, table(p, r), r) for p in (64, 96) for r in (np.float32, np.float64)}
    for _ in range(2):
        verify(eng.sasa(xyz, vdw, probe=PROBE, npoints=96, want_exposed=True), xyz, vdw, PROBE, 96, ref=refs[96])
        verify(eng.sasa(small, vs, probe=PROBE, npoints=64, want_exposed=True), small, vs, PROBE, 64, ref=ref_small[(64, np.float32)])
        verify(m64.sasa(small, vs, probe=PROBE, npoints=96, want_exposed=True), small, vs, PROBE, 96, np.float64,
               ref=ref_small[(96, np.float64)])
        verify(eng.sasa(xyz, vdw, probe=PROBE, npoints=192, want_exposed=True), xyz, vdw, PROBE, 192, ref=refs[192])
        verify(m64.sasa(small, vs, probe=PROBE, npoints=64, want_exposed=True), small, vs, PROBE, 64, np.float64,
               ref=ref_small[(64, np.float64)])
        verify(eng.sasa(small, vs, probe=PROBE, npoints=96, want_exposed=True), small, vs, PROBE, 96, ref=ref_small[(96, np.float32)])
    eng.close()


def test_cached_search_survives_a_sasa_call(api, eng, case_c):
    xyz, vdw, _ = case_c
    rng = np.random.default_rng(19)
    other = rng.uniform(0, 3.0, (3000, 3)).astype(np.float32)
    n = eng.search_count(api.SEARCH_SINGLE, 0.4, other)
    want = eng.search_fill(n)
    n2 = eng.search_count(api.SEARCH_SINGLE, 0.4, other)
    eng.sasa(xyz, vdw, probe=PROBE, npoints=96)
    got = eng.search_fill(n2)
    assert n2 == n and n > 0
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- n: device tensors in and out
def test_device_tensors(eng, case_c):
    import torch
    xyz, vdw_all, _ = case_c
    idx = np.arange(0, 2000, 3, dtype=np.uint64)
    vdw = vdw_all[idx.astype(np.int64)]
    host = eng.sasa(xyz, vdw, idx=idx, probe=PROBE, npoints=96, want_exposed=True)
    dev = eng.sasa(torch.from_numpy(xyz).cuda(), torch.from_numpy(vdw).cuda(), idx=torch.from_numpy(idx.astype(np.int64)).cuda(),
                   probe=PROBE, npoints=96, want_exposed=True)
    assert dev.areas.is_cuda and dev.exposed.is_cuda
    assert np.array_equal(dev.areas.cpu().numpy(), host.areas)
    assert np.array_equal(dev.exposed.cpu().numpy().astype(np.uint32), host.exposed)
    assert dev.total_area == host.total_area
    fr = torch.from_numpy(np.stack([xyz, xyz[::-1].copy()])).cuda()
    a, t = eng.sasa_frames(fr, vdw_all, probe=PROBE, npoints=96)
    assert a.is_cuda and np.array_equal(a[0].cpu().numpy(), eng.sasa(xyz, vdw_all, probe=PROBE, npoints=96).areas)


# ---- o: argument checks
@pytest.mark.parametrize("kw", [dict(npoints=0), dict(npoints=4097), dict(probe=-0.1), dict(probe=float("nan"))])
def test_errors(api, eng, m64, kw):
    xyz = np.zeros((3, 3), np.float32)
    for call, x in ((eng.sasa, xyz), (m64.sasa, xyz.astype(np.float64))):
        with pytest.raises(api.MolarHipError) as e:
            call(x, [0.1, 0.1, 0.1], **kw)
        assert e.value.code == 50 and ("npoints" in str(e.value) or "probe" in str(e.value))
    with pytest.raises(api.MolarHipError) as e:
        eng.sasa_frames(xyz[None], [0.1, 0.1, 0.1], **kw)
    assert e.value.code == 50


def test_n_beyond_natoms_without_an_index(api, eng):
    xyz = np.zeros((3, 3), np.float32)
    vdw = np.full(4, 0.1, np.float32)
    total = C.c_double(-1.0)
    rc = eng.lib.molar_hip_sasa(eng.ctx, xyz.ctypes.data, 3, None, 4, vdw.ctypes.data, C.c_float(0.14), 96, None, None, C.byref(total))
    assert rc == 50 and b"natoms" in eng.lib.molar_hip_last_error()


def test_empty_selection(eng):
    xyz = np.zeros((3, 3), np.float32)
    res = eng.sasa(xyz, np.zeros(0, np.float32), idx=np.zeros(0, np.uint64), probe=PROBE, npoints=96, want_exposed=True)
    assert res.total_area == 0.0 and res.areas.shape == (0,) and res.exposed.shape == (0,)


# ---- the selection's method, end to end
def test_sel_sasa(api, eng, case_c):
    xyz, vdw, refs = case_c
    top = api.Topology(np.ones(2000, np.float32), vdw)
    sel = api.Sel(top, api.State(xyz), np.arange(100, 1900), engine=eng)
    res = sel.sasa(probe=PROBE, npoints=96)
    ex, ar, tot = sr.sasa_ref(xyz[100:1900], vdw[100:1900], PROBE, table(96))
    assert np.all(np.abs(res.areas.astype(np.float64) - ar.astype(np.float64)) <= 1e-6 * np.abs(ar.astype(np.float64)))
    s = float(np.sum(res.areas.astype(np.float64)))
    assert abs(res.total_area - s) <= 1e-12 * s and abs(res.total_area - tot) <= 1e-6 * tot
    assert res.areas.shape == (1800,)
