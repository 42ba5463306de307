"""The volume variant of the fused surface-area kernel (sasa.hip, molar_hip_sasa_vol) against the numpy restatement of its
definition (tests/sasa_vol_ref.py) in the same precision.  Every case checks three things:
  exposed and areas equal those of the area call on the same input bit for bit;
  |volume_i - ref_i| <= rtol ref_i + 1e-12 (4 pi / 3) R_i^3 with rtol 1e-6 (f32) / 1e-12 (f64): the intervals are bit-defined in
    Real, what is left is the order of a double sum of at most 4096 non-negative cubes and one rounding to Real;
  total_volume against the double sum of the returned volumes to 1e-12.
The cases reach the batch mapping and its tail, both cuts of a ray and the empty interval, several cells, hidden atoms, the
overflow of the LDS chunk (the cells are walked again per batch), mixed radii, selections, non-finite input, coordinates
far from the origin, the strict neighbour compare at the bit level, the frames form, device tensors and state reuse."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sasa_ref as sr  # noqa: E402
import sasa_vol_ref as vr  # noqa: E402
from test_gpu_sasa import TWO, VDW_SET, blob, lattice  # noqa: E402  (the inputs of the area cases)

pytestmark = pytest.mark.gpu

PROBE = 0.14


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


def verify(res, base, xyz_sel, vdw, probe, npoints, real=np.float32, ref=None):
    """`res` (a Sasa of a volume call with exposed) against `base` (the area call on the same input) and the restatement of
    the volumes over the selected atoms; returns the reference volumes."""
    real = np.dtype(real).type
    assert np.array_equal(np.asarray(res.exposed), np.asarray(base.exposed))
    assert np.array_equal(np.asarray(res.areas), np.asarray(base.areas)) and res.total_area == base.total_area
    want = ref if ref is not None else vr.sasa_vol_ref(xyz_sel, vdw, probe, table(npoints, real), real)[0]
    got = np.asarray(res.volumes)
    assert got.dtype == np.dtype(real) and got.shape == want.shape
    with np.errstate(invalid="ignore"):
        R = (np.asarray(vdw, real) + real(probe)).astype(np.float64)
    ball = (4.0 * np.pi / 3.0) * np.where(np.isfinite(R) & (R > 0), R, 0.0) ** 3
    rtol = 1e-6 if real == np.float32 else 1e-12
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    tol = rtol * want.astype(np.float64) + 1e-12 * ball
    bad = np.nonzero(~(err <= tol))[0]
    print(f"volumes: {len(got)} atoms, worst error / tolerance {float(np.max(err / np.maximum(tol, 1e-300))) if len(got) else 0:.3g}, "
          f"{int((want == 0).sum())} with volume 0")
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
    s = float(np.sum(got.astype(np.float64)))
    assert abs(res.total_volume - s) <= 1e-12 * abs(s)
    return want


def both(call_area, call_vol, *args, **kw):
    return call_vol(*args, want_exposed=True, **kw), call_area(*args, want_exposed=True, **kw)


@pytest.fixture(scope="module")
def case_c():
    """2000 atoms at 100 atoms / nm^3 (edge 2.7 nm) and the restatement's volumes at 96 and 192 points"""
    xyz, vdw = blob(2000, 100.0, 11)
    refs = {p: vr.sasa_vol_ref(xyz, vdw, PROBE, table(p))[0] for p in (96, 192)}
    return xyz, vdw, refs


@pytest.fixture(scope="module")
def case_e():
    rng = np.random.default_rng(14)
    xyz = rng.uniform(0, 0.8, (700, 3)).astype(np.float32)
    R = rng.uniform(0.45, 0.55, 700).astype(np.float32)
    return xyz, R


# ---- one atom: the batch mapping and its tail
@pytest.mark.parametrize("npoints", [1, 63, 64, 65, 96, 960, 4096])
def test_one_atom(eng, npoints):
    xyz = np.array([[0.3, -1.0, 2.0]], np.float32)
    res, base = both(eng.sasa, eng.sasa_vol, xyz, [0.17], probe=PROBE, npoints=npoints)
    v = verify(res, base, xyz, [0.17], PROBE, npoints)
    R = float(np.float32(0.17) + np.float32(PROBE))
    assert abs(float(v[0]) - 4 * np.pi * R ** 3 / 3) <= 1e-6 * 4 * np.pi * R ** 3 / 3


# ---- two atoms: both cuts, the empty interval, a == 0
TWO_VOL = dict(TWO)
TWO_VOL["swallowed centre"] = ([[0, 0, 0], [0.3, 0, 0]], [0.4, 0.15])        # the small ball's rays start at lo_k > 0
TWO_VOL["equal radii at d = R"] = ([[0, 0, 0], [0, 0.25, 0]], [0.25, 0.25])


@pytest.mark.parametrize("name", list(TWO_VOL))
@pytest.mark.parametrize("real", [np.float32, np.float64])
def test_two_atoms(eng, m64, name, real):
    xyz, R = TWO_VOL[name]
    xyz, R = np.array(xyz, real), np.array(R, real)
    area, vol = (eng.sasa, eng.sasa_vol) if real == np.float32 else (m64.sasa, m64.sasa_vol)
    for npoints in (96, 960):
        res, base = both(area, vol, xyz, R, probe=0.0, npoints=npoints)
        v = verify(res, base, xyz, R, 0.0, npoints, real).astype(np.float64)
        ball = 4 * np.pi * R.astype(np.float64) ** 3 / 3
        if name in ("coincident", "tangent"):
            assert np.all(np.abs(v - ball) <= 1e-6 * ball)              # each keeps its full ball
        if name == "inside":                                           # the radical plane lies beyond both balls: an empty cell
            assert v[1] == 0 and abs(v[0] - ball[0]) <= 1e-6 * ball[0]
        if name == "swallowed centre":
            assert 0 < v[1] < 0.2 * ball[1] and 0.99 * ball[0] < v[0] < ball[0]
        if name in ("half", "equal radii at d = R"):
            assert abs(v[0] - v[1]) <= 1e-2 * v[0] and 0.5 * ball[0] < v[0] < ball[0]


# ---- several cells, hidden atoms
@pytest.mark.parametrize("npoints", [96, 192])
def test_blob(eng, case_c, npoints):
    xyz, vdw, refs = case_c
    res, base = both(eng.sasa, eng.sasa_vol, xyz, vdw, probe=PROBE, npoints=npoints)
    v = verify(res, base, xyz, vdw, PROBE, npoints, ref=refs[npoints])
    assert np.any(v == 0) and np.array_equal(res.volumes == 0, v == 0)              # hidden power cells: exactly 0
    assert np.all(res.volumes >= 0)


def test_blob_960_points(eng, case_c):
    xyz, vdw, _ = case_c
    res, base = both(eng.sasa, eng.sasa_vol, xyz[:600], vdw[:600], probe=PROBE, npoints=960)
    verify(res, base, xyz[:600], vdw[:600], PROBE, 960)


# ---- one crowded cell: the neighbours overflow the chunk, the cells are walked again per batch of points
def test_crowded(eng, case_e):
    xyz, R = case_e
    res, base = both(eng.sasa, eng.sasa_vol, xyz, R, probe=0.0, npoints=192)
    verify(res, base, xyz, R, 0.0, 192)


def test_crowded_f64(m64, case_e):
    xyz, R = case_e
    x64, r64 = xyz.astype(np.float64) * (1 + 1e-12), R.astype(np.float64)
    res, base = both(m64.sasa, m64.sasa_vol, x64, r64, probe=0.0, npoints=192)
    verify(res, base, x64, r64, 0.0, 192, np.float64)


def test_blob_f64(m64, case_c):
    xyz, vdw, _ = case_c
    x64, v64 = xyz.astype(np.float64) + 1e-9, vdw.astype(np.float64)
    res, base = both(m64.sasa, m64.sasa_vol, x64, v64, probe=PROBE, npoints=192)
    verify(res, base, x64, v64, PROBE, 192, np.float64)


# ---- mixed radii
def test_mixed_radii(eng):
    rng = np.random.default_rng(15)
    xyz = rng.uniform(0, 5.0, (1500, 3)).astype(np.float32)
    R = np.array([0.05, 0.3, 1.0], np.float32)[rng.integers(0, 3, 1500)]
    res, base = both(eng.sasa, eng.sasa_vol, xyz, R, probe=0.0, npoints=96)
    v = verify(res, base, xyz, R, 0.0, 96)
    assert np.any(v[R == np.float32(0.05)] == 0) and np.any(v > 0)


# ---- a selection of a larger frame, in permuted order
def test_selection(eng):
    xyz, vdw_all = blob(5000, 100.0, 12)
    rng = np.random.default_rng(13)
    idx = np.sort(rng.choice(5000, 2000, replace=False)).astype(np.uint64)
    vdw = vdw_all[idx.astype(np.int64)]
    res, base = both(eng.sasa, eng.sasa_vol, xyz, vdw, idx=idx, probe=PROBE, npoints=96)
    assert res.volumes.shape == (2000,)
    verify(res, base, xyz[idx.astype(np.int64)], vdw, PROBE, 96)
    perm = rng.permutation(2000)
    res2 = eng.sasa_vol(xyz, vdw[perm], idx=idx[perm], probe=PROBE, npoints=96, want_exposed=True)
    assert np.array_equal(res2.exposed, res.exposed[perm]) and np.array_equal(res2.areas, res.areas[perm])
    assert np.array_equal(res2.volumes, res.volumes[perm])              # min and max: the neighbours' order cannot matter


# ---- atoms that take no part
def test_non_finite(eng):
    xyz, vdw = blob(200, 100.0, 17)
    xyz, vdw = xyz.copy(), vdw.copy()
    xyz[17, 1] = np.nan
    vdw[60] = np.nan
    vdw[133] = np.float32(-PROBE)
    res, base = both(eng.sasa, eng.sasa_vol, xyz, vdw, probe=PROBE, npoints=96)
    verify(res, base, xyz, vdw, PROBE, 96)
    keep = np.setdiff1d(np.arange(200), [17, 60, 133])
    alone = eng.sasa_vol(xyz[keep], vdw[keep], probe=PROBE, npoints=96)
    assert np.array_equal(res.volumes[keep], alone.volumes) and res.volumes[[17, 60, 133]].tolist() == [0, 0, 0]


# ---- far from the origin, d is taken from the stored coordinates
def test_far_origin(eng, case_c):
    xyz, vdw, _ = case_c
    far = (xyz + np.array([1000.0, -2000.0, 3000.0], np.float32)).astype(np.float32)
    res, base = both(eng.sasa, eng.sasa_vol, far, vdw, probe=PROBE, npoints=96)
    verify(res, base, far, vdw, PROBE, 96)


# ---- the strict < of the neighbour filter at the bit level
@pytest.mark.parametrize("real", [np.float32, np.float64])
@pytest.mark.parametrize("shrink", [False, True])
def test_lattice(eng, m64, real, shrink):
    R = 0.25                                                          # vdw 0.125 + probe 0.125, exact in both precisions
    spacing = 2 * R * (1 - 2.0 ** -20) if shrink else 2 * R
    xyz = lattice(spacing, real)
    vdw = np.full(216, 0.125, real)
    area, vol = (eng.sasa, eng.sasa_vol) if real == np.float32 else (m64.sasa, m64.sasa_vol)
    res, base = both(area, vol, xyz, vdw, probe=0.125, npoints=192)
    v = verify(res, base, xyz, vdw, 0.125, 192, real).astype(np.float64)
    ball = 4 * np.pi * R ** 3 / 3
    if not shrink:
        assert np.all(np.abs(v - ball) <= 1e-6 * ball)                # d2 == (2R)^2: nobody is anybody's neighbour
    else:
        assert np.all(v <= ball * (1 + 1e-6)) and np.all(v > 0.999 * ball)


# ---- frames against single calls
def test_frames_equal_single_calls(eng, case_c):
    xyz, vdw, _ = case_c
    rng = np.random.default_rng(18)
    natoms, F, stride = 2000, 4, 3 * 2000 + 7
    buf = np.full(F * stride, np.nan, np.float32)                    # the padding is never read
    frames = []
    for f in range(F):
        fr = (xyz + rng.normal(0, 0.02, xyz.shape).astype(np.float32)).astype(np.float32)
        frames.append(fr)
        buf[f * stride:f * stride + 3 * natoms] = fr.reshape(-1)
    areas, volumes = np.zeros((F, natoms), np.float32), np.zeros((F, natoms), np.float32)
    totals, vtotals = np.zeros(F, np.float64), np.zeros(F, np.float64)
    from molar_amd._lib import check
    check(eng.lib.molar_hip_sasa_vol_frames(eng.ctx, buf.ctypes.data, F, stride, natoms, None, natoms, vdw.ctypes.data, C.c_float(PROBE), 96,
                                            areas.ctypes.data, totals.ctypes.data, volumes.ctypes.data, vtotals.ctypes.data))
    singles = [eng.sasa_vol(fr, vdw, probe=PROBE, npoints=96) for fr in frames]
    for f in range(F):
        assert np.array_equal(areas[f], singles[f].areas) and totals[f] == singles[f].total_area
        assert np.array_equal(volumes[f], singles[f].volumes) and vtotals[f] == singles[f].total_volume
    assert len(set(vtotals.tolist())) == F
    a2, t2, v2, vt2 = eng.sasa_vol_frames(np.stack(frames), vdw, probe=PROBE, npoints=96)
    assert np.array_equal(a2, areas) and np.array_equal(t2, totals) and np.array_equal(v2, volumes) and np.array_equal(vt2, vtotals)
    # totals alone
    t3, vt3 = np.zeros(F, np.float64), np.zeros(F, np.float64)
    check(eng.lib.molar_hip_sasa_vol_frames(eng.ctx, buf.ctypes.data, F, stride, natoms, None, natoms, vdw.ctypes.data, C.c_float(PROBE), 96,
                                            None, t3.ctypes.data, None, vt3.ctypes.data))
    assert np.array_equal(t3, totals) and np.array_equal(vt3, vtotals)
    # the volumes' total alone
    vt4 = np.zeros(F, np.float64)
    check(eng.lib.molar_hip_sasa_vol_frames(eng.ctx, buf.ctypes.data, F, stride, natoms, None, natoms, vdw.ctypes.data, C.c_float(PROBE), 96,
                                            None, None, None, vt4.ctypes.data))
    assert np.array_equal(vt4, vtotals)


# ---- device tensors in and out
def test_device_tensors(eng, case_c):
    import torch
    xyz, vdw_all, _ = case_c
    idx = np.arange(0, 2000, 3, dtype=np.uint64)
    vdw = vdw_all[idx.astype(np.int64)]
    host = eng.sasa_vol(xyz, vdw, idx=idx, probe=PROBE, npoints=96, want_exposed=True)
    dev = eng.sasa_vol(torch.from_numpy(xyz).cuda(), torch.from_numpy(vdw).cuda(), idx=torch.from_numpy(idx.astype(np.int64)).cuda(),
                       probe=PROBE, npoints=96, want_exposed=True)
    assert dev.areas.is_cuda and dev.exposed.is_cuda and dev.volumes.is_cuda
    assert np.array_equal(dev.areas.cpu().numpy(), host.areas) and np.array_equal(dev.volumes.cpu().numpy(), host.volumes)
    assert np.array_equal(dev.exposed.cpu().numpy().astype(np.uint32), host.exposed)
    assert dev.total_area == host.total_area and dev.total_volume == host.total_volume
    fr = torch.from_numpy(np.stack([xyz, xyz[::-1].copy()])).cuda()
    a, t, v, vt = eng.sasa_vol_frames(fr, vdw_all, probe=PROBE, npoints=96)
    single = eng.sasa_vol(xyz, vdw_all, probe=PROBE, npoints=96)
    assert a.is_cuda and v.is_cuda and np.array_equal(v[0].cpu().numpy(), single.volumes) and vt[0] == single.total_volume


# ---- an area call, a volume call and an area call again on one engine
def test_state_reuse(api, case_c):
    xyz, vdw, refs = case_c
    eng = api.Engine(0)
    m64 = api.MeasureF64(eng)
    small, vs = xyz[:37], vdw[:37]
    a1 = eng.sasa(xyz, vdw, probe=PROBE, npoints=96, want_exposed=True)
    verify(eng.sasa_vol(xyz, vdw, probe=PROBE, npoints=96, want_exposed=True), a1, xyz, vdw, PROBE, 96, ref=refs[96])
    a2 = eng.sasa(xyz, vdw, probe=PROBE, npoints=96, want_exposed=True)
    assert np.array_equal(a1.areas, a2.areas) and np.array_equal(a1.exposed, a2.exposed) and a1.total_area == a2.total_area
    assert a2.volumes is None and a2.total_volume is None
    # another shape, point count and precision in between, then the first shape again
    s64 = m64.sasa(small, vs, probe=PROBE, npoints=64, want_exposed=True)
    verify(m64.sasa_vol(small, vs, probe=PROBE, npoints=64, want_exposed=True), s64, small, vs, PROBE, 64, np.float64)
    a3 = eng.sasa(xyz, vdw, probe=PROBE, npoints=192, want_exposed=True)
    verify(eng.sasa_vol(xyz, vdw, probe=PROBE, npoints=192, want_exposed=True), a3, xyz, vdw, PROBE, 192, ref=refs[192])
    verify(eng.sasa_vol(xyz, vdw, probe=PROBE, npoints=96, want_exposed=True), a1, xyz, vdw, PROBE, 96, ref=refs[96])
    eng.close()


def test_cached_search_survives_a_volume_call(api, eng, case_c):
    xyz, vdw, _ = case_c
    rng = np.random.default_rng(19)
    other = rng.uniform(0, 3.0, (3000, 3)).astype(np.float32)
    n = eng.search_count(api.SEARCH_SINGLE, 0.4, other)
    want = eng.search_fill(n)
    n2 = eng.search_count(api.SEARCH_SINGLE, 0.4, other)
    eng.sasa_vol(xyz, vdw, probe=PROBE, npoints=96)
    got = eng.search_fill(n2)
    assert n2 == n and n > 0
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- argument checks: those of the area calls, with the same texts
@pytest.mark.parametrize("kw", [dict(npoints=0), dict(npoints=4097), dict(probe=-0.1), dict(probe=float("nan"))])
def test_errors(api, eng, m64, kw):
    xyz = np.zeros((3, 3), np.float32)
    for call, ref_call, x in ((eng.sasa_vol, eng.sasa, xyz), (m64.sasa_vol, m64.sasa, xyz.astype(np.float64))):
        with pytest.raises(api.MolarHipError) as e:
            call(x, [0.1, 0.1, 0.1], **kw)
        with pytest.raises(api.MolarHipError) as e0:
            ref_call(x, [0.1, 0.1, 0.1], **kw)
        assert e.value.code == 50 and ("npoints" in str(e.value) or "probe" in str(e.value))
        assert str(e.value).split(":", 1)[1] == str(e0.value).split(":", 1)[1]          # the same text behind the call's name
    with pytest.raises(api.MolarHipError) as e:
        eng.sasa_vol_frames(xyz[None], [0.1, 0.1, 0.1], **kw)
    assert e.value.code == 50


def test_empty_selection(eng):
    xyz = np.zeros((3, 3), np.float32)
    res = eng.sasa_vol(xyz, np.zeros(0, np.float32), idx=np.zeros(0, np.uint64), probe=PROBE, npoints=96, want_exposed=True)
    assert res.total_area == 0.0 and res.total_volume == 0.0 and res.volumes.shape == (0,) and res.areas.shape == (0,)


# ---- the selection's method, end to end
def test_sel_sasa_vol(api, eng, case_c):
    xyz, vdw, _ = case_c
    top = api.Topology(np.ones(2000, np.float32), vdw)
    sel = api.Sel(top, api.State(xyz), np.arange(100, 1900), engine=eng)
    res = sel.sasa_vol(probe=PROBE, npoints=96)
    base = sel.sasa(probe=PROBE, npoints=96)
    assert np.array_equal(res.areas, base.areas) and res.total_area == base.total_area
    want, tot = vr.sasa_vol_ref(xyz[100:1900], vdw[100:1900], PROBE, table(96))
    got = res.volumes.astype(np.float64)
    R = (vdw[100:1900] + np.float32(PROBE)).astype(np.float64)
    assert np.all(np.abs(got - want) <= 1e-6 * want + 1e-12 * (4 * np.pi / 3) * R ** 3)
    assert abs(res.total_volume - float(got.sum())) <= 1e-12 * float(got.sum()) and res.volumes.shape == (1800,)
