"""The internal-coordinate calls without a GPU: the numpy reference (tests/intcoord_ref.py) against hand-known answers, the
plan entry (a pure host function), the errors of the arguments alone, and the host helpers."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import intcoord_ref as ir  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from molar_amd import _lib, build
    build.build_library()
    return _lib.load()


def error_codes():
    hdr = open(os.path.join(ROOT, "include", "molar_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"(MOLAR_HIP_ERR_\w+)\s*=\s*(-?\d+)", hdr)}


def one(points, kind=None, **kw):
    """the reference's value of one tuple over all the points given, one frame"""
    x = np.asarray(points, np.float64)[None]
    t = np.arange(x.shape[1], dtype=np.uint64)[None]
    return ir.reference(x, t, kind, **kw)


def gmx_sign_dihedral(a, b, c, d):
    """The arithmetic of the reference project's DSSP dihedral written out: degrees, 360 for a degenerate one."""
    ba, cd, cb = a - b, d - c, b - c
    p = np.cross(cb, ba)
    q = np.cross(cb, cd)
    r = np.cross(cb, q)
    qq, rr = q @ q, r @ r
    if qq > 0 and rr > 0:
        return np.degrees(np.arctan2((p @ r) / np.sqrt(rr), (p @ q) / np.sqrt(qq)))
    return 360.0


def butane(phi_deg):
    """four atoms with bond angles of 110 degrees and the IUPAC dihedral phi"""
    th, ph = np.radians(110.0), np.radians(phi_deg)
    b, c = np.array([0.0, 0.0, 0.0]), np.array([1.5, 0.0, 0.0])
    a = b + 1.5 * np.array([np.cos(np.pi - th), np.sin(np.pi - th), 0.0])
    # D: A's direction about the axis turned by phi, mirrored to C's side
    d = c + 1.5 * np.array([-np.cos(np.pi - th), np.sin(np.pi - th) * np.cos(ph), np.sin(np.pi - th) * np.sin(ph)])
    return a, b, c, d


def test_reference_known_dihedrals_and_the_sign_of_the_reference_project():
    for phi in (0.0, 180.0, 60.0, -60.0, 120.0, -150.0, 5.0):
        a, b, c, d = butane(phi)
        ref = one([a, b, c, d])
        got = np.degrees(ref.values[0, 0])
        assert abs((got - phi + 180.0) % 360.0 - 180.0) < 1e-12, (phi, got)
        g = gmx_sign_dihedral(a, b, c, d)
        assert abs((got - g + 180.0) % 360.0 - 180.0) < 1e-9, (phi, got, g)
        if phi not in (0.0, 180.0):
            assert np.sign(got) == np.sign(phi) == np.sign(g)
            # ... which is the sign of (b1 x b2) . b3
            assert np.sign(np.cross(b - a, c - b) @ (d - c)) == np.sign(phi)
    # cis and trans to the last bit that matters
    assert abs(one(butane(0.0)).values[0, 0]) < 1e-15
    assert abs(abs(one(butane(180.0)).values[0, 0]) - np.pi) < 1e-15


def test_reference_water_angle_and_distances_across_the_boundary():
    th = np.radians(104.5)
    o = np.array([0.3, -0.2, 0.1])
    h1 = o + 0.9572 * np.array([1.0, 0.0, 0.0])
    h2 = o + 0.9572 * np.array([np.cos(th), np.sin(th), 0.0])
    ref = one([h1, o, h2])
    assert abs(np.degrees(ref.values[0, 0]) - 104.5) < 1e-12 and ref.valid[0] == 1
    # a 3-4-5 triangle across the faces of an orthorhombic cell: A near the origin corner, B on the far side
    box = ir.ortho_box((10.0, 12.0, 14.0))
    a = np.array([1.0, 1.5, 7.0])
    b = a + np.array([-3.0, -4.0, 0.0]) + np.array([10.0, 12.0, 0.0])
    ref = one([a, b], boxes=box)
    assert abs(ref.values[0, 0] - 5.0) < 1e-15
    assert abs(one([a, b]).values[0, 0] - np.linalg.norm(b - a)) < 1e-14            # without a box: the long way
    assert abs(one([a, b], boxes=box, pbc=1).values[0, 0] - np.hypot(3.0, 8.0)) < 1e-14   # x alone is periodic
    # ... and of a triclinic one: B moved by a lattice vector that no orthorhombic reduction undoes
    tb = ir.tric_box((10.0, 12.0, 14.0))
    rows = tb.reshape(3, 3).astype(np.float64)
    b = a + np.array([3.0, 0.0, 4.0]) + rows[1] - rows[2]
    ref = one([a, b], boxes=tb)
    assert abs(ref.values[0, 0] - 5.0) < 1e-13


def test_reference_binning_statistics_and_invalid_values():
    # two tuples over three frames of dihedrals with known values
    phis = np.array([[15.0, -165.0], [25.0, 165.0], [35.0, np.nan]])
    fr = np.zeros((3, 8, 3))
    for f in range(3):
        for t in range(2):
            pts = butane(phis[f, t] if np.isfinite(phis[f, t]) else 0.0)
            fr[f, 4 * t:4 * t + 4] = pts
    fr[2, 5, 1] = np.nan
    tu = np.arange(8, dtype=np.uint64).reshape(2, 4)
    ref = ir.reference(fr, tu, nbins=36, pairs=[[0, 1], [1, 1]], map_bins=4, labels=[1, 0], ngroups=3)
    ir.margin_ok(ref)
    assert list(ref.valid) == [3, 2] and np.isnan(ref.values[2, 1]) and ref.bound[2, 1] == 0
    assert ref.hist.shape == (3, 36) and int(ref.hist.sum()) == 5 and int(ref.hist[2].sum()) == 0
    assert ref.hist[1, 19] == 1 and ref.hist[1, 20] == 1 and ref.hist[1, 21] == 1 and ref.hist[0, 1] == 1 and ref.hist[0, 34] == 1
    assert ref.map.shape == (1, 4, 4) and int(ref.map.sum()) == 4 and ref.map[0, 2, 0] == 1 and ref.map[0, 2, 3] == 1
    assert ref.map[0, 0, 0] == 1 and ref.map[0, 3, 3] == 1
    assert abs(np.degrees(ref.mean[0]) - 25.0) < 1e-3 and abs(abs(np.degrees(ref.mean[1])) - 180.0) < 1e-9
    c = np.cos(np.radians(phis[:, 0]))
    s = np.sin(np.radians(phis[:, 0]))
    assert abs(ref.spread[0] - (1 - np.hypot(c.sum(), s.sum()) / 3)) < 1e-15
    # a tuple with A == B, three collinear atoms, and one that is invalid in every frame
    x = np.array([[[0, 0, 0], [0, 0, 0], [1, 0, 0], [1, 1, 0], [2, 0, 0], [3, 0, 0], [3, 1, 1]]], np.float64)
    ra = ir.reference(x, np.array([[0, 1, 2], [1, 2, 3]], np.uint64), nbins=4)
    assert np.isnan(ra.values[0, 0]) and abs(ra.values[0, 1] - np.pi / 2) < 1e-15 and list(ra.valid) == [0, 1]
    assert np.isnan(ra.mean[0]) and np.isnan(ra.spread[0]) and int(ra.hist.sum()) == 1
    rd = ir.reference(x, np.array([[1, 2, 4, 6], [3, 2, 4, 5], [3, 2, 5, 6]], np.uint64))
    assert np.isnan(rd.values[0, 0]) and np.isnan(rd.values[0, 1]) and np.isfinite(rd.values[0, 2]) and list(rd.valid) == [0, 0, 1]
    assert one([[0, 0, 0], [0, 0, 0]]).values[0, 0] == 0 and one([[0, 0, 0], [0, 0, 0]]).valid[0] == 1      # a distance of 0 is valid
    # distances are binned in [lo, hi) only
    rr = ir.reference(np.array([[[0, 0, 0], [1.0, 0, 0], [2.5, 0, 0], [2.75, 0, 0]]]), np.array([[0, 1], [0, 2], [0, 3], [1, 2]], np.uint64), nbins=3,
                      range=(1.0, 2.5))
    assert list(rr.hist[0]) == [1, 1, 0]


def test_generators_keep_the_margins_for_every_shape():
    for kind in (2, 3, 4):
        rng = (0.6, 2.0) if kind == 2 else None
        for box in ("none", "ortho", "tric"):
            for F, T in ((1, 1), (2, 257), (65, 65), (129, 1)):
                fr, tu, bx, ref = ir.make_case(7, F, T, kind, box=box, nbins=36, range=rng)
                assert ir.margin_ok(ref) and fr.dtype == np.float32 and tu.shape == (T, kind)
                assert (ref.valid == F).all() and ref.bound.max() < 1e-9
    fr, tu, bx, ref = ir.make_case(8, 3, 40, 4, box="ortho", pbc=5, nbins=10)
    assert ir.margin_ok(ref)


def spec(kind=4, nbins=0, map_bins=0, lo=0.0, hi=1.0, reserved=0):
    from molar_amd import _lib
    s = _lib.IntcoordSpec()
    s.kind, s.nbins, s.map_bins, s.reserved, s.lo, s.hi = kind, nbins, map_bins, reserved, lo, hi
    return s


def test_abi_of_the_three_entries(lib):
    from molar_amd import _lib, build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_ffi as gen
    raw = open(gen.HEADER).read()
    funcs = {name: params for name, _, params in gen.c_functions(raw)}
    assert len(funcs["molar_hip_intcoord_plan"]) == len(_lib.SYMBOLS["molar_hip_intcoord_plan"][1]) == 11
    assert len(funcs["molar_hip_intcoord"]) == len(_lib.SYMBOLS["molar_hip_intcoord"][1]) == 24
    assert len(funcs["molar_hip_intcoord_f64"]) == len(_lib.SYMBOLS["molar_hip_intcoord_f64"][1]) == 24
    assert [t for t, _ in funcs["molar_hip_intcoord"]] == [t.replace("double", "float") for t, _ in funcs["molar_hip_intcoord_f64"]]
    for name in ("molar_hip_intcoord_plan", "molar_hip_intcoord", "molar_hip_intcoord_f64"):
        assert hasattr(lib, name)
    body = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*molar_hip_intcoord_spec\s*;", gen.strip_comments(raw)).group(1)
    cfields = [re.search(r"(\w+)\s*$", part.strip()).group(1) for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert cfields == ["kind", "nbins", "map_bins", "reserved", "lo", "hi"] == [f for f, _ in _lib.IntcoordSpec._fields_]
    assert C.sizeof(_lib.IntcoordSpec) == 32
    rs = open(os.path.join(ROOT, "rust", "molar_hip", "src", "types.rs")).read()
    rbody = re.search(r"#\[repr\(C\)\]\n#\[derive\([^)]*\)\]\npub struct MolarHipIntcoordSpec\s*\{(.*?)\n\}", rs, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): ([^,]+),", rbody) == [("kind", "u32"), ("nbins", "u32"), ("map_bins", "u32"), ("reserved", "u32"), ("lo", "f64"),
                                                         ("hi", "f64")]
    hpp = open(os.path.join(ROOT, "include", "molar_hip.hpp")).read()
    assert "inline InternalCoords internal_coords(" in hpp and "internal_coords_f64(" in hpp and "(molar_hip_intcoord," in hpp and "(molar_hip_intcoord_f64," in hpp
    lib_rs = open(os.path.join(ROOT, "rust", "molar_hip", "src", "lib.rs")).read()
    assert "pub fn internal_coords(" in lib_rs
    assert "intcoord.hip" in build.SOURCES


def test_plan_needs_no_gpu_and_is_monotone(lib):
    from molar_amd import api
    assert api.intcoord_plan(0, 100, 4)[0] == 0 and api.intcoord_plan(100, 0, 4)[0] == 0
    ws, fc, tc, lc = api.intcoord_plan(256, 5000, 4, nbins=72, map_bins=72, npairs=100)
    assert fc >= 1 and tc >= 64 and lc >= 1024
    sizes = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096, 65536, 1000000]
    for kind, rng in ((2, (0.0, 3.0)), (3, None), (4, None)):
        for stats in (False, True):
            grid = [[api.intcoord_plan(F, T, kind, range=rng, want_stats=stats) for T in sizes] for F in sizes]
            for i in range(len(sizes)):
                row = [grid[i][j][0] for j in range(len(sizes))]
                col = [grid[j][i][0] for j in range(len(sizes))]
                assert row == sorted(row) and col == sorted(col)
                assert all(g[1:] == (fc, tc, lc) for g in grid[i])
            # the chunk partials: two doubles and a count per tuple and chunk of frames
            if stats:
                assert grid[-1][-1][0] >= 20 * sizes[-1] * ((sizes[-1] + fc - 1) // fc)
            assert grid[3][3][0] >= (grid[3][3][0] if stats else 0)
        assert api.intcoord_plan(100, 100, kind, range=rng, want_stats=True)[0] >= api.intcoord_plan(100, 100, kind, range=rng, want_stats=False)[0]
    codes = error_codes()
    inv = codes["MOLAR_HIP_ERR_INVALID_ARGUMENT"]
    plan = lib.molar_hip_intcoord_plan
    for bad in (spec(kind=1), spec(kind=5), spec(kind=0), spec(kind=2, lo=1.0, hi=1.0), spec(kind=2, lo=2.0, hi=1.0), spec(kind=2, lo=0.0, hi=np.inf),
                spec(kind=2, lo=np.nan, hi=1.0), spec(reserved=1)):
        assert plan(10, 10, 1, 0, 1, C.addressof(bad), 1, None, None, None, None) == inv
    assert plan(10, 10, 1, 0, 1, None, 1, None, None, None, None) == inv
    s = spec(nbins=1 << 16)
    assert plan(10, 10, (1 << 15) - 1, 0, 1, C.addressof(s), 1, None, None, None, None) == 0
    assert plan(10, 10, 1 << 15, 0, 1, C.addressof(s), 1, None, None, None, None) == inv            # G nbins = 2^31
    s = spec(map_bins=1 << 15)
    assert plan(10, 10, 1, 4, 1, C.addressof(s), 1, None, None, None, None) == 0
    assert plan(10, 10, 1, 4, 2, C.addressof(s), 1, None, None, None, None) == inv                  # G2 map_bins^2 = 2^31
    ok = spec(kind=2, lo=0.0, hi=1.0)
    assert plan(10, 10, 0, 0, 0, C.addressof(ok), 0, None, None, None, None) == 0


def raw_call(fn, ctx, real, frames, tuples, sp, F=None, stride=None, natoms=None, T=None, labels=None, G=1, boxes=None, box_stride=0, pbc=0, pairs=None,
             P=0, plabels=None, G2=1, values=None, ld=None, hist=None, hmap=None, mean=None, spread=None, valid=None):
    fr = np.ascontiguousarray(frames, real)
    tu = np.ascontiguousarray(tuples, np.uint64)
    keep = [fr, tu]

    def ptr(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dt)
        keep.append(a)
        return a.ctypes.data

    F = fr.shape[0] if F is None else F
    natoms = fr.shape[1] if natoms is None else natoms
    stride = 3 * fr.shape[1] if stride is None else stride
    T = tu.shape[0] if T is None else T
    ld = T if ld is None else ld
    out = lambda a: None if a is None else a.ctypes.data
    return fn(ctx, fr.ctypes.data, F, stride, natoms, tu.ctypes.data if tu.size else None, T, ptr(labels, np.uint32), G, ptr(boxes, real), box_stride, pbc,
              None if sp is None else C.addressof(sp), ptr(pairs, np.uint64), P, ptr(plabels, np.uint32), G2, out(values), ld, out(hist), out(hmap),
              out(mean), out(spread), out(valid))


def test_argument_errors_need_no_device(lib):
    codes = error_codes()
    inv, nopbc, sizes = codes["MOLAR_HIP_ERR_INVALID_ARGUMENT"], codes["MOLAR_HIP_ERR_NO_PBC"], codes["MOLAR_HIP_ERR_SIZES"]
    ctx = C.create_string_buffer(1 << 16)                    # never read: the arguments are judged before the context is used
    c = C.addressof(ctx)
    tu = np.array([[0, 1, 2, 3], [1, 2, 3, 4]], np.uint64)
    box = ir.ortho_box((5, 5, 5))
    for fn, real in ((lib.molar_hip_intcoord, np.float32), (lib.molar_hip_intcoord_f64, np.float64)):
        fr = np.zeros((2, 5, 3), real)
        vals = np.full((2, 2), 7, real)
        h = np.full((1, 4), 7, np.uint64)
        cases = [
            ("null context", inv, dict(ctx=None, sp=spec())),
            ("null spec", inv, dict(sp=None)),
            ("kind 1", inv, dict(sp=spec(kind=1))),
            ("kind 5", inv, dict(sp=spec(kind=5))),
            ("reserved", inv, dict(sp=spec(reserved=3))),
            ("distance lo == hi", inv, dict(sp=spec(kind=2, lo=1.0, hi=1.0), tuples=tu[:, :2])),
            ("distance range not finite", inv, dict(sp=spec(kind=2, lo=0.0, hi=np.inf), tuples=tu[:, :2])),
            ("labels and ngroups 0", sizes, dict(sp=spec(), labels=[0, 0], G=0)),
            ("pair labels and npair_groups 0", sizes, dict(sp=spec(), plabels=[0], pairs=[[0, 1]], P=1, G2=0)),
            ("G nbins 2^31", inv, dict(sp=spec(nbins=1 << 16), labels=[0, 0], G=1 << 15)),
            ("G2 map_bins^2 2^31", inv, dict(sp=spec(map_bins=1 << 15), plabels=[0], pairs=[[0, 1]], P=1, G2=2)),
            ("pbc 8", inv, dict(sp=spec(), pbc=8, boxes=box)),
            ("box_stride 3", inv, dict(sp=spec(), pbc=7, boxes=box, box_stride=3)),
            ("hist without nbins", inv, dict(sp=spec(), hist=h)),
            ("map without map_bins", inv, dict(sp=spec(), hmap=h, pairs=[[0, 1]], P=1)),
            ("map without pairs", inv, dict(sp=spec(map_bins=2), hmap=h)),
            ("ld below T", inv, dict(sp=spec(), values=vals, ld=1)),
            ("null tuples", inv, dict(sp=spec(), tuples=np.zeros((0, 4), np.uint64), T=2)),
            ("natoms 0", inv, dict(sp=spec(), natoms=0)),
            ("stride below 3 natoms", inv, dict(sp=spec(), stride=14)),
            ("pbc without boxes", nopbc, dict(sp=spec(), pbc=7)),
            ("null frames", inv, dict(sp=spec(), frames=None)),
            ("index not below natoms", inv, dict(sp=spec(), tuples=[[0, 1, 2, 5], [0, 1, 2, 3]], values=vals)),
            ("label not below ngroups", inv, dict(sp=spec(nbins=4), labels=[0, 1], G=1, hist=h)),
            ("pair not below T", inv, dict(sp=spec(map_bins=2), pairs=[[0, 2]], P=1, hmap=h)),
            ("pair label not below groups", inv, dict(sp=spec(map_bins=2), pairs=[[0, 1]], P=1, plabels=[1], G2=1, hmap=h)),
        ]
        for what, want, kw in cases:
            kw = dict(kw)
            cc = kw.pop("ctx", c)
            frames = kw.pop("frames", fr)
            tuples = kw.pop("tuples", tu)
            sp = kw.pop("sp")
            if frames is None:
                got = fn(cc, None, 2, 15, 5, tu.ctypes.data, 2, None, 1, None, 0, 0, C.addressof(sp), None, 0, None, 1, None, 2, None, None, None, None, None)
            else:
                got = raw_call(fn, cc, real, frames, tuples, sp, **kw)
            assert got == want, (what, want, got, lib.molar_hip_last_error())
        assert (vals == 7).all() and (h == 7).all(), "no output is touched after an error"
        # the two no-ops, and they come after the checks of the arguments alone
        assert raw_call(fn, c, real, np.zeros((0, 5, 3), real), tu, spec(), F=0, values=vals) == 0
        assert raw_call(fn, c, real, fr, np.zeros((0, 4), np.uint64), spec(), values=np.zeros((2, 0), real)) == 0
        assert raw_call(fn, c, real, np.zeros((0, 5, 3), real), tu, spec(kind=7), F=0) == inv
        assert (vals == 7).all()


def test_backbone_dihedrals_on_a_small_peptide():
    from molar_amd import api
    names = ["N", "H", "CA", "C", "O"] * 3
    resids = [5] * 5 + [6] * 5 + [7] * 5
    phi, psi, omega, rphi, rpsi, rom, pairs = api.backbone_dihedrals(names, resids)
    assert phi.dtype == np.uint64 and phi.tolist() == [[3, 5, 7, 8], [8, 10, 12, 13]] and rphi.tolist() == [1, 2]
    assert psi.tolist() == [[0, 2, 3, 5], [5, 7, 8, 10]] and rpsi.tolist() == [0, 1]
    assert omega.tolist() == [[2, 3, 5, 7], [7, 8, 10, 12]] and rom.tolist() == [0, 1]
    assert pairs.tolist() == [[0, 3]]                    # residue 6 alone has both; psi rows counted from len(phi)
    # a missing atom: no CA in the middle residue
    keep = [i for i in range(15) if i != 7]
    phi, psi, omega, rphi, rpsi, rom, pairs = api.backbone_dihedrals([names[i] for i in keep], [resids[i] for i in keep])
    assert phi.tolist() == [[7, 9, 11, 12]] and rphi.tolist() == [2]
    assert psi.tolist() == [[0, 2, 3, 5]] and rpsi.tolist() == [0]
    assert omega.tolist() == [] and omega.shape == (0, 4) and pairs.shape == (0, 2)
    # a chain break: by the chain column, and by a gap in the residue numbers
    for kw in (dict(chains=["A"] * 5 + ["B"] * 10), ):
        phi, psi, omega, rphi, rpsi, rom, pairs = api.backbone_dihedrals(names, resids, **kw)
        assert phi.tolist() == [[8, 10, 12, 13]] and psi.tolist() == [[5, 7, 8, 10]] and omega.tolist() == [[7, 8, 10, 12]] and pairs.shape == (0, 2)
    phi, psi, omega, rphi, rpsi, rom, pairs = api.backbone_dihedrals(names, [5] * 5 + [7] * 5 + [8] * 5)
    assert phi.tolist() == [[8, 10, 12, 13]] and rphi.tolist() == [2] and psi.tolist() == [[5, 7, 8, 10]]
    # gro.GroTopology's columns go straight in
    from molar_amd import gro
    assert hasattr(gro, "GroTopology")


def test_circular_std_degrees_and_edges():
    from molar_amd import api
    v = np.array([0.0, 1 - np.exp(-0.5), 1.0, np.nan])
    s = api.circular_std(v)
    assert s[0] == 0 and abs(s[1] - 1.0) < 1e-15 and np.isinf(s[2]) and np.isnan(s[3])
    # a narrow distribution: the circular standard deviation is the ordinary one
    rng = np.random.default_rng(0)
    phi = 2.0 + 0.01 * rng.normal(size=20000)
    V = 1 - np.hypot(np.cos(phi).sum(), np.sin(phi).sum()) / phi.size
    assert abs(api.circular_std(V) - phi.std()) < 1e-5
    assert api.intcoord_degrees(np.pi) == 180.0
    e = api.intcoord_edges(4, 36)
    assert e.shape == (37,) and e[0] == -np.pi and e[-1] == np.pi
    assert api.intcoord_edges(3, 2).tolist() == [0.0, np.pi / 2, np.pi]
    assert api.intcoord_edges(2, 3, (1.0, 2.5)).tolist() == [1.0, 1.5, 2.0, 2.5]
