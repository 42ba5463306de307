"""Van Hove, everything that needs no GPU: the arithmetic of molar_hip_vanhove_plan and the bound on the pairs between two flushes
of the on-chip counters, the argument errors the library reports before it touches the context, the host helpers of api.py
(density, F_s, the J0 quadrature, the lags), and the reference of tests/vanhove_ref.py - against plain loops, and its own
assertions on every case the GPU tests use."""
import ctypes as C
import decimal
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vanhove_ref as vr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = vr.error_codes(open(os.path.join(ROOT, "include", "molar_hip.h")).read())
I, S, TL = CODES["INVALID_ARGUMENT"], CODES["SIZES"], CODES["TOO_LARGE"]


@pytest.fixture(autouse=True)
def plain_plan(monkeypatch):
    monkeypatch.delenv("MOLAR_HIP_VANHOVE_ONCHIP", raising=False)
    monkeypatch.delenv("MOLAR_HIP_VANHOVE_COMBINE", raising=False)


def test_the_three_entries_are_bound_on_every_side():
    from molar_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    assert "vanhove.hip" in build.SOURCES
    for name, nargs in (("molar_hip_vanhove_plan", 14), ("molar_hip_vanhove", 22), ("molar_hip_vanhove_f64", 22)):
        assert hasattr(lib, name) and len(_lib.SYMBOLS[name][1]) == nargs, name
    header = " ".join(open(os.path.join(ROOT, "include", "molar_hip.h")).read().split())
    ffi = open(os.path.join(ROOT, "rust", "molar_hip", "src", "ffi.rs")).read()
    for name in ("molar_hip_vanhove_plan", "molar_hip_vanhove", "molar_hip_vanhove_f64"):
        assert f"int {name}(" in header and f'b"{name}\\0"' in ffi, name
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_ffi as gen
    assert open(gen.OUT).read() == gen.render(gen.c_functions(open(gen.HEADER).read())), "run python tools/gen_rust_ffi.py"
    hpp = open(os.path.join(ROOT, "include", "molar_hip.hpp")).read()
    assert "van_hove(" in hpp and "van_hove_f64(" in hpp and "(molar_hip_vanhove," in hpp and "(molar_hip_vanhove_f64," in hpp
    lib_rs = open(os.path.join(ROOT, "rust", "molar_hip", "src", "lib.rs")).read()
    types_rs = open(os.path.join(ROOT, "rust", "molar_hip", "src", "types.rs")).read()
    assert "pub fn van_hove(" in lib_rs and "pub fn van_hove_plan(" in lib_rs and "pub struct VanHove {" in types_rs


def test_plan_sizes_and_monotone_workspace(monkeypatch):
    from molar_amd import api
    p = api.vanhove_plan(1000, 100, 2, 12, 200, 3)
    assert p.origins_per_pass >= 64 and p.origins_per_pass % 64 == 0, "whole waves of origins"
    assert p.particles_per_wg >= 1 and p.lds_cells >= 1024
    # the lag tile: as many lags as the on-chip cells hold bins for, within its largest size
    widest = api.vanhove_plan(1000, 100, 1, 12, 1, 3).lag_tile
    for nbins in (1, 16, 200, 256, 257, 512, 1000, p.lds_cells // 2, p.lds_cells // 2 + 1, p.lds_cells - 1, p.lds_cells):
        q = api.vanhove_plan(1000, 100, 1, 12, nbins, 3)
        assert q.on_chip == 1 and q.lag_tile == max(1, min(widest, p.lds_cells // nbins)) and q.lag_tile * nbins <= p.lds_cells, nbins
    # the documented limit: nbins above lds_cells goes to memory, and the override sends everything there
    assert api.vanhove_plan(1000, 100, 1, 12, p.lds_cells + 1, 3).on_chip == 0
    monkeypatch.setenv("MOLAR_HIP_VANHOVE_ONCHIP", "0")
    assert api.vanhove_plan(1000, 100, 1, 12, 16, 3).on_chip == 0
    monkeypatch.delenv("MOLAR_HIP_VANHOVE_ONCHIP")
    # never smaller for a larger argument
    base = (1000, 100, 2, 12, 200, 2)
    ws = api.vanhove_plan(*base).workspace_bytes
    assert ws >= 1000 * 100 * 2 * 8
    for k in range(6):
        for grow in (1, 7, 1000):
            args = list(base)
            args[k] = args[k] + grow if k < 5 else 3
            assert api.vanhove_plan(*args).workspace_bytes >= ws, args
    grid = np.array([[api.vanhove_plan(F, n, 1, 4, 16, 3).workspace_bytes for n in (1, 7, 8, 9, 500)] for F in (1, 2, 1023, 1024, 1025, 5000)])
    assert (np.diff(grid, axis=0) >= 0).all() and (np.diff(grid, axis=1) >= 0).all()
    assert api.vanhove_plan(0, 100).workspace_bytes == 0 and api.vanhove_plan(100, 0).workspace_bytes == 0
    for bad in (dict(ndims=0), dict(ndims=4)):
        with pytest.raises(api.MolarHipError) as e:
            api.vanhove_plan(10, 10, **bad)
        assert e.value.code == I
    with pytest.raises(api.MolarHipError) as e:
        api.vanhove_plan(1 << 31, 10)
    assert e.value.code == TL


def test_no_on_chip_counter_can_overflow():
    """pairs_per_flush - the particles a workgroup walks times the origins it walks - bounds what one 32-bit cell receives
    between two flushes; below 2^32 for every plan of the grid, and never below the pairs of one particle over one pass."""
    from molar_amd import api
    worst = 0
    for F in (1, 2, 1000, 1024, 1025, 65536, 1 << 20, (1 << 20) + 1, 1 << 24, 1 << 29, (1 << 31) - 1000):
        for n in (1, 8, 9, 256, 100000):
            for nlags, nbins in ((1, 1), (12, 200), (32, 512), (100, 16), (1, 1 << 14)):
                p = api.vanhove_plan(F, n, 1, nlags, nbins, 1)
                assert p.pairs_per_flush < 1 << 32, (F, n, nlags, nbins)
                assert p.pairs_per_flush >= min(F, p.origins_per_pass) * min(p.particles_per_wg, 1), (F, n)
                passes = -(-F // p.origins_per_pass)
                per_wg = -(-passes // p.pass_splits)
                assert p.pairs_per_flush == p.particles_per_wg * min(F, per_wg * p.origins_per_pass)
                worst = max(worst, p.pairs_per_flush)
    print("largest pairs_per_flush of the grid:", worst)


def raw_call(fn, ctx, real, F=4, natoms=10, stride=None, idx=None, n=4, labels=None, G=1, lags=(0, 1), nlags=None, null_lags=False, os=1, dims=7, flags=0, lo=0.0,
             hi=1.0, nbins=8, null_traj=False, want=("hist", "outside", "norigins", "nvalid", "bad")):
    """One call through ctypes with host arrays; the status and the outputs."""
    traj = np.zeros((max(F, 1), natoms, 3), real)
    keep = []

    def ptr(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dt)
        keep.append(a)
        return a.ctypes.data
    L = len(lags) if nlags is None else nlags
    Gs = G if labels is not None else 1
    shapes = {"hist": ((Gs, L, nbins), np.uint64), "outside": ((Gs, L), np.uint64), "norigins": ((L,), np.uint64), "nvalid": ((Gs,), np.uint64), "bad": ((n,), np.uint32)}
    cells = Gs * L * nbins
    outs = {k: (np.full(shapes[k][0] if cells < 1 << 20 or k != "hist" else (1,), 77, shapes[k][1]) if k in want else None) for k in shapes}
    o = {k: (None if v is None else v.ctypes.data) for k, v in outs.items()}
    rc = fn(ctx, None if null_traj else traj.ctypes.data, F, 3 * natoms if stride is None else stride, natoms, ptr(idx, np.uint64), n, ptr(labels, np.uint32), G,
            None if null_lags else ptr(np.asarray(lags, np.uint64) if len(lags) else np.zeros(1, np.uint64), np.uint64), L, os, dims, flags, lo, hi, nbins, o["hist"],
            o["outside"], o["norigins"], o["nvalid"], o["bad"])
    return rc, outs


def test_argument_errors_need_no_device():
    from molar_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    ctx = C.create_string_buffer(1 << 16)                    # never read: the arguments are judged before the context is used
    inf, nan = float("inf"), float("nan")
    errors = [
        ("n = 0", S, dict(n=0)),
        ("no lags", S, dict(lags=())),
        ("labels with ngroups = 0", S, dict(labels=[0, 0, 0, 0], G=0)),
        ("2^31 cells", TL, dict(labels=[0, 0, 0, 0], G=1 << 12, lags=(0, 1), nbins=1 << 18, want=())),
        ("a lag not below F", I, dict(lags=(0, 4))),
        ("lags that repeat", I, dict(lags=(1, 1))),
        ("lags that decrease", I, dict(lags=(2, 1))),
        ("null lags", I, dict(null_lags=True)),
        ("origin_stride = 0", I, dict(os=0)),
        ("dims = 0", I, dict(dims=0)),
        ("dims = 8", I, dict(dims=8)),
        ("an unknown flag", I, dict(flags=2)),
        ("signed with two components", I, dict(dims=3, flags=1)),
        ("signed with three components", I, dict(dims=7, flags=1)),
        ("lo = hi", I, dict(lo=1.0, hi=1.0)),
        ("lo above hi", I, dict(lo=2.0, hi=1.0)),
        ("lo not finite", I, dict(lo=-inf)),
        ("hi not finite", I, dict(hi=inf)),
        ("hi NaN", I, dict(hi=nan)),
        ("nbins = 0", I, dict(nbins=0)),
        ("a label not below G", I, dict(labels=[0, 1, 2, 1], G=2)),
        ("an index not below natoms", I, dict(idx=[0, 1, 2, 10])),
        ("n above natoms without an index", I, dict(n=11)),
        ("natoms = 0", I, dict(natoms=0)),
        ("a stride below 3 natoms", I, dict(stride=29)),
        ("null trajectory", I, dict(null_traj=True)),
    ]
    for fn, real in ((lib.molar_hip_vanhove, np.float32), (lib.molar_hip_vanhove_f64, np.float64)):
        for what, want, kw in errors:
            got, outs = raw_call(fn, C.addressof(ctx), real, **kw)
            assert got == want, (what, want, got, lib.molar_hip_last_error())
            assert all((v == 77).all() for v in outs.values() if v is not None), (what, "an output was touched")
        got, outs = raw_call(fn, C.addressof(ctx), real, F=0, lags=(0,))
        assert got == 0 and all((v == 77).all() for v in outs.values()), "nframes == 0 is a successful no-op"
        assert raw_call(fn, None, real)[0] == I, "a null context"
        assert raw_call(fn, C.addressof(ctx), real, dims=4, flags=1, F=0)[0] == 0, "signed with one component is accepted"


def test_lags_helper():
    from molar_amd import api
    for F in (1, 2, 3, 10, 11, 100, 1024, 65536, 100001):
        for per in (1, 3, 8, 20):
            lags = api.vanhove_lags(F, per)
            assert lags.dtype == np.uint64 and lags.shape[0] >= 1
            v = lags.astype(np.int64)
            assert (np.diff(v) > 0).all() and v[-1] < F and v[0] == (0 if F == 1 else 1), (F, per)
            if F > 100:
                decade = v[(v >= 100) & (v < 1000)] if F > 1000 else None
                assert decade is None or abs(decade.shape[0] - per) <= 1
    assert list(api.vanhove_lags(40, 4)) == [1, 2, 3, 6, 10, 18, 32]
    assert api.tcf_lags(50, 49, 7)[[0, 44, 49]].tolist() == [8, 1, 1], "the norigins formula is the one of tcf_lags"


def j0_series(x):
    """sum (-1)^k (x^2 / 4)^k / (k!)^2 in 80 decimal digits (the terms reach e^x before they cancel)."""
    decimal.getcontext().prec = 80
    q = decimal.Decimal(x) * decimal.Decimal(x) / 4
    term = total = decimal.Decimal(1)
    for k in range(1, 400):
        term = -term * q / (k * k)
        total += term
    return float(total)


def test_j0_quadrature_against_the_power_series():
    from molar_amd import api
    xs = np.concatenate([np.linspace(0.0, 50.0, 201), [2.404825557695773, 5.520078110286311, 1e-9, 49.99]])
    got = api.bessel_j0(xs)
    want = np.array([j0_series(float(x)) for x in xs])
    # the quadrature adds up to 100 terms of size <= 1 in double: a few 1e-16 each
    assert np.abs(got - want).max() < 1e-14, np.abs(got - want).max()
    assert api.bessel_j0(-3.0) == api.bessel_j0(3.0) and api.bessel_j0(np.zeros((2, 3))).shape == (2, 3)


def gaussian_masses(edges, sigma, ndims):
    """The probability of every bin for the length of an isotropic Gaussian displacement in ndims dimensions (for 1: the signed
    component), from the distribution functions."""
    e = np.asarray(edges, np.float64)
    if ndims == 1:
        cdf = np.array([0.5 * (1.0 + math.erf(x / (sigma * math.sqrt(2.0)))) for x in e])
    elif ndims == 2:
        cdf = 1.0 - np.exp(-e * e / (2.0 * sigma * sigma))
    else:
        cdf = np.array([math.erf(x / (sigma * math.sqrt(2.0))) - math.sqrt(2.0 / math.pi) * x / sigma * math.exp(-x * x / (2.0 * sigma * sigma)) for x in e])
    return cdf[1:] - cdf[:-1]


@pytest.mark.parametrize("ndims", (1, 2, 3))
def test_fs_of_a_gaussian_histogram(ndims):
    from molar_amd import api
    sigma, nbins = 0.3, 240
    lo, hi = (-12 * sigma, 12 * sigma) if ndims == 1 else (0.0, 12 * sigma)
    edges = api.vanhove_edges((lo, hi), nbins)
    dr = (hi - lo) / nbins
    scale = 1e15
    hist = np.round(gaussian_masses(edges, sigma, ndims) * scale).reshape(1, 1, nbins)
    outside = np.zeros((1, 1))
    q = np.array([0.0, 0.5, 1.0, 2.0, 3.5, 5.0, 8.0])
    fs = api.vanhove_fs(hist, outside, edges, q, ndims)[0, 0]
    want = np.exp(-q * q * sigma * sigma / 2.0)
    # the stated binning term, 5/24 (q dr)^2; the masses are rounded to 1e-15 each and the tail beyond 12 sigma is below 1e-30
    tol = 5.0 / 24.0 * (q * dr) ** 2 + nbins * 1e-15 + 1e-14
    err = np.abs(fs - want)
    print("ndims", ndims, "error over tolerance:", (err / tol).round(3))
    assert (err <= tol).all(), (err, tol)
    assert err[1:].max() > 1e-9 or ndims == 0, "the binning term is really there: the tolerance is not an empty one"
    # a truncated distribution has no transform
    assert np.isnan(api.vanhove_fs(hist, np.ones((1, 1)), edges, q, ndims)).all()
    assert np.isnan(api.vanhove_fs(np.zeros_like(hist), outside, edges, 1.0, ndims)).all()


@pytest.mark.parametrize("ndims", (1, 2, 3))
def test_density_integrates_to_the_fraction_inside(ndims):
    from molar_amd import api
    rng = np.random.default_rng(5 + ndims)
    G, L, nbins = 3, 4, 25
    edges = api.vanhove_edges((0.0 if ndims > 1 else -0.7, 1.9), nbins)
    hist = rng.integers(0, 500, (G, L, nbins)).astype(np.uint64)
    norigins = np.array([40, 39, 30, 20], np.uint64)
    # the identity nvalid * norigins = hist + outside gives `outside`
    nvalid = np.array([900, 1000, 1100], np.uint64)
    total = nvalid[:, None] * norigins[None, :]
    outside = total - hist.sum(axis=2)
    assert (outside.astype(np.int64) >= 0).all()
    dens = api.vanhove_density(hist, nvalid, norigins, edges, ndims)
    e = edges
    vol = e[1:] - e[:-1] if ndims == 1 else math.pi * (e[1:] ** 2 - e[:-1] ** 2) if ndims == 2 else 4.0 / 3.0 * math.pi * (e[1:] ** 3 - e[:-1] ** 3)
    integral = (dens * vol).sum(axis=2)
    assert np.allclose(integral, 1.0 - outside / total, rtol=1e-13, atol=0)
    # a uniform density in 3-D comes out flat only with the exact shell volumes
    if ndims == 3:
        e3 = api.vanhove_edges((0.0, 1.0), 10)
        h = ((e3[1:] ** 3 - e3[:-1] ** 3) * 1e6).reshape(1, 1, 10)
        d = api.vanhove_density(h, [1], [1e6], e3, 3)[0, 0]
        assert np.allclose(d, 3.0 / (4.0 * math.pi), rtol=1e-12)
    assert np.isnan(api.vanhove_density(np.zeros((1, 1, nbins)), [0], [5], edges, ndims)).all()


def test_reference_against_plain_loops():
    x = vr.plant(vr.random_walk(3, 7, 5, step=0.2), [(2, 3, 1, float("nan"))]).astype(np.float32)
    for kw in (dict(dims=7), dict(dims=5, origin_stride=2), dict(dims=2, signed=True), dict(dims=7, idx=[4, 0, 2, 3], labels=[1, 0, 1, 2], G=4)):
        lo, hi = (-0.35, 0.45) if kw.get("signed") else (0.1, 0.7)
        a = vr.reference(x, (0, 1, 3, 6), lo, hi, 9, **kw)
        b = vr.brute_force(x, (0, 1, 3, 6), lo, hi, 9, **kw)
        for name in ("hist", "outside", "norigins", "nvalid", "bad"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), (kw, name)
        assert a.hist.sum() > 0 and a.outside.sum() > 0
    assert vr.reference(x, (0,), 0.1, 0.7, 9).bad.tolist() == [0, 0, 0, 1, 0]


def test_reference_refuses_a_displacement_on_an_edge():
    x = np.zeros((3, 1, 3), np.float32)
    x[1, 0, 0] = 0.5
    x[2, 0, 0] = 1.5
    with pytest.raises(AssertionError):
        vr.reference(x, (1,), 0.0, 1.0, 2)                     # |dx| = 0.5 is the edge between the two bins
    assert vr.reference(x, (0,), 0.0, 1.0, 2).hist[0, 0].tolist() == [3, 0], "an exact zero at lo is decided alike on both sides"


@pytest.mark.parametrize("name", sorted(vr.cases()))
def test_every_gpu_case_passes_the_reference_assertions(name):
    c = vr.cases()[name]
    r = vr.case_ref(name)
    assert r.hist.shape == (c.G, len(c.lags), c.nbins)
    print(name, "pairs", int(r.hist.sum() + r.outside.sum()), "outside", int(r.outside.sum()), "clearance over the bound", r.min_clearance)


def test_the_cases_stand_where_they_are_meant_to():
    cs = vr.cases()
    PASS, PW, LT, CELLS = vr.plan_sizes(16)
    r = vr.case_ref("outside_both_sides")
    x = np.asarray(vr.case_traj("outside_both_sides"), np.float64)
    short = np.sqrt(((x[1:] - x[:-1]) ** 2).sum(axis=2))
    far = np.sqrt(((x[150:] - x[:-150]) ** 2).sum(axis=2))
    assert (short < 0.2).any() and (far >= 0.8).any() and r.outside.sum() > 0 and r.hist.sum() > 0
    r = vr.case_ref("stationary")
    assert r.hist[0, :, 0].tolist() == [5 * (PASS + 1), 5 * PASS] and r.hist[0, :, 1:].sum() == 0
    r = vr.case_ref("bad_particles")
    assert r.bad.tolist() == [0, 1, 0, 0, 0, 1, 0, 0, 0] and r.nvalid.tolist() == [3, 2, 2]
    assert vr.case_ref("bad_outside_dims").bad.sum() == 0, "a NaN in a component that dims leaves out harms nobody"
    r = vr.case_ref("groups")
    assert r.nvalid.tolist() == [0, 5, 0, 2 * PW - 1, 1, 0]
    assert vr.case_ref(f"stride_{2 * PASS + 5}").norigins.tolist() == [2, 2, 2, 1]
    assert cs[f"bins_{CELLS}"].nbins == CELLS and len(cs[f"lags_{LT}"].lags) == LT
