"""Internal coordinates on the GPU (molar_hip_intcoord / _f64) against the longdouble reference of tests/intcoord_ref.py.
Every case first asserts, from the reference, that every value is further from every bin edge than the bound derived for
the device's f64 evaluation, that no bond angle has a sine below 0.1 and that the bounds are below 1e-9 rad
(intcoord_ref.margin_ok); then hist, map and valid are compared for EQUALITY and values, mean and spread within the derived
bounds (plus half an f32 ulp for the f32 entry).  Both entries see the same numbers (f32 frames and boxes, cast to f64 for
the f64 entry), so one reference serves both."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import intcoord_ref as ir  # noqa: E402

pytestmark = pytest.mark.gpu

REALS = (np.float32, np.float64)
KINDS = (2, 3, 4)
KNOB = "MOLAR_HIP_INTCOORD_GLOBAL"
ERR_INVALID = 50                 # MOLAR_HIP_ERR_INVALID_ARGUMENT
WORST = {}                       # output -> the worst observed fraction of its bound


@pytest.fixture(scope="module")
def eng():
    from molar_amd import api
    return api.Engine()


@pytest.fixture(scope="module")
def m64(eng):
    from molar_amd import api
    return api.MeasureF64(eng)


def rng_of(kind):
    return (0.7, 1.9) if kind == 2 else None


def plan_of(kind):
    from molar_amd import api
    ws, fc, tc, lc = api.intcoord_plan(10, 10, kind, range=rng_of(kind))
    return fc, tc, lc


def call(eng, m64, real, frames, tuples, **kw):
    entry = eng if real == np.float32 else m64
    kw = dict(kw)
    if kw.get("boxes") is not None:
        kw["boxes"] = np.asarray(kw["boxes"], real)
    return entry.internal_coords(np.asarray(frames, real), tuples, **kw)


def same_bits(a, b):
    for x, y in zip(a[:6], b[:6]):
        if (x is None) != (y is None):
            return False
        if x is not None and not np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)):
            return False
    return True


def within(got, want, bound, real, name, what):
    got = np.asarray(got).astype(np.float64)
    lost = np.isnan(want)
    assert np.array_equal(np.isnan(got), lost), (what, name)
    tol = bound + 2.0 ** -52 * np.abs(want)                    # (the reference rounded to float64 for the comparison)
    if real == np.float32:
        tol = tol + ir.half_ulp32(want)
    err = np.abs(got - want)
    assert (err[~lost] <= tol[~lost]).all(), (what, name, float((err - tol)[~lost].max()))
    if real == np.float64 and (~lost).any():
        frac = float((err[~lost] / tol[~lost]).max())
        WORST[name] = max(WORST.get(name, 0.0), frac)


def compare(got, ref, real, what=""):
    """The integers for equality, the rest within the reference's bounds."""
    ir.margin_ok(ref)
    if got.values is not None:
        within(got.values, ref.values, ref.bound, real, "values", what)
    if got.hist is not None:
        assert np.array_equal(got.hist, ref.hist), what
    if got.map is not None:
        assert np.array_equal(got.map, ref.map), what
    if got.valid is not None:
        assert np.array_equal(got.valid, ref.valid), what
    if got.mean is not None:
        within(got.mean, ref.mean, ref.mean_bound, real, "mean", what)
    if got.spread is not None:
        within(got.spread, ref.spread, ref.spread_bound, real, "spread", what)


def both(eng, m64, frames, tuples, ref, what="", **kw):
    """The case through both entries against the one reference; returns (f32 result, f64 result)."""
    res = []
    for real in REALS:
        got = call(eng, m64, real, frames, tuples, **kw)
        compare(got, ref, real, (what, real.__name__))
        res.append(got)
    return res


def case(seed, F, T, kind, box="none", pbc=7, **kw):
    """make_case and the arguments of the call that go with it"""
    ref_args = dict(kw)
    if kind == 2 and (ref_args.get("nbins") or ref_args.get("map_bins")):
        ref_args.setdefault("range", rng_of(2))
    fr, tu, bx, ref = ir.make_case(seed, F, T, kind, box=box, pbc=pbc, **ref_args)
    args = {k: v for k, v in ref_args.items() if k not in ("natoms", "noise", "windows", "base", "tuples")}
    args["boxes"] = bx
    args["pbc"] = pbc
    return fr, tu, ref, args


# ---------------------------------------------------------------- launch edges

@pytest.mark.parametrize("kind", KINDS)
def test_launch_edges_over_the_tuples(eng, m64, kind):
    fc, tc, lc = plan_of(kind)
    for F in (1, 2):
        for T in (1, 63, 64, 65, 255, 256, 257, tc - 1, tc, tc + 1, 2 * tc + 1):
            fr, tu, ref, args = case(100 * kind + F, F, T, kind, box="ortho" if T in (65, tc + 1) else "none", nbins=24, labels=np.arange(T) % 3, ngroups=3)
            both(eng, m64, fr, tu, ref, (kind, F, T), **args)


@pytest.mark.parametrize("kind", KINDS)
def test_launch_edges_over_the_frames(eng, m64, kind):
    fc, tc, lc = plan_of(kind)
    for T in (1, 65):
        for F in (fc - 1, fc, fc + 1, 2 * fc + 1):
            pairs = None if T == 1 else np.stack([np.arange(T - 1), np.arange(1, T)], 1)
            fr, tu, ref, args = case(200 * kind + T, F, T, kind, box="tric" if F == fc + 1 else "none", nbins=18, pairs=pairs, map_bins=6 if T > 1 else 0)
            both(eng, m64, fr, tu, ref, (kind, F, T), **args)


# ---------------------------------------------------------------- the two histogram routes

def knob_forced(eng, m64, fr, tu, ref, what, **args):
    assert KNOB not in os.environ
    a, b = both(eng, m64, fr, tu, ref, what, **args)
    os.environ[KNOB] = "1"
    try:
        a2, b2 = both(eng, m64, fr, tu, ref, (what, "global"), **args)
    finally:
        del os.environ[KNOB]
    assert same_bits(a, a2) and same_bits(b, b2), what


@pytest.mark.parametrize("kind", KINDS)
def test_histogram_route_edge(eng, m64, kind):
    fc, tc, lc = plan_of(kind)
    T, F = 300, 3
    for cells in (lc - 1, lc, lc + 1):
        G = next(g for g in (2, 3, 1) if cells % g == 0)
        nbins = cells // G
        assert G * nbins == cells
        fr, tu, ref, args = case(300 + kind, F, T, kind, nbins=nbins, labels=np.arange(T) % G, ngroups=G)
        assert int(ref.hist.sum()) > 0
        knob_forced(eng, m64, fr, tu, ref, (kind, "hist", cells), **args)


@pytest.mark.parametrize("kind", KINDS)
def test_map_route_edge(eng, m64, kind):
    fc, tc, lc = plan_of(kind)
    T, F = 300, 3
    rng = np.random.default_rng(5)
    pairs = rng.integers(0, T, size=(400, 2))
    for cells in (lc - 1, lc, lc + 1):
        mb = next(m for m in (64, 3, 1) if cells % (m * m) == 0)
        G2 = cells // (mb * mb)
        assert G2 * mb * mb == cells
        plabels = rng.integers(0, G2, size=400)
        plabels[0] = G2 - 1
        fr, tu, ref, args = case(400 + kind, F, T, kind, map_bins=mb, pairs=pairs, pair_labels=plabels, npair_groups=G2)
        assert int(ref.map.sum()) > 0
        knob_forced(eng, m64, fr, tu, ref, (kind, "map", cells), **args)


# ---------------------------------------------------------------- boxes

@pytest.mark.parametrize("kind", KINDS)
def test_boxes(eng, m64, kind):
    T, F = 130, 5
    pairs = np.stack([np.arange(T - 1), np.arange(1, T)], 1)
    for box, pbc in (("none", 7), ("ortho", 7), ("tric", 7), ("ortho", 1), ("ortho", 2), ("ortho", 4), ("ortho", 3), ("ortho", 5), ("ortho", 6), ("ortho", 0)):
        fr, tu, ref, args = case(500 + kind, F, T, kind, box=box, pbc=pbc, nbins=30, pairs=pairs, map_bins=5)
        both(eng, m64, fr, tu, ref, (kind, box, pbc), **args)
        if box != "none" and pbc == 7:
            # the atoms were wrapped one by one: without the box the same frames give other values
            raw = ir.reference(fr, tu, kind)
            assert np.nanmax(np.abs(raw.values - ref.values)) > 0.1


CORNER = np.array([[0.94, 0.94, 0.95], [1.06, 0.98, 0.98], [0.97, 1.05, 1.04], [0.91, 0.95, 0.96]])     # fractional, unwrapped, about the far corner


@pytest.mark.parametrize("tric", (False, True))
def test_bonds_that_cross_one_two_and_three_faces(eng, m64, tric):
    box = ir.tric_box((9.0, 10.0, 11.0)) if tric else ir.ortho_box((9.0, 10.0, 11.0))
    m = box.reshape(3, 3).astype(np.float64).T
    cell = np.floor(CORNER).astype(int)
    crossed = [int((cell[i + 1] != cell[i]).sum()) for i in range(3)]
    assert crossed == [1, 3, 2]
    corner = (m @ CORNER.T).T
    wrapped = ir.wrap_into(corner, box).astype(np.float32)[None]
    assert (np.floor(np.linalg.solve(m, wrapped[0].astype(np.float64).T).T + 1e-6) == 0).all()
    plain = corner.astype(np.float32)[None]
    for tu in ([[0, 1], [1, 2], [2, 3], [3, 0]], [[0, 1, 2], [1, 2, 3], [3, 2, 1]], [[0, 1, 2, 3], [3, 2, 1, 0]]):
        tu = np.asarray(tu, np.uint64)
        kind = tu.shape[1]
        rng = (0.3, 2.9) if kind == 2 else None
        ref = ir.reference(wrapped, tu, kind, boxes=box, nbins=7, range=rng)
        a, b = both(eng, m64, wrapped, tu, ref, (tric, kind), boxes=box, nbins=7, range=rng)
        # ... the values of the molecule that was never cut (f32 rounding of the wrapped coordinates apart)
        whole = ir.reference(plain, tu, kind)
        assert np.abs(whole.values - b.values).max() < 1e-5


# ---------------------------------------------------------------- groups

@pytest.mark.parametrize("kind", KINDS)
def test_groups_with_an_empty_group_and_pairs_that_repeat(eng, m64, kind):
    T, F = 70, 4
    labels = np.arange(T) % 4
    labels[labels == 2] = 3                                     # group 2 is empty
    pairs = np.array([[0, 1], [5, 5], [5, 5], [69, 0], [7, 3], [1, 0]])
    plabels = np.array([0, 2, 2, 4, 0, 4])                        # groups 1 and 3 are empty, and so is 5
    fr, tu, ref, args = case(600 + kind, F, T, kind, box="ortho", nbins=12, labels=labels, ngroups=5, pairs=pairs, map_bins=4, pair_labels=plabels,
                             npair_groups=6)
    a, b = both(eng, m64, fr, tu, ref, kind, **args)
    assert int(b.hist[2].sum()) == 0 and int(b.hist[4].sum()) == 0 and int(b.hist.sum()) > 0
    assert int(b.map[1].sum()) == 0 and int(b.map[3].sum()) == 0 and int(b.map[5].sum()) == 0
    assert int(np.trace(b.map[2])) == int(b.map[2].sum()) and int(b.map[2].sum()) > 0       # the same tuple twice: the diagonal


# ---------------------------------------------------------------- invalid values

@pytest.mark.parametrize("kind", KINDS)
def test_a_coordinate_that_is_not_finite(eng, m64, kind):
    T, F = 40, 5
    pairs = np.stack([np.arange(T - 1), np.arange(1, T)], 1)
    fr, tu, ref0, args = case(700 + kind, F, T, kind, box="ortho", nbins=9, pairs=pairs, map_bins=3, windows="all")
    for bad in (np.nan, np.inf):
        fr2 = fr.copy()
        fr2[2, 11, 1] = bad
        ref = ir.reference(fr2, tu, kind, **args)
        hit = (tu == 11).any(1)
        assert hit.any() and not hit.all()
        assert np.isnan(ref.values[2, hit]).all() and (ref.valid[hit] == F - 1).all() and (ref.valid[~hit] == F).all()
        a, b = both(eng, m64, fr2, tu, ref, (kind, bad), **args)
        # everything else is what it was
        keep = np.ones((F, T), bool)
        keep[2, hit] = False
        base = call(eng, m64, np.float64, fr, tu, **args)
        assert np.array_equal(b.values[keep], base.values[keep]) and np.array_equal(b.mean[~hit], base.mean[~hit])


def test_degenerate_tuples_placed_exactly(eng, m64):
    # small integers: every difference and every product is exact in f64 and in longdouble, so both decide alike.  No box: a
    # reduction in fractional coordinates would not leave collinear bonds collinear to the last bit.
    x = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [1, 1, 0], [2, 0, 0], [3, 0, 0], [3, 1, 1], [4, 2, 1]], np.float32)
    good = x.copy()
    good[1] = (0, 1, 1)
    good[4] = (2, 1, 0)
    good[5] = (3, 0, 1)
    fr = np.stack([good, x, good + 1, x * 2])                    # frames 1 and 3 are degenerate
    ta = np.array([[0, 1, 2], [2, 1, 0], [1, 2, 3], [2, 3, 6]], np.uint64)      # A == B in the first two
    ra = ir.reference(fr, ta, 3, nbins=5)
    assert np.isnan(ra.values[[1, 3]][:, :2]).all() and np.isfinite(ra.values[[0, 2]]).all() and list(ra.valid) == [2, 2, 4, 4]
    both(eng, m64, fr, ta, ra, "angle", nbins=5)
    td = np.array([[1, 2, 4, 6], [6, 5, 4, 2], [3, 2, 4, 5], [0, 1, 2, 3], [2, 3, 6, 7]], np.uint64)     # 2, 4, 5 collinear; 0 == 1
    rd = ir.reference(fr, td, 4, nbins=5, pairs=[[0, 4], [4, 4]], map_bins=2)
    assert np.isnan(rd.values[[1, 3]][:, :4]).all() and np.isfinite(rd.values[:, 4]).all() and list(rd.valid[:4]) == [2, 2, 2, 2]
    both(eng, m64, fr, td, rd, "dihedral", nbins=5, pairs=np.array([[0, 4], [4, 4]]), map_bins=2)
    # a distance of zero is a value
    r2 = ir.reference(fr, np.array([[0, 1], [2, 3]], np.uint64), 2, nbins=4, range=(0.0, 4.0))
    assert r2.values[1, 0] == 0 and list(r2.valid) == [4, 4]
    # (0 is the lower end of the range: the reference's margin does not hold there, the count must)
    got = m64.internal_coords(fr.astype(np.float64), np.array([[0, 1], [2, 3]], np.uint64), nbins=4, range=(0.0, 4.0))
    assert got.values[1, 0] == 0 and np.array_equal(got.hist, r2.hist) and np.array_equal(got.valid, r2.valid)


def test_a_tuple_invalid_in_every_frame(eng, m64):
    fr, tu, ref0, args = case(800, 3, 20, 4, nbins=6, windows="all")
    fr[:, 7, 0] = np.nan
    ref = ir.reference(fr, tu, 4, **args)
    hit = (tu == 7).any(1)
    assert (ref.valid[hit] == 0).all() and np.isnan(ref.mean[hit]).all() and np.isnan(ref.spread[hit]).all()
    a, b = both(eng, m64, fr, tu, ref, "all frames", **args)
    assert np.isnan(a.mean[hit]).all() and np.isnan(b.spread[hit]).all() and np.isfinite(b.mean[~hit]).all()


# ---------------------------------------------------------------- errors

PATTERN = 7


def outputs(real, F, T, G, nbins, G2, mb, torch_device=None):
    out = [np.full((F, T), PATTERN, real), np.full((G, nbins), PATTERN, np.uint64), np.full((G2, mb, mb), PATTERN, np.uint64), np.full(T, PATTERN, real),
           np.full(T, PATTERN, real), np.full(T, PATTERN, np.uint64)]
    if torch_device is not None:
        import torch
        out = [torch.from_numpy(o.astype(np.int64) if o.dtype == np.uint64 else o).to(torch_device) for o in out]
    return out


def untouched(out):
    return all(bool((np.asarray(o.cpu() if hasattr(o, "cpu") else o) == PATTERN).all()) for o in out)


@pytest.mark.parametrize("where", ("host", "device"))
def test_errors_leave_the_outputs_alone(eng, m64, where):
    import torch
    from molar_amd import _lib
    F, T, natoms, G, nbins, G2, mb = 3, 10, 12, 2, 4, 2, 3
    fr, tu, ref, _ = case(900, F, T, 4, natoms=natoms)
    labels = np.arange(T) % G
    pairs = np.stack([np.arange(T - 1), np.arange(1, T)], 1)
    plabels = np.arange(T - 1) % G2
    dev = torch.device("cuda") if where == "device" else None

    def put(a, dt):
        a = np.asarray(a)
        if dev is None:
            return a
        return torch.from_numpy(a.astype(dt)).to(dev)

    for real, entry in ((np.float32, eng), (np.float64, m64)):
        for what in ("index", "label", "pair", "pair label"):
            t2, l2, p2, pl2 = tu.astype(np.int64), labels.copy(), pairs.copy(), plabels.copy()
            if what == "index":
                t2[T - 1, 2] = natoms
            elif what == "label":
                l2[T - 1] = G
            elif what == "pair":
                p2[T - 2, 1] = T
            else:
                pl2[T - 2] = G2
            out = outputs(real, F, T, G, nbins, G2, mb, dev)
            frames = put(fr.astype(real), real)
            with pytest.raises(_lib.MolarHipError) as e:
                entry.internal_coords(frames, put(t2, np.int64), labels=put(l2, np.int32), ngroups=G, nbins=nbins, pairs=put(p2, np.int64),
                                      pair_labels=put(pl2, np.int32), npair_groups=G2, map_bins=mb, out=out)
            assert e.value.code == ERR_INVALID, (what, str(e.value))
            assert untouched(out), what
        # the good call on the same outputs
        out = outputs(real, F, T, G, nbins, G2, mb, dev)
        got = entry.internal_coords(put(fr.astype(real), real), put(tu.astype(np.int64), np.int64), labels=put(labels, np.int32), ngroups=G, nbins=nbins,
                                    pairs=put(pairs, np.int64), pair_labels=put(plabels, np.int32), npair_groups=G2, map_bins=mb, out=out)
        eng.synchronize()
        assert not untouched(out[:1]) and got.values is out[0]


def test_stride_and_ld_errors(eng, m64):
    import ctypes as C
    from molar_amd import _lib
    lib = eng.lib
    fr, tu, ref, _ = case(901, 3, 6, 3, natoms=9)
    sp = _lib.IntcoordSpec()
    sp.kind = 3
    for fn, real in ((lib.molar_hip_intcoord, np.float32), (lib.molar_hip_intcoord_f64, np.float64)):
        x = np.ascontiguousarray(fr, real)
        vals = np.full((3, 6), PATTERN, real)
        rc = fn(eng.ctx, x.ctypes.data, 3, 26, 9, tu.ctypes.data, 6, None, 1, None, 0, 0, C.addressof(sp), None, 0, None, 1, vals.ctypes.data, 6, None, None,
                None, None, None)
        assert rc == ERR_INVALID and "stride" in _lib.last_error()
        rc = fn(eng.ctx, x.ctypes.data, 3, 27, 9, tu.ctypes.data, 6, None, 1, None, 0, 0, C.addressof(sp), None, 0, None, 1, vals.ctypes.data, 5, None, None,
                None, None, None)
        assert rc == ERR_INVALID and "ld" in _lib.last_error()
        assert (vals == PATTERN).all()


# ---------------------------------------------------------------- plumbing

@pytest.mark.parametrize("kind", KINDS)
def test_frame_stride_and_ld_above_the_minimum(eng, m64, kind):
    F, T = 5, 33
    fr, tu, ref, args = case(1000 + kind, F, T, kind, box="ortho", nbins=8)
    for real in REALS:
        wide = np.full((F, fr.shape[1] + 3, 3), np.nan, real)
        wide[:, :fr.shape[1]] = fr
        view = wide[:, :fr.shape[1]]                              # a frame stride of 3 (natoms + 3)
        vals = np.full((F, T + 5), PATTERN, real)
        entry = eng if real == np.float32 else m64
        a = dict(args)
        a["boxes"] = np.asarray(a["boxes"], real)
        got = entry.internal_coords(view, tu, out=(vals[:, :T], None, None, None, None, None), **a)
        assert np.shares_memory(got.values, vals)
        compare(got, ref, real, (kind, "wide"))
        assert (vals[:, T:] == PATTERN).all()
        plain = call(eng, m64, real, fr, tu, **args)
        assert same_bits(got, plain)


@pytest.mark.parametrize("kind", KINDS)
def test_every_output_alone(eng, m64, kind):
    F, T = 4, 50
    pairs = np.stack([np.arange(T - 1), np.arange(1, T)], 1)
    fr, tu, ref, args = case(1100 + kind, F, T, kind, box="tric", nbins=8, pairs=pairs, map_bins=3)
    full = both(eng, m64, fr, tu, ref, kind, **args)
    names = ("values", "hist", "map", "mean", "spread", "valid")
    for k, name in enumerate(names):
        for real, whole in zip(REALS, full):
            got = call(eng, m64, real, fr, tu, want=(name,), **args)
            assert [g is not None for g in got[:6]] == [j == k for j in range(6)], name
            assert np.array_equal(np.asarray(got[k]).view(np.uint8), np.asarray(whole[k]).view(np.uint8)), name


@pytest.mark.parametrize("kind", KINDS)
def test_torch_in_and_out(eng, m64, kind):
    import torch
    F, T = 6, 70
    pairs = np.stack([np.arange(T - 1), np.arange(1, T)], 1)
    labels = np.arange(T) % 3
    fr, tu, ref, args = case(1200 + kind, F, T, kind, box="tric", nbins=8, pairs=pairs, map_bins=3, labels=labels, ngroups=3)
    dev = torch.device("cuda")
    for real, entry in ((np.float32, eng), (np.float64, m64)):
        host = call(eng, m64, real, fr, tu, **args)
        a = dict(args)
        a["boxes"] = torch.from_numpy(np.asarray(args["boxes"], real)).to(dev)
        a["pairs"] = torch.from_numpy(pairs.astype(np.int64)).to(dev)
        a["labels"] = torch.from_numpy(labels.astype(np.int32)).to(dev)
        x = torch.from_numpy(fr.astype(real)).to(dev)
        t = torch.from_numpy(tu.astype(np.int64)).to(dev)
        got = entry.internal_coords(x, t, **a)
        assert all(g.is_cuda for g in got[:6]) and got.hist.dtype == torch.int64 and got.values.dtype == x.dtype
        eng.synchronize()
        back = [g.cpu().numpy() for g in got[:6]]
        back = [b.view(np.uint64) if b.dtype == np.int64 else b for b in back]
        assert same_bits(back, host)
        # out=: the same destinations written again, a row stride above T for the values
        wide = torch.full((F, T + 3), float(PATTERN), dtype=x.dtype, device=dev)
        out = (wide[:, :T], torch.zeros_like(got.hist), torch.zeros_like(got.map), torch.zeros_like(got.mean), torch.zeros_like(got.spread),
               torch.zeros_like(got.valid))
        again = entry.internal_coords(x, t, out=out, **a)
        eng.synchronize()
        assert again.values is out[0] and bool((wide[:, T:] == PATTERN).all())
        back2 = [g.cpu().numpy() for g in again[:6]]
        back2 = [b.view(np.uint64) if b.dtype == np.int64 else b for b in back2]
        assert same_bits(back2, host)


@pytest.mark.parametrize("kind", KINDS)
def test_same_bits_twice_and_a_smaller_call_after_a_larger_one(eng, m64, kind):
    fc, tc, lc = plan_of(kind)
    big = case(1300 + kind, fc + 3, tc + 9, kind, box="ortho", nbins=16, pairs=np.array([[0, 1], [3, 2]]), map_bins=4)
    small = case(1400 + kind, 3, 17, kind, box="ortho", nbins=5, pairs=np.array([[0, 1], [3, 2]]), map_bins=2)
    fr, tu, ref, args = small
    first = both(eng, m64, fr, tu, ref, (kind, "small"), **args)
    bfr, btu, bref, bargs = big
    b1 = both(eng, m64, bfr, btu, bref, (kind, "big"), **bargs)
    b2 = both(eng, m64, bfr, btu, bref, (kind, "big again"), **bargs)
    assert same_bits(b1[0], b2[0]) and same_bits(b1[1], b2[1])
    after = both(eng, m64, fr, tu, ref, (kind, "small after big"), **args)
    assert same_bits(first[0], after[0]) and same_bits(first[1], after[1])


# ---------------------------------------------------------------- end to end

def test_ramachandran_map_of_a_chain(eng, m64):
    from molar_amd import api
    nres, F = 24, 16
    rng = np.random.default_rng(11)
    back = ir.make_chain(rng, 3 * nres)                          # N, CA, C of every residue along one chain
    per = ["N", "CA", "C", "O", "CB"]
    base = np.zeros((5 * nres, 3))
    for r in range(nres):
        base[5 * r:5 * r + 3] = back[3 * r:3 * r + 3]
        base[5 * r + 3] = back[3 * r + 2] + rng.normal(size=3) * 0.7      # O on C
        base[5 * r + 4] = back[3 * r + 1] + rng.normal(size=3) * 0.9      # CB on CA
    names = per * nres
    resids = np.repeat(np.arange(1, nres + 1), 5)
    phi, psi, omega, rphi, rpsi, rom, pairs = api.backbone_dihedrals(names, resids)
    assert phi.shape == (nres - 1, 4) and psi.shape == (nres - 1, 4) and omega.shape == (nres - 1, 4) and pairs.shape == (nres - 2, 2)
    assert (rphi[pairs[:, 0].astype(int)] == rpsi[(pairs[:, 1] - len(phi)).astype(int)]).all()
    tuples = np.concatenate([phi, psi, omega])
    labels = np.repeat([0, 1, 2], [len(phi), len(psi), len(omega)])
    fr, tu, bx, ref = ir.make_case(12, F, len(tuples), 4, box="tric", base=base, tuples=tuples, nbins=36, labels=labels, ngroups=3, pairs=pairs, map_bins=36)
    a, b = both(eng, m64, fr, tu, ref, "rama", boxes=bx, nbins=36, labels=labels, ngroups=3, pairs=pairs, map_bins=36)
    assert int(b.map.sum()) == F * (nres - 2) and b.map.shape == (1, 36, 36)
    assert np.array_equal(b.hist.sum(1), np.full(3, F * (nres - 1), np.uint64))
    assert b.edges.shape == (37,)
    # the map is the joint histogram of the series
    bins = np.floor((b.values + np.pi) / (2 * np.pi) * 36).astype(int) % 36
    joint = np.zeros((36, 36), np.uint64)
    np.add.at(joint, (bins[:, pairs[:, 0].astype(int)], bins[:, pairs[:, 1].astype(int)]), 1)
    assert np.array_equal(joint, b.map[0])


def test_worst_fractions_of_the_bounds_are_reported():
    """Not a check beyond <= 1 (which every comparison above made): the figures of DESIGN 8l."""
    for k in sorted(WORST, key=str):
        print("worst fraction of the bound:", k, "%.3g" % WORST[k])
    assert all(v <= 1.0 for v in WORST.values())
