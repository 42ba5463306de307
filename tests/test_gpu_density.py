"""Density profiles and maps on the GPU (molar_hip_density / _f64) against the numpy reference of tests/density_ref.py.  Every
case first asserts, from the reference, that no atom is within 1e-3 bin widths of an edge and that the derived rounding bound
on the bin coordinate is below that margin (density_ref.margin_ok); then count, outside and the weights' scale are compared
for EQUALITY and density, centre and binvol within the bounds derived there.  Both entries see the same numbers (f32 frames,
weights and boxes, cast to f64 for the f64 entry), so one reference serves both."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import density_ref as dr  # noqa: E402
from density_ref import BOX, LAB  # noqa: E402

pytestmark = pytest.mark.gpu

REALS = (np.float32, np.float64)
KNOB = "MOLAR_HIP_DENSITY_GLOBAL"


@pytest.fixture(scope="module")
def eng():
    from molar_amd import api
    return api.Engine()


@pytest.fixture(scope="module")
def m64(eng):
    from molar_amd import api
    return api.MeasureF64(eng)


def f32(x):
    return None if x is None else np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


ORTHO, TRIC = f32(dr.ORTHO), f32(dr.TRICLINIC)


def plan(grd, F=1, n=1, G=1):
    from molar_amd import api
    return api.density_plan(F, n, grd, G)


def call(eng, m64, real, frames, grd, **kw):
    entry = eng if real == np.float32 else m64
    kw = dict(kw)
    for k in ("weight", "boxes", "centre_weight"):
        if kw.get(k) is not None:
            kw[k] = np.asarray(kw[k], real)
    return entry.density(np.asarray(frames, real), grd, **kw)


def same_bits(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(a[:5], b[:5])) and a[5] == b[5]


def compare(got, ref, real, what=""):
    """The integers for equality, the rest within the reference's bounds; returns the reference's margin."""
    m = dr.margin_ok(ref)
    G, nb = ref["G"], ref["nb"]
    assert got.weight_scale_log2 == ref["S"], what
    assert np.array_equal(got.count.reshape(G, nb), ref["count"]), what
    assert np.array_equal(got.outside, ref["outside"]), what
    d64 = ref["density"].astype(np.float64)
    tol = ref["dens_bound"] + 2.0 ** -52 * np.abs(d64)                    # (the reference rounded to float64 for the comparison)
    if real == np.float32:
        tol = tol + dr.half_ulp32(d64)
    err = np.abs(got.density.reshape(G, nb).astype(np.float64) - d64)
    assert (err <= tol).all(), (what, float((err - tol).max()))
    assert (got.density.reshape(G, nb)[ref["count"] == 0] == 0).all(), what
    c64 = ref["centre"].astype(np.float64)
    ctol = ref["centre_bound"] + (dr.half_ulp32(c64) if real == np.float32 else 2.0 ** -52 * np.abs(c64))
    lost = np.isnan(c64)                                                  # a centre that is not finite is not finite in both
    assert np.array_equal(np.isnan(got.centre), lost), what
    assert (np.abs(got.centre.astype(np.float64) - c64) <= ctol)[~lost].all(), what
    b64 = ref["binvol"].astype(np.float64)
    btol = (ref["binvol_rel"] + 2.0 ** -51) * b64 + (dr.half_ulp32(b64) if real == np.float32 else 0.0)
    assert (np.abs(got.binvol.astype(np.float64) - b64) <= btol).all(), what
    return m


def both(eng, m64, frames, grd, what="", **kw):
    """The case through both entries against one reference; returns (reference, f32 result, f64 result)."""
    frames = np.asarray(frames, np.float32)
    for k in ("weight", "boxes", "centre_weight"):
        kw[k] = f32(kw.get(k))
    ref = dr.density(frames, grd, **kw)
    res = []
    for real in REALS:
        got = call(eng, m64, real, frames, grd, **kw)
        compare(got, ref, real, (what, real.__name__))
        res.append(got)
    return ref, res[0], res[1]


# ---------------------------------------------------------------- launch edges

def atom_counts():
    ac = plan(dr.grid(BOX, (1, 1, 20)))[2]
    return [1, 63, 64, 65, 255, 256, 257, ac - 1, ac, ac + 1, 2 * ac + 1]


@pytest.mark.parametrize("k", range(11))
def test_atoms_per_workgroup_edges(eng, m64, k):
    n = atom_counts()[k]
    grd = dr.grid(BOX, (1, 1, 20))
    rng = np.random.default_rng(n)
    w = rng.uniform(-3, 3, n)
    labels = rng.integers(0, 2, n)
    for F in (1, 2):
        fr = dr.scatter_box(100 + n + F, F, n, grd.nbins, ORTHO)
        ref, a, b = both(eng, m64, fr, grd, (n, F), weight=w, labels=labels, ngroups=2, boxes=ORTHO)
        assert int(ref["count"].sum()) == F * n


@pytest.mark.parametrize("n", [1, 65, 257])
def test_frames_per_chunk_edges(eng, m64, n):
    grd = dr.grid(BOX, (1, 1, 20))
    fc = plan(grd, 100, n, 2)[1]
    assert fc > 2
    rng = np.random.default_rng(n)
    w = rng.uniform(0.5, 3, n)
    labels = rng.integers(0, 2, n)
    for F in (fc - 1, fc, fc + 1):
        boxes = dr.mr.scaled_boxes(F, F, ORTHO).astype(np.float32)
        fr = dr.scatter_box(200 + n + F, F, n, grd.nbins, f32(boxes))
        both(eng, m64, fr, grd, (n, F), weight=w, labels=labels, ngroups=2, boxes=boxes)


# ---------------------------------------------------------------- grids

@pytest.mark.parametrize("nb", [1, 2, 63, 64, 65])
def test_bin_counts_along_one_axis(eng, m64, nb):
    for axis in (2, 0):
        nbins = [1, 1, 1]
        nbins[axis] = nb
        grd = dr.grid(BOX, nbins)
        fr = dr.scatter_box(300 + nb + axis, 2, 300, nbins, TRIC)
        ref, a, b = both(eng, m64, fr, grd, (nb, axis), boxes=TRIC)
        assert (ref["outside"] == 0).all() and int(ref["count"].sum()) == 600


SHAPES = [(1, 1, 7), (1, 7, 1), (7, 1, 1), (5, 6, 1), (5, 1, 6), (1, 5, 6), (3, 4, 5)]


@pytest.mark.parametrize("nbins", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_grid_shapes_box_and_lab(eng, m64, nbins):
    n, F = 400, 2
    w = np.random.default_rng(1).uniform(1, 16, n)
    fr = dr.scatter_box(400 + sum(nbins), F, n, nbins, TRIC, pbc=5)
    ref, _, _ = both(eng, m64, fr, dr.grid(BOX, nbins), ("box", nbins), weight=w, boxes=TRIC, pbc=5)
    assert 0 < int(ref["outside"].sum()) < n * F
    lo, hi = (-1.0, 0.5, 2.0), (2.0, 3.0, 2.75)
    fr = dr.scatter_lab(500 + sum(nbins), F, n, nbins, lo, hi)
    ref, _, _ = both(eng, m64, fr, dr.grid(LAB, nbins, lo, hi), ("lab", nbins), weight=w)
    assert 0 < int(ref["outside"].sum()) < n * F
    # the bin index is (bx ny + by) nz + bz: a lone atom in the last bin of x and the first of the others
    one = np.array([[[lo[0] + (nbins[0] - 0.5) * (hi[0] - lo[0]) / nbins[0], lo[1] + 0.25 * (hi[1] - lo[1]) / nbins[1], lo[2] + 0.25 * (hi[2] - lo[2]) / nbins[2]]]])
    got = eng.density(one.astype(np.float32), dr.grid(LAB, nbins, lo, hi))
    assert got.count.reshape(-1)[(nbins[0] - 1) * nbins[1] * nbins[2]] == 1 and got.count.sum() == 1


@pytest.mark.parametrize("G", [1, 2, 5])
def test_groups_with_an_empty_one(eng, m64, G):
    n, F, nbins = 500, 3, (1, 1, 30)
    rng = np.random.default_rng(G)
    labels = rng.integers(0, max(G - 1, 1), n)                      # the last group stays empty (G > 1)
    w = rng.uniform(-1, 1, n)
    fr = dr.scatter_box(600 + G, F, n, nbins, ORTHO)
    ref, a, _ = both(eng, m64, fr, dr.grid(BOX, nbins), G, weight=w, labels=labels, ngroups=G, boxes=ORTHO)
    if G > 1:
        assert (ref["count"][G - 1] == 0).all() and (a.density[G - 1] == 0).all() and (ref["count"][0] > 0).any()


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_kernel_switch(eng, m64, delta):
    """G nb = lds_cells - 1, lds_cells, lds_cells + 1: the last one is beyond the on-chip kernel; the first two also through the
    global kernel (the knob the library reads per call), which must give the same integers and the same density bits."""
    lc = plan(dr.grid(BOX, (1, 1, 20)))[3]
    cells = lc + delta
    G = 3 if cells % 3 == 0 else 1
    nbins = (1, 1, cells // G)
    assert G * nbins[2] == cells
    n, F = 3000, 3
    rng = np.random.default_rng(cells)
    w, labels = rng.uniform(-5, 5, n), rng.integers(0, G, n)
    fr = dr.scatter_box(700 + delta, F, n, nbins, ORTHO)
    assert KNOB not in os.environ
    ref, a, b = both(eng, m64, fr, dr.grid(BOX, nbins), cells, weight=w, labels=labels, ngroups=G, boxes=ORTHO)
    os.environ[KNOB] = "1"
    try:
        ref2, a2, b2 = both(eng, m64, fr, dr.grid(BOX, nbins), (cells, "global"), weight=w, labels=labels, ngroups=G, boxes=ORTHO)
    finally:
        del os.environ[KNOB]
    assert same_bits(a, a2) and same_bits(b, b2)


# ---------------------------------------------------------------- contention and exactness

def test_all_atoms_in_one_bin(eng, m64):
    n, F, nbins = 4096, 2, (1, 1, 100)
    rng = np.random.default_rng(8)
    u = np.zeros((F, n, 3))
    u[:, :, :2] = rng.uniform(0.1, 0.9, size=(F, n, 2))
    u[:, :, 2] = (37 + 0.5 + rng.uniform(-0.4, 0.4, size=(F, n))) / 100
    fr = u @ dr.box_of(ORTHO, 0).T
    w = rng.uniform(1, 250, n)
    ref, a, _ = both(eng, m64, fr, dr.grid(BOX, nbins), weight=w, boxes=ORTHO)
    assert ref["count"][0, 37] == F * n and int(ref["count"].sum()) == F * n and np.count_nonzero(a.density) == 1


def test_paired_charges_cancel_exactly(eng, m64):
    n, F, nbins = 600, 3, (4, 1, 25)
    fr = dr.scatter_box(9, F, n // 2, nbins, TRIC)
    fr = np.concatenate([fr, fr], axis=1)                           # atom k + n / 2 sits on atom k
    q = np.random.default_rng(9).uniform(0.1, 2, n // 2)
    w = np.concatenate([q, -q])
    ref, a, b = both(eng, m64, fr, dr.grid(BOX, nbins), weight=w, boxes=TRIC)
    assert (ref["I"] == 0).all() and int(ref["count"].sum()) == F * n
    for got in (a, b):
        assert (got.density == 0).all() and not np.signbit(got.density).any()


def test_lab_power_of_two_volume_is_exact(eng, m64):
    n, nbins, lo, hi = 500, (4, 2, 8), (0.0, 0.0, 0.0), (2.0, 4.0, 1.0)          # bin volume 1/2 * 2 * 1/8 = 1/8
    fr = dr.scatter_lab(10, 1, n, nbins, lo, hi, out_frac=0.3)
    w = np.random.default_rng(10).integers(-40, 41, n) / 8.0                      # multiples of 1/8: exact under any S
    ref, a, b = both(eng, m64, fr, dr.grid(LAB, nbins, lo, hi), weight=w)
    assert ref["exact"] and ref["u_bound"] == 0.0
    exact = ref["I"][0].astype(np.float64) * 2.0 ** -ref["S"] * 8.0               # Python-side integers, exact in float64
    assert np.array_equal(b.density.reshape(1, -1), exact) and np.array_equal(a.density.reshape(1, -1).astype(np.float64), exact)


def test_half_open_edges(eng, m64):
    """LAB, lo = 0, bin widths 1/2, 1/4 and 1: atoms exactly on lo, on every interior edge and on hi, and one ulp on either side
    of each (2^-100 either side of 0).  Every operation is exact here (density_ref: the bound is 0), so the margin assertion does not apply and the
    integers are compared as they are: an atom on an interior edge belongs to the upper bin, one on hi is outside."""
    nbins, lo, hi = (8, 4, 1), (0.0, 0.0, 0.0), (4.0, 1.0, 1.0)
    grd = dr.grid(LAB, nbins, lo, hi)
    for real in REALS:
        rows, want_bin = [], []
        for d, (k, width) in enumerate(((8, 0.5), (4, 0.25))):
            for e in range(k + 1):
                edge = real(e * width)
                # (about 0 the step is 2^-100, not the subnormal neighbour: scaled by 1 / (hi - lo) that one underflows to -0.0)
                below, above = (real(-2.0 ** -100), real(2.0 ** -100)) if e == 0 else (np.nextafter(edge, real(-1)), np.nextafter(edge, real(9)))
                for v, bin_ in ((edge, e), (below, e - 1), (above, e)):
                    p = [0.25, 0.125, 0.5]
                    p[d] = v
                    rows.append(p)
                    want_bin.append((d, bin_ if 0 <= bin_ < k and 0 <= v < hi[d] else None))
        fr = np.array(rows, real)[None]
        ref = dr.density(fr, grd)
        assert ref["exact"] and ref["u_bound"] == 0.0 and ref["margin_bin"] == 0.0
        want = np.zeros(nbins, np.uint64)
        for d, b in want_bin:
            if b is not None:
                want[(b, 0, 0) if d == 0 else (0, b, 0)] += 1
        assert np.array_equal(ref["count"].reshape(nbins), want)
        got = call(eng, m64, real, fr, grd)
        assert np.array_equal(got.count.reshape(nbins), want) and got.outside[0] == sum(b is None for _, b in want_bin) == ref["outside"][0]


# ---------------------------------------------------------------- periodicity

@pytest.mark.parametrize("pbc", [7, 3, 4, 0])
@pytest.mark.parametrize("box", ["ortho", "tric"])
def test_periodic_images_and_open_dimensions(eng, m64, box, pbc):
    n, F, nbins = 500, 2, (3, 4, 11)
    box9 = ORTHO if box == "ortho" else TRIC
    fr = dr.scatter_box(800 + pbc, F, n, nbins, box9, pbc=pbc, images=3)
    w = np.random.default_rng(pbc).uniform(1, 30, n)
    ref, _, _ = both(eng, m64, fr, dr.grid(BOX, nbins), (box, pbc), weight=w, boxes=box9, pbc=pbc)
    assert (ref["outside"] == 0).all() if pbc == 7 else (ref["outside"] > 0).all()
    assert np.abs(fr).max() > 9.0 or pbc == 0                       # atoms really are box lengths away


# ---------------------------------------------------------------- centring

def test_split_slab_centred_on_itself(eng, m64):
    F, npairs, nz = 4, 150, 40
    grd = dr.grid(BOX, (1, 1, nz), centre_dims=4)
    ids = np.arange(2 * npairs)
    w = np.repeat(np.random.default_rng(11).uniform(1, 20, npairs), 2)              # the two atoms of a pair weigh the same
    rng = np.random.default_rng(12)
    split = dr.slab(13, F, npairs, nz, np.array([0.01, 0.99, 0.03, 0.0]))          # across the cell boundary in every frame
    whole = dr.slab(13, F, npairs, nz, np.array([0.51, 0.49, 0.53, 0.5]))          # the same slab half a box away
    moved = dr.slab(13, F, npairs, nz, rng.uniform(0, 1, F), shift=np.concatenate([rng.uniform(-2, 2, (F, 2)), np.zeros((F, 1))], 1))
    refs = []
    for fr in (split, whole, moved):
        ref, a, b = both(eng, m64, fr, grd, weight=w, boxes=ORTHO, centre_idx=ids, centre_weight=w)
        assert ref["resultant"] > 0.1
        refs.append((ref, a, b))
    assert (split[0, :, 2].astype(np.float64) / 4.0 % 1.0).std() > 0.3              # it IS split: both ends of the cell are populated
    for ref, a, b in refs[1:]:
        assert np.array_equal(a.count, refs[0][1].count) and np.array_equal(b.count, refs[0][2].count)
    assert refs[0][1].count.reshape(-1)[0] == 0 and refs[0][1].count.sum() == F * 2 * npairs


def test_centre_set_apart_from_the_selection(eng, m64):
    """The centre set (a weighted slab) and the selection (other atoms, placed on the grid as it is centred) differ; z is
    periodic (the circular mean); and the same with z open (pbc = 3: the plain mean of the fractional coordinate)."""
    F, npairs, n, nz = 3, 60, 300, 24
    rng = np.random.default_rng(14)
    z0 = np.array([0.4, 0.55, 0.47])
    sl = dr.slab(15, F, npairs, nz, z0, boxes=TRIC, half_width=0.1)
    u = np.zeros((F, n, 3))
    u[:, :, :2] = rng.uniform(0.05, 0.95, size=(F, n, 2))
    u[:, :, 2] = z0[:, None] - 0.5 + (rng.integers(0, nz, (F, n)) + 0.5 + rng.uniform(-0.4, 0.4, (F, n))) / nz
    fr = np.concatenate([sl, (u @ dr.box_of(TRIC, 0).T).astype(np.float32)], axis=1)
    cw = np.zeros(2 * npairs + n)
    cw[:2 * npairs] = np.repeat(rng.uniform(0.5, 3, npairs), 2)
    sel, cset = np.arange(2 * npairs, 2 * npairs + n), np.arange(2 * npairs)
    grd = dr.grid(BOX, (1, 1, nz), centre_dims=4)
    for pbc in (7, 3):
        ref, a, _ = both(eng, m64, fr, grd, pbc, idx=sel, boxes=TRIC, pbc=pbc, centre_idx=cset, centre_weight=cw)
        assert (ref["outside"] == 0).all() and np.abs(ref["centre"][:, 2].astype(np.float64) - z0).max() < 1e-5
        assert (pbc == 7) == (ref["resultant"] < np.inf)


def test_lab_grid_centred(eng, m64):
    F, n, nbins, lo, hi = 3, 300, (4, 5, 6), (-1.0, -1.5, -0.75), (1.0, 1.5, 0.75)
    rng = np.random.default_rng(16)
    origin = rng.uniform(-5, 5, (F, 3))
    d = rng.uniform(0.1, 0.6, (20, 3))
    pairs = np.concatenate([origin[:, None] + d[None], origin[:, None] - d[None]], axis=1)          # their mean is the origin
    fr = np.concatenate([pairs.astype(np.float32), dr.scatter_lab(17, F, n, nbins, lo, hi, origin=origin)], axis=1)
    ref, a, _ = both(eng, m64, fr, dr.grid(LAB, nbins, lo, hi, centre_dims=7), idx=np.arange(40, 40 + n), centre_idx=np.arange(40))
    assert np.abs(ref["centre"].astype(np.float64) - origin).max() < 1e-5 and 0 < int(ref["outside"].sum()) < F * n


# ---------------------------------------------------------------- boxes per frame

def test_fluctuating_boxes(eng, m64):
    F, n, nbins = 6, 400, (1, 1, 50)
    boxes = dr.mr.scaled_boxes(F, 18, TRIC).astype(np.float32)
    fr = dr.scatter_box(19, F, n, nbins, f32(boxes))
    w = np.random.default_rng(19).uniform(1, 16, n)
    ref, a, _ = both(eng, m64, fr, dr.grid(BOX, nbins), weight=w, boxes=boxes)
    v = ref["binvol"].astype(np.float64)
    assert v.max() / v.min() > 1.03                                  # +-2 % of the lengths
    # one box for all frames gives the bits of that box repeated F times
    fr = dr.scatter_box(20, F, n, nbins, TRIC)
    for real in REALS:
        one = call(eng, m64, real, fr, dr.grid(BOX, nbins), weight=w, boxes=TRIC)
        rep = call(eng, m64, real, fr, dr.grid(BOX, nbins), weight=w, boxes=np.tile(TRIC, (F, 1)))
        assert same_bits(one, rep)


# ---------------------------------------------------------------- plumbing

def test_index_with_gaps_and_a_long_stride(eng, m64):
    F, natoms, nbins = 3, 700, (2, 3, 9)
    fr = dr.scatter_box(21, F, natoms, nbins, ORTHO)
    idx = np.flatnonzero(np.arange(natoms) % 7 != 3)[::-1].copy()                 # gaps, and not in order
    w = f32(np.random.default_rng(21).uniform(-2, 2, natoms))            # as both() hands them to the entries
    labels = (np.arange(len(idx)) % 3)
    ref, a, b = both(eng, m64, fr, dr.grid(BOX, nbins), idx=idx, weight=w, labels=labels, ngroups=3, boxes=ORTHO)
    for real, got in zip(REALS, (a, b)):
        wide = np.full((F, natoms + 5, 3), np.nan, real)                          # a stride above 3 natoms: a view into a wider block
        wide[:, :natoms] = fr
        again = call(eng, m64, real, wide[:, :natoms], dr.grid(BOX, nbins), idx=idx, weight=w, labels=labels, ngroups=3, boxes=ORTHO)
        assert same_bits(got, again)
        twice = call(eng, m64, real, fr, dr.grid(BOX, nbins), idx=idx, weight=w, labels=labels, ngroups=3, boxes=ORTHO)
        assert same_bits(got, twice)


def test_host_and_device_memory_for_every_argument(eng):
    import torch
    from molar_amd import _lib
    lib = _lib.load()
    F, natoms, nbins = 3, 300, (1, 2, 16)
    rng = np.random.default_rng(22)
    grd = dr.grid(BOX, nbins, centre_dims=4)
    idx = rng.permutation(natoms)[:250].astype(np.uint64)
    cidx = np.arange(0, natoms, 3).astype(np.uint64)
    for fn, real in ((lib.molar_hip_density, np.float32), (lib.molar_hip_density_f64, np.float64)):
        ins = dict(frames=dr.scatter_box(23, F, natoms, nbins, ORTHO).astype(real), idx=idx, weight=rng.uniform(-2, 2, natoms).astype(real),
                   labels=rng.integers(0, 3, 250).astype(np.uint32), boxes=np.tile(ORTHO, (F, 1)).astype(real), centre_idx=cidx,
                   centre_weight=rng.uniform(1, 2, natoms).astype(real))
        outs = dict(density=np.zeros(3 * 32, real), count=np.zeros(3 * 32, np.uint64), outside=np.zeros(F, np.uint64), centre=np.zeros(F * 3, real),
                    binvol=np.zeros(F, real))

        def dev(a):
            view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype)
            return torch.from_numpy(a.view(view).copy()).cuda()

        def run(on_device):
            args = {k: (dev(v) if k in on_device else v) for k, v in ins.items()}
            res = {k: (dev(v) if k in on_device else v.copy()) for k, v in outs.items()}
            frames = args.pop("frames")
            torch.cuda.synchronize()
            st, S = dr.raw_density(fn, eng.ctx, frames, grd, real, n=250, ngroups=3, box_stride=9, ncentre=len(cidx), **args, **res)
            assert st == 0, lib.molar_hip_last_error()
            eng.synchronize()
            return [(v.cpu().numpy() if k in on_device else v).view(np.uint8).copy() for k, v in res.items()] + [S]

        base = run(())
        assert base[1].view(np.uint64).sum() > 0
        for name in list(ins) + list(outs):
            got = run((name,))
            assert all(np.array_equal(x, y) for x, y in zip(got, base)), name
        assert all(np.array_equal(x, y) for x, y in zip(run(tuple(ins) + tuple(outs)), base))


def test_weight_scale(eng, m64):
    grd = dr.grid(BOX, (1, 1, 10))
    rng = np.random.default_rng(24)
    small = rng.uniform(-0.99, 0.99, 5000)
    small[0] = 0.75
    cases = ((250, np.arange(1.0, 251.0), 62 - 8 - 8),            # weights 1 .. 250: n <= 2^8, max < 2^8
             (5000, small, 62 - 13 - 0),                          # |w| < 1 = 2^0, n <= 2^13
             (250, small[:250] / 1024, 52),                       # 62 - 8 + 10 = 64, clamped
             (250, None, 0), (250, np.zeros(250), 52))
    for n, w, want in cases:
        fr = dr.scatter_box(24, 1, n, grd.nbins, ORTHO)
        ref, a, b = both(eng, m64, fr, grd, n, weight=w, boxes=ORTHO)
        assert a.weight_scale_log2 == b.weight_scale_log2 == ref["S"] == want, n


# ---------------------------------------------------------------- values that are not finite

def test_nan_coordinate_in_the_selection(eng, m64):
    F, n, nbins = 3, 200, (1, 1, 12)
    fr = dr.scatter_box(25, F, n, nbins, ORTHO)
    fr[1, 17, 0] = np.nan
    fr[2, 5, 2] = np.inf
    ref, a, _ = both(eng, m64, fr, dr.grid(BOX, nbins), boxes=ORTHO)
    assert list(ref["outside"]) == [0, 1, 1] and int(ref["count"].sum()) == F * n - 2


def test_nan_in_the_centre_set_drops_the_frame(eng, m64):
    F, npairs, nz = 3, 50, 20
    fr = dr.slab(26, F, npairs, nz, np.array([0.2, 0.4, 0.9]))
    fr[1, 3, 2] = np.nan
    ref, a, b = both(eng, m64, fr, dr.grid(BOX, (1, 1, nz), centre_dims=4), boxes=ORTHO, centre_idx=np.arange(2 * npairs))
    assert list(ref["outside"]) == [0, 2 * npairs, 0] and np.isnan(a.centre[1, 2]) and np.isnan(b.centre[1, 2])
    assert int(ref["count"].sum()) == 2 * 2 * npairs


def test_bad_weights_and_labels_in_device_memory(eng):
    import torch
    from molar_amd import _lib
    lib = _lib.load()
    F, n, nbins = 2, 100, (1, 1, 8)
    grd = dr.grid(BOX, nbins)
    for fn, real in ((lib.molar_hip_density, np.float32), (lib.molar_hip_density_f64, np.float64)):
        fr = dr.scatter_box(27, F, n, nbins, ORTHO).astype(real)
        for bad in ("weight", "labels", "weight_host", "index"):
            w = np.ones(n, real)
            labels = np.zeros(n, np.int32)
            idx = np.arange(n, dtype=np.int64)
            if bad.startswith("weight"):
                w[41] = np.inf if real == np.float32 else np.nan
            elif bad == "labels":
                labels[77] = 2
            else:
                idx[9] = n
            outs = dict(density=np.full(8 * 2, 7, real), count=np.full(8 * 2, 7, np.uint64), outside=np.full(F, 7, np.uint64), centre=np.full(F * 3, 7, real),
                        binvol=np.full(F, 7, real))
            keep = {k: v.copy() for k, v in outs.items()}
            torch.cuda.synchronize()
            st, S = dr.raw_density(fn, eng.ctx, fr, grd, real, idx=torch.from_numpy(idx).cuda(), weight=w if bad == "weight_host" else torch.from_numpy(w).cuda(),
                                   labels=torch.from_numpy(labels).cuda(), ngroups=2, boxes=ORTHO, **outs)
            assert st == dr.ERR_INVALID, (bad, st)
            assert S == -999 and all(np.array_equal(outs[k], keep[k]) for k in outs), bad
    # and the context still works
    got = eng.density(dr.scatter_box(27, F, n, nbins, ORTHO), grd, boxes=ORTHO.astype(np.float32))
    assert got.count.sum() == F * n
