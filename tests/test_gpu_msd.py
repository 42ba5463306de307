"""Mean-squared displacement on the GPU (molar_hip_msd / _f64: no-jump unwrap, particle displacements, drift removal, lag sums)
against the numpy reference of tests/msd_ref.py, entry by entry within the bounds derived there.  Both entries see the same
numbers (f32 frames and boxes, cast to f64 for the f64 entry), so one reference serves both; every reference is computed
once per module.  The largest used fraction of each bound is printed by the last test."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msd_ref as mr  # noqa: E402
from msd_ref import ERR_INVALID, ERR_INVERSE, ERR_SIZES, ERR_TOO_LARGE, ERR_ZERO_LENGTH, ERR_ZERO_MASS, argument_errors, raw_msd  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from molar_amd import api
    return api.Engine()


@pytest.fixture(scope="module")
def m64(eng):
    from molar_amd import api
    return api.MeasureF64(eng)


def f32box(b):
    return np.asarray(b, np.float64).astype(np.float32).astype(np.float64)


ORTHO, TRIC = f32box(mr.ORTHO), f32box(mr.TRICLINIC)


def freeze(kw):
    return tuple(sorted((k, v.tobytes() + str(v.shape).encode() if isinstance(v, np.ndarray) else v) for k, v in kw.items()))


_REFS = {}


def reference(frames, **kw):
    key = (frames.tobytes(), frames.shape, freeze(kw))
    if key not in _REFS:
        _REFS[key] = mr.msd(frames, **kw)
    return _REFS[key]


def plan_of(ref, kw, F):
    from molar_amd import api
    n = ref["disp"].shape[1] if kw.get("groups") is None else int(np.asarray(kw["groups"])[-1])
    nref = 0 if kw.get("ref_idx") is None else len(kw["ref_idx"])
    L = F - 1 if kw.get("max_lag") is None else kw["max_lag"]
    return api.msd_plan(F, n, ref["P"], nref, L)


def call(entry, frames, real, **kw):
    kw = dict(kw)
    if kw.get("mass") is not None:
        kw["mass"] = np.asarray(kw["mass"], real)
    if kw.get("boxes") is not None:
        kw["boxes"] = np.asarray(kw["boxes"], real)
    else:
        kw["pbc"] = 0
    return entry.msd(np.asarray(frames, real), per_particle=True, disp=True, **kw)


def both(eng, m64, frames, what, **kw):
    """The f32 and the f64 entry on the same numbers against one reference; returns the two results."""
    assert frames.dtype == np.float32
    if kw.get("mass") is not None:
        kw["mass"] = np.asarray(kw["mass"], np.float32).astype(np.float64)          # the numbers both entries and the reference see
    if kw.get("boxes") is None:
        kw.pop("boxes", None)
        ref = reference(frames, boxes=None, pbc=0, **{k: v for k, v in kw.items() if k != "pbc"})
    else:
        ref = reference(frames, **kw)
    _, chunk, _ = plan_of(ref, kw, frames.shape[0])
    out = []
    for entry, real, eps in ((eng, np.float32, mr.EPS32), (m64, np.float64, mr.EPS64)):
        got = call(entry, frames, real, **kw)
        mr.check(got, ref, eps, chunk, what=f"{what} {np.dtype(real).name}")
        out.append(got)
    return out, ref


@functools.lru_cache(maxsize=None)
def walk(F, n, seed, kind="ortho", step=None):
    box = TRIC if kind == "tric" else ORTHO
    fr, _ = mr.wrapped_walk(F, n, seed, box, step or (0.3 if kind == "tric" else 0.45))
    return fr


@pytest.mark.parametrize("F", [1, 2, 3, 63, 64, 65, 66, 129, 130])
def test_frames(eng, m64, F):
    both(eng, m64, walk(F, 3, 1000 + F), f"F={F}", boxes=ORTHO)


@pytest.mark.parametrize("L", [0, 1, 33])
def test_max_lag(eng, m64, L):
    (g32, g64), ref = both(eng, m64, walk(66, 3, 7), f"max_lag={L}", boxes=ORTHO, max_lag=L)
    assert g32.msd.shape == (L + 1,) and g64.msd_particle.shape == (3, L + 1)


@pytest.mark.parametrize("L1", [255, 256, 257])
def test_lag_block_edges(eng, m64, L1):
    from molar_amd import api
    assert api.msd_plan(258, 2)[2] == 256
    both(eng, m64, walk(258, 2, 8), f"lags={L1}", boxes=ORTHO, max_lag=L1 - 1)


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 63, 64, 65])
def test_particles(eng, m64, P):
    both(eng, m64, walk(10, P, 20 + P), f"P={P}", boxes=ORTHO)


@pytest.mark.parametrize("P,last", [(8192, 0), (8193, 1), (8195, 3)])
def test_particle_chunk_edges(eng, m64, P, last):
    """Four particles per workgroup of the lag kernel (the plan says so); the last workgroup holds chunk, 1 and chunk - 1."""
    from molar_amd import api
    chunk = api.msd_plan(3, P)[1]
    assert chunk == 4 and P % chunk == last
    both(eng, m64, walk(3, P, 30), f"P={P}", boxes=ORTHO)


# The lag kernel stages the origins in segments of 512 frames with windows of 768 and takes the origins that every lane of a block
# reaches four at a time: frames either side of 512 and 768, two and three segments, 0 .. 3 origins left over by the unrolled
# loop, strides that do not divide 512, and a stride (600) that leaves whole segments without an origin.
SEGMENTS = [(F, 1) for F in (511, 512, 513, 767, 768, 769, 1030, 1031, 1032, 1033, 1300)] + \
           [(F, s) for F in (513, 769, 1030, 1300) for s in (3, 7, 600)]


@pytest.mark.parametrize("F,stride", SEGMENTS)
def test_origin_segments(eng, m64, F, stride):
    P = 2 + F % 2
    both(eng, m64, walk(F, P, 2000 + F, step=0.3), f"F={F} origin_stride={stride}", boxes=ORTHO, origin_stride=stride)


def test_particle_chunk_at_its_clamp(eng, m64):
    """64 particles per workgroup, the most the plan gives, with a last workgroup of one; and a chunk that does not divide 2048."""
    from molar_amd import api
    for P, want in ((2048 * 64 + 1, 64), (2048 * 7 + 5, 7)):
        assert api.msd_plan(3, P)[1] == want
        both(eng, m64, walk(3, P, 31), f"P={P} chunk={want}", boxes=ORTHO)


@pytest.mark.parametrize("stride", [1, 2, 7, 69])
def test_origin_stride(eng, m64, stride):
    (g32, _), ref = both(eng, m64, walk(66, 3, 7), f"origin_stride={stride}", boxes=ORTHO, origin_stride=stride)
    assert ref["count"][0] == -(-66 // stride) and (stride < 66 or np.all(ref["count"] == 1))


def test_dims(eng, m64):
    fr = walk(40, 5, 41)
    res = {d: both(eng, m64, fr, f"dims={d}", boxes=ORTHO, dims=d) for d in range(1, 8)}
    for k, eps in ((0, mr.EPS32), (1, mr.EPS64)):
        parts = sum(res[d][0][k].msd.astype(np.float64) for d in (1, 2, 4))
        lim = sum(mr.bounds(res[d][1], eps)[1] for d in (1, 2, 4, 7))
        assert mr.worst(np.abs(parts - res[7][0][k].msd.astype(np.float64)), lim) <= 1.0
    assert np.array_equal(res[3][0][1].disp, res[7][0][1].disp), "the components of the lags do not touch the displacements"


def test_groups_of_one_equal_the_null_form(eng, m64):
    fr = walk(20, 70, 51)
    mass = np.random.default_rng(1).uniform(1, 16, 70)
    for entry, real in ((eng, np.float32), (m64, np.float64)):
        a = call(entry, fr, real, boxes=ORTHO, mass=mass)
        b = call(entry, fr, real, boxes=ORTHO, mass=mass, groups=np.arange(71, dtype=np.uint64))
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_groups_unequal(eng, m64):
    n = 100
    mass = np.random.default_rng(2).uniform(1, 16, n)
    both(eng, m64, walk(20, n, 52), "groups 1..9", boxes=ORTHO, mass=mass, groups=mr.groups_unequal(n))
    idx = np.random.default_rng(3).permutation(n)[:60].astype(np.uint64)
    both(eng, m64, walk(20, n, 52), "groups 1..9 of a selection", boxes=ORTHO, mass=mass, idx=idx, groups=mr.groups_unequal(60))


def test_large_group_beside_singletons(eng, m64):
    n = 310
    off = np.array([0, 1, 2, 302] + list(range(303, n + 1)), dtype=np.uint64)              # 1, 1, 300, then singletons
    mass = np.random.default_rng(4).uniform(1, 16, n)
    both(eng, m64, walk(12, n, 53), "a group of 300", boxes=ORTHO, mass=mass, groups=off)
    both(eng, m64, walk(12, n, 53), "a group of 300, unit weights", boxes=ORTHO, groups=off)
    two = np.array([0, 300, n], dtype=np.uint64)
    both(eng, m64, walk(12, n, 53), "300 + 10", boxes=ORTHO, groups=two)
    big = np.array([0, 257, 770], dtype=np.uint64)                                         # 257 and 513 atoms: pieces of 256 + 1
    both(eng, m64, walk(6, 770, 54), "257 + 513", boxes=ORTHO, groups=big)


def test_zero_weights(eng, m64):
    from molar_amd import api
    n = 30
    fr = walk(12, n, 55)
    mass = np.random.default_rng(5).uniform(1, 16, n)
    mass[[1, 4, 5, 17]] = 0.0
    off = np.arange(0, n + 1, 3, dtype=np.uint64)
    both(eng, m64, fr, "zero-weight atoms in groups", boxes=ORTHO, mass=mass, groups=off)
    mass[3:6] = 0.0                                                                         # group 1 has no weight at all
    for entry, real in ((eng, np.float32), (m64, np.float64)):
        with pytest.raises(api.MolarHipError) as e:
            call(entry, fr, real, boxes=ORTHO, mass=mass, groups=off)
        assert e.value.code == ERR_ZERO_MASS
    with pytest.raises(api.MolarHipError) as e:                                             # ... and so has a reference set
        call(eng, fr, np.float32, boxes=ORTHO, mass=mass, ref_idx=np.array([3, 4, 5], dtype=np.uint64))
    assert e.value.code == ERR_ZERO_MASS


def test_boxes(eng, m64):
    both(eng, m64, walk(30, 12, 61), "one orthorhombic box", boxes=ORTHO)
    both(eng, m64, walk(30, 12, 62, "tric"), "a skewed cell, full mask", boxes=TRIC)
    boxes = f32box(mr.scaled_boxes(30, 3))
    fr = mr.wrapped_walk(30, 12, 63, ORTHO, 0.3, boxes=boxes)[0]
    both(eng, m64, fr, "per-frame boxes", boxes=boxes)
    tb = f32box(mr.scaled_boxes(20, 4, TRIC))
    both(eng, m64, mr.wrapped_walk(20, 12, 64, TRIC, 0.25, boxes=tb)[0], "per-frame skewed cells", boxes=tb)
    both(eng, m64, walk(30, 12, 62, "tric"), "a skewed cell, mask xz", boxes=TRIC, pbc=5)


def test_mask_xy_with_z_that_never_wraps(eng, m64):
    x = mr.random_walk(30, 12, 65, ORTHO, 0.45)
    x[..., 2] = 2.0 + 0.8 * np.sin(np.arange(30)[:, None] * 0.7 + np.arange(12)[None])      # stays inside (1.2, 2.8) of 4
    w = mr.wrap(x, ORTHO)
    assert np.allclose(w[..., 2], x[..., 2])
    (g32, _), _ = both(eng, m64, w.astype(np.float32), "mask xy", boxes=ORTHO, pbc=3)
    assert np.abs(g32.disp[..., 2] - (x[..., 2] - x[0, :, 2])).max() <= 1e-6


def test_unwrapped_input_equals_wrapped_input(eng, m64):
    x = mr.grid_walk(40, 9, 66)
    w = mr.wrap_ortho(x, ORTHO)
    assert np.array_equal(w.astype(np.float32).astype(np.float64), w) and np.abs(x).max() > 2 * 4.0
    (a32, a64), ra = both(eng, m64, x.astype(np.float32), "unwrapped, no boxes", boxes=None)
    (b32, b64), rb = both(eng, m64, w.astype(np.float32), "its wrapped copy", boxes=ORTHO)
    for a, b, eps in ((a32, b32, mr.EPS32), (a64, b64, mr.EPS64)):
        for k, (la, lb) in enumerate(zip(mr.bounds(ra, eps), mr.bounds(rb, eps))):
            order = (3, 0, 1, 2)[k]                                                         # bounds: disp, msd, m4, msd_particle
            assert mr.worst(np.abs(a[order].astype(np.float64) - b[order].astype(np.float64)), la + lb) <= 1.0


def test_walk_that_crosses_the_box_many_times(eng, m64):
    rng = np.random.default_rng(67)
    F, n = 40, 8
    L = ORTHO[[0, 4, 8]]
    steps = (0.25 + rng.uniform(-0.2, 0.2, size=(F - 1, n, 3))) * L
    x = np.concatenate([np.zeros((1, n, 3)), np.cumsum(steps, axis=0)]) + rng.random((n, 3)) * L
    assert np.all((x[-1] - x[0]) / L > 5)
    (g32, _), ref = both(eng, m64, mr.wrap(x, ORTHO).astype(np.float32), "more than five crossings", boxes=ORTHO)
    assert np.abs(g32.disp - (x - x[0])).max() <= 1e-4


@pytest.mark.parametrize("which", ["equal", "subset", "disjoint", "large"])
def test_drift_removal(eng, m64, which):
    F, n = 30, 40
    if which == "large":
        n = 600                                                                             # a reference set of three pieces
    x = mr.random_walk(F, n, 70, ORTHO, 0.25)
    drift = np.cumsum(np.random.default_rng(71).uniform(-0.15, 0.15, size=(F, 1, 3)) * ORTHO[[0, 4, 8]], axis=0)
    fr0 = mr.wrap(x, ORTHO).astype(np.float32)
    fr1 = mr.wrap(x + drift, ORTHO).astype(np.float32)
    sel = {"equal": np.arange(n), "subset": np.arange(n), "disjoint": np.arange(0, n // 2), "large": np.arange(n)}[which]
    refset = {"equal": np.arange(n), "subset": np.arange(0, n, 3), "disjoint": np.arange(n // 2, n), "large": np.arange(n - 1, -1, -1)}[which]
    kw = dict(boxes=ORTHO, idx=sel.astype(np.uint64), ref_idx=refset.astype(np.uint64), mass=np.random.default_rng(72).uniform(1, 16, n))
    (a32, a64), ra = both(eng, m64, fr0, f"drift {which}, none added", **kw)
    (b32, b64), rb = both(eng, m64, fr1, f"drift {which}, a common drift added", **kw)
    # the common drift disappears: to the f32 rounding of the two sets of positions (they are different numbers)
    assert np.abs(a64.disp - b64.disp).max() <= 16 * 2.0 ** -23 * 4.0
    assert np.abs(a64.msd - b64.msd).max() <= 1e-4 * a64.msd.max()
    if which in ("equal", "large"):
        w = kw["mass"].astype(np.float32).astype(np.float64)[sel]          # the masses the entries saw
        assert np.abs((a64.disp * w[None, :, None]).sum(1)).max() <= 1e-9, "the weighted mean displacement of the set itself is zero"


def test_memory_sides_and_strided_frames(eng, m64):
    import torch
    fr = walk(24, 70, 80)
    mass = np.random.default_rng(81).uniform(1, 16, 70).astype(np.float32)
    off = mr.groups_unequal(70)
    refset = np.arange(0, 70, 2, dtype=np.uint64)
    kw = dict(boxes=ORTHO.astype(np.float32), mass=mass, groups=off, ref_idx=refset, per_particle=True, disp=True)
    host = eng.msd(fr, **kw)
    dkw = dict(boxes=torch.from_numpy(kw["boxes"]).cuda(), mass=torch.from_numpy(mass).cuda(), groups=torch.from_numpy(off.astype(np.int64)).cuda(),
               ref_idx=torch.from_numpy(refset.astype(np.int64)).cuda(), per_particle=True, disp=True)
    dev = eng.msd(torch.from_numpy(fr).cuda(), **dkw)
    eng.synchronize()
    for a, b in zip(host, dev):
        assert np.array_equal(a, b.cpu().numpy())
    # every second frame, read in place
    view = fr[::2]
    assert fr.flags.c_contiguous and not view.flags.c_contiguous
    a = eng.msd(view, **kw)
    b = eng.msd(np.ascontiguousarray(view), **kw)
    tv = torch.from_numpy(fr).cuda()[::2]
    c = eng.msd(tv, **dkw)
    eng.synchronize()
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z.cpu().numpy())
    # a destination wider than the lags, on the device: the rest of a row is not touched
    P, L = len(off) - 1, 23
    wide = torch.full((P, L + 9), -1.0, dtype=torch.float32, device="cuda")
    msd = torch.zeros(L + 1, dtype=torch.float32, device="cuda")
    rc = eng.lib.molar_hip_msd(eng.ctx, tv.data_ptr(), 12, tv.stride(0), 70, None, 70, dkw["mass"].data_ptr(), dkw["boxes"].data_ptr(), 0, 7,
                               dkw["groups"].data_ptr(), P, dkw["ref_idx"].data_ptr(), len(refset), 11, 1, 7, msd.data_ptr(), None, wide.data_ptr(), L + 9, None)
    eng.synchronize()
    assert rc == 0, eng.lib.molar_hip_last_error()
    assert np.array_equal(wide[:, :12].cpu().numpy(), a.msd_particle) and bool((wide[:, 12:] == -1).all())
    assert np.array_equal(msd[:12].cpu().numpy(), a.msd)


def test_stages(eng, m64):
    fr = walk(30, 12, 61)
    full = eng.msd(fr, boxes=ORTHO.astype(np.float32), per_particle=True, disp=True)
    only_disp = eng.msd(fr, boxes=ORTHO.astype(np.float32), msd=False, m4=False, disp=True)
    assert only_disp.msd is None and only_disp.m4 is None and only_disp.msd_particle is None
    assert np.array_equal(only_disp.disp, full.disp)
    only_msd = eng.msd(fr, boxes=ORTHO.astype(np.float32), m4=False)
    assert only_msd.m4 is None and only_msd.disp is None and np.array_equal(only_msd.msd, full.msd)
    only_m4 = eng.msd(fr, boxes=ORTHO.astype(np.float32), msd=False)
    assert np.array_equal(only_m4.m4, full.m4)


def test_same_call_same_bits(eng, m64):
    fr = walk(130, 65, 90)
    kw = dict(boxes=ORTHO, groups=mr.groups_unequal(65), ref_idx=np.arange(0, 65, 2, dtype=np.uint64))
    for entry, real in ((eng, np.float32), (m64, np.float64)):
        a = call(entry, fr, real, **kw)
        b = call(entry, fr, real, **kw)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_coordinate(eng, m64, bad):
    F, n = 20, 12
    fr = walk(F, n, 95).copy()
    off = np.arange(0, n + 1, 3, dtype=np.uint64)
    for entry, real in ((eng, np.float32), (m64, np.float64)):
        clean = call(entry, fr, real, boxes=ORTHO, groups=off)
        hurt = fr.copy()
        hurt[7, 4, 1] = bad                                                                 # atom 4 is in particle 1
        got = call(entry, hurt, real, boxes=ORTHO, groups=off)
        assert np.array_equal(got.disp[:7], clean.disp[:7])
        assert np.all(np.isnan(got.disp[7:, 1, :][:, 1])) and np.array_equal(np.delete(got.disp, 1, axis=1), np.delete(clean.disp, 1, axis=1))
        assert np.array_equal(np.delete(got.msd_particle, 1, axis=0), np.delete(clean.msd_particle, 1, axis=0))
        # lags 0 .. F-1: every lag has an origin pair that touches a frame from 7 on
        assert np.all(np.isnan(got.msd_particle[1])) and np.all(np.isnan(got.msd)) and np.all(np.isnan(got.m4))
        # with the atom in the reference set everything is NaN from that frame on, hence every lag sum
        ref = call(entry, hurt, real, boxes=ORTHO, groups=off, ref_idx=np.array([4, 9], dtype=np.uint64))
        assert np.all(np.isnan(ref.disp[7:, :, 1])) and np.all(np.isnan(ref.msd_particle)) and np.all(np.isnan(ref.msd))


def test_errors(eng, m64):
    from molar_amd import api
    for fn, real in ((eng.lib.molar_hip_msd, np.float32), (eng.lib.molar_hip_msd_f64, np.float64)):
        for what, want, got in argument_errors(fn, eng.ctx, real):
            assert got == want, (what, want, got)
        assert raw_msd(fn, eng.ctx, np.zeros((0, 5, 3), real), F=0) == 0
    fr = walk(6, 5, 99)
    import torch
    # the checks that only the device can make: an index in device memory, offsets in device memory
    with pytest.raises(api.MolarHipError) as e:
        eng.msd(torch.from_numpy(fr).cuda(), idx=torch.tensor([0, 9], dtype=torch.int64, device="cuda"))
    assert e.value.code == ERR_INVALID
    with pytest.raises(api.MolarHipError) as e:
        eng.msd(torch.from_numpy(fr).cuda(), ref_idx=torch.tensor([5], dtype=torch.int64, device="cuda"))
    assert e.value.code == ERR_INVALID
    with pytest.raises(api.MolarHipError) as e:
        eng.msd(torch.from_numpy(fr).cuda(), groups=torch.tensor([0, 3, 2, 5], dtype=torch.int64, device="cuda"))
    assert e.value.code == ERR_SIZES
    # the engine still works afterwards
    assert eng.msd(fr, boxes=ORTHO.astype(np.float32)).msd[0] == 0


def test_workspace_that_cannot_be_allocated(eng, m64):
    """One atom selected 200 000 times over 100 000 frames: 1.2 MB of frames, 480 GB of particle trajectories.  The workspace is the
    first thing the call asks the device for, before any launch."""
    from molar_amd import api
    F, n, L = 100000, 200000, 10
    idx = np.zeros(n, np.uint64)
    want = api.msd_plan(F, n, n, 0, L)[0]
    assert want > 24 * F * n
    for fn, real in ((eng.lib.molar_hip_msd, np.float32), (eng.lib.molar_hip_msd_f64, np.float64)):
        fr = np.zeros((F, 1, 3), real)
        out = np.zeros(L + 1, real)
        assert raw_msd(fn, eng.ctx, fr, real, idx=idx, n=n, L=L, msd=out) == ERR_TOO_LARGE
        assert str(want) in eng.lib.molar_hip_last_error().decode(), eng.lib.molar_hip_last_error()
    small = walk(6, 5, 99)
    assert eng.msd(small, boxes=ORTHO.astype(np.float32)).msd[0] == 0 and m64.msd(small.astype(np.float64), boxes=ORTHO).msd[0] == 0


def test_boxes_that_are_none(eng, m64):
    from molar_amd import api
    fr = walk(6, 5, 99)
    flat = ORTHO.copy()
    flat[8] = 0.0                                            # the third vector has no length
    singular = np.array([1.0, 0, 0, 2.0, 0, 0, 0, 0, 3.0])   # two parallel vectors
    per_frame = np.tile(ORTHO, (6, 1))
    per_frame[4] = singular
    for entry, real in ((eng, np.float32), (m64, np.float64)):
        for boxes, code in ((flat, ERR_ZERO_LENGTH), (singular, ERR_INVERSE), (per_frame, ERR_INVERSE)):
            with pytest.raises(api.MolarHipError) as e:
                call(entry, fr, real, boxes=boxes)
            assert e.value.code == code


def test_ballistic_known_answer(eng, m64):
    F, n = 33, 7
    fr, v = mr.ballistic(F, n, 11)
    (g32, g64), ref = both(eng, m64, fr, "ballistic", boxes=None)
    v2 = (v * v).sum(1)
    tau = np.arange(F, dtype=np.float64)
    # exact inputs, exact differences (binary fractions): only the sums round
    assert np.abs(g64.msd - v2.mean() * tau ** 2).max() <= (F + n + 8) * mr.U * v2.mean() * tau[-1] ** 2
    assert np.array_equal(g64.disp, fr.astype(np.float64) - fr[0].astype(np.float64))


def test_report_used_fractions():
    """Not a check of its own: prints the largest fraction of each bound that the tests above used."""
    print("largest used fraction per output:", {k: f"{v:.3g}" for k, v in sorted(mr.REPORT.items())})
    assert all(v <= 1.0 for v in mr.REPORT.values())
