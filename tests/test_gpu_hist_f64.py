"""The fused histogram in f64 (molar_hip_search_histogram_f64 / _frames_f64: search + the f64 Histogram1D::add_one of
molar_membrane/src/stats.rs:29-35 in one pass) against the f64 build of the CPU checker: integer bins equal to the checker's
histogram of its own distance stream, for every class of plan entry, both call forms and device-resident inputs."""
import ctypes as C

import numpy as np
import pytest

from molar_amd import synth

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, NO_SEARCH = 50, 52       # MOLAR_HIP_ERR_*


@pytest.fixture(scope="module")
def eng():
    from molar_amd import build
    from molar_amd.api import Engine
    build.build_library()
    return Engine(0)


def api():
    import molar_amd.api as a
    return a


def ref_dist(orc64, kind, rc, pos, idx1=None, idx2=None, box=None, pbc=7, vdw1=None, vdw2=None):
    """The checker's f64 distance stream of the request (the same pairs search_count_f64 / _fill_f64 report)."""
    a = api()
    ob = None if box is None else orc64.box_from_matrix(box)
    if kind == a.SEARCH_SINGLE:
        p = pos if idx1 is None else pos[idx1.astype(np.int64)]
        r = orc64.search_single(rc, p, nthreads=8) if ob is None else orc64.search_single_pbc(rc, p, ob, pbc, nthreads=8)
        return r["d"]
    p1, p2 = pos[idx1.astype(np.int64)], pos[idx2.astype(np.int64)]
    if kind == a.SEARCH_DOUBLE_VDW:
        r = orc64.search_double_vdw(p1, p2, vdw1, vdw2, nthreads=8) if ob is None else \
            orc64.search_double_vdw_pbc(p1, p2, vdw1, vdw2, ob, pbc, nthreads=8)
        return r["d"]
    r = orc64.search_double(rc, p1, p2, nthreads=8) if ob is None else orc64.search_double_pbc(rc, p1, p2, ob, pbc, nthreads=8)
    return r["d"]


def hist(orc64, hmin, hmax, nbins, d):
    return orc64.histogram_add(hmin, hmax, nbins, d).astype(np.uint64)


@pytest.mark.timeout(1200)
def test_c4_size_equals_the_f64_checker(eng, orc64):
    """BASELINE config 4's shape in f64: 250k atoms, box A, rc 1.2 nm, 1200 bins, full periodicity."""
    a = api()
    n, rc, nbins = 250_000, 1.2, 1200
    box = synth.box_a(n).astype(np.float64)
    pos = synth.frame(n, box, 3).astype(np.float64)
    ref = orc64.search_single_pbc(rc, pos, orc64.box_from_matrix(box), 7, nthreads=8)
    want = hist(orc64, 0.0, rc, nbins, ref["d"])
    bins, cnt = eng.search_histogram_f64(a.SEARCH_SINGLE, rc, 0.0, rc, nbins, pos, box=box, pbc=7)
    assert cnt == len(ref["d"]) and cnt > 10_000_000
    assert np.array_equal(bins, want)
    bins2, cnt2 = eng.search_histogram_f64(a.SEARCH_SINGLE, rc, 0.0, rc, nbins, pos, box=box, pbc=7, bins=bins)
    assert np.array_equal(bins2, 2 * want) and cnt2 == cnt
    half, cnt3 = eng.search_histogram_f64(a.SEARCH_SINGLE, rc, 0.0, rc / 2, nbins, pos, box=box, pbc=7)
    assert np.array_equal(half, hist(orc64, 0.0, rc / 2, nbins, ref["d"])) and cnt3 == cnt


CASES = ["ortho", "tric_a", "hex_b", "rhombic_dodecahedron", "big_cells", "big_cells_two_sets", "big_cells_no_box", "few_cells",
         "pbc_1", "pbc_3", "pbc_5", "pbc_6", "no_box", "hmin_pos", "hmin_neg", "vdw", "vdw_no_box", "two_sets", "empty_selection",
         "nbins_1", "nbins_8192"]


@pytest.mark.parametrize("case", CASES)
def test_every_entry_class_equals_the_distance_stream(eng, orc64, case):
    """Plain, same-cell and wrapped entries (band-classified with >= 4 cells per periodic dimension, exact with fewer and for a
    triclinic box's full-periodicity corner entries), second cells of more than 256 atoms (the chunk loop), partial
    periodicity, no box, vdW radii, two sets, ranges that start above and below zero, 1 and 8192 bins."""
    a = api()
    rng = np.random.default_rng(31)
    kind, n, rc, nbins, hmin, pbc = a.SEARCH_SINGLE, 24_000, 0.9, 450, 0.0, 7
    rd = np.array([[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, np.sqrt(0.5)]])
    box = synth.box_a(n).astype(np.float64)
    use_box = True
    if case == "ortho":
        box = synth.box_ortho(n).astype(np.float64)
    elif case == "hex_b":
        box = synth.box_b(n).astype(np.float64)
    elif case == "rhombic_dodecahedron":
        box = rd * ((n / 100.0) / abs(np.linalg.det(rd))) ** (1 / 3)
    elif case in ("big_cells", "big_cells_two_sets", "big_cells_no_box"):
        n, rc, nbins = 20_000, 1.45, 600          # 4 x 4 x 4 cells of ~310 atoms: second cells > 256 atoms
        box = np.diag([6.0, 6.0, 6.0])
        kind = a.SEARCH_DOUBLE if case == "big_cells_two_sets" else kind
        use_box = case != "big_cells_no_box"
    elif case == "few_cells":
        n, rc = 4000, 1.2                         # 2-3 cells per dimension: wrapped entries evaluated exactly
        box = synth.box_b(n).astype(np.float64)
    elif case.startswith("pbc_"):
        pbc = int(case[4:])
    elif case == "no_box":
        use_box = False
    elif case == "hmin_pos":
        hmin = 0.35
    elif case == "hmin_neg":
        hmin = -0.2
    elif case in ("vdw", "vdw_no_box"):
        kind, use_box = a.SEARCH_DOUBLE_VDW, case == "vdw"
    elif case == "two_sets":
        kind, box = a.SEARCH_DOUBLE, synth.box_b(n).astype(np.float64)
    elif case == "nbins_1":
        nbins = 1
    elif case == "nbins_8192":
        nbins = 8192
    if box.shape == (3, 3) and case.startswith("big_cells"):
        pos = rng.random((n, 3)) * 6.0 + rng.normal(0, 0.05, (n, 3))
    else:
        pos = synth.frame(n, box.astype(np.float32), 5).astype(np.float64) + rng.normal(0, 1e-7, (n, 3))
    hmax = rc
    idx1 = idx2 = vdw1 = vdw2 = None
    if kind != a.SEARCH_SINGLE:
        idx1 = np.sort(rng.choice(n, n // 2, replace=False)).astype(np.uint64)
        idx2 = np.setdiff1d(np.arange(n, dtype=np.uint64), idx1)
        if kind == a.SEARCH_DOUBLE_VDW:
            rc, hmax, nbins = None, 0.5, 250
            vdw1, vdw2 = rng.uniform(0.1, 0.22, len(idx1)), rng.uniform(0.1, 0.22, len(idx2))
    if case == "empty_selection":
        idx1 = np.zeros(0, np.uint64)
    b = box if use_box else None
    if case == "empty_selection":
        d = np.zeros(0)
    else:
        d = ref_dist(orc64, kind, rc, pos, idx1, idx2, b, pbc, vdw1, vdw2)
        assert len(d) > 1000
    want = hist(orc64, hmin, hmax, nbins, d)
    xyz2 = pos if kind != a.SEARCH_SINGLE else None
    bins, cnt = eng.search_histogram_f64(kind, rc, hmin, hmax, nbins, pos, idx1, xyz2, idx2, box=b, pbc=pbc, vdw1=vdw1, vdw2=vdw2)
    assert cnt == len(d)
    assert np.array_equal(bins, want)


def test_f64_decides(eng, orc64):
    """Pairs at bin edges * (1 +- 1e-12) and at the cutoff * (1 +- 1e-12): the f64 fused histogram equals the f64 checker,
    the f32 fused histogram of the same frame (coordinates rounded to f32) cannot - the new path is double end to end."""
    a = api()
    rng = np.random.default_rng(7)
    rc, L, nbins = 1.2, 9.0, 1200
    box = np.diag([L, L, L])
    npairs = 6000
    pa = 0.2 * L + 0.6 * L * rng.random((npairs, 3))
    u = rng.normal(size=(npairs, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
    edge = np.where(rng.random(npairs) < 0.2, rc, rng.integers(1, nbins, npairs) * (rc / nbins))
    e = 10.0 ** rng.uniform(-14.0, -10.0, npairs) * rng.choice([-1.0, 1.0], npairs)
    pb = pa + (edge * (1.0 + e))[:, None] * u
    pos = np.concatenate([pa, pb, L * rng.random((20_000, 3))])
    ob = orc64.box_from_matrix(box)
    ref = orc64.search_single_pbc(rc, pos, ob, 7, nthreads=8)
    want = hist(orc64, 0.0, rc, nbins, ref["d"])
    bins, cnt = eng.search_histogram_f64(a.SEARCH_SINGLE, rc, 0.0, rc, nbins, pos, box=box, pbc=7)
    assert cnt == len(ref["d"]) and np.array_equal(bins, want)
    # distances within 1e-9 of a bin edge: where f32 arithmetic cannot follow
    assert (np.abs(ref["d"] * (nbins / rc) - np.round(ref["d"] * (nbins / rc))) < 1e-6).sum() > 1000
    b32, c32 = eng.search_histogram(a.SEARCH_SINGLE, rc, 0.0, rc, nbins, pos.astype(np.float32), box=box.astype(np.float32), pbc=7)
    assert not np.array_equal(b32, want)


def test_device_inputs_and_asynchronous_bins(eng, orc64):
    """float64 coordinates and int64 bins in HBM; want_count=False returns before the kernel ends - synchronize() first."""
    import torch
    a = api()
    n, rc, nbins = 30_000, 1.0, 500
    box = synth.box_b(n).astype(np.float64)
    pos = synth.frame(n, box.astype(np.float32), 9).astype(np.float64)
    d = ref_dist(orc64, a.SEARCH_SINGLE, rc, pos, box=box)
    want = hist(orc64, 0.0, rc, nbins, d)
    dpos = torch.from_numpy(pos).cuda()
    dbins = torch.zeros(nbins, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for _ in range(3):
        out, cnt = eng.search_histogram_f64(a.SEARCH_SINGLE, rc, 0.0, rc, nbins, dpos, box=box, pbc=7, bins=dbins, want_count=False)
        assert cnt is None and out is dbins
    eng.synchronize()
    assert np.array_equal(dbins.cpu().numpy().astype(np.uint64), 3 * want)
    dbins.zero_()
    torch.cuda.synchronize()
    _, cnt = eng.search_histogram_f64(a.SEARCH_SINGLE, rc, 0.0, rc, nbins, dpos, box=box, pbc=7, bins=dbins)
    assert cnt == len(d)
    assert np.array_equal(dbins.cpu().numpy().astype(np.uint64), want)


def test_frames_form_strided_window_per_frame_boxes(eng, orc64):
    """17 frames taken as a window (with gaps) of a larger HBM buffer, one box per frame: the sums of the single calls and of
    the checker; host frames and host bins give the same."""
    import torch
    a = api()
    n, rc, nbins, nf = 6000, 0.9, 300, 17
    base = synth.box_a(n).astype(np.float64)
    boxes = np.stack([base * (1.0 + 0.01 * k) for k in range(nf)])
    frames = np.stack([synth.frame(n, boxes[k].astype(np.float32), k).astype(np.float64) for k in range(nf)])
    big = torch.zeros((nf + 3, n + 5, 3), dtype=torch.float64)
    big[2:2 + nf, 4:4 + n] = torch.from_numpy(frames)
    big = big.cuda()
    win = big[2:2 + nf, 4:4 + n]
    assert win.stride(0) == (n + 5) * 3 and not win.is_contiguous()
    want = np.zeros(nbins, np.uint64)
    single = np.zeros(nbins, np.uint64)
    for k in range(nf):
        want += hist(orc64, 0.0, rc, nbins, ref_dist(orc64, a.SEARCH_SINGLE, rc, frames[k], box=boxes[k]))
        eng.search_histogram_f64(a.SEARCH_SINGLE, rc, 0.0, rc, nbins, frames[k], box=boxes[k], pbc=7, bins=single)
    assert np.array_equal(single, want)
    dbins = torch.zeros(nbins, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.search_histogram_frames_f64(a.SEARCH_SINGLE, rc, 0.0, rc, nbins, win, box=boxes, pbc=7, bins=dbins)
    eng.synchronize()
    assert np.array_equal(dbins.cpu().numpy().astype(np.uint64), want)
    hb = eng.search_histogram_frames_f64(a.SEARCH_SINGLE, rc, 0.0, rc, nbins, frames, box=boxes, pbc=7)
    assert np.array_equal(hb, want)


def test_frames_form_two_sets(eng, orc64):
    """SEARCH_DOUBLE frames with `frames2`: the second set's frames from a buffer of their own."""
    import torch
    a = api()
    rng = np.random.default_rng(41)
    n, rc, nbins, nf = 8000, 0.8, 320, 4
    box = synth.box_b(n).astype(np.float64)
    fr1 = np.stack([synth.frame(n, box.astype(np.float32), k).astype(np.float64) for k in range(nf)])
    fr2 = np.stack([synth.frame(n, box.astype(np.float32), 50 + k).astype(np.float64) for k in range(nf)])
    i1 = np.sort(rng.choice(n, 3000, replace=False)).astype(np.uint64)
    i2 = np.sort(rng.choice(n, 2500, replace=False)).astype(np.uint64)
    want = np.zeros(nbins, np.uint64)
    for k in range(nf):
        r = orc64.search_double_pbc(rc, fr1[k][i1.astype(np.int64)], fr2[k][i2.astype(np.int64)], orc64.box_from_matrix(box), 7, nthreads=8)
        want += hist(orc64, 0.0, rc, nbins, r["d"])
    d1, d2 = torch.from_numpy(fr1).cuda(), torch.from_numpy(fr2).cuda()
    dbins = torch.zeros(nbins, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.search_histogram_frames_f64(a.SEARCH_DOUBLE, rc, 0.0, rc, nbins, d1, idx1=i1, box=box, pbc=7, bins=dbins, frames2=d2, idx2=i2)
    eng.synchronize()
    assert np.array_equal(dbins.cpu().numpy().astype(np.uint64), want)


def test_lds_counters_flushed_mid_kernel(eng, orc64, monkeypatch):
    """The overflow guard: a wave that has added more than MOLAR_HIP_HIST64_FLUSH hits since its last flush moves the
    workgroup's LDS counters into the bins while the other waves keep counting.  With a tiny threshold (flushes all the
    time, register and chunk paths) the bins stay the same."""
    a = api()
    n, rc, nbins = 20_000, 1.45, 600
    rng = np.random.default_rng(43)
    box = np.diag([6.0, 6.0, 6.0])
    pos = rng.random((n, 3)) * 6.0
    small = synth.frame(n, synth.box_a(n), 1).astype(np.float64)
    want_big = hist(orc64, 0.0, rc, nbins, ref_dist(orc64, a.SEARCH_SINGLE, rc, pos, box=box))
    want_small = hist(orc64, 0.0, 0.9, 450, ref_dist(orc64, a.SEARCH_SINGLE, 0.9, small, box=synth.box_a(n).astype(np.float64)))
    monkeypatch.setenv("MOLAR_HIP_HIST64_FLUSH", "1000")
    b1, _ = eng.search_histogram_f64(a.SEARCH_SINGLE, rc, 0.0, rc, nbins, pos, box=box, pbc=7)
    b2, _ = eng.search_histogram_f64(a.SEARCH_SINGLE, 0.9, 0.0, 0.9, 450, small, box=synth.box_a(n).astype(np.float64), pbc=7)
    monkeypatch.delenv("MOLAR_HIP_HIST64_FLUSH")
    assert np.array_equal(b1, want_big) and np.array_equal(b2, want_small)


def test_errors_and_the_cached_search(eng):
    """WITHIN, nbins 0 / 8193 and hmin >= hmax are INVALID_ARGUMENT.  A histogram call invalidates the cached f64 search
    (fill_f64 returns NO_SEARCH) and leaves search_f64's results as they were."""
    a = api()
    from molar_amd._lib import MolarHipError
    n = 8000
    box = synth.box_a(n).astype(np.float64)
    pos = synth.frame(n, box.astype(np.float32), 2).astype(np.float64)
    for kind, hmin, hmax, nbins, extra in ((a.SEARCH_WITHIN, 0.0, 0.8, 100, dict(xyz2=pos)), (a.SEARCH_SINGLE, 0.0, 0.8, 0, {}),
                                           (a.SEARCH_SINGLE, 0.0, 0.8, 8193, {}), (a.SEARCH_SINGLE, 0.8, 0.8, 100, {}),
                                           (a.SEARCH_SINGLE, 0.9, 0.8, 100, {})):
        with pytest.raises(MolarHipError) as e:
            eng.search_histogram_f64(kind, 0.8, hmin, hmax, nbins, pos, box=box, pbc=7, **extra)
        assert e.value.code == INVALID_ARGUMENT
    before = eng.search_f64(a.SEARCH_SINGLE, 0.8, pos, box=box, pbc=7)
    eng.search_histogram_f64(a.SEARCH_SINGLE, 0.8, 0.0, 0.8, 100, pos, box=box, pbc=7)
    i = np.empty(len(before[0]), np.uint64); j = np.empty_like(i); d = np.empty(len(i), np.float64)
    rc = eng.lib.molar_hip_search_fill_f64(eng.ctx, i.ctypes.data, j.ctypes.data, d.ctypes.data)
    assert rc == NO_SEARCH
    dims = (C.c_uint64 * 3)()
    assert eng.lib.molar_hip_search_grid_dims_f64(eng.ctx, dims) == NO_SEARCH
    after = eng.search_f64(a.SEARCH_SINGLE, 0.8, pos, box=box, pbc=7)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
