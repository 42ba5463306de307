"""Slots cut from the LIVE rows of a plan entry (live_rows_kernel -> plan_tiles_kernel -> the regular count / fill kernels).

Every case is the oracle's ordered list bit for bit - ids, order, distance bits - as in test_gpu_search.py, and every case asks
molar_hip_search_slot_counts how the plan was cut, so that it cannot pass with the path silently off: strictly fewer slots than
consecutive rows would have given where rows are pruned, the same number where the case is built for none.
"""
import numpy as np
import pytest

from molar_amd import synth

pytestmark = pytest.mark.gpu

RC = 1.2


@pytest.fixture(scope="module")
def a():
    from molar_amd import build
    import molar_amd.api as api
    build.build_library()
    return api


@pytest.fixture(scope="module")
def eng(a):
    return a.Engine(0)


@pytest.fixture(scope="module")
def frame20k():
    """Box A at 20 000 atoms: grid 4 x 4 x 4 at 1.2 nm, ~310 atoms per cell (five row groups per entry), band classification on."""
    n = 20000
    box = synth.box_a(n)
    return n, box, synth.frame(n, box, sigma=0.08)


def same(pairs, d, ref):
    assert len(pairs) == len(ref["i"]) > 0, (len(pairs), len(ref["i"]))
    assert np.array_equal(pairs[:, 0].astype(np.uint64), ref["i"])
    assert np.array_equal(pairs[:, 1].astype(np.uint64), ref["j"])
    assert np.array_equal(d, ref["d"])


def count_fill(a, e, kind, rc, *args, **kw):
    cnt = e.search_count(kind, rc, *args, **kw)
    slots = e.search_slot_counts()
    pairs, d = e.search_fill(cnt)
    return pairs, d, slots


@pytest.mark.parametrize("pbc", [7, 3, 0, None])
def test_single_box_a_every_entry_class(a, eng, orc32, frame20k, pbc):
    """Plain, same-cell, band-classified wrapped (matrix-core count with history, replayed by the fill) and triclinic corner
    entries in one frame; pbc None = the same atoms without a box."""
    n, box, pos = frame20k
    if pbc is None:
        ref = orc32.search_single(RC, pos, nthreads=4)
        pairs, d, (slots, rows) = count_fill(a, eng, a.SEARCH_SINGLE, RC, pos)
    else:
        ref = orc32.search_single_pbc(RC, pos, orc32.box_from_matrix(box), pbc, nthreads=4)
        pairs, d, (slots, rows) = count_fill(a, eng, a.SEARCH_SINGLE, RC, pos, box=box, pbc=pbc)
        assert eng.grid_dims() == (4, 4, 4)
    assert eng.search_cell_kernels()[0] == 0
    same(pairs, d, ref)
    print("slots", slots, "of", rows)
    assert 0 < slots < rows, (slots, rows)


@pytest.mark.parametrize("overlap", [False, True])
def test_double_box_a(a, eng, orc32, frame20k, overlap):
    n, box, pos = frame20k
    i1 = np.arange(0, n // 2 if not overlap else (3 * n) // 5, dtype=np.uint64)
    i2 = np.arange(n // 2 if not overlap else (2 * n) // 5, n, dtype=np.uint64)
    ref = orc32.search_double_pbc(RC, pos[i1.astype(int)], pos[i2.astype(int)], orc32.box_from_matrix(box), 7, ids1=i1, ids2=i2, nthreads=4)
    pairs, d, (slots, rows) = count_fill(a, eng, a.SEARCH_DOUBLE, RC, pos, i1, pos, i2, box=box, pbc=7)
    assert eng.search_cell_kernels()[0] == 0
    same(pairs, d, ref)
    assert 0 < slots < rows, (slots, rows)


def test_wrapped_entries_evaluated_exactly_keep_consecutive_slots(a, eng, orc32):
    """Box A at 6 000 atoms, grid 3 x 3 x 3 (at a cutoff of 1.0 nm; 1.2 nm gives 2 x 2 x 3 under the box's shear): fewer than four
    cells per periodic dimension, so wrapped entries are evaluated exactly and prune nothing.  The plain entries of the same grid are what pbc 0 leaves (atoms strictly inside the box, so
    the cells hold the same atoms either way): the difference of the two plans is the wrapped entries' share, and it must be
    the same number of slots as consecutive rows give."""
    n = 6000
    box = synth.box_a(n)
    pos = synth.frame(n, box, sigma=0.0)
    ob = orc32.box_from_matrix(box)
    got = {}
    for pbc in (7, 0):
        ref = orc32.search_single_pbc(1.0, pos, ob, pbc, nthreads=4)
        pairs, d, got[pbc] = count_fill(a, eng, a.SEARCH_SINGLE, 1.0, pos, box=box, pbc=pbc)
        assert eng.grid_dims() == (3, 3, 3) and eng.search_cell_kernels()[0] == 0
        same(pairs, d, ref)
    (s7, r7), (s0, r0) = got[7], got[0]
    assert 0 < s0 < r0, (s0, r0)                      # plain entries are pruned ...
    assert s7 - s0 == r7 - r0 > 0, (got[7], got[0])   # ... the wrapped ones are not


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_input_order_along_x(a, eng, orc32, frame20k, order):
    """Atoms sorted by x: inside a cell the live rows of an entry then sit all in its last or its first row groups, and whole
    groups are empty."""
    n, box, pos = frame20k
    o = np.argsort(pos[:, 0], kind="stable")
    pos = np.ascontiguousarray(pos[o if order == "ascending" else o[::-1]])
    ref = orc32.search_single_pbc(RC, pos, orc32.box_from_matrix(box), 7, nthreads=4)
    pairs, d, (slots, rows) = count_fill(a, eng, a.SEARCH_SINGLE, RC, pos, box=box, pbc=7)
    same(pairs, d, ref)
    assert 0 < slots < rows, (slots, rows)


def two_cell_frame(m):
    """No box, cutoff 1: the bounding box starts at the origin and is padded by the cutoff, so the grid is 3 x 2 x 2 with cells
    of 1.2 nm along x from -1 (boundaries at 0.2 and 1.4) and of 1.31 nm along y and z (boundary at 0.31).  The cell at x = 1
    holds 200 atoms at x in [0.25, 1.35], its neighbour 100 at x in [1.5, 1.6] that span the first cell's y and z range, so a
    row of the first cell is live exactly when 1.5 - x <= 1: m atoms at x >= 0.51, the others at x <= 0.49, interleaved in
    input order."""
    rng = np.random.default_rng(100 + m)
    na, nb = 200, 100
    live = np.zeros(na, bool)
    live[np.linspace(0, na - 1, m).round().astype(int)] = True
    assert live.sum() == m
    xa = np.where(live, rng.uniform(0.51, 1.35, na), rng.uniform(0.25, 0.49, na))
    A = np.stack([xa, rng.uniform(0.602, 0.618, na), rng.uniform(0.602, 0.618, na)], 1)
    B = np.stack([rng.uniform(1.5, 1.6, nb), rng.uniform(0.6, 0.62, nb), rng.uniform(0.6, 0.62, nb)], 1)
    B[0] = (1.5, 0.6, 0.6)
    B[1] = (1.6, 0.62, 0.62)
    pos = np.concatenate([A, B]).astype(np.float32)
    # the f32 predicate of the kernels on this construction, with its margin of 1e-3
    lo, hi = pos[na:].min(0), pos[na:].max(0)
    e = np.maximum(np.maximum(lo - pos[:na], pos[:na] - hi), np.float32(0))
    d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    assert d2.dtype == np.float32 and np.array_equal(d2 <= np.float32(1.0), live)
    assert np.all(np.abs(np.sqrt(d2.astype(np.float64)) - 1.0) >= 1.0e-3)
    return pos, na, nb


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 128])
def test_live_count_at_the_slot_edge(a, eng, orc32, m):
    pos, na, nb = two_cell_frame(m)
    ref = orc32.search_single(1.0, pos, nthreads=2)
    assert ref["dims"] == (3, 2, 2)
    pairs, d, (slots, rows) = count_fill(a, eng, a.SEARCH_SINGLE, 1.0, pos)
    assert eng.grid_dims() == (3, 2, 2) and eng.search_cell_kernels()[0] == 0
    same(pairs, d, ref)
    cross = int(np.sum((ref["i"] < na) != (ref["j"] < na)))
    assert (cross > 0) == (m > 0)
    # the two same-cell entries keep consecutive slots (4 + 2); the entry (cell 1, cell 2) has ceil(m / 64) - none for m = 0
    assert rows == 4 + 2 + 4 and slots == 4 + 2 + (m + 63) // 64, (m, slots, rows)


class _Dev:
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def _fetch(res):
    import torch
    cnt, pp, dp = res
    pairs = torch.as_tensor(_Dev(pp, cnt * 2, "<i4"), device="cuda").cpu().numpy().view(np.uint32).reshape(-1, 2)
    dist = None if dp is None else torch.as_tensor(_Dev(dp, cnt, "<f4"), device="cuda").cpu().numpy()
    return pairs, dist


def test_two_frames_in_flight(a, frame20k):
    """search_resident_begin / _end over A, B, A, B - the frame and its x-sorted copy, which differ in every mask - on a fresh
    context (the first frames also outgrow the buffers and are repeated): each result equals the synchronous one, which
    masks read from the other grid generation would not."""
    import torch
    n, box, pos = frame20k
    frames = [pos, np.ascontiguousarray(pos[np.argsort(pos[:, 0], kind="stable")])]
    e1, e2 = a.Engine(0), a.Engine(0)
    want = []
    for f in frames:
        cnt = e1.search_count(a.SEARCH_SINGLE, RC, f, box=box, pbc=7)
        want.append(e1.search_fill(cnt))
    dev = [torch.from_numpy(f).cuda() for f in frames]
    descs = [e2.make_search_desc(a.SEARCH_SINGLE, RC, f, box=box, pbc=7) for f in dev]
    seq, prev = [0, 1, 0, 1, 1, 0], None

    def check(k, res):
        pairs, dist = _fetch(res)
        assert np.array_equal(pairs, want[k][0]) and np.array_equal(dist, want[k][1]), k

    for k in seq:
        t = e2.search_resident_begin(descs[k][0])
        if prev is not None:
            check(prev[0], e2.search_resident_end(prev[1]))
        prev = (k, t)
    check(prev[0], e2.search_resident_end(prev[1]))
    slots, rows = e2.search_slot_counts()
    assert 0 < slots < rows


def test_pairs_only_plane_and_first_search_of_a_context(a, orc32, frame20k):
    """A fresh context: the hit history of the first regular search does not fit, the host grows it and the passes repeat -
    over the same live-ranked slots.  Then the (i, j)-only plane."""
    n, box, pos = frame20k
    ref = orc32.search_single_pbc(RC, pos, orc32.box_from_matrix(box), 7, nthreads=4)
    e = a.Engine(0)
    res = e.search_resident(a.SEARCH_SINGLE, RC, pos, box=box, pbc=7)
    pairs, dist = _fetch(res)
    same(pairs, dist, ref)
    slots, rows = e.search_slot_counts()
    assert 0 < slots < rows
    e.search_resident_planes(False)
    res = e.search_resident(a.SEARCH_SINGLE, RC, pos, box=box, pbc=7)
    assert res[2] is None
    pairs, _ = _fetch(res)
    assert np.array_equal(pairs[:, 0].astype(np.uint64), ref["i"]) and np.array_equal(pairs[:, 1].astype(np.uint64), ref["j"])
    e.search_resident_planes(True)


def test_slab_that_switches_kernel_family(a, orc32):
    """A slab in a mostly empty box: the first searches go by the mean population (small-cell kernels), later ones by the
    occupied cells (regular kernels); both keep consecutive slots - the liveness kernel's cost goes with all cells of the grid,
    so the rule asks 96 atoms per cell over ALL of them - and every frame is the oracle's list."""
    e = a.Engine(0)
    rng = np.random.default_rng(5)
    L, H, thick, rc = 6.0, 24.0, 2.7, 0.9
    n = int(L * L * thick * 100)
    box = np.diag([L, L, H]).astype(np.float32)
    ob = orc32.box_from_matrix(box)
    lanes, cut = [], []
    for f in range(3):
        pos = (rng.random((n, 3)) * np.array([L, L, thick]) + np.array([0, 0, 0.5 * (H - thick)])).astype(np.float32)
        ref = orc32.search_single_pbc(rc, pos, ob, 7, nthreads=4)
        res = e.search_resident(a.SEARCH_SINGLE, rc, pos, box=box, pbc=7)
        pairs, dist = _fetch(res)
        same(pairs, dist, ref)
        lanes.append(e.search_cell_kernels()[0])
        cut.append(e.search_slot_counts())
    assert lanes[0] in (16, 32) and lanes[-1] == 0, lanes
    assert all(s == r > 0 for s, r in cut), cut
