"""`within` as a set, SearchConnectivity and unwrap_connectivity for MolAR's `f64` feature against the oracle's f64 build:
ids, order, offsets and coordinates bit for bit - there is no tolerance anywhere in this file."""
import ctypes as C
import os

import numpy as np
import pytest

from molar_amd import synth

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT, ERR_NO_SEARCH, ERR_NO_PBC = 50, 52, 4
EPS = 2.220446049250313e-16


@pytest.fixture(scope="module")
def eng():
    from molar_amd import build
    from molar_amd.api import Engine
    build.build_library()
    return Engine(0)


@pytest.fixture(scope="module")
def orc64():
    from oracle.oracle import Oracle
    return Oracle("f64")


def boxes(n):
    rd = np.array([[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, np.sqrt(0.5)]])
    rd = rd * ((n / 100.0) / abs(np.linalg.det(rd))) ** (1 / 3)
    return {"ortho": synth.box_ortho(n).astype(np.float64), "tric_a": synth.box_a(n).astype(np.float64),
            "hex_b": synth.box_b(n).astype(np.float64), "rhombic_dodecahedron": rd}


def frame64(n, box32, seed=0):
    """a synthetic frame with digits an f32 frame does not have"""
    pos = synth.frame(n, box32, seed).astype(np.float64)
    return pos + np.random.default_rng(seed + 100).normal(0, 1e-9, pos.shape)


def cuda_ids(k):
    import torch
    return torch.empty(k, dtype=torch.int64, device="cuda")


# ---------------------------------------------------------------------------------------------- 1. set = unique(stream)
@pytest.mark.parametrize("name", ["ortho", "tric_a", "hex_b", "rhombic_dodecahedron"])
def test_set_is_unique_of_the_stream_on_all_boxes(eng, orc64, name):
    import molar_amd.api as a
    n, rc = 2400, 0.55
    box = boxes(n)[name]
    rng = np.random.default_rng(17)
    pos = (rng.random((n, 3)) @ box.T + rng.normal(0, 0.08, (n, 3)))                # f64 coordinates, some outside the cell
    ob = orc64.box_from_matrix(box)
    i1 = np.arange(0, n, 2, dtype=np.uint64); i2 = np.arange(0, n, 40, dtype=np.uint64)
    p1, p2 = pos[i1.astype(int)], pos[i2.astype(int)]
    for pbc in (7, 6, 5, 3, 1):
        stream = orc64.search_within_pbc(rc, p1, p2, ob, pbc, ids1=i1, ids2=i2)["i"]
        want = np.unique(stream)
        got = eng.within_set_f64(rc, pos, i1, pos, i2, box=box, pbc=pbc)
        print(name, "pbc", pbc, "stream", len(stream), "set", len(want), "got", len(got))
        assert got.dtype == np.uint64 and np.array_equal(got, want)
        assert len(stream) > len(want) and 0 < len(want) < len(i1)       # duplicates and non-members are exercised
        assert np.array_equal(got, np.unique(eng.search_f64(a.SEARCH_WITHIN, rc, pos, i1, pos, i2, box=box, pbc=pbc)))
    lo = p1.min(0) - (rc + EPS); up = p1.max(0) + (rc + EPS)
    stream = orc64.search_within(rc, p1, p2, lo, up, ids1=i1, ids2=i2)["i"]
    got = eng.within_set_f64(rc, pos, i1, pos, i2, lower=lo, upper=up)
    print(name, "non-periodic stream", len(stream), "set", len(np.unique(stream)), "got", len(got))
    assert np.array_equal(got, np.unique(stream)) and len(stream) > len(got) > 0
    assert np.array_equal(got, np.unique(eng.search_f64(a.SEARCH_WITHIN, rc, pos, i1, pos, i2, lower=lo, upper=up)))
    # local ids: positions in the selection
    got = eng.within_set_f64(rc, pos, i1, pos, i2, box=box, pbc=7, ids_local=True)
    assert np.array_equal(got, np.unique(orc64.search_within_pbc(rc, p1, p2, ob, 7)["i"]))
    got = eng.within_set_f64(rc, pos, i1, pos, i2, lower=lo, upper=up, ids_local=True)
    assert np.array_equal(got, np.unique(orc64.search_within(rc, p1, p2, lo, up)["i"]))


@pytest.mark.parametrize("name", ["ortho", "tric_a", "hex_b", "rhombic_dodecahedron"])
@pytest.mark.parametrize("rc", [0.8, 1.3, 2.6])
def test_set_on_grids_of_fewer_than_four_cells(eng, orc64, name, rc):
    """Grids with 3, 2 or 1 cells along a dimension: where that dimension is periodic, wrapped entries are not band-classified
    (every candidate goes through PeriodicBox::distance_squared, no row pruning), a cell meets itself across the boundary
    and partners repeat."""
    n = 1500
    box = boxes(n)[name]
    rng = np.random.default_rng(41)
    pos = rng.random((n, 3)) @ box.T + rng.normal(0, 0.08, (n, 3))
    ob = orc64.box_from_matrix(box)
    i1 = np.arange(0, n, 2, dtype=np.uint64); i2 = np.arange(1, n, 150, dtype=np.uint64)
    p1, p2 = pos[i1.astype(int)], pos[i2.astype(int)]
    for pbc in (7, 5, 2):
        ref = orc64.search_within_pbc(rc, p1, p2, ob, pbc, ids1=i1, ids2=i2)
        got = eng.within_set_f64(rc, pos, i1, pos, i2, box=box, pbc=pbc)
        print(name, "rc", rc, "pbc", pbc, "dims", ref["dims"], "stream", len(ref["i"]), "set", len(got))
        assert min(ref["dims"]) < 4
        assert np.array_equal(got, np.unique(ref["i"])) and len(got) > 0


# ---------------------------------------------------------------------------------------------- 2. f64 decides
def test_f64_decides_the_set_where_f32_cannot(eng, orc64):
    """4000 isolated pairs at rc * (1 +- 1e-14 .. 1e-9) in a 60 nm cube: the f64 set is the f64 reference's (grid search AND
    brute force); the f32 set of the rounded coordinates is a different set."""
    rng = np.random.default_rng(3)
    L, rc = 60.0, 0.8
    pa = L * rng.random((4000, 3))
    u = rng.normal(size=(4000, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
    e = 10.0 ** rng.uniform(-14.0, -9.0, 4000) * rng.choice([-1.0, 1.0], 4000)
    pb = pa + rc * (1.0 + e)[:, None] * u
    box = np.diag([L, L, L])
    ob = orc64.box_from_matrix(box)
    got = eng.within_set_f64(rc, pa, None, pb, None, box=box, pbc=7)
    want = np.unique(orc64.search_within_pbc(rc, pa, pb, ob, 7)["i"])
    brute = np.unique(orc64.brute_double(rc, pa, pb, ob, 7)["i"])
    got32 = eng.within_set(rc, pa.astype(np.float32), None, pb.astype(np.float32), None, box=box.astype(np.float32), pbc=7)
    print("f64 set", len(got), "reference", len(want), "brute force", len(brute), "f32 set", len(got32), "differ in", len(np.setxor1d(got, got32)))
    assert np.array_equal(got, want) and np.array_equal(got, brute)
    assert 1000 < len(got) < 3000
    assert len(np.setxor1d(got, got32)) > 1000


@pytest.mark.parametrize("name", ["tric_a", "hex_b"])
def test_isolated_pairs_at_the_cutoff_edge_in_sheared_boxes(eng, orc64, name):
    """The same isolated pairs in boxes of the same volume with sheared cells: a pair straddling a face is decided by the
    set kernel's own copy of the band classification, and nothing else is near enough to hide a wrong decision."""
    rng = np.random.default_rng(5)
    rc = 0.8
    box = boxes(21_600_000)[name]
    pa = rng.random((4000, 3)) @ box.T
    u = rng.normal(size=(4000, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
    e = 10.0 ** rng.uniform(-14.0, -9.0, 4000) * rng.choice([-1.0, 1.0], 4000)
    pb = pa + rc * (1.0 + e)[:, None] * u
    ob = orc64.box_from_matrix(box)
    for pbc in (7, 5):
        got = eng.within_set_f64(rc, pa, None, pb, None, box=box, pbc=pbc)
        want = np.unique(orc64.search_within_pbc(rc, pa, pb, ob, pbc)["i"])
        print(name, "pbc", pbc, "set", len(want), "got", len(got))
        assert np.array_equal(got, want) and 1000 < len(want) < 3000
    inside = np.unique(orc64.search_within_pbc(rc, pa, pb, ob, 0)["i"])
    assert len(inside) < len(np.unique(orc64.search_within_pbc(rc, pa, pb, ob, 7)["i"]))       # pairs do straddle the faces


# ---------------------------------------------------------------------------------------------- 3. across the boundary
@pytest.mark.parametrize("name", ["ortho", "tric_a", "hex_b"])
def test_set_across_the_periodic_boundary_at_the_cutoff_edge(eng, orc64, name):
    """First atoms near a cell face, partners at rc * (1 +- 1e-15 .. 1e-8): the band classification of wrapped entries decides.
    Coordinates and selections resident in HBM, the set left there."""
    import torch
    rng = np.random.default_rng(23)
    n = 30_000
    box = boxes(n)[name]
    rc = 0.7
    ob = orc64.box_from_matrix(box)
    npairs = 6000
    frac = rng.random((npairs, 3))
    dim = rng.integers(0, 3, npairs)
    frac[np.arange(npairs), dim] = rng.choice([0.0, 1.0], npairs) + rng.normal(0, 0.01, npairs)
    pa = frac @ box.T
    u = rng.normal(size=(npairs, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
    e = 10.0 ** rng.uniform(-15.5, -8.0, npairs) * rng.choice([-1.0, 1.0], npairs)
    pb = pa + rc * (1.0 + e)[:, None] * u
    pos = np.concatenate([pa, pb, rng.random((n - 2 * npairs, 3)) @ box.T])
    i1 = np.arange(npairs, dtype=np.uint64); i2 = np.arange(npairs, 2 * npairs, dtype=np.uint64)
    dpos = torch.from_numpy(pos).cuda()
    d1, d2 = torch.from_numpy(i1.astype(np.int64)).cuda(), torch.from_numpy(i2.astype(np.int64)).cuda()
    for pbc in (7, 3):
        ref = orc64.search_within_pbc(rc, pa, pb, ob, pbc, ids1=i1, ids2=i2)
        assert min(ref["dims"]) >= 4
        want = np.unique(ref["i"])
        got = eng.within_set_f64(rc, dpos, d1, dpos, d2, box=box, pbc=pbc, device_out=cuda_ids)
        assert got.is_cuda and got.dtype == torch.int64
        got = got.cpu().numpy().view(np.uint64)
        print(name, "pbc", pbc, "set", len(want), "got", len(got))
        assert np.array_equal(got, want) and len(want) > 1000
    # the same first atoms against everything else
    i3 = np.arange(npairs, n, dtype=np.uint64)
    want = np.unique(orc64.search_within_pbc(rc, pa, pos[npairs:], ob, 7, ids1=i1, ids2=i3)["i"])
    assert np.array_equal(eng.within_set_f64(rc, dpos, d1, pos, i3, box=box, pbc=7), want)


# ---------------------------------------------------------------------------------------------- 4. cell sizes
def test_set_with_cells_of_more_than_256_atoms(eng, orc64):
    rng = np.random.default_rng(31)
    n, rc = 30_000, 1.6
    L = (n / 100.0) ** (1 / 3)                      # density 100 / nm^3: 4 x 4 x 4 cells of about 470 atoms
    box = np.diag([L, L, L])
    pos = rng.random((n, 3)) * L + rng.normal(0, 0.05, (n, 3))
    ob = orc64.box_from_matrix(box)
    i1 = np.arange(0, n, 8, dtype=np.uint64)
    i2 = np.setdiff1d(np.arange(n, dtype=np.uint64), i1)
    ref = orc64.search_within_pbc(rc, pos[i1.astype(int)], pos[i2.astype(int)], ob, 7, ids1=i1, ids2=i2, nthreads=8)
    assert tuple(ref["dims"]) == (4, 4, 4)
    assert np.array_equal(eng.within_set_f64(rc, pos, i1, pos, i2, box=box, pbc=7), np.unique(ref["i"]))
    # the same crowded cells without a box
    p1 = pos[i1.astype(int)]
    lo = p1.min(0) - (rc + EPS); up = p1.max(0) + (rc + EPS)
    ref = orc64.search_within(rc, p1, pos[i2.astype(int)], lo, up, ids1=i1, ids2=i2, nthreads=8)
    assert np.array_equal(eng.within_set_f64(rc, pos, i1, pos, i2, lower=lo, upper=up), np.unique(ref["i"]))


def test_set_around_a_20_atom_selection_and_of_a_selection_with_itself(eng, orc64):
    n, rc = 100_000, 0.8
    b32 = synth.box_a(n)
    box = b32.astype(np.float64)
    pos = frame64(n, b32, 5)
    ob = orc64.box_from_matrix(box)
    inner = np.arange(40_000, 40_020, dtype=np.uint64)
    want = np.unique(orc64.search_within_pbc(rc, pos, pos[inner.astype(int)], ob, 7, ids2=inner, nthreads=8)["i"])
    got = eng.within_set_f64(rc, pos, None, pos, inner, box=box, pbc=7)
    print("within 0.8 of 20 atoms:", len(got))
    assert np.array_equal(got, want) and 20 <= len(got) < 5000
    # the inner selection is the whole outer one: every atom finds itself
    sel = np.sort(np.random.default_rng(1).choice(n, 6000, replace=False)).astype(np.uint64)
    got = eng.within_set_f64(0.5, pos, sel, pos, sel, box=box, pbc=7)
    want = np.unique(orc64.search_within_pbc(0.5, pos[sel.astype(int)], pos[sel.astype(int)], ob, 7, ids1=sel, ids2=sel)["i"])
    assert np.array_equal(got, want) and np.array_equal(got, sel)


# ---------------------------------------------------------------------------------------------- 5. edges and state
def test_set_edges_and_context_state(eng, orc64):
    import molar_amd.api as a
    from molar_amd._lib import MolarHipError
    n, rc = 4000, 0.5
    b32 = synth.box_b(n)
    box = b32.astype(np.float64)
    pos = frame64(n, b32, 2)
    ob = orc64.box_from_matrix(box)
    rng = np.random.default_rng(9)
    # empty second set: count 0, nothing to fill
    got = eng.within_set_f64(rc, pos, None, pos, np.zeros(0, np.uint64), box=box, pbc=7)
    assert got.dtype == np.uint64 and len(got) == 0
    assert eng.lib.molar_hip_within_fill_f64(eng.ctx, None) == 0
    # no atom of the second set within the cutoff of any of the first
    g = np.stack(np.meshgrid(np.arange(5.0), np.arange(5.0), np.arange(4.0), indexing="ij"), -1).reshape(-1, 3)
    cube = np.diag([5.0, 5.0, 4.0])
    assert len(orc64.search_within_pbc(0.3, g + 0.25, g + 0.75, orc64.box_from_matrix(cube), 7)["i"]) == 0
    assert len(eng.within_set_f64(0.3, g + 0.25, None, g + 0.75, None, box=cube, pbc=7)) == 0
    assert eng.lib.molar_hip_within_fill_f64(eng.ctx, None) == 0
    # every outer atom found
    got = eng.within_set_f64(1.2, pos, None, pos[::3], None, box=box, pbc=7)
    assert np.array_equal(got, np.arange(n, dtype=np.uint64))
    assert np.array_equal(got, np.unique(orc64.search_within_pbc(1.2, pos, pos[::3], ob, 7)["i"]))
    # selections with global ids
    s1 = np.sort(rng.choice(n, 1500, replace=False)).astype(np.uint64)
    s2 = np.sort(rng.choice(n, 300, replace=False)).astype(np.uint64)
    want = np.unique(orc64.search_within_pbc(rc, pos[s1.astype(int)], pos[s2.astype(int)], ob, 7, ids1=s1, ids2=s2)["i"])
    got = eng.within_set_f64(rc, pos, s1, pos, s2, box=box, pbc=7)
    assert np.array_equal(got, want) and 0 < len(got) < len(s1)
    # the set call leaves no cached f64 search behind; the next search is exact again
    ids = np.zeros(n, np.uint64)
    assert eng.lib.molar_hip_search_fill_ids_f64(eng.ctx, ids.ctypes.data) == ERR_NO_SEARCH
    d = np.zeros(n)
    assert eng.lib.molar_hip_search_fill_f64(eng.ctx, ids.ctypes.data, ids.ctypes.data, d.ctypes.data) == ERR_NO_SEARCH
    dims = (C.c_uint64 * 3)()
    assert eng.lib.molar_hip_search_grid_dims_f64(eng.ctx, dims) == ERR_NO_SEARCH
    ref = orc64.search_single_pbc(rc, pos, ob, 7)
    i, j, dist = eng.search_f64(a.SEARCH_SINGLE, rc, pos, box=box, pbc=7)
    assert np.array_equal(i, ref["i"]) and np.array_equal(j, ref["j"]) and np.array_equal(dist, ref["d"])
    # ... and a search in between ends the cached set
    assert eng.lib.molar_hip_within_fill_f64(eng.ctx, ids.ctypes.data) == ERR_NO_SEARCH
    # twice on one context with different sizes
    big = eng.within_set_f64(0.9, pos, None, pos, s2, box=box, pbc=7)
    small = eng.within_set_f64(0.3, pos[:500], None, pos, s2[:20], box=box, pbc=7)
    assert np.array_equal(big, np.unique(orc64.search_within_pbc(0.9, pos, pos[s2.astype(int)], ob, 7)["i"]))
    assert np.array_equal(small, np.unique(orc64.search_within_pbc(0.3, pos[:500], pos[s2[:20].astype(int)], ob, 7)["i"]))
    assert len(big) > len(small)
    # kind and bounds are checked
    with pytest.raises(MolarHipError):
        eng.within_set_f64(rc, pos, None, pos, s2)                                 # non-periodic needs lower / upper
    desc, keep = a._search_desc_f64(a.SEARCH_DOUBLE, rc, pos, None, pos, s2, box, 7)
    cnt = C.c_uint64(0)
    assert eng.lib.molar_hip_within_count_f64(eng.ctx, C.byref(desc), C.byref(cnt)) == ERR_INVALID_ARGUMENT
    bad = s1.copy(); bad[5] = n + 3
    with pytest.raises(MolarHipError):
        eng.within_set_f64(rc, pos, bad, pos, s2, box=box, pbc=7)


# ---------------------------------------------------------------------------------------------- 6. connectivity
def csr_in_push_order(ref, rows):
    """SearchConnectivity::from_iter (connectivity.rs:19-35): pair p pushes j onto i's list (entry 2p), i onto j's (2p + 1)"""
    npairs = len(ref["i"])
    row = np.empty(2 * npairs, np.uint64); nb = np.empty(2 * npairs, np.uint64)
    row[0::2], row[1::2] = ref["i"], ref["j"]
    nb[0::2], nb[1::2] = ref["j"], ref["i"]
    order = np.argsort(row, kind="stable")
    off = np.searchsorted(row[order], np.arange(rows + 1, dtype=np.uint64)).astype(np.uint64)
    return off, nb[order]


def test_connectivity_csr_in_push_order(eng, orc64):
    import molar_amd.api as a
    n, rc = 3000, 0.35
    b32 = synth.box_a(n)
    box = b32.astype(np.float64)
    pos = frame64(n, b32, 1)
    ob = orc64.box_from_matrix(box)
    ref = orc64.search_single_pbc(rc, pos, ob, 7)
    print("pairs", len(ref["i"]))
    assert len(ref["i"]) > 10_000
    off, nb = eng.search_connectivity_f64(rc, pos, box=box, pbc=7)
    woff, wnb = csr_in_push_order(ref, n)
    assert off.dtype == np.uint64 and nb.dtype == np.uint64
    assert len(off) == n + 1 and off[0] == 0 and off[-1] == 2 * len(ref["i"]) == len(nb)
    assert np.array_equal(off, woff) and np.array_equal(nb, wnb)
    # a selection: local ids (rows = its length) and global ids (rows = natoms; atoms outside it have empty lists)
    sel = np.sort(np.random.default_rng(n).choice(n, n // 2, replace=False)).astype(np.uint64)
    ref = orc64.search_single_pbc(0.5, pos[sel.astype(int)], ob, 7)
    off, nb = eng.search_connectivity_f64(0.5, pos, sel, box=box, pbc=7, ids_local=True)
    woff, wnb = csr_in_push_order(ref, len(sel))
    assert len(off) == len(sel) + 1 and np.array_equal(off, woff) and np.array_equal(nb, wnb)
    ref = orc64.search_single_pbc(0.5, pos[sel.astype(int)], ob, 7, ids=sel)
    off, nb = eng.search_connectivity_f64(0.5, pos, sel, box=box, pbc=7, ids_local=False)
    woff, wnb = csr_in_push_order(ref, n)
    assert len(off) == n + 1 and np.array_equal(off, woff) and np.array_equal(nb, wnb)
    outside = np.setdiff1d(np.arange(n), sel.astype(int))
    assert np.all(off[outside + 1] == off[outside]) and len(nb) > 0
    # non-periodic
    ref = orc64.search_single(rc, pos)
    off, nb = eng.search_connectivity_f64(rc, pos)
    woff, wnb = csr_in_push_order(ref, n)
    assert np.array_equal(off, woff) and np.array_equal(nb, wnb)
    # only a single-selection search has one id range
    desc, keep = a._search_desc_f64(a.SEARCH_DOUBLE, rc, pos, None, pos, None, box, 7)
    rows, ent = C.c_uint64(0), C.c_uint64(0)
    assert eng.lib.molar_hip_search_connectivity_f64(eng.ctx, C.byref(desc), C.byref(rows), C.byref(ent)) == ERR_INVALID_ARGUMENT
    desc, keep = a._search_desc_f64(a.SEARCH_WITHIN, rc, pos, None, pos, None, box, 7)
    assert eng.lib.molar_hip_search_connectivity_f64(eng.ctx, C.byref(desc), C.byref(rows), C.byref(ent)) == ERR_INVALID_ARGUMENT


def test_connectivity_with_lists_of_several_hundred_entries(eng, orc64):
    n, rc = 25_000, 1.0
    b32 = synth.box_a(n)
    box = b32.astype(np.float64)
    pos = frame64(n, b32, 4)
    ref = orc64.search_single_pbc(rc, pos, orc64.box_from_matrix(box), 7, nthreads=8)
    off, nb = eng.search_connectivity_f64(rc, pos, box=box, pbc=7)
    woff, wnb = csr_in_push_order(ref, n)
    print("entries", len(nb), "longest list", int(np.diff(woff.astype(np.int64)).max()))
    assert int(np.diff(woff.astype(np.int64)).max()) > 300
    assert np.array_equal(off, woff) and np.array_equal(nb, wnb)


# ---------------------------------------------------------------------------------------------- 7. unwrap
def wrapped_chains(orc64):
    rng = np.random.default_rng(7)
    box = np.array([[4.0, 1.0, 0.5], [0.0, 4.0, -0.7], [0.0, 0.0, 4.0]])       # columns a, b, c
    ob = orc64.box_from_matrix(box)
    beads = []
    for c in range(40):
        p = box @ rng.random(3)
        beads.append(p)
        for k in range(1, 40):
            d = rng.normal(size=3); d /= np.linalg.norm(d)
            p = p + 0.15 * d
            beads.append(p)
    whole = np.array(beads)
    wrapped = np.array([orc64.wrap_point(ob, p) for p in whole], np.float64)
    return box, ob, np.ascontiguousarray(wrapped)


def same_groups(got, ref):
    return len(got) == len(ref) and all(np.array_equal(x, y) for x, y in zip(got, ref))


def test_unwrap_connectivity_chains_in_a_triclinic_box(eng, orc64):
    import torch
    from molar_amd.api import MeasureF64
    from molar_amd._lib import MolarHipError
    m = MeasureF64(eng)
    box, ob, wrapped = wrapped_chains(orc64)
    sel = np.concatenate([np.arange(40 * c, 40 * (c + 1)) for c in range(0, 40, 2)]).astype(np.uint64)
    for dims, idx in ((7, None), (3, None), (7, sel)):
        ref, rgroups = orc64.unwrap_connectivity(wrapped, ob, 0.2, dims, idx=idx)
        got = wrapped.copy()
        groups = m.unwrap_connectivity(got, box, 0.2, dims, idx=idx)
        moved = int(np.any(ref != wrapped, axis=1).sum())
        print("dims", dims, "selection", idx is not None, "groups", len(rgroups), "moved", moved)
        assert got.dtype == np.float64 and np.array_equal(got, ref)
        assert same_groups(groups, rgroups)
        assert len(rgroups) > 1 and moved > 100
    ref, rgroups = orc64.unwrap_connectivity(wrapped, ob, 0.2, 7)
    dgot = torch.from_numpy(wrapped.copy()).cuda()
    torch.cuda.synchronize()
    g2 = m.unwrap_connectivity(dgot, box, 0.2, 7)
    assert np.array_equal(dgot.cpu().numpy(), ref) and same_groups(g2, rgroups)
    # an f32 unwrap of the rounded frame is not this result
    got32 = wrapped.astype(np.float32)
    eng.unwrap_connectivity(got32, box.astype(np.float32), 0.2, 7)
    assert not np.array_equal(got32.astype(np.float64), ref)
    with pytest.raises(MolarHipError) as err:
        m.unwrap_connectivity(wrapped.copy(), None, 0.2, 7)
    assert err.value.code == ERR_NO_PBC


def test_unwrap_connectivity_f64_100k_atoms_against_the_oracle_entry(eng, orc64):
    """The helix system of the f32 suite built in float64: 2000 molecules of 60 atoms wrapped into a triclinic box."""
    from molar_amd.api import MeasureF64
    m = MeasureF64(eng)
    rng = np.random.default_rng(11)
    nx, ny, nz, length = 13, 13, 12, 60
    nmol = nx * ny * nz - 28
    box = np.diag([nx * 2.4, ny * 2.4, nz * 3.6])
    box[0, 2] = -2.0; box[1, 2] = -1.5
    k = np.arange(length)
    th = np.deg2rad(27.0) * k
    helix = np.stack([0.3 * np.cos(th), 0.3 * np.sin(th), 0.05 * k], 1)
    parts = []
    for mol in range(nmol):
        cx, cy, cz = mol % nx, (mol // nx) % ny, mol // (nx * ny)
        rot = rng.uniform(0, 2 * np.pi)
        R = np.array([[np.cos(rot), -np.sin(rot), 0], [np.sin(rot), np.cos(rot), 0], [0, 0, 1.0]])
        parts.append(helix @ R.T + np.array([cx * 2.4 + 1.2, cy * 2.4 + 1.2, cz * 3.6 + 0.3]) + rng.normal(0, 0.005, (length, 3)))
    whole = np.concatenate(parts) + np.array([0.9, 1.1, 1.7])
    fr = whole @ np.linalg.inv(box).T
    wrapped = np.ascontiguousarray((fr - np.floor(fr)) @ box.T)
    n = len(wrapped)
    assert n >= 100_000 and wrapped.dtype == np.float64
    ob = orc64.box_from_matrix(box)
    ref, rgroups = orc64.unwrap_connectivity(wrapped, ob, 0.17, 7, nthreads=min(os.cpu_count() or 4, 16))
    assert len(rgroups) >= 1000
    split = sum(1 for mol in range(nmol) if np.abs(np.diff(wrapped[mol * length:(mol + 1) * length], axis=0)).max() > 1.0)
    assert split > 200
    got = wrapped.copy()
    groups = m.unwrap_connectivity(got, box, 0.17, 7)
    assert np.array_equal(got, ref) and same_groups(groups, rgroups)
    idx = np.concatenate([np.arange(mol * length, (mol + 1) * length) for mol in range(0, nmol, 2)]).astype(np.uint64)
    ref3, rg3 = orc64.unwrap_connectivity(wrapped, ob, 0.17, 3, idx=idx, nthreads=min(os.cpu_count() or 4, 16))
    got3 = wrapped.copy()
    g3 = m.unwrap_connectivity(got3, box, 0.17, 3, idx=idx)
    assert np.array_equal(got3, ref3) and same_groups(g3, rg3)
