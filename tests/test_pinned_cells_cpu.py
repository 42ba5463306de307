"""The frames of tests/pinned_cells.py on the reference alone: what makes the cases of tests/test_gpu_contacts_pinned.py and
tests/test_gpu_clusters_pinned.py worth comparing.  For every frame those tests use: the oracle's grid is the intended one, the
population of every cell (fractional binning with the oracle's dims) is the table asked for, and the pair list is not empty; the
label runs, the cell pairs of the two-set cases, the home cells of the two-rows-per-slot cases and the component counts are what
the cases are named after.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clusters_ref as cl  # noqa: E402
import contacts_ref as cr  # noqa: E402
import pinned_cells as pc  # noqa: E402
from test_contacts_cpu import brute_pairs  # noqa: E402

RC = pc.CUTOFF


def oracle_single(orc32, pos, box, pbc):
    return orc32.search_single_pbc(RC, pos, orc32.box_from_matrix(box), pbc, nthreads=4)


def pinned(orc32, pos, box, pops, dims, pbc, pos2=None):
    """dims, populations, a non-empty list; returns the list"""
    ob = orc32.box_from_matrix(box)
    ref = orc32.search_single_pbc(RC, pos, ob, pbc, nthreads=4) if pos2 is None else orc32.search_double_pbc(RC, pos, pos2, ob, pbc, nthreads=4)
    assert ref["dims"] == tuple(dims)
    assert np.array_equal(pc.binned(pos, box, ref["dims"]), pops)
    assert len(ref["i"]) > 0
    return ref


# ---------------------------------------------------------------- the generator

def test_grids_of_the_reference(orc32):
    """dims = floor(L / cutoff) for the orthorhombic boxes; the triclinic one from a probe frame"""
    rng = np.random.default_rng(0)
    for dims, edge in (((4, 4, 4), 1.02), ((3, 3, 3), 1.3), ((4, 4, 4), 1.24), ((5, 5, 5), 1.04)):
        box = pc.ortho_box(dims, RC, edge)
        pos = pc.frame(box, dims, np.full(pc.ncells(dims), 2), rng)[0]
        assert oracle_single(orc32, pos, box, 7)["dims"] == dims
    box = pc.tric_box()
    ob = orc32.box_from_matrix(box)
    assert ob.nshift != 0                                   # lattice shifts: the entries that wrap in x, y and z get 2 rows per slot
    probe = (rng.random((200, 3)) @ box.astype(np.float64).T).astype(np.float32)
    assert orc32.search_single_pbc(RC, probe, ob, 7)["dims"] == pc.TRIC_DIMS


@pytest.mark.parametrize("order", pc.ORDERS)
@pytest.mark.parametrize("variant", list(pc.VARIANTS))
def test_edge_frames(orc32, variant, order):
    pos, box, pops, cell, dims, pbc = pc.edge_frame(variant, order=order)
    ref = pinned(orc32, pos, box, pops, dims, pbc)
    assert set(pops.tolist()) == set(pc.EDGE_TABLE)           # every table value realised exactly
    assert np.array_equal(pc.cell_of(pos, box, dims), cell)
    if order == "cell_major":
        assert np.all(np.diff(cell) >= 0)
    if variant == "ortho7":
        assert len(pos) == 5944 and pos.dtype == np.float32
    # same-cell entries at every size, second cells of up to four chunks: pairs inside one cell exist for the crowded cells
    i, j = cell[ref["i"].astype(np.int64)], cell[ref["j"].astype(np.int64)]
    same = np.bincount(i[i == j], minlength=len(pops))
    assert np.all(same[pops >= 62] > 0)


def test_crowded_reference_is_the_brute_force(orc32, monkeypatch):
    """contacts_ref.single over the oracle's list of a pinned frame against the O(N^2) minimum image (test_contacts_cpu.brute_pairs);
    a (4, 4, 4) grid with one cell each of 62 .. 66, 127 and 129 atoms among cells of 0 .. 3 (some 700 atoms: the number of pairs
    closer to the cutoff than brute_pairs allows grows with the square of it)"""
    import test_contacts_cpu as tc
    monkeypatch.setattr(tc, "CUTOFF", RC)
    dims = (4, 4, 4)
    box = pc.ortho_box(dims)
    rng = np.random.default_rng(8)
    pops = np.resize((0, 1, 2, 3), 64)
    pops[:7] = (62, 63, 64, 65, 66, 127, 129)
    pops = rng.permutation(pops)
    pos = pc.frame(box, dims, pops, rng)[0]
    n = len(pos)
    ref = pinned(orc32, pos, box, pops, dims, 7)
    g = (np.arange(n) // 3).astype(np.uint32)
    G = int(g.max()) + 1
    count, deg, m = cr.single(ref, n, g, G)
    bi, bj = brute_pairs(pos, pos, float(box[0, 0]), True)
    assert count == len(bi) > 0
    assert np.array_equal(deg, (np.bincount(bi, minlength=n) + np.bincount(bj, minlength=n)).astype(np.uint64))
    bm = np.zeros((G, G), np.uint64)
    np.add.at(bm, (g[bi].astype(np.int64), g[bj].astype(np.int64)), 1)
    assert np.array_equal(m, bm)


# ---------------------------------------------------------------- the two-set cases

@pytest.mark.parametrize("variant", ["ortho7", "tric7"])
def test_double_frames(orc32, variant):
    every, idx1, idx2, p1, p2, box, pops1, pops2, dims, pbc = pc.double_frames(variant)
    assert np.array_equal(every[idx1.astype(np.int64)], p1) and np.array_equal(every[idx2.astype(np.int64)], p2)
    assert len(np.intersect1d(idx1, idx2)) > 100             # overlapping selections
    ref = pinned(orc32, p1, box, pops1, dims, pbc, pos2=p2)
    assert np.array_equal(pc.binned(p2, box, ref["dims"]), pops2)
    assert set(pops1.tolist()) == set(pops2.tolist()) == set(pc.EDGE_TABLE) and not np.array_equal(pops1, pops2)
    got = set((int(pops1[a]), int(pops2[b])) for a, b in pc.neighbours(dims, pbc, faces_only=True))
    for pair in pc.DOUBLE_PAIRS:
        assert pair in got, pair
    assert any(a == 0 and b > 64 for a, b in got) and any(a > 64 and b == 0 for a, b in got)
    # ... and those cell pairs do hold listed pairs: atoms of a cell of n1 of set 1 against a cell of n2 of set 2
    c1, c2 = pc.cell_of(p1, box, dims)[ref["i"].astype(np.int64)], pc.cell_of(p2, box, dims)[ref["j"].astype(np.int64)]
    listed = set(zip(pops1[c1[c1 != c2]].tolist(), pops2[c2[c1 != c2]].tolist()))
    for pair in pc.DOUBLE_PAIRS:
        assert pair in listed, pair


# ---------------------------------------------------------------- label runs

def cells_in_row_order(g, cell):
    return {int(c): g[cell == c].astype(np.int64) for c in np.unique(cell)}


def test_run_frame(orc32):
    pos, box, pops, cell, dims, pbc = pc.run_frame()
    pinned(orc32, pos, box, pops, dims, pbc)
    assert np.all(np.diff(cell) >= 0)
    assert np.array_equal(pops, np.resize(pc.RUN_POPS, 64)) and {129, 193} <= set(pops.tolist())


@pytest.mark.parametrize("pattern", list(pc.RUN_PATTERNS))
def test_label_runs_are_what_they_are_named_after(pattern):
    pos, box, pops, cell, dims, pbc = pc.run_frame()
    g, G = pc.run_labels(pattern, cell)
    assert int(g.max()) < G and G * G <= 1 << 24
    per = cells_in_row_order(g, cell)
    big = [c for c in per if pops[c] in (129, 193)]
    assert len(big) == 16
    for c in big:
        lab = per[c]
        runs = pc.runs_of(lab)
        start = np.cumsum([0] + [length for _, length in runs])[:-1]          # row / lane (mod 64) at which each run starts
        spans = [(int(s), int(s) + length - 1, length, label) for s, (label, length) in zip(start, runs)]
        if pattern == "ends_at_lane_63":
            assert any(first // 64 == last // 64 and last % 64 == 63 and 1 < length < 64 for first, last, length, _ in spans)
        elif pattern == "aligned_64":
            assert any(first % 64 == 0 and length == 64 for first, _, length, _ in spans)
        elif pattern == "crossing_64":
            assert any(first % 64 == 1 and length == 64 for first, _, length, _ in spans)
        elif pattern == "run_of_65":
            assert any(length == 65 for _, _, length, _ in spans)
        elif pattern == "a_b_a":
            # one label twice in one chunk with another label between: two runs, one map word
            assert any(s0[3] == s2[3] != s1[3] and s0[0] // 64 == s2[1] // 64 for s0, s1, s2 in zip(spans, spans[1:], spans[2:]))
        elif pattern == "distinct_beside_runs":
            assert len(set(lab[:64].tolist())) == 64 and len(set(lab[64:128].tolist())) < 8
        else:
            # the group of the rows changes at rows 1, 32 and 63 of a slot (slots of 64 rows)
            assert all(lab[r - 1] != lab[r] for r in (1, 32, 63, 64 + 1, 64 + 32, 64 + 63))
            assert lab[1] == lab[31] and lab[32] == lab[62]


@pytest.mark.parametrize("bases", ["ascending", "descending", "shared"])
def test_both_sides_of_the_swap(orc32, bases):
    pos, box, pops, cell, dims, pbc = pc.run_frame()
    ref = oracle_single(orc32, pos, box, pbc)
    g, G = pc.run_labels("a_b_a", cell, bases)
    gi, gj = g[ref["i"].astype(np.int64)], g[ref["j"].astype(np.int64)]
    assert np.any(gi < gj) and np.any(gi > gj) and np.any(gi == gj)


# ---------------------------------------------------------------- two rows per slot

@pytest.mark.parametrize("home", pc.RPS_HOME)
def test_rps_frames(orc32, home):
    pos, box, pops, cell, dims, pbc = pc.rps_frame(home)
    assert len(pos) < 1500
    pinned(orc32, pos, box, pops, dims, pbc)
    assert orc32.box_from_matrix(box).nshift != 0 and pbc == 7
    dx, dy, dz = dims
    assert pops[pc.cell_index(dims, dx - 1, dy - 1, dz - 1)] == home
    first_cells = [pops[pc.cell_index(dims, *c)] for c in ((dx - 1, dy - 1, dz - 1), (0, 0, dz - 1), (0, dy - 1, 0), (dx - 1, 0, 0))]
    assert sorted(first_cells) == sorted(pc.RPS_HOME)
    pos2, _, pops2, _, _, _ = pc.rps_frame(home, seed=40)
    pinned(orc32, pos, box, pops, dims, pbc, pos2=pos2)
    assert pops2[pc.cell_index(dims, dx - 1, dy - 1, dz - 1)] == home


# ---------------------------------------------------------------- corner blobs

@pytest.mark.parametrize("order", pc.ORDERS)
@pytest.mark.parametrize("pbc,ncomp", [(7, 27), (3, 36)])
def test_corner_blobs(orc32, pbc, ncomp, order):
    pos, box, pops, cell, dims, _ = pc.blob_frame(pbc, order=order)
    assert dims == (3, 3, 3) and len(pos) < 3000
    ref = pinned(orc32, pos, box, pops, dims, pbc)
    assert set(pops.tolist()) == set(pc.BLOB_TABLE)
    C, comp_of, sizes, _, _ = cl.components(ref, len(pos))
    assert C == ncomp and int(sizes.min()) >= 8
    # every cell holds atoms of 8 different components; a chunk of 64 rows of a crowded cell interleaves several of them
    for c in range(27):
        members = comp_of[cell == c]
        assert len(set(members.tolist())) == 8
        if order == "permuted" and pops[c] >= 63:
            assert len(set(members[:63].tolist())) == 8
    # with particles of two atoms next to each other (cell-major): hits inside one particle exist, the components stay
    if order == "cell_major":
        g, G = pc.pair_labels(cell)
        assert int(g.max()) + 1 == G and np.all(np.diff(g.astype(np.int64)) >= 0) and np.all(np.bincount(g) <= 2)
        assert int((g[ref["i"].astype(np.int64)] == g[ref["j"].astype(np.int64)]).sum()) > 500
        assert cl.components(ref, len(pos), g, G)[0] == ncomp


def test_corner_blobs_need_their_margin(orc32):
    """blobs at 0.1 / 0.9 with a jitter of 0.02: one component"""
    dims = pc.BLOB_DIMS
    box = pc.ortho_box(dims, RC, 1.3)
    rng = np.random.default_rng(5)
    pos = pc.frame(box, dims, pc.table_pops(dims, rng, pc.BLOB_TABLE), rng, corners=(0.1, 0.9, 0.02))[0]
    assert cl.components(oracle_single(orc32, pos, box, 7), len(pos))[0] == 1


@pytest.mark.parametrize("order", pc.ORDERS)
def test_edge_table_blobs(orc32, order):
    pos, box, pops, cell, dims, pbc = pc.edge_blob_frame(order=order)
    ref = pinned(orc32, pos, box, pops, dims, pbc)
    assert set(pops.tolist()) == set(pc.EDGE_TABLE)
    C, comp_of, sizes, _, _ = cl.components(ref, len(pos))
    assert int((sizes >= 2).sum()) >= 8 and int(sizes.max()) >= 65
    # the same table filled uniformly is one giant component at every cutoff that keeps the grid (cells of 1 .. 1.25 cutoffs)
    upos, ubox, upops, _, udims, _ = pc.edge_frame("ortho7")
    usizes = cl.components(oracle_single(orc32, upos, ubox, 7), len(upos))[2]
    assert int((usizes >= 2).sum()) == 1


# ---------------------------------------------------------------- blocks of frames

def test_blocks_of_frames(orc32):
    frames, box, pops, dims, pbc = pc.edge_block()
    assert frames.shape == (3, 5944, 3)
    n = frames.shape[1]
    g = (np.arange(n) // 3).astype(np.uint32)
    G = int(g.max()) + 1
    maps = [cr.single(pinned(orc32, frames[f], box, pops[f], dims, pbc), n, g, G)[2] for f in range(3)]
    assert len(set(p.tobytes() for p in pops)) == 3
    occ = cr.occupancy(maps)
    assert np.any(occ == 1) and np.any(occ == 3)               # group pairs that touch in one frame only, and in every frame
    fr1, fr2, box, pops1, pops2, dims, pbc = pc.double_block()
    assert fr1.shape[0] == fr2.shape[0] == 3
    n1, n2 = fr1.shape[1], fr2.shape[1]
    g1 = (np.arange(n1) // 3).astype(np.uint32)
    g2, G2 = cr.ragged_labels(n2)
    maps = []
    for f in range(3):
        ref = pinned(orc32, fr1[f], box, pops1[f], dims, pbc, pos2=fr2[f])
        assert np.array_equal(pc.binned(fr2[f], box, dims), pops2[f])
        maps.append(cr.double(ref, n1, n2, g1, int(g1.max()) + 1, g2, G2)[3])
    assert np.any(cr.occupancy(maps) == 1)
    frames, box, pops, dims, pbc = pc.blob_block()
    sizes = []
    for f in range(3):
        C, _, s, _, _ = cl.components(pinned(orc32, frames[f], box, pops[f], dims, pbc), frames.shape[1])
        assert C == 27
        sizes.append(s.tobytes())
    assert len(set(sizes)) == 3
