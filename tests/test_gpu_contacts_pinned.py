"""contact_kernel<SINGLE | DOUBLE> (contact_kernels.hpp) at chosen cell occupancies and label runs: frames of tests/pinned_cells.py,
whose cells hold 0, 1, 2, 3, 62 .. 66, 127 .. 129, 191 .. 193 and 200 atoms, against the ORACLE's pair list folded by numpy
(tests/contacts_ref.py).  Everything is an integer and compared with np.array_equal: no tolerances.  That the frames are what they
were built to be - the oracle's grid, the population of every cell, the label runs inside the cells, the cell pairs of the two-set
cases - is asserted on the reference alone in tests/test_pinned_cells_cpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contacts_ref as cr  # noqa: E402
import pinned_cells as pc  # noqa: E402

pytestmark = pytest.mark.gpu

RC = pc.CUTOFF


@pytest.fixture(scope="module")
def eng():
    from molar_amd import build
    from molar_amd.api import Engine
    build.build_library()
    return Engine(0)


def api():
    import molar_amd.api as a
    return a


def thirds(n):
    g = (np.arange(n) // 3).astype(np.uint32)
    return g, int(g.max()) + 1


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def single_ref(orc32, pos, box, pbc):
    return orc32.search_single_pbc(RC, pos, orc32.box_from_matrix(box), pbc, nthreads=8)


def double_ref(orc32, p1, p2, box, pbc):
    return orc32.search_double_pbc(RC, p1, p2, orc32.box_from_matrix(box), pbc, nthreads=8)


def check_single(c, ref, n, g, G):
    count, deg, m = cr.single(ref, n, g, G)
    assert count > 0
    assert c.count == count
    assert np.array_equal(np.asarray(c.deg1, np.uint64), deg)
    assert c.deg2 is None
    assert c.map.shape == (G, G) and np.array_equal(np.asarray(c.map, np.uint64), m)


def check_double(c, ref, n1, n2, g1, G1, g2, G2):
    count, deg1, deg2, m = cr.double(ref, n1, n2, g1, G1, g2, G2)
    assert count > 0
    assert c.count == count
    assert np.array_equal(np.asarray(c.deg1, np.uint64), deg1) and np.array_equal(np.asarray(c.deg2, np.uint64), deg2)
    assert c.map.shape == (G1, G2) and np.array_equal(np.asarray(c.map, np.uint64), m)


# ---------------------------------------------------------------- 1. SINGLE, the edge table

@pytest.mark.parametrize("order", pc.ORDERS)
@pytest.mark.parametrize("variant", list(pc.VARIANTS))
def test_single_edge_table(eng, orc32, variant, order):
    """same-cell entries of 65, 128, 129 and 193 atoms (the chunk skip of the j > i half, odd last slots), second cells of one to
    four chunks with a ragged last one; labels pos // 3: runs of 3 in cell-major order, no locality in permuted order"""
    a = api()
    pos, box, pops, cell, dims, pbc = pc.edge_frame(variant, order=order)
    ref = cached(("s", variant, order), lambda: single_ref(orc32, pos, box, pbc))
    assert ref["dims"] == dims
    g, G = thirds(len(pos))
    c = eng.search_contacts(a.SEARCH_SINGLE, RC, pos, box=box, pbc=pbc, group1=g, ngroups1=G)
    check_single(c, ref, len(pos), g, G)


# ---------------------------------------------------------------- 2. DOUBLE, the edge table for both sets

@pytest.mark.parametrize("form", ["overlapping", "separate"])
@pytest.mark.parametrize("variant", ["ortho7", "tric7"])
def test_double_edge_table(eng, orc32, variant, form):
    """second cells of several chunks (deg2 and the labels of set 2 in every chunk), first cells of several slots; the map is
    not square"""
    a = api()
    every, idx1, idx2, p1, p2, box, pops1, pops2, dims, pbc = cached(("df", variant), lambda: pc.double_frames(variant))
    ref = cached(("d", variant), lambda: double_ref(orc32, p1, p2, box, pbc))
    assert ref["dims"] == dims
    g1, G1 = thirds(len(p1))
    g2, G2 = cr.ragged_labels(len(p2))
    assert G1 != G2
    if form == "overlapping":
        c = eng.search_contacts(a.SEARCH_DOUBLE, RC, every, idx1, every, idx2, box=box, pbc=pbc, group1=g1, ngroups1=G1, group2=g2, ngroups2=G2)
    else:
        c = eng.search_contacts(a.SEARCH_DOUBLE, RC, p1, None, p2, None, box=box, pbc=pbc, group1=g1, ngroups1=G1, group2=g2, ngroups2=G2)
    check_double(c, ref, len(p1), len(p2), g1, G1, g2, G2)


# ---------------------------------------------------------------- 3. label runs

def run_case(orc32):
    def make():
        pos, box, pops, cell, dims, pbc = pc.run_frame()
        return pos, box, cell, pbc, single_ref(orc32, pos, box, pbc), double_ref(orc32, pos, pos, box, pbc)
    return cached("runs", make)


@pytest.mark.parametrize("pattern", list(pc.RUN_PATTERNS))
def test_label_runs_single(eng, orc32, pattern):
    """the pattern in the lanes of every chunk AND in the rows of every slot of cells of 129 and 193 atoms"""
    a = api()
    pos, box, cell, pbc, ref, _ = run_case(orc32)
    g, G = pc.run_labels(pattern, cell)
    c = eng.search_contacts(a.SEARCH_SINGLE, RC, pos, box=box, pbc=pbc, group1=g, ngroups1=G)
    check_single(c, ref, len(pos), g, G)


@pytest.mark.parametrize("bases", ["ascending", "descending", "shared"])
def test_label_runs_single_both_sides_of_the_swap(eng, orc32, bases):
    """[min][max]: the label of the lane's atom below, above and equal to the label of the run of rows"""
    a = api()
    pos, box, cell, pbc, ref, _ = run_case(orc32)
    g, G = pc.run_labels("a_b_a", cell, bases)
    gi, gj = g[ref["i"].astype(np.int64)], g[ref["j"].astype(np.int64)]
    assert np.any(gi < gj) and np.any(gi > gj) and np.any(gi == gj)
    c = eng.search_contacts(a.SEARCH_SINGLE, RC, pos, box=box, pbc=pbc, group1=g, ngroups1=G)
    check_single(c, ref, len(pos), g, G)


@pytest.mark.parametrize("side", ["set2_lanes", "set1_rows"])
@pytest.mark.parametrize("pattern", list(pc.RUN_PATTERNS))
def test_label_runs_double(eng, orc32, pattern, side):
    """the pattern in the labels of the second set (the lanes' segmented scan) or of the first set (the runs of rows); the other
    side carries pos // 3 or ragged labels, ngroups1 != ngroups2"""
    a = api()
    pos, box, cell, pbc, _, ref = run_case(orc32)
    n = len(pos)
    if side == "set2_lanes":
        (g1, G1), (g2, G2) = thirds(n), pc.run_labels(pattern, cell)
    else:
        (g1, G1), (g2, G2) = pc.run_labels(pattern, cell), cr.ragged_labels(n)
    assert G1 != G2
    c = eng.search_contacts(a.SEARCH_DOUBLE, RC, pos, None, pos, None, box=box, pbc=pbc, group1=g1, ngroups1=G1, group2=g2, ngroups2=G2)
    check_double(c, ref, n, n, g1, G1, g2, G2)


# ---------------------------------------------------------------- 4. two rows per slot

@pytest.mark.parametrize("home", pc.RPS_HOME)
def test_two_rows_per_slot(eng, orc32, home):
    """triclinic box with lattice shifts: the entries that wrap in x, y and z are cut into slots of 2 rows; first cells of 1, 2, 3
    and 65 atoms (fewer rows than a slot, an odd last slot)"""
    a = api()
    pos, box, pops, cell, dims, pbc = pc.rps_frame(home)
    pos2 = pc.rps_frame(home, seed=40)[0]
    n, n2 = len(pos), len(pos2)
    ref = single_ref(orc32, pos, box, pbc)
    assert ref["dims"] == dims
    g, G = thirds(n)
    check_single(eng.search_contacts(a.SEARCH_SINGLE, RC, pos, box=box, pbc=pbc, group1=g, ngroups1=G), ref, n, g, G)
    g2, G2 = cr.ragged_labels(n2, hi=9)
    refd = double_ref(orc32, pos, pos2, box, pbc)
    c = eng.search_contacts(a.SEARCH_DOUBLE, RC, pos, None, pos2, None, box=box, pbc=pbc, group1=g, ngroups1=G, group2=g2, ngroups2=G2)
    check_double(c, refd, n, n2, g, G, g2, G2)


# ---------------------------------------------------------------- 5. frames form: the per-frame 32-bit map and contact_fold_kernel

def test_frames_single(eng, orc32):
    a = api()
    frames, box, _, dims, pbc = pc.edge_block()
    n = frames.shape[1]
    g, G = thirds(n)
    folds = [cr.single(single_ref(orc32, f, box, pbc), n, g, G) for f in frames]
    occ = cr.occupancy([f[2] for f in folds])
    assert np.any(occ == 1) and np.any(occ == len(frames))
    c = eng.search_contacts_frames(a.SEARCH_SINGLE, RC, frames, box=box, pbc=pbc, group1=g, ngroups1=G)
    assert np.array_equal(c.deg1, sum(f[1] for f in folds))
    assert np.array_equal(c.map, sum(f[2] for f in folds))
    assert np.array_equal(c.occupancy, occ)


def test_frames_double_with_frames2(eng, orc32):
    a = api()
    fr1, fr2, box, _, _, dims, pbc = pc.double_block()
    n1, n2 = fr1.shape[1], fr2.shape[1]
    g1, G1 = thirds(n1)
    g2, G2 = cr.ragged_labels(n2)
    folds = [cr.double(double_ref(orc32, fr1[f], fr2[f], box, pbc), n1, n2, g1, G1, g2, G2) for f in range(len(fr1))]
    occ = cr.occupancy([f[3] for f in folds])
    assert np.any(occ == 1)
    c = eng.search_contacts_frames(a.SEARCH_DOUBLE, RC, fr1, box=box, pbc=pbc, frames2=fr2, group1=g1, ngroups1=G1, group2=g2, ngroups2=G2)
    assert np.array_equal(c.deg1, sum(f[1] for f in folds)) and np.array_equal(c.deg2, sum(f[2] for f in folds))
    assert np.array_equal(c.map, sum(f[3] for f in folds))
    assert np.array_equal(c.occupancy, occ)
