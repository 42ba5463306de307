"""cluster_kernel (cluster_kernels.hpp) on CROWDED cells with structure: frames of tests/pinned_cells.py whose cells hold 63 .. 200
atoms belonging to 8 different components each (corner blobs), so that the lanes of a chunk and the rows of a slot interleave
components and the members cached in the wave (croot per lane, rroot in lane r) are reused and refreshed all the time.  Against
the ORACLE's pair list folded by scipy (tests/clusters_ref.py), exact.  The component counts and the populations of the cells are
asserted on the reference alone in tests/test_pinned_cells_cpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clusters_ref as cl  # noqa: E402
import pinned_cells as pc  # noqa: E402
from test_gpu_clusters import check, host  # noqa: E402

pytestmark = pytest.mark.gpu

RC = pc.CUTOFF
BLOB_COMPONENTS = {7: 27, 3: 36}


@pytest.fixture(scope="module")
def eng():
    from molar_amd import build
    from molar_amd.api import Engine
    build.build_library()
    return Engine(0)


def single_ref(orc32, pos, box, pbc):
    return orc32.search_single_pbc(RC, pos, orc32.box_from_matrix(box), pbc, nthreads=8)


# ---------------------------------------------------------------- 1. corner blobs

@pytest.mark.parametrize("order", pc.ORDERS)
@pytest.mark.parametrize("pbc", [7, 3])
def test_corner_blobs(eng, orc32, pbc, order):
    pos, box, pops, cell, dims, _ = pc.blob_frame(pbc, order=order)
    ref = single_ref(orc32, pos, box, pbc)
    assert ref["dims"] == dims
    c = eng.search_clusters(RC, pos, box=box, pbc=pbc)
    assert c.ncomponents == BLOB_COMPONENTS[pbc]
    check(c, cl.components(ref, len(pos)))


@pytest.mark.parametrize("pbc", [7, 3])
def test_corner_blobs_groups(eng, orc32, pbc):
    """particles of two atoms next to each other in a cell and a blob: hits inside one particle are dropped"""
    pos, box, pops, cell, dims, _ = pc.blob_frame(pbc, order="cell_major")
    n = len(pos)
    ref = single_ref(orc32, pos, box, pbc)
    g, G = pc.pair_labels(cell)
    assert int((g[ref["i"].astype(np.int64)] == g[ref["j"].astype(np.int64)]).sum()) > 500
    want = cl.components(ref, n, g, G)
    assert want[0] == BLOB_COMPONENTS[pbc]
    check(eng.search_clusters(RC, pos, box=box, pbc=pbc, group=g, ngroups=G), want)


# ---------------------------------------------------------------- 2. the edge table

@pytest.mark.parametrize("order", pc.ORDERS)
def test_edge_table_blobs(eng, orc32, order):
    pos, box, pops, cell, dims, pbc = pc.edge_blob_frame(order=order)
    ref = single_ref(orc32, pos, box, pbc)
    assert ref["dims"] == dims
    want = cl.components(ref, len(pos))
    assert int((want[2] >= 2).sum()) >= 8 and int(want[2].max()) >= 65
    check(eng.search_clusters(RC, pos, box=box, pbc=pbc), want)


# ---------------------------------------------------------------- 3. two rows per slot

@pytest.mark.parametrize("home", pc.RPS_HOME)
def test_two_rows_per_slot(eng, orc32, home):
    pos, box, pops, cell, dims, pbc = pc.rps_frame(home)
    ref = single_ref(orc32, pos, box, pbc)
    assert ref["dims"] == dims and len(ref["i"]) > 0
    check(eng.search_clusters(RC, pos, box=box, pbc=pbc), cl.components(ref, len(pos)))


# ---------------------------------------------------------------- 4. frames form

def test_frames_form(eng, orc32):
    frames, box, _, dims, pbc = pc.blob_block()
    nf, n = frames.shape[:2]
    per = [cl.components(single_ref(orc32, f, box, pbc), n) for f in frames]
    assert all(p[0] == BLOB_COMPONENTS[pbc] for p in per)
    assert len(set(p[2].tobytes() for p in per)) == nf          # other tables: other sizes in every frame
    hist = sum(np.bincount(p[2], minlength=n + 1) for p in per).astype(np.uint64)
    b = eng.search_clusters_frames(RC, frames, box=box, pbc=pbc, want_comp_of=True)
    assert np.array_equal(b.ncomponents, [p[0] for p in per])
    assert np.array_equal(b.largest, [int(p[2].max()) for p in per])
    assert np.array_equal(b.size_hist, hist)
    assert np.array_equal(np.asarray(b.comp_of, np.uint32), np.stack([p[1] for p in per]))


# ---------------------------------------------------------------- 5. determinism; both paths of a hit ran

def test_same_bytes_twice_and_counters(eng, orc32):
    pos, box, pops, cell, dims, pbc = pc.blob_frame(7)
    ref = single_ref(orc32, pos, box, pbc)
    first = eng.search_clusters(RC, pos, box=box, pbc=pbc)
    eng.clusters_counters(True)
    again = eng.search_clusters(RC, pos, box=box, pbc=pbc)
    hits, reached, _, _ = eng.clusters_counters(False)
    for name in ("comp_of", "sizes", "offsets", "members"):
        assert host(getattr(again, name)).tobytes() == host(getattr(first, name)).tobytes(), name
    check(again, cl.components(ref, len(pos)))
    assert hits == len(ref["i"])
    assert 0 < reached < hits          # some hits went to the forest, others ended at the members cached in the wave
