"""Connected components of the contact graph (molar_hip_search_clusters / _frames, cluster_kernels.hpp) against the ORACLE's
pair list folded by scipy (tests/clusters_ref.py).  Every output is an integer array in a canonical form (components numbered
by their smallest particle, members ascending), so everything is compared with np.array_equal.  That the inputs have structure
- many components, singletons, a large one, components that exist only through the periodic boundary - is asserted on the
reference alone in tests/test_clusters_cpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clusters_ref as cl  # noqa: E402
import contacts_ref as cr  # noqa: E402

from molar_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = 50       # MOLAR_HIP_ERR_*


@pytest.fixture(scope="module")
def eng():
    from molar_amd import build
    from molar_amd.api import Engine
    build.build_library()
    return Engine(0)


def api():
    import molar_amd.api as a
    return a


def host(x):
    return x.cpu().numpy() if type(x).__module__.startswith("torch") else np.asarray(x)


def check(c, want, members=True):
    """a Clusters against clusters_ref.components' tuple"""
    C, comp_of, sizes, offsets, memb = want
    assert c.ncomponents == C
    assert np.array_equal(host(c.comp_of).astype(np.uint32), comp_of)
    assert np.array_equal(host(c.sizes).astype(np.uint32), sizes)
    if members:
        assert np.array_equal(host(c.offsets).astype(np.uint64), offsets)
        assert np.array_equal(host(c.members).astype(np.uint32), memb)
    else:
        assert c.offsets is None and c.members is None


# ---------------------------------------------------------------- 1. every class of plan entry, with structure

@pytest.mark.parametrize("case", cl.CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[3]}")
def test_entry_classes_with_structure(eng, orc32, case):
    boxname, n, _, cutoff, pbc = case
    pos, box, ref = cl.case_ref(orc32, case)
    want = cl.components(ref, n)
    assert 8 < want[0] < n
    c = eng.search_clusters(cutoff, pos, box=box, pbc=pbc)
    check(c, want)
    parts = c.split()
    assert len(parts) == want[0] and np.array_equal(np.concatenate(parts), want[4])


# ---------------------------------------------------------------- 2. grids of very few cells

def test_tiny_grid_dense(eng, orc32):
    """grid (2, 2, 3): repeated cell pairs, cells against their own image, second cells of ~2500 atoms (2418..2585 by fractional binning with
    the oracle's dims); one component.  Crowded cells WITH structure are in test_gpu_clusters_pinned.py"""
    n, cutoff = 30000, 2.1
    box = synth.box_a(n)
    pos = synth.frame(n, box)
    ref = orc32.search_single_pbc(cutoff, pos, orc32.box_from_matrix(box), 7, nthreads=8)
    assert ref["dims"] == (2, 2, 3)
    c = eng.search_clusters(cutoff, pos, box=box, pbc=7)
    assert c.ncomponents == 1
    check(c, cl.components(ref, n))


def test_tiny_grid_blobs(eng, orc32):
    pos, box, lab = cl.blob_frame()
    ref = orc32.search_single_pbc(cl.BLOB_CUTOFF, pos, orc32.box_from_matrix(box), 7)
    c = eng.search_clusters(cl.BLOB_CUTOFF, pos, box=box, pbc=7)
    assert c.ncomponents == 6 and np.array_equal(c.comp_of, cl.canonical(lab))          # by construction
    check(c, cl.components(ref, len(pos)))


# ---------------------------------------------------------------- 3. union-find adversaries

_CHAIN = {}


def chain_case(orc32, cut_from):
    if cut_from not in _CHAIN:
        pos = cl.chain(cut_from)
        box = np.diag(cl.CHAIN_BOX).astype(np.float32)
        ref = orc32.search_single_pbc(cl.CHAIN_CUTOFF, pos, orc32.box_from_matrix(box), 7, nthreads=8)
        _CHAIN[cut_from] = (pos, box, ref)
    return _CHAIN[cut_from]


def reordered(pos, ref, order):
    """the frame with atom k taken from pos[order[k]], and its pair list renumbered (the list as a set: order is irrelevant)"""
    new_of_old = np.empty(len(order), np.int64)
    new_of_old[order] = np.arange(len(order))
    return np.ascontiguousarray(pos[order]), (new_of_old[ref["i"].astype(np.int64)], new_of_old[ref["j"].astype(np.int64)])


@pytest.mark.parametrize("cut_from", [0, 64], ids=["whole", "cut"])
@pytest.mark.parametrize("order", ["ascending", "descending", "permuted"])
def test_chain(eng, orc32, order, cut_from):
    """a path graph of 5000 atoms (diameter 5000: deep paths, chained hooks), whole and cut into segments of 64, 65, 66 ..."""
    pos, box, ref = chain_case(orc32, cut_from)
    n = len(pos)
    perm = {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "permuted": np.random.default_rng(2).permutation(n)}[order]
    p, pairs = reordered(pos, ref, perm)
    want = cl.components(pairs, n)
    c = eng.search_clusters(cl.CHAIN_CUTOFF, p, box=box, pbc=7)
    if not cut_from:
        assert c.ncomponents == 1
    else:
        assert want[0] >= 8
    check(c, want)


def test_no_pair_at_all(eng):
    pos, box = cl.lattice()
    n = len(pos)
    c = eng.search_clusters(0.3, pos, box=box, pbc=7)
    assert c.ncomponents == n
    check(c, (n, np.arange(n, dtype=np.uint32), np.ones(n, np.uint32), np.arange(n + 1, dtype=np.uint64), np.arange(n, dtype=np.uint32)))


def test_empty_selection(eng):
    box = synth.box_ortho(1000)
    pos = synth.frame(1000, box)
    c = eng.search_clusters(0.3, pos, np.zeros(1, np.uint64)[:0], box=box, pbc=7)
    assert c.ncomponents == 0 and len(c.comp_of) == 0 and len(c.sizes) == 0 and len(c.members) == 0
    assert np.array_equal(c.offsets, [0]) and c.split() == []


# ---------------------------------------------------------------- 4. groups

GROUP_CASE = cl.CASES[3]          # box_b, 6000 atoms
# Groups multiply the degree, so each labelling has its own cutoff near ITS percolation threshold (found on the oracle's lists):
# at these the group graph has at least 8 components of two or more groups, singletons, and one of at least 65.
GROUP_CUTOFF = {"thirds": 0.10, "ragged": 0.06, "permuted": 0.09, "with_empty_groups": 0.09, "one_group": 0.10}


@pytest.mark.parametrize("labels", ["thirds", "ragged", "permuted", "with_empty_groups", "one_group"])
def test_groups(eng, orc32, labels):
    _, n, _, _, pbc = GROUP_CASE
    pos, box, _ = cl.case_ref(orc32, GROUP_CASE)
    cutoff = GROUP_CUTOFF[labels]
    ref = orc32.search_single_pbc(cutoff, pos, orc32.box_from_matrix(box), pbc)
    if labels == "thirds":
        g = (np.arange(n) // 3).astype(np.uint32)
        G = int(g.max()) + 1
    elif labels == "ragged":
        g, G = cr.ragged_labels(n)
    elif labels == "permuted":                       # no locality at all: neighbours in the cell carry unrelated labels
        g = np.random.default_rng(9).permutation(n).astype(np.uint32) // 4
        G = int(g.max()) + 1
    elif labels == "with_empty_groups":              # labels 0, 2, 4 ... of 2 * used + 7 groups: the others are singletons
        g = (2 * (np.arange(n) // 5)).astype(np.uint32)
        G = int(g.max()) + 8
    else:
        g, G = np.zeros(n, np.uint32), 1
    want = cl.components(ref, n, g, G)
    c = eng.search_clusters(cutoff, pos, box=box, pbc=pbc, group=g, ngroups=G)
    assert len(c.comp_of) == G
    if labels == "one_group":
        assert c.ncomponents == 1
    else:
        sizes = want[2]
        assert int((sizes >= 2).sum()) >= 8 and int((sizes == 1).sum()) >= 1 and int(sizes.max()) >= 65
        if labels == "with_empty_groups":
            assert int((sizes == 1).sum()) >= G - len(np.unique(g)) > 1000
    check(c, want)


# ---------------------------------------------------------------- 5. selections and memory

def test_strided_selection(eng, orc32):
    """idx with stride 3: ids are positions in the selection"""
    _, n, _, _, pbc = cl.CASES[0]
    pos, box, _ = cl.case_ref(orc32, cl.CASES[0])
    idx = np.arange(0, n, 3, dtype=np.uint64)
    cutoff = 0.27                                    # a third of the density: the same mean degree at 0.19 * 3^(1/3)
    ref = orc32.search_single_pbc(cutoff, pos[::3], orc32.box_from_matrix(box), pbc, nthreads=8)
    want = cl.components(ref, len(idx))
    assert 8 < want[0] < len(idx) and want[2].max() >= 65
    check(eng.search_clusters(cutoff, pos, idx, box=box, pbc=pbc), want)


def test_device_tensors_members_and_repeat(eng, orc32):
    import torch
    _, n, _, cutoff, pbc = GROUP_CASE
    pos, box, ref = cl.case_ref(orc32, GROUP_CASE)
    g, G = cr.ragged_labels(n)
    d_pos = torch.from_numpy(pos).cuda()
    d_g = torch.from_numpy(g.astype(np.int32)).cuda()
    want = cl.components(ref, n)
    c = eng.search_clusters(cutoff, d_pos, box=box, pbc=pbc)
    assert c.comp_of.is_cuda and c.members.is_cuda and c.comp_of.dtype == torch.int32 and c.offsets.dtype == torch.int64
    check(c, want)
    check(eng.search_clusters(cutoff, d_pos, box=box, pbc=pbc, want_members=False), want, members=False)
    rc_g = GROUP_CUTOFF["ragged"]
    ref_g = orc32.search_single_pbc(rc_g, pos, orc32.box_from_matrix(box), pbc)
    check(eng.search_clusters(rc_g, d_pos, box=box, pbc=pbc, group=d_g, ngroups=G), cl.components(ref_g, n, g, G))
    again = eng.search_clusters(cutoff, d_pos, box=box, pbc=pbc)
    for name in ("comp_of", "sizes", "offsets", "members"):
        assert host(getattr(again, name)).tobytes() == host(getattr(c, name)).tobytes(), name


# ---------------------------------------------------------------- 6. frames form

def test_frames_form(eng, orc32):
    import torch
    n, nframes, cutoff = 4000, 5, 0.17
    boxes = np.stack([synth.box_ortho(n) * np.float32(1.0 + 0.02 * f) for f in range(nframes)]).astype(np.float32)
    frames = np.stack([synth.frame(n, boxes[f], f) for f in range(nframes)])
    per = [eng.search_clusters(cutoff, frames[f], box=boxes[f], pbc=7) for f in range(nframes)]
    assert len(set(p.ncomponents for p in per)) > 1 and all(8 < p.ncomponents < n for p in per)
    last = nframes - 1                               # the per-frame calls themselves: one of them against the oracle here
    check(per[last], cl.components(orc32.search_single_pbc(cutoff, frames[last], orc32.box_from_matrix(boxes[last]), 7), n))
    hist = sum(np.bincount(p.sizes, minlength=n + 1) for p in per).astype(np.uint64)
    start = (np.arange(n + 1) % 7).astype(np.uint64)
    b = eng.search_clusters_frames(cutoff, frames, box=boxes, pbc=7, size_hist=start.copy(), want_comp_of=True)
    assert np.array_equal(b.ncomponents, [p.ncomponents for p in per])
    assert np.array_equal(b.largest, [int(p.sizes.max()) for p in per])
    assert np.array_equal(b.size_hist, start + hist)
    assert np.array_equal(b.comp_of, np.stack([p.comp_of for p in per]))
    # everything on the device
    d_hist = torch.from_numpy(start.astype(np.int64)).cuda()
    d = eng.search_clusters_frames(cutoff, torch.from_numpy(frames).cuda(), box=boxes, pbc=7, size_hist=d_hist, want_comp_of=True)
    assert np.array_equal(host(d.ncomponents), b.ncomponents) and np.array_equal(host(d.largest), b.largest)
    assert np.array_equal(host(d.size_hist).astype(np.uint64), b.size_hist) and np.array_equal(host(d.comp_of).astype(np.uint32), b.comp_of)


# ---------------------------------------------------------------- 7. the caller's cached search

def test_count_waiting_for_its_fill(eng, orc32):
    a = api()
    _, n, _, cutoff, pbc = GROUP_CASE
    pos, box, ref = cl.case_ref(orc32, GROUP_CASE)
    e = a.Engine(0)
    cnt = e.search_count(a.SEARCH_SINGLE, 0.5, pos, box=box, pbc=7)
    f = a.Engine(0)
    want_pairs, want_dist = f.search_fill(f.search_count(a.SEARCH_SINGLE, 0.5, pos, box=box, pbc=7))
    check(e.search_clusters(cutoff, pos, box=box, pbc=pbc), cl.components(ref, n))          # in between: another cutoff, another grid
    pairs, dist = e.search_fill(cnt)
    assert cnt == len(want_pairs) > 0 and pairs.tobytes() == want_pairs.tobytes() and dist.tobytes() == want_dist.tobytes()


# ---------------------------------------------------------------- 8. errors

def test_errors(eng):
    import ctypes as C
    import torch
    a = api()
    n = 1000
    box = synth.box_ortho(n)
    pos = synth.frame(n, box)
    d, keep = eng._contacts_desc(a.SEARCH_DOUBLE, 0.3, pos, None, pos, None, 0)
    out = np.zeros(n, np.uint32)
    cnt = C.c_uint32(0)
    rc = eng.lib.molar_hip_search_clusters(eng.ctx, C.byref(d), None, out.ctypes.data, None, None, None, C.byref(cnt))
    assert rc == INVALID_ARGUMENT
    rc = eng.lib.molar_hip_search_clusters_frames(eng.ctx, C.byref(d), None, 1, 3 * n, None, out.ctypes.data, None, None, None)
    assert rc == INVALID_ARGUMENT
    g = (np.arange(n) // 4).astype(np.uint32)
    G = int(g.max()) + 1
    g[n // 2] = G
    for labels in (g, torch.from_numpy(g.astype(np.int32)).cuda()):
        with pytest.raises(a.MolarHipError) as err:
            eng.search_clusters(0.3, pos, box=box, pbc=7, group=labels, ngroups=G)
        assert err.value.code == INVALID_ARGUMENT
