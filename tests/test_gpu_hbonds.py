"""Hydrogen bonds on the GPU (molar_hip_hbonds_*, hbonds.hip) against tests/hbonds_ref.py: the ORACLE's two-set list, then
longdouble numpy.  tests/test_hbonds_cpu.py asserts from the reference alone that no candidate of any case compared here lies
inside the band of a threshold, so the triples are compared for exact equality, order included; the f64 columns are held to
the bounds the reference derives (roundings, below 1e-9 degrees and 1e-12 nm)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hbonds_ref as hr  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, TOO_LARGE, NO_SEARCH = 50, 51, 52       # MOLAR_HIP_ERR_*
KIND = {hr.DHA: "dha", hr.HDA: "hda"}
WORST = {"da": 0.0, "ha": 0.0, "angle": 0.0}              # the largest fraction of a bound any comparison came to


@pytest.fixture(scope="module")
def eng():
    from molar_amd import build
    from molar_amd.api import Engine
    build.build_library()
    return Engine(0)


def api():
    import molar_amd.api as a
    return a


def run(e, c, **kw):
    return e.hbonds(c["xyz"], c["donors"], (c["hoff"], c["hidx"]), c["acceptors"], box=c["box"], pbc=c["pbc"], cutoff=c["cutoff"],
                    angle=c["angle"], angle_kind=KIND[c["kind"]], max_ha=c["max_ha"], **kw)


def check_columns(got_da, got_ha, got_ang, ref):
    for key, got, want, bound in (("da", got_da, ref["dist_da"], ref["bound_da"]), ("ha", got_ha, ref["dist_ha"], ref["bound_ha"]),
                                  ("angle", got_ang, ref["angle"], ref["bound_angle"])):
        got = np.asarray(got, np.float64)
        assert got.shape == want.shape
        if len(want):
            frac = np.abs(got - want) / bound
            WORST[key] = max(WORST[key], float(frac.max()))
            print(f"worst fraction of the bound, {key}: {float(frac.max()):.3g}")
            assert np.all(frac <= 1.0), (key, float(frac.max()))


def check(r, ref, c):
    assert r.count == len(ref["triples"])
    assert np.array_equal(np.asarray(r.triples, np.uint32), ref["triples"])
    check_columns(r.dist_da, r.dist_ha, r.angle, ref)
    don, acc, _ = hr.counts_of(c, ref)
    assert np.array_equal(np.asarray(r.don_count, np.uint64), don)
    assert np.array_equal(np.asarray(r.acc_count, np.uint64), acc)


# ---------------------------------------------------------------- 1. every class of plan entry

@pytest.mark.parametrize("name", ["ortho_pbc7", "tric_a_pbc7", "hex_b_pbc7", "tric_a_pbc1", "ortho_pbc3", "no_box", "two_cells"])
def test_plan_entry_classes(eng, orc32, name):
    c, ref = hr.case(name), hr.reference(orc32, name)
    assert ref["n_list"] > ref["n_unique"]                  # the oracle's list really has duplicates
    r = run(eng, c)
    assert r.count > 0
    check(r, ref, c)
    if name == "two_cells":
        assert min(eng.grid_dims()[:2]) == 2


# ---------------------------------------------------------------- 2. criteria

@pytest.mark.parametrize("name", ["hda30_ha025", "dha0", "dha180"])
def test_criteria(eng, orc32, name):
    c, ref = hr.case(name), hr.reference(orc32, name)
    r = run(eng, c)
    check(r, ref, c)
    if name == "dha0":
        assert r.count == ref["n_candidates"] > 0           # every candidate, none of them degenerate
    if name == "dha180":
        assert r.count == 0 and r.triples.shape == (0, 3)
    if name == "hda30_ha025":
        assert r.count > 0 and float(np.max(r.dist_ha)) <= 0.25 and float(np.max(r.angle)) <= 30.0


# ---------------------------------------------------------------- 3. ragged and degenerate donors

@pytest.mark.parametrize("name", ["ragged", "self_hydrogen", "strided_unsorted"])
def test_donor_shapes(eng, orc32, name):
    c, ref = hr.case(name), hr.reference(orc32, name)
    r = run(eng, c)
    assert r.count > 0
    check(r, ref, c)
    t = np.asarray(r.triples)
    assert np.all(t[:, 0] != t[:, 2])                       # donors and acceptors overlap: self pairs are dropped
    assert np.all(t[:, 0] != t[:, 1])                       # a donor listed as its own hydrogen is never a bond
    if name == "ragged":
        nh = np.diff(c["hoff"].astype(np.int64))
        assert set(nh.tolist()) == {0, 1, 3} and np.all(np.asarray(r.don_count)[nh == 0] == 0)


def test_hydrogen_forms(eng, orc32):
    """one index per donor and a list of lists give what the CSR gives"""
    c, ref = hr.case("ragged"), hr.reference(orc32, "ragged")
    off, hidx = c["hoff"].astype(np.int64), c["hidx"]
    rows = [hidx[off[p]:off[p + 1]].tolist() for p in range(len(off) - 1)]
    r = eng.hbonds(c["xyz"], c["donors"], rows, c["acceptors"], box=c["box"], pbc=c["pbc"])
    assert np.array_equal(r.triples, ref["triples"])
    c1 = hr.case("ortho_pbc7")
    first = c1["hidx"][c1["hoff"][:-1].astype(np.int64)]
    r1 = eng.hbonds(c1["xyz"], c1["donors"], first, c1["acceptors"], box=c1["box"], pbc=7)
    full = hr.reference(orc32, "ortho_pbc7")
    assert np.array_equal(r1.triples, full["triples"][np.isin(full["triples"][:, 1], first)])


# ---------------------------------------------------------------- 4. launch-shape edges

def trio_case(n, nbent, nfar):
    xyz, box = hr.trios(n, nbent, nfar)
    t = np.arange(n, dtype=np.uint64) * 3
    return dict(xyz=xyz, box=box, pbc=7, donors=t, hoff=np.arange(n + 1, dtype=np.uint64), hidx=t + 1, acceptors=t + 2, kind=hr.DHA, angle=150.0,
                max_ha=0.0, cutoff=0.35)


# hr.trios never puts a donor and its acceptor into one grid cell, so the list has no duplicates: its length - the lanes of the
# filter - is n - nfar, and the keys the filter appends - the input of the sort and of the unique pass - are the hits,
# n - nfar - nbent, which are also the lanes of the measure kernel.  All three are asserted from the oracle's list.  Workgroups
# of 256 (filter, measure), waves of 64: list lengths and key counts of 0, 1, 63, 64, 65, 255, 256, 257, then more than one
# workgroup.  (Lists WITH duplicates at odd lengths are what every water case is.)
@pytest.mark.parametrize("n,nbent,nfar", [(3, 0, 3), (2, 2, 0), (1, 0, 0), (63, 0, 0), (64, 0, 0), (65, 0, 0), (64, 1, 0), (66, 1, 0), (255, 0, 0),
                                          (256, 0, 0), (257, 0, 0), (256, 1, 0), (258, 1, 0), (258, 0, 1), (513, 1, 0)])
def test_launch_shape_edges(eng, orc32, n, nbent, nfar):
    c = trio_case(n, nbent, nfar)
    ref = hr.reference(orc32, ("trios", n, nbent, nfar), c)
    assert c["oracle_dims"] == (hr.trio_grid(n)[2],) * 3            # the grid the trios were placed on
    assert ref["n_list"] == ref["n_unique"] == ref["n_candidates"] == n - nfar
    assert ref["n_keys"] == len(ref["triples"]) == n - nfar - nbent
    if ref["n_candidates"]:
        assert float(ref["clearance"].min()) > 1.0
    r = run(eng, c)
    check(r, ref, c)


def test_launch_shape_edges_cover_the_sizes_asked_for(orc32):
    """the table above, from the reference alone: which list lengths and key counts it reaches"""
    marks = [m for m in test_launch_shape_edges.pytestmark if m.name == "parametrize"][0]
    lists, keys = set(), set()
    for n, nbent, nfar in marks.args[1]:
        ref = hr.reference(orc32, ("trios", n, nbent, nfar), trio_case(n, nbent, nfar))
        lists.add(ref["n_list"])
        keys.add(ref["n_keys"])
    edges = {0, 1, 63, 64, 65, 255, 256, 257}
    assert edges <= lists and edges <= keys and max(lists) > 512


def test_one_donor(eng, orc32):
    c = dict(hr.case("ortho_pbc7"))
    ref_all = hr.reference(orc32, "ortho_pbc7")
    p = int(ref_all["pos"][0, 0])                           # a donor that has a bond
    c["donors"] = c["donors"][p:p + 1]
    c["hoff"] = np.array([0, 2], np.uint64)
    c["hidx"] = hr.case("ortho_pbc7")["hidx"][2 * p:2 * p + 2]
    ref = hr.reference(orc32, ("one_donor", p), c)
    r = run(eng, c)
    assert r.count > 0
    check(r, ref, c)
    assert np.array_equal(r.triples, ref_all["triples"][ref_all["pos"][:, 0] == p])


def test_fresh_context_grows_its_key_buffer(orc32):
    from molar_amd.api import Engine
    c, ref = hr.case("grow"), hr.reference(orc32, "grow")
    assert len(ref["triples"]) > 2048                       # far more keys than the buffer of a fresh context holds
    e = Engine(0)
    try:
        check(run(e, c), ref, c)                            # filtered twice: into the first buffer, then into the grown one
        check(run(e, c), ref, c)                            # filtered once
    finally:
        e.close()


# ---------------------------------------------------------------- 5. counts

def labels(n, k):
    g = (np.arange(n) // k).astype(np.uint32)
    return g, int(g.max()) + 1


def test_counts_and_map_accumulate_into(eng, orc32):
    c, ref = hr.case("tric_a_pbc7"), hr.reference(orc32, "tric_a_pbc7")
    g1, G1 = labels(len(c["donors"]), 7)
    g2, G2 = labels(len(c["acceptors"]), 5)
    don, acc, m = hr.counts_of(c, ref, g1, g2, G1, G2)
    assert m.sum() == len(ref["triples"]) > 0
    r = run(eng, c, group1=g1, ngroups1=G1, group2=g2, ngroups2=G2)
    assert np.array_equal(r.don_count, don) and np.array_equal(r.acc_count, acc) and np.array_equal(r.map, m)
    # INTO pre-filled arrays, twice
    d0 = np.arange(len(don), dtype=np.uint64)
    a0 = np.full(len(acc), 5, np.uint64)
    m0 = np.full((G1, G2), 1 << 40, np.uint64)
    d1, a1, m1 = d0.copy(), a0.copy(), m0.copy()
    for _ in range(2):
        run(eng, c, group1=g1, ngroups1=G1, group2=g2, ngroups2=G2, don_count=d1, acc_count=a1, cmap=m1)
    assert np.array_equal(d1, d0 + 2 * don) and np.array_equal(a1, a0 + 2 * acc) and np.array_equal(m1, m0 + 2 * m)


def test_device_tensors_in_and_out(eng, orc32):
    import torch
    c, ref = hr.case("hex_b_pbc7"), hr.reference(orc32, "hex_b_pbc7")
    g1, G1 = labels(len(c["donors"]), 4)
    g2, G2 = labels(len(c["acceptors"]), 9)
    don, acc, m = hr.counts_of(c, ref, g1, g2, G1, G2)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()
    don_t = torch.full((len(don),), 3, dtype=torch.int64, device="cuda")
    r = eng.hbonds(dev(c["xyz"], np.float32), dev(c["donors"], np.int64), (dev(c["hoff"], np.int64), dev(c["hidx"], np.int64)),
                   dev(c["acceptors"], np.int64), box=c["box"], pbc=7, group1=dev(g1, np.int32), ngroups1=G1, group2=dev(g2, np.int32),
                   ngroups2=G2, don_count=don_t)
    assert r.triples.is_cuda and r.angle.is_cuda and r.map.is_cuda and r.don_count is don_t
    assert np.array_equal(r.triples.cpu().numpy().astype(np.uint32), ref["triples"])
    check_columns(r.dist_da.cpu().numpy(), r.dist_ha.cpu().numpy(), r.angle.cpu().numpy(), ref)
    assert np.array_equal(don_t.cpu().numpy().astype(np.uint64), don + 3)
    assert np.array_equal(r.acc_count.cpu().numpy().astype(np.uint64), acc)
    assert np.array_equal(r.map.cpu().numpy().astype(np.uint64), m)


def test_counts_without_out_count_then_synchronize(eng, orc32):
    """the form of the contacts call that does not ask for the count: device outputs, out_count NULL, synchronize, read"""
    import torch
    c, ref = hr.case("ortho_pbc7"), hr.reference(orc32, "ortho_pbc7")
    don, acc, _ = hr.counts_of(c, ref)
    xyz = torch.from_numpy(c["xyz"]).cuda()
    d, keep, n1, n2, req = eng._hbonds_request(c["donors"], (c["hoff"], c["hidx"]), c["acceptors"], 0.35, 7, 150.0, "dha", xyz.shape[0])
    d.xyz1 = d.xyz2 = xyz.data_ptr()
    b9 = np.ascontiguousarray(c["box"].T).reshape(9)
    d.box9 = b9.ctypes.data
    don_t = torch.zeros(n1, dtype=torch.int64, device="cuda")
    acc_t = torch.zeros(n2, dtype=torch.int64, device="cuda")
    rc = eng.lib.molar_hip_hbonds_counts(eng.ctx, C.byref(d), req[0], req[1], req[2], req[3], req[4], 0.0, None, don_t.data_ptr(),
                                         acc_t.data_ptr(), None, None)
    assert rc == 0
    eng.synchronize()
    assert np.array_equal(don_t.cpu().numpy().astype(np.uint64), don) and np.array_equal(acc_t.cpu().numpy().astype(np.uint64), acc)
    t = np.empty((len(ref["triples"]), 3), np.uint32)
    assert eng.lib.molar_hip_hbonds_fill(eng.ctx, t.ctypes.data, None, None, None) == 0         # every column is optional
    assert np.array_equal(t, ref["triples"])


# ---------------------------------------------------------------- 6. the frames form

@pytest.mark.parametrize("name", ["block5", "block17"])
def test_frames(eng, orc32, name):
    b = hr.frames_case(name)
    F = b["frames"].shape[0]
    refs = [hr.reference(orc32, (name, f), hr.frame_of(b, f)) for f in range(F)]
    g1, G1 = labels(len(b["donors"]), 6)
    g2, G2 = labels(len(b["acceptors"]), 11)
    r = eng.hbonds_frames(b["frames"], b["donors"], (b["hoff"], b["hidx"]), b["acceptors"], box=b["boxes"], pbc=7, group1=g1, ngroups1=G1,
                          group2=g2, ngroups2=G2)
    # the fill of a single frame is refused now: the block replaced the frame's result
    assert eng.lib.molar_hip_hbonds_fill(eng.ctx, None, None, None, None) == NO_SEARCH
    per = np.array([len(x["triples"]) for x in refs], np.uint64)
    assert np.array_equal(r.per_frame, per) and per[F - 2] == 0 and per.sum() > 0
    assert np.array_equal(r.frame_offsets, np.concatenate([[0], np.cumsum(per)]).astype(np.uint64))
    don = np.zeros(len(b["donors"]), np.uint64)
    acc = np.zeros(len(b["acceptors"]), np.uint64)
    m = np.zeros((G1, G2), np.uint64)
    for f in range(F):
        lo, hi = int(r.frame_offsets[f]), int(r.frame_offsets[f + 1])
        assert np.array_equal(r.triples[lo:hi], refs[f]["triples"])
        check_columns(r.dist_da[lo:hi], r.dist_ha[lo:hi], r.angle[lo:hi], refs[f])
        d_, a_, m_ = hr.counts_of(hr.frame_of(b, f), refs[f], g1, g2, G1, G2)
        don, acc, m = don + d_, acc + a_, m + m_
        # ... and the single call of the frame gives the same bits
        if f in (0, F - 2, F - 1):
            c = hr.frame_of(b, f)
            one = run(eng, c)
            assert np.array_equal(one.triples, r.triples[lo:hi]) and np.array_equal(one.angle, r.angle[lo:hi])
            assert np.array_equal(one.dist_da, r.dist_da[lo:hi]) and np.array_equal(one.dist_ha, r.dist_ha[lo:hi])
    assert np.array_equal(r.don_count, don) and np.array_equal(r.acc_count, acc) and np.array_equal(r.map, m)
    # the table: rows in the order of the positions (the selections are sorted and the CSR follows the atoms, so the positions'
    # order is the order of (hydrogen, acceptor) as atoms)
    pos = np.concatenate([x["pos"] for x in refs])
    keys = pos[:, 1].astype(np.uint64) << np.uint64(32) | pos[:, 2].astype(np.uint64)
    uniq, first, inverse, counts = np.unique(keys, return_index=True, return_inverse=True, return_counts=True)
    trip = np.concatenate([x["triples"] for x in refs])
    assert np.array_equal(r.table, trip[first])
    assert np.array_equal(r.occupancy, counts.astype(np.uint32))
    assert np.array_equal(r.bond_of_entry, inverse.astype(np.uint32))
    assert counts.max() > 1 and counts.min() == 1 and counts.max() <= F - 1
    # the single calls above replaced the block's result
    assert eng.lib.molar_hip_hbonds_frames_fill(eng.ctx, None, None, None, None, None, None, None, None) == NO_SEARCH


def test_frames_on_the_device_with_a_gap(eng, orc32):
    import torch
    b = hr.frames_case("block5")
    F, n = b["frames"].shape[:2]
    padded = torch.zeros((F, n + 5, 3), dtype=torch.float32, device="cuda")
    padded[:, :n] = torch.from_numpy(b["frames"]).cuda()
    don_t = torch.full((len(b["donors"]),), 3, dtype=torch.int64, device="cuda")
    r = eng.hbonds_frames(padded[:, :n], b["donors"], (b["hoff"], b["hidx"]), b["acceptors"], box=b["boxes"], pbc=7, don_count=don_t)
    # device count outputs of a block are added INTO at the end of the call, through the call's own sums
    don = sum(hr.counts_of(hr.frame_of(b, f), hr.reference(orc32, ("block5", f), hr.frame_of(b, f)))[0] for f in range(F))
    acc = sum(hr.counts_of(hr.frame_of(b, f), hr.reference(orc32, ("block5", f), hr.frame_of(b, f)))[1] for f in range(F))
    assert r.don_count is don_t and np.array_equal(don_t.cpu().numpy().astype(np.uint64), don + 3)
    assert r.acc_count.is_cuda and np.array_equal(r.acc_count.cpu().numpy().astype(np.uint64), acc)
    want = np.concatenate([hr.reference(orc32, ("block5", f), hr.frame_of(b, f))["triples"] for f in range(F)])
    assert r.triples.is_cuda and np.array_equal(r.triples.cpu().numpy().astype(np.uint32), want)
    assert int(r.occupancy.sum()) == len(want) and int(r.bond_of_entry.max()) == r.table.shape[0] - 1


# ---------------------------------------------------------------- 7. the context's state, determinism

def test_two_calls_give_equal_bits(eng):
    c = hr.case("tric_a_pbc7")
    a, b = run(eng, c), run(eng, c)
    for x, y in ((a.triples, b.triples), (a.dist_da, b.dist_da), (a.dist_ha, b.dist_ha), (a.angle, b.angle), (a.don_count, b.don_count)):
        assert x.tobytes() == y.tobytes()


def test_cached_search_is_replaced_and_planes_are_restored(eng, orc32):
    a = api()
    c, ref = hr.case("ortho_pbc7"), hr.reference(orc32, "ortho_pbc7")
    other = hr.case("no_box")
    n0 = eng.search_count(a.SEARCH_SINGLE, 0.3, other["xyz"])
    assert n0 > 0
    run(eng, c)
    # the cached search is now the donor-acceptor search of the call: its list, ids as positions
    n = ref["n_list"]
    pairs = np.full((2 * n + 64, 2), 0xFFFFFFFF, np.uint32)      # (room to spare: a wrong count must fail the test, not the process)
    assert eng.lib.molar_hip_search_fill(eng.ctx, pairs.ctypes.data, None) == 0
    assert np.all(pairs[n:] == 0xFFFFFFFF)
    pairs = pairs[:n]
    i, j = hr.oracle_list(orc32, c)
    assert np.array_equal(pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))], np.stack([i, j], 1)[np.lexsort((j, i))].astype(np.uint32))
    # the caller's plane setting survives the call, either way
    p1, p2 = c["xyz"][c["donors"].astype(np.int64)], c["xyz"][c["acceptors"].astype(np.int64)]
    try:
        eng.search_resident_planes(False)
        run(eng, c)
        assert eng.search_resident(a.SEARCH_DOUBLE, 0.35, p1, None, p2, None, box=c["box"], pbc=7)[2] is None
        eng.search_resident_planes(True)
        run(eng, c)
        n, _, dist = eng.search_resident(a.SEARCH_DOUBLE, 0.35, p1, None, p2, None, box=c["box"], pbc=7)
        assert n == ref["n_list"] and dist is not None
    finally:
        eng.search_resident_planes(True)


def test_within_hold_ends_with_the_call(eng, orc32):
    """molar_hip_within_hold promises reuse until "any other search on the context": a hydrogen-bond call is one, and the
    request after it is staged and binned again - it must not see the grid of the call's donors"""
    c = hr.case("ortho_pbc7")
    ox = c["donors"]
    inner = c["donors"][:40] + 1
    want = eng.within_set(0.3, c["xyz"], ox, c["xyz"], inner, box=c["box"], pbc=7)
    assert len(want) > 0
    try:
        eng.within_hold(True)
        assert np.array_equal(eng.within_set(0.3, c["xyz"], ox, c["xyz"], inner, box=c["box"], pbc=7), want)
        run(eng, hr.case("tric_a_pbc7"))
        assert np.array_equal(eng.within_set(0.3, c["xyz"], ox, c["xyz"], inner, box=c["box"], pbc=7), want)
    finally:
        eng.within_hold(False)


# ---------------------------------------------------------------- 8. the error table

def raw_call(eng, c, *, kind=1, xyz2_shift=0, natoms2=None, n2=None, hoff=None, hidx=None, nh=None, angle_kind=0, angle=150.0, max_ha=0.0, groups=None,
             want_map=False, frames=False):
    """the C entry with pre-filled outputs; returns (status, outputs untouched?)"""
    a = api()
    d, keep = eng._contacts_desc(kind, 0.35, None, c["donors"], None, c["acceptors"], 7)
    d.xyz1 = c["xyz"].ctypes.data
    d.xyz2 = c["xyz"].ctypes.data + xyz2_shift
    d.natoms1 = len(c["xyz"])
    d.natoms2 = len(c["xyz"]) if natoms2 is None else natoms2
    if n2 is not None:
        d.n2 = n2                                  # (refused before the index is read)
    b9 = np.ascontiguousarray(c["box"].T).reshape(9)
    d.box9 = b9.ctypes.data
    hoff = c["hoff"] if hoff is None else hoff
    hidx = c["hidx"] if hidx is None else hidx
    nh = len(hidx) if nh is None else nh
    don = np.full(len(c["donors"]), 7, np.uint64)
    acc = np.full(len(c["acceptors"]), 8, np.uint64)
    G = 4
    m = np.full((G, G), 9, np.uint64)
    g = None
    if groups is not None:
        g = a.ContactGroups()
        g.group1, g.group2 = groups[0].ctypes.data, groups[1].ctypes.data
        g.ngroups1, g.ngroups2 = groups[2], groups[3]
    cnt = C.c_uint64(12345)
    mp = m.ctypes.data if (want_map or groups is not None) else None
    if frames:
        per = np.full(1, 6, np.uint64)
        tot, uni = C.c_uint64(1), C.c_uint64(2)
        rc = eng.lib.molar_hip_hbonds_frames(eng.ctx, C.byref(d), hoff.ctypes.data, hidx.ctypes.data, nh, angle_kind, angle, max_ha, 1, 0, None,
                                             C.byref(g) if g else None, per.ctypes.data, don.ctypes.data, acc.ctypes.data, mp, C.byref(tot),
                                             C.byref(uni))
        clean = per[0] == 6 and tot.value == 1 and uni.value == 2
    else:
        rc = eng.lib.molar_hip_hbonds_counts(eng.ctx, C.byref(d), hoff.ctypes.data, hidx.ctypes.data, nh, angle_kind, angle, max_ha,
                                             C.byref(g) if g else None, don.ctypes.data, acc.ctypes.data, mp, C.byref(cnt))
        clean = cnt.value == 12345
    return rc, bool(clean and np.all(don == 7) and np.all(acc == 8) and np.all(m == 9))


def bad_labels(c, where):
    g1 = np.zeros(len(c["donors"]), np.uint32)
    g2 = np.zeros(len(c["acceptors"]), np.uint32)
    (g1 if where == 1 else g2)[-1] = 4
    return g1, g2, 4, 4


@pytest.mark.parametrize("frames", [False, True])
def test_error_table(eng, frames):
    c = hr.case("ortho_pbc7")
    off, hidx = c["hoff"], c["hidx"]
    dec = off.copy(); dec[5] = dec[4] - 1
    short = off.copy(); short[-1] -= 1
    late = off.copy(); late[0] = 1
    wild = hidx.copy(); wild[17] = len(c["xyz"])
    rows = [
        (dict(kind=0), INVALID_ARGUMENT), (dict(kind=2), INVALID_ARGUMENT), (dict(kind=3), INVALID_ARGUMENT),
        (dict(xyz2_shift=12), INVALID_ARGUMENT), (dict(natoms2=len(c["xyz"]) - 1), INVALID_ARGUMENT),
        (dict(hidx=wild), INVALID_ARGUMENT),
        (dict(hoff=dec), INVALID_ARGUMENT), (dict(hoff=short), INVALID_ARGUMENT), (dict(hoff=late), INVALID_ARGUMENT),
        (dict(nh=len(hidx) + 1), INVALID_ARGUMENT),
        (dict(angle=-0.5), INVALID_ARGUMENT), (dict(angle=180.5), INVALID_ARGUMENT), (dict(angle=float("nan")), INVALID_ARGUMENT),
        (dict(max_ha=-0.1), INVALID_ARGUMENT), (dict(angle_kind=2), INVALID_ARGUMENT), (dict(angle_kind=-1), INVALID_ARGUMENT),
        (dict(want_map=True), INVALID_ARGUMENT),                                  # a map without labels
        (dict(groups=bad_labels(c, 1)), INVALID_ARGUMENT), (dict(groups=bad_labels(c, 2)), INVALID_ARGUMENT),
        (dict(nh=1 << 32), TOO_LARGE), (dict(n2=1 << 32), TOO_LARGE),
        (dict(groups=(np.zeros(len(c["donors"]), np.uint32), np.zeros(len(c["acceptors"]), np.uint32), 1 << 13, (1 << 11) + 1)), TOO_LARGE),
    ]
    for kw, want in rows:
        rc, untouched = raw_call(eng, c, frames=frames, **kw)
        assert rc == want, (kw.keys(), rc)
        assert untouched, kw.keys()
        assert eng.lib.molar_hip_last_error()
    # a good request through the same path, so that the rows above mean something
    rc, untouched = raw_call(eng, c, frames=frames)
    assert rc == 0 and not untouched


def test_labels_and_hydrogens_in_device_memory_are_checked(eng):
    import torch
    a = api()
    c = hr.case("ortho_pbc7")
    wild = c["hidx"].astype(np.int64); wild[3] = len(c["xyz"])
    with pytest.raises(a.MolarHipError) as ei:
        eng.hbonds(c["xyz"], c["donors"], (c["hoff"], torch.from_numpy(wild).cuda()), c["acceptors"], box=c["box"], pbc=7)
    assert ei.value.code == INVALID_ARGUMENT
    g1, g2, G1, G2 = bad_labels(c, 2)
    m = torch.full((G1, G2), 9, dtype=torch.int64, device="cuda")
    with pytest.raises(a.MolarHipError) as ei:
        eng.hbonds(c["xyz"], c["donors"], (c["hoff"], c["hidx"]), c["acceptors"], box=c["box"], pbc=7, group1=torch.from_numpy(g1.astype(np.int32)).cuda(),
                   ngroups1=G1, group2=torch.from_numpy(g2.astype(np.int32)).cuda(), ngroups2=G2, cmap=m)
    assert ei.value.code == INVALID_ARGUMENT and bool((m == 9).all())


def test_fill_without_count_and_pipelined_searches(orc32):
    from molar_amd.api import Engine
    a = api()
    c = hr.case("ortho_pbc7")
    e = Engine(0)
    try:
        assert e.lib.molar_hip_hbonds_fill(e.ctx, None, None, None, None) == NO_SEARCH
        assert e.lib.molar_hip_hbonds_frames_fill(e.ctx, None, None, None, None, None, None, None, None) == NO_SEARCH
        import torch
        xyz = torch.from_numpy(c["xyz"]).cuda()
        d, keep = e.make_search_desc(a.SEARCH_SINGLE, 0.35, xyz, box=c["box"], pbc=7)
        t = e.search_resident_begin(d)
        with pytest.raises(a.MolarHipError) as ei:
            run(e, c)
        assert ei.value.code == INVALID_ARGUMENT and "pipelined" in str(ei.value)
        e.search_resident_end(t)
        assert run(e, c).count == len(hr.reference(orc32, "ortho_pbc7")["triples"])
    finally:
        e.close()


def test_pymolar_style_front_end(eng, orc32):
    """hbond_donors and hbonds() on selections.  The cell is 1.5 times as long as water density makes it: no hydrogen is
    nearer than 0.13 nm to an oxygen of another water, so the nearest heavy atom within 0.12 nm is the generator's own."""
    from molar_amd import synth
    a = api()
    nw = 400
    c = dict(hr.case("ortho_pbc7"))
    c["box"] = synth.box_ortho(3 * nw) * np.float32(1.5)
    c["xyz"] = hr.waters(nw, c["box"], 31, 7)
    c["donors"], c["hoff"], c["hidx"], c["acceptors"] = hr.water_topology(nw)
    ref = hr.reference(orc32, "front_end", c)
    assert float(ref["clearance"].min()) > 1.0 and len(ref["triples"]) > 0
    top = a.Topology(np.ones(3 * nw, np.float32))
    state = a.State(c["xyz"], a.PeriodicBox.from_matrix(c["box"]))
    ox = a.Sel(top, state, c["donors"], engine=eng)
    hyd = a.Sel(top, state, c["hidx"], engine=eng)
    off, hidx = a.hbond_donors(ox, hyd)
    assert np.array_equal(off, c["hoff"]) and np.array_equal(hidx, c["hidx"])
    r = a.hbonds(ox, ox, sel_h=hyd, dims=(True, True, True), groups1=np.arange(nw) % 3, groups2=np.arange(nw) % 2)
    assert np.array_equal(r.triples, ref["triples"]) and r.map.shape == (3, 2) and int(r.map.sum()) == r.count


def test_worst_fractions_are_reported():
    """(runs last: prints the largest fraction of each bound the comparisons above came to)"""
    print("worst fractions of the bounds:", WORST)
    assert all(v <= 1.0 for v in WORST.values())
