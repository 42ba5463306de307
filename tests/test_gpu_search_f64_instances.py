"""Every instance of the f64 pair search (search_f64.hip) against the f64 oracle, on inputs built to reach it: the register
instances of 1-4 chunks and the chunk loop for every kind at pinned cell occupancies (64/65, 128/129, 192/193, 256/257), the
same-cell chunk skip, the seven wrap masks with either sign of the adjacent-image shift, plans of more than 2^20 slots, the
grid-stride reductions of the bounding box and of the radii, non-finite and degenerate inputs, and a slice of the randomised
differential test.  Every comparison is exact: ids and order, distances as float64, histogram bins as integers.  The inputs
are those of tests/search_f64_cases.py, checked without a GPU by tests/test_search_f64_cases_cpu.py."""
import importlib.util
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import search_f64_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = sc.EPS


@pytest.fixture(scope="module")
def eng():
    from molar_amd import build
    from molar_amd.api import Engine
    build.build_library()
    return Engine(0)


def api():
    import molar_amd.api as a
    return a


def to_host(got):
    if isinstance(got, tuple):
        return tuple(to_host(g) for g in got)
    if hasattr(got, "data_ptr"):
        h = got.cpu().numpy()
        return h.view(np.uint64) if h.dtype == np.int64 else h
    return got


def same(got, ref, what=""):
    """(i, j, d) equal to the oracle's, entry by entry; on a mismatch the first differing index is reported."""
    got = to_host(got)
    want = (ref["i"], ref["j"], ref["d"])
    assert got[2].dtype == np.float64
    n = min(len(got[0]), len(want[0]))
    bad = np.zeros(n, bool)
    for g, w in zip(got, want):
        bad |= g[:n] != w[:n]                       # (no NaN distance is ever a hit)
    if bad.any() or len(got[0]) != len(want[0]):
        k = int(np.argmax(bad)) if bad.any() else n
        lo, hi = max(k - 1, 0), k + 2
        pytest.fail(f"{what}: {len(got[0])} pairs, oracle {len(want[0])}; first difference at {k}: engine "
                    f"{[g[lo:hi].tolist() for g in got]}, oracle {[w[lo:hi].tolist() for w in want]}")
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def same_ids(got, ref, what=""):
    got = to_host(got)
    if not np.array_equal(got, ref["i"]):
        n = min(len(got), len(ref["i"]))
        bad = np.flatnonzero(got[:n] != ref["i"][:n])
        pytest.fail(f"{what}: {len(got)} ids, oracle {len(ref['i'])}; first difference at {int(bad[0]) if len(bad) else n}")


# ---------------------------------------------------------------------------------------------------------- 2. instance sweep

def run_case(eng, c, device=False):
    """The engine's result for a case of search_f64_cases.sweep_case: host arrays, or coordinates resident and the result left
    on the device."""
    a = api()
    kind = {"single": a.SEARCH_SINGLE, "double": a.SEARCH_DOUBLE, "vdw": a.SEARCH_DOUBLE_VDW, "within": a.SEARCH_WITHIN}[c["kind"]]
    kw = dict(box=c["box"], pbc=c["pbc"]) if c["pbc"] else {}
    if c["kind"] == "within" and not c["pbc"]:
        kw = dict(lower=c["lower"], upper=c["upper"])
    p1, p2 = c["p1"], c["p2"]
    if device:
        import torch
        p1 = torch.from_numpy(p1).cuda()
        p2 = None if p2 is None else torch.from_numpy(p2).cuda()
        kw["device_out"] = True
    rc = None if c["kind"] == "vdw" else c["rc"]
    return eng.search_f64(kind, rc, p1, None, p2, None, vdw1=c["v1"], vdw2=c["v2"], **kw), kind, kw


@pytest.mark.parametrize("situation", sc.SITUATIONS)
@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("K2", sc.K2S)
def test_every_instance_of_every_kind_at_pinned_occupancies(eng, orc64, K2, kind, situation):
    """Exactly K2 atoms in every second cell (without a box: the fullest second cell in K2's bucket), rows in three slots per
    entry with a short last one (two sets: 130 per cell; one set: K2, so that same-cell entries have slots with i0 >= 64 from
    65 atoms on and the chunk skip sees i = 62, 63, 64, 127, 128).  Box situations: >= 4 cells per dimension (wrapped entries
    classified by the adjacent image, a triclinic box's corner entries exact), 2-3 cells (every wrapped entry exact, duplicate
    cell pairs), partial periodicity, no box.  The list, the fused histogram and the within set must all be the oracle's."""
    c = sc.sweep_case(K2, kind, situation)
    ref = sc.sweep_reference(orc64, c)
    slots = sc.sweep_check_inputs(c, ref)              # dims, occupancies, the result's size: asserted
    assert slots > 0
    what = f"{kind} K2={c['K2']} K1={c['K1']} {situation} dims {ref['dims']} slots {slots}"
    got, akind, kw = run_case(eng, c)
    assert eng.grid_dims_f64() == ref["dims"]
    if kind == "within":
        same_ids(got, ref, what)
        wkw = {k: v for k, v in kw.items() if k != "device_out"}
        ids = eng.within_set_f64(c["rc"], c["p1"], None, c["p2"], None, **wkw)
        assert np.array_equal(ids, np.unique(ref["i"])), what
        return
    same(got, ref, what)
    if kind in ("single", "double"):
        got, _, _ = run_case(eng, c, device=True)
        assert eng.grid_dims_f64() == ref["dims"]
        same(got, ref, what + " (resident)")
    nbins, hmax = 300, 1.0
    want = orc64.histogram_add(0.0, hmax, nbins, ref["d"]).astype(np.uint64)
    bins, cnt = eng.search_histogram_f64(akind, None if kind == "vdw" else c["rc"], 0.0, hmax, nbins, c["p1"], None, c["p2"], None,
                                         vdw1=c["v1"], vdw2=c["v2"], **kw)
    assert cnt == len(ref["d"]) and np.array_equal(bins, want), what + " (histogram)"


# ------------------------------------------------------------------------------------------ 3. the seven wrap masks, both signs

def test_the_seven_wrap_masks_with_either_sign_of_the_shift(eng, orc64):
    """Entries across the periodic boundary are classified by the distance to the second cell's adjacent image, b + S, where S
    adds or subtracts the box vector of every wrapped dimension according to which of the two cells went round.  Pairs at
    rc * (1 +- 1e-15.5 .. 1e-8) planted across each face, edge and corner of a sheared cell of 10 x 10 x 10 cells, first atom
    on either side: at least 200 oracle hits within 1e-9 of the cutoff for EACH of the seven masks, and the engine's lists
    equal to the oracle's for one set and for two."""
    a = api()
    box, rc, pos = sc.wrap_masks_case()
    ob = orc64.box_from_matrix(box)
    ref = orc64.search_single_pbc(rc, pos, ob, 7, nthreads=16)
    assert min(ref["dims"]) >= 4
    per_mask = sc.near_cutoff_hits_per_mask(pos, box, rc, ref)
    print("hits within 1e-9 of the cutoff per wrap mask:", per_mask.tolist())
    assert (per_mask[1:] >= 200).all(), per_mask
    same(eng.search_f64(a.SEARCH_SINGLE, rc, pos, box=box, pbc=7), ref, "single")
    assert eng.grid_dims_f64() == ref["dims"]
    # two sets: the first atom of every planted pair in the first set, its partner in the second; both orders of every entry
    p1, p2 = pos[0::2], pos[1::2]
    ref2 = orc64.search_double_pbc(rc, p1, p2, ob, 7, nthreads=16)
    near = np.abs(ref2["d"] / rc - 1.0) < 1e-9
    c1, c2 = sc.cells_box(p1[ref2["i"][near].astype(int)], box, ref2["dims"]), sc.cells_box(p2[ref2["j"][near].astype(int)], box, ref2["dims"])
    d = c2 - c1
    dims = np.asarray(ref2["dims"])
    for dim in range(3):                   # the second atom's cell went round (+) and the first atom's did (-), in every dimension
        assert ((d[:, dim] == -(dims[dim] - 1)).sum() >= 200) and ((d[:, dim] == dims[dim] - 1).sum() >= 200), (dim, d[:, dim])
    same(eng.search_f64(a.SEARCH_DOUBLE, rc, p1, None, p2, None, box=box, pbc=7), ref2, "double")
    for pbc in (3, 5, 6):
        same(eng.search_f64(a.SEARCH_SINGLE, rc, pos, box=box, pbc=pbc), orc64.search_single_pbc(rc, pos, ob, pbc, nthreads=16), f"pbc {pbc}")


@pytest.mark.timeout(900)
@pytest.mark.parametrize("boxkind,L,floor_pairs,floor_near", [("dodecahedron", 60.0, 6000, 1500), ("sheared", 40.0, 5000, 600),
                                                              ("sheared_huge", 160.0, 4000, 600)])
def test_wrapped_entries_in_large_sheared_boxes(eng, orc64, boxkind, L, floor_pairs, floor_near):
    """The shift convention and the pruning margin at large L / rc: a 60 nm rhombic dodecahedron and a strongly sheared 40 nm
    box at rc 0.3, the same shear at 160 nm and rc 1.0, 12 000 pairs across the faces at rc * (1 +- 1e-15.5 .. 1e-8).  (The
    reference's half-shell grid is incomplete in positively sheared boxes, so not every planted pair is found: the floors are
    well below what the oracle finds.)"""
    a = api()
    rc = 0.3 if L < 100 else 1.0
    if boxkind == "dodecahedron":
        box = np.array([[L, 0, L / 2], [0, L, L / 2], [0, 0, L * np.sqrt(2) / 2]])
    else:
        box = np.array([[L, 0.45 * L, 0.9 * L], [0, L, 0.8 * L], [0, 0, L]])
    pos = sc.boundary_pairs(box, rc, 12000, seed=int(L))
    ref = orc64.search_single_pbc(rc, pos, orc64.box_from_matrix(box), 7, nthreads=16)
    assert min(ref["dims"]) >= 4
    near = int((np.abs(ref["d"] / rc - 1.0) < 1e-9).sum())
    print(boxkind, "pairs", len(ref["i"]), "within 1e-9 of the cutoff", near)
    assert len(ref["i"]) > floor_pairs and near > floor_near
    same(eng.search_f64(a.SEARCH_SINGLE, rc, pos, box=box, pbc=7), ref, boxkind)
    assert eng.grid_dims_f64() == ref["dims"]


# ------------------------------------------------------------------------------------------ 4. launch shapes and reductions

def same_in_blocks(got, ref):
    i, j, d = got
    assert len(i) == len(ref["i"])
    step = 1 << 24
    for k in range(0, len(i), step):
        same((i[k:k + step], j[k:k + step], d[k:k + step]), {n: ref[n][k:k + step] for n in "ijd"}, f"block at {k}")


def test_plan_of_more_than_2_20_slots_takes_the_2d_launch(eng, orc64):
    """400 000 atoms at 100 nm^-3, rc 0.3: more slots than one grid dimension of the launch is given (2^20), so the slot is
    blockIdx.y * gridDim.x + blockIdx.x.  Frame and result resident."""
    import torch
    a = api()
    box, rc, pos = sc.many_slots_case()
    ref = orc64.search_single_pbc(rc, pos, orc64.box_from_matrix(box), 7, nthreads=16)
    slots = sc.plan_slots(sc.occupancy_box(pos, box, ref["dims"]), None, ref["dims"], 7)
    assert slots > 2 ** 20 and len(ref["i"]) > 2_000_000
    got = eng.search_f64(a.SEARCH_SINGLE, rc, torch.from_numpy(pos).cuda(), box=box, pbc=7, device_out=True)
    assert eng.grid_dims_f64() == ref["dims"]
    same_in_blocks(got, ref)
    want = orc64.histogram_add(0.0, rc, 200, ref["d"]).astype(np.uint64)
    bins, cnt = eng.search_histogram_f64(a.SEARCH_SINGLE, rc, 0.0, rc, 200, pos, box=box, pbc=7)
    assert cnt == len(ref["d"]) and np.array_equal(bins, want)


@pytest.mark.parametrize("side", ["positive", "negative"])
def test_bounding_box_of_200k_atoms_without_a_box(eng, orc64, side):
    """Selections above 256 * 256 atoms take the grid-stride loop of the bounding-box reduction.  All coordinates positive, or
    all negative: one corner of the box is then the zero the reference seeds its minimum and maximum with."""
    import torch
    a = api()
    rng = np.random.default_rng(13)
    n, rc = 200_000, 0.5
    pos = rng.random((n, 3)) * 12.6 + (0.3 if side == "positive" else -12.9)
    assert (pos > 0).all() if side == "positive" else (pos < 0).all()
    ref = orc64.search_single(rc, pos, nthreads=16)
    lower, upper = sc.bounding_box(rc, pos)
    assert ref["dims"] == sc.dims_of(lower, upper, rc) == (27, 27, 27)
    assert (lower == -(rc + EPS)).all() if side == "positive" else (upper == rc + EPS).all()       # the zero seed
    assert len(ref["i"]) > 4_000_000
    xyz = torch.from_numpy(pos).cuda() if side == "negative" else pos
    same_in_blocks(to_host(eng.search_f64(a.SEARCH_SINGLE, rc, xyz)), ref)
    assert eng.grid_dims_f64() == ref["dims"]
    perm = rng.permutation(n)
    i1, i2 = np.sort(perm[:100_000]).astype(np.uint64), np.sort(perm[100_000:]).astype(np.uint64)
    assert min(len(i1), len(i2)) > 65_536
    ref = orc64.search_double(rc, pos[i1.astype(int)], pos[i2.astype(int)], ids1=i1, ids2=i2, nthreads=16)
    assert len(ref["i"]) > 2_000_000
    if side == "negative":
        i1, i2 = torch.from_numpy(i1.astype(np.int64)).cuda(), torch.from_numpy(i2.astype(np.int64)).cuda()
    same_in_blocks(to_host(eng.search_f64(a.SEARCH_DOUBLE, rc, xyz, i1, xyz, i2)), ref)
    assert eng.grid_dims_f64() == ref["dims"]


@pytest.mark.parametrize("use_box", [True, False])
def test_vdw_maximum_over_more_than_65536_radii_with_nans(eng, orc64, use_box):
    """vdw.iter().cloned().reduce(Float::max) ignores NaN (distance_search.rs:781-783).  70 000 radii per set, on the host
    (the std::fmax loop) and on the device (fmax64_kernel: 256 workgroups, so a thread of the first 18 reads two radii, 65 536
    apart).  NaN at every 64th radius (all that lane 0 of a wave reads), one aligned block of 256 NaNs read by a workgroup
    that reads nothing else (its partial is NaN), and a NaN 65 536 after each set's largest radius, so that the thread which
    holds the maximum reads a NaN next.  Both forms must give the oracle's list."""
    import torch
    a = api()
    rng = np.random.default_rng(19)
    n = 70_000
    L = (2 * n / 100.0) ** (1.0 / 3.0)
    box = np.diag([L, L, L])
    p1, p2 = rng.random((n, 3)) * L, rng.random((n, 3)) * L
    vs = []
    for w in range(2):
        v = rng.uniform(0.1, 0.19, n)
        v[::64] = np.nan
        v[25_600:25_856] = np.nan                  # workgroup 100 reads these 256 and (25 600 + 65 536 > n) nothing else
        v[1000 + w] = 0.2                          # the maximum, and what the same thread reads after it
        v[1000 + w + 65_536] = np.nan
        assert np.nanmax(v) == 0.2 and np.isnan(v).sum() > 1300
        vs.append(v)
    v1, v2 = vs
    if use_box:
        ref = orc64.search_double_vdw_pbc(p1, p2, v1, v2, orc64.box_from_matrix(box), 7, nthreads=16)
        kw = dict(box=box, pbc=7)
    else:
        ref = orc64.search_double_vdw(p1, p2, v1, v2, nthreads=16)
        kw = {}
    cutoff = (0.2 + 0.2) + EPS
    assert ref["dims"] == (sc.dims_of(np.zeros(3), np.diag(box), cutoff) if use_box else sc.dims_of(*sc.bounding_box(cutoff, p1, p2), cutoff))
    assert len(ref["i"]) > 100_000
    host = eng.search_f64(a.SEARCH_DOUBLE_VDW, None, p1, None, p2, None, vdw1=v1, vdw2=v2, **kw)
    assert eng.grid_dims_f64() == ref["dims"]
    same(host, ref, "host radii")
    dev = eng.search_f64(a.SEARCH_DOUBLE_VDW, None, p1, None, p2, None, vdw1=torch.from_numpy(v1).cuda(), vdw2=torch.from_numpy(v2).cuda(), **kw)
    assert eng.grid_dims_f64() == ref["dims"]
    same(dev, ref, "device radii")
    nan1, nan2 = np.flatnonzero(np.isnan(v1)), np.flatnonzero(np.isnan(v2))
    assert not np.isin(host[0], nan1).any() and not np.isin(host[1], nan2).any()


# ------------------------------------------------------------------------------------------ 5. degenerate and non-finite inputs

def test_non_finite_coordinates_and_degenerate_inputs_f64(eng, orc64):
    """NaN / inf coordinates never compare as hits in the reference (and land in cell 0 through the saturating `as usize`
    cast, where they enter that cell's bounding box and the row pruning as inf - inf); the engine must agree and must not
    fault.  Also: coincident atoms (d == 0.0 exactly), an empty second set."""
    from molar_amd import synth
    a = api()
    n = 3000
    box = synth.box_a(n).astype(np.float64)
    pos = synth.frame(n, synth.box_a(n)).astype(np.float64) + np.random.default_rng(1).normal(0, 1e-9, (n, 3))
    pos[10] = [np.nan, 1.0, 1.0]
    pos[11] = [np.inf, 1.0, 1.0]
    pos[12] = [1.0, -np.inf, np.nan]
    pos[500] = pos[499]                      # coincident pair: d2 == 0, sqrt(0) == 0 exactly
    ob = orc64.box_from_matrix(box)
    for pbc in (7, 3, 5, 6):
        ref = orc64.search_single_pbc(0.5, pos, ob, pbc)
        got = eng.search_f64(a.SEARCH_SINGLE, 0.5, pos, box=box, pbc=pbc)
        same(got, ref, f"pbc {pbc}")
        gi, gj, gd = got
        assert len(gi) > 1000 and not np.isin([10, 11, 12], np.concatenate([gi, gj])).any()
        hit = (gi == 499) & (gj == 500)
        assert hit.sum() == 1 and gd[hit][0] == 0.0
    i1, i2 = np.arange(0, n, 2, dtype=np.uint64), np.arange(1, n, 2, dtype=np.uint64)
    same(eng.search_f64(a.SEARCH_DOUBLE, 0.5, pos, i1, pos, i2, box=box, pbc=7),
         orc64.search_double_pbc(0.5, pos[0::2], pos[1::2], ob, 7, ids1=i1, ids2=i2), "double")
    same_ids(eng.search_f64(a.SEARCH_WITHIN, 0.5, pos, i1, pos, i2, box=box, pbc=7),
             orc64.search_within_pbc(0.5, pos[0::2], pos[1::2], ob, 7, ids1=i1, ids2=i2), "within")
    want = orc64.histogram_add(0.0, 0.5, 100, orc64.search_single_pbc(0.5, pos, ob, 7)["d"]).astype(np.uint64)
    bins, _ = eng.search_histogram_f64(a.SEARCH_SINGLE, 0.5, 0.0, 0.5, 100, pos, box=box, pbc=7)
    assert np.array_equal(bins, want)
    # non-periodic driver: NaN only (an infinite coordinate makes the reference's zero-seeded bounding box, hence its grid,
    # infinite - it cannot run there either)
    pos2 = pos.copy()
    pos2[11] = [2.0, 1.0, 1.0]
    pos2[12] = [1.0, 2.0, np.nan]
    ref = orc64.search_single(0.5, pos2)
    assert len(ref["i"]) > 1000
    same(eng.search_f64(a.SEARCH_SINGLE, 0.5, pos2), ref, "no box")
    # an empty second set, an empty first set
    none, some = np.zeros(0, np.uint64), np.arange(100, dtype=np.uint64)
    for s1, s2 in ((some, none), (none, some), (none, none)):
        for kw in (dict(box=box, pbc=7), {}):
            i, j, d = eng.search_f64(a.SEARCH_DOUBLE, 0.5, pos2, s1, pos2, s2, **kw)
            assert len(i) == len(j) == len(d) == 0
            ref = orc64.search_double_pbc(0.5, pos2[s1.astype(int)], pos2[s2.astype(int)], ob, 7) if kw \
                else orc64.search_double(0.5, pos2[s1.astype(int)], pos2[s2.astype(int)])
            assert len(ref["i"]) == 0
        assert len(eng.search_f64(a.SEARCH_WITHIN, 0.5, pos2, s1, pos2, s2, box=box, pbc=7)) == 0
        assert len(eng.within_set_f64(0.5, pos2, s1, pos2, s2, box=box, pbc=7)) == 0
    assert len(eng.search_f64(a.SEARCH_SINGLE, 0.5, pos2, none, box=box, pbc=7)[0]) == 0


def test_tiny_inputs_f64(eng, orc64):
    a = api()
    box = np.diag([5.0, 5.0, 5.0])
    ob = orc64.box_from_matrix(box)
    for pos in ([[1.0, 1.0, 1.0]], [[1.0, 1.0, 1.0], [1.2, 1.0, 1.0]], [[0.1, 0.1, 0.1], [4.9, 4.9, 4.9]],
                [[1.0, 1.0, 1.0], [3.0, 3.0, 3.0]], [[1.0, 1.0, 1.0], [1.0, 1.0, 1.0]]):
        pos = np.array(pos, np.float64)
        same(eng.search_f64(a.SEARCH_SINGLE, 0.5, pos, box=box, pbc=7), orc64.search_single_pbc(0.5, pos, ob, 7), "box")
        same(eng.search_f64(a.SEARCH_SINGLE, 0.5, pos), orc64.search_single(0.5, pos), "no box")
        if len(pos) == 2:
            same(eng.search_f64(a.SEARCH_DOUBLE, 0.5, pos[:1], None, pos[1:], None, box=box, pbc=7),
                 orc64.search_double_pbc(0.5, pos[:1], pos[1:], ob, 7), "double")
    ref = orc64.search_single_pbc(0.5, np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0]]), ob, 7)
    assert len(ref["i"]) == 1 and ref["d"][0] == 0.0


def test_local_and_global_ids_f64(eng, orc64):
    """ids_local=True numbers the atoms by their place in the selection, as the reference does when it is given no ids."""
    from molar_amd import synth
    a = api()
    n = 6000
    box = synth.box_a(n).astype(np.float64)
    rng = np.random.default_rng(8)
    pos = rng.random((n, 3)) @ box.T + rng.normal(0, 0.05, (n, 3))
    ob = orc64.box_from_matrix(box)
    sel = np.sort(rng.choice(n, n // 2, replace=False)).astype(np.uint64)
    sel2 = np.setdiff1d(np.arange(n, dtype=np.uint64), sel)
    p1, p2 = pos[sel.astype(int)], pos[sel2.astype(int)]
    for local in (False, True):
        ids1, ids2 = (None, None) if local else (sel, sel2)
        ref = orc64.search_single_pbc(0.6, p1, ob, 7, ids=ids1)
        assert len(ref["i"]) > 1000 and (ref["i"].max() >= n // 2) == (not local)
        same(eng.search_f64(a.SEARCH_SINGLE, 0.6, pos, sel, box=box, pbc=7, ids_local=local), ref, f"single local={local}")
        same(eng.search_f64(a.SEARCH_SINGLE, 0.6, pos, sel, ids_local=local), orc64.search_single(0.6, p1, ids=ids1), f"no box local={local}")
        same(eng.search_f64(a.SEARCH_DOUBLE, 0.6, pos, sel, pos, sel2, box=box, pbc=7, ids_local=local),
             orc64.search_double_pbc(0.6, p1, p2, ob, 7, ids1=ids1, ids2=ids2), f"double local={local}")
        same_ids(eng.search_f64(a.SEARCH_WITHIN, 0.6, pos, sel, pos, sel2, box=box, pbc=7, ids_local=local),
                 orc64.search_within_pbc(0.6, p1, p2, ob, 7, ids1=ids1, ids2=ids2), f"within local={local}")
        want = np.unique(orc64.search_within_pbc(0.6, p1, p2, ob, 7, ids1=ids1, ids2=ids2)["i"])
        assert np.array_equal(eng.within_set_f64(0.6, pos, sel, pos, sel2, box=box, pbc=7, ids_local=local), want)


def test_frame_dropped_whole_by_a_non_periodic_dimension(eng, orc64):
    """Atoms outside the box in a non-periodic dimension are dropped; when that is every atom the plan has no slots: the
    engine returns nothing (and launches nothing over zero slots), and the next search on the same context is right."""
    a = api()
    rng = np.random.default_rng(4)
    box = np.diag([4.0, 4.0, 4.0])
    inside = rng.random((2000, 3)) * 4.0
    outside = inside + np.array([0.0, 0.0, 7.0])            # z is not periodic with pbc = 3
    ob = orc64.box_from_matrix(box)
    ref = orc64.search_single_pbc(0.6, outside, ob, 3)
    assert len(ref["i"]) == 0
    i, j, d = eng.search_f64(a.SEARCH_SINGLE, 0.6, outside, box=box, pbc=3)
    assert len(i) == len(j) == len(d) == 0
    assert len(eng.search_f64(a.SEARCH_DOUBLE, 0.6, outside, None, inside, None, box=box, pbc=3)[0]) == 0
    assert len(eng.search_f64(a.SEARCH_WITHIN, 0.6, outside, None, inside, None, box=box, pbc=3)) == 0
    assert len(eng.within_set_f64(0.6, outside, None, inside, None, box=box, pbc=3)) == 0
    bins, cnt = eng.search_histogram_f64(a.SEARCH_SINGLE, 0.6, 0.0, 0.6, 50, outside, box=box, pbc=3)
    assert cnt == 0 and not bins.any()
    ref = orc64.search_single_pbc(0.6, inside, ob, 3)
    assert len(ref["i"]) > 1000
    same(eng.search_f64(a.SEARCH_SINGLE, 0.6, inside, box=box, pbc=3), ref, "after the empty frame")
    same(eng.search_f64(a.SEARCH_SINGLE, 0.6, outside, box=box, pbc=7), orc64.search_single_pbc(0.6, outside, ob, 7), "wrapped instead")


def test_empty_device_selection_selects_nothing(eng, orc64):
    """Regression (found by the randomised slice): an empty torch index tensor has data_ptr() == 0, and a NULL index means
    "all atoms" to the library - an empty selection resident in HBM came back as a search over every atom.  f64 and f32."""
    import torch
    a = api()
    rng = np.random.default_rng(6)
    box = np.diag([4.0, 4.0, 4.0])
    pos = rng.random((3000, 3)) * 4.0
    dpos = torch.from_numpy(pos).cuda()
    none = torch.zeros(0, dtype=torch.int64, device="cuda")
    some = torch.arange(100, dtype=torch.int64, device="cuda")
    assert len(orc64.search_single_pbc(0.6, pos[:0], orc64.box_from_matrix(box), 7)["i"]) == 0
    for kw in (dict(box=box, pbc=7), {}):
        assert len(eng.search_f64(a.SEARCH_SINGLE, 0.6, dpos, none, **kw)[0]) == 0
        for s1, s2 in ((some, none), (none, some)):
            assert len(eng.search_f64(a.SEARCH_DOUBLE, 0.6, dpos, s1, dpos, s2, **kw)[0]) == 0
    assert len(eng.search_f64(a.SEARCH_WITHIN, 0.6, dpos, some, dpos, none, box=box, pbc=7)) == 0
    assert len(eng.within_set_f64(0.6, dpos, none, dpos, some, box=box, pbc=7)) == 0
    bins, cnt = eng.search_histogram_f64(a.SEARCH_DOUBLE, 0.6, 0.0, 0.6, 50, dpos, some, dpos, none, box=box, pbc=7)
    assert cnt == 0 and not bins.any()
    pos32 = pos.astype(np.float32)
    assert eng.search_count(a.SEARCH_SINGLE, 0.6, pos32, none, box=box.astype(np.float32), pbc=7) == 0
    assert eng.search_count(a.SEARCH_DOUBLE, 0.6, pos32, some, pos32, none, box=box.astype(np.float32), pbc=7) == 0
    assert eng.search_count(a.SEARCH_DOUBLE, 0.6, pos32, some.cpu().numpy().astype(np.uint64), pos32, some + 200, box=box.astype(np.float32), pbc=7) > 0


# ------------------------------------------------------------------------------------------ 6. the fuzzer in the suite

def test_randomised_differential_f64(eng):
    """tools/fuzz_search_f64.py: random boxes / cutoffs / densities / periodicity masks / selections / kinds, local ids,
    non-finite coordinates, NaN radii, empty selections, crowded cells, host and resident inputs - every case bit-identical to
    the f64 oracle, few cases skipped, and enough of them with entries classified by the adjacent image."""
    spec = importlib.util.spec_from_file_location("fuzz_search_f64", os.path.join(ROOT, "tools", "fuzz_search_f64.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    stats = mod.run(250, 11, eng=eng, verbose=True)
    assert stats["fails"] == 0
    assert stats["skipped"] <= 250 * 5 // 100
    assert stats["full_pbc_4cells"] >= 15
