"""Minimum distances on the GPU (molar_hip_mindist / _f64: the partition by label, the rows passes, the groups pass with its
segmented minimum and 64-bit atomicMin, the folds over column splits, rows and frames) against the longdouble numpy reference
of tests/mindist_ref.py: every distance within the bound derived there, and pair, near1, mat_freq, frame_ok, nvalid and the
positions of NaN and inf for equality - the reference asserts on its own inputs that every such decision is separated by more
than the bounds, so no case is left out.  Both entries see the same numbers (f32 inputs, cast to f64 for the f64 entry).
The column splits are overridden to 3 and frame_block to 2, so that the small shapes stand either side of every size
molar_hip_mindist_plan reports.  The largest used fraction of each bound is printed by the last test."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mindist_ref as mr  # noqa: E402

pytestmark = pytest.mark.gpu
FLOATS = (("dist", "b_dist"), ("atom1", "b_atom1"), ("atom2", "b_atom2"), ("mat", "b_mat"), ("mat_mean", "b_mean"), ("mat_min", "b_min"))
INTS = ("pair", "near1", "mat_freq", "frame_ok")
ALL = ("dist", "pair", "atom1", "near1", "atom2", "mat", "mat_mean", "mat_min", "mat_freq", "frame_ok", "nvalid")
FRACTIONS = {}
COL_SPLITS, FRAME_BLOCK, RW, RB, CT = mr.COL_SPLITS, mr.FRAME_BLOCK, mr.ROWS_WAVE, mr.ROWS_BLOCK, mr.COL_TILE
SIZES, SIZE_CASES, FRAME_CASES, ALL_CASES = mr.SIZES, mr.SIZE_CASES, mr.FRAME_CASES, mr.ALL_CASES


@pytest.fixture(autouse=True)
def small_plan(monkeypatch):
    monkeypatch.setenv("MOLAR_HIP_MINDIST_COL_SPLITS", str(COL_SPLITS))
    monkeypatch.setenv("MOLAR_HIP_MINDIST_FRAME_BLOCK", str(FRAME_BLOCK))


@pytest.fixture(scope="module")
def eng():
    from molar_amd import api
    return api.Engine()


@pytest.fixture(scope="module")
def m64(eng):
    from molar_amd import api
    return api.MeasureF64(eng)


def names_of(case, want=ALL):
    return tuple(n for n in want if not (case.same and n == "atom2"))


def call(entry, case, real, want=ALL, inputs=None, out=None, cutoff=mr.CUTOFF, frame_block=0):
    frames, boxes, idx1, idx2, lab1, lab2 = mr.case_inputs(case) if inputs is None else inputs
    return entry.min_distances(np.asarray(frames, real), idx1=idx1, idx2=idx2, labels1=lab1, labels2=lab2, ngroups1=case.G1 if lab1 is not None else None,
                               ngroups2=case.G2 if lab2 is not None else None, boxes=None if boxes is None else np.asarray(boxes, real), pbc=case.pbc,
                               same=case.same, exclude_same_group=case.excl, cutoff=cutoff, frame_block=frame_block, want=names_of(case, want), out=out,
                               n1=case.n1, n2=case.n2)


def check(got, ref, what):
    """Every distance within its bound, NaN and inf where the reference has them, integers equal; the fractions used are kept
    for the last test."""
    for name, bname in FLOATS:
        g = getattr(got, name)
        if g is None:
            continue
        g = np.asarray(g, np.float64)
        r, b = getattr(ref, name), getattr(ref, bname)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (what, name, "NaN positions")
        assert np.array_equal(np.isposinf(g), np.isposinf(r)), (what, name, "inf positions")
        fin = np.isfinite(r)
        if fin.any():
            err = np.abs(g[fin] - r[fin])
            # the reference is rounded to f64 for the comparison: one more half ulp
            bound = b[fin] + mr.U * np.abs(r[fin])
            frac = float(np.max(err / bound))
            print(f"{what}: {name} uses {frac:.3f} of its bound")
            FRACTIONS[name] = max(FRACTIONS.get(name, 0.0), frac)
            assert frac <= 1.0, (what, name, frac)
    for name in INTS:
        g = getattr(got, name)
        if g is not None:
            assert np.array_equal(np.asarray(g), getattr(ref, name)), (what, name)
    if got.nvalid is not None:
        assert int(got.nvalid[0]) == ref.nvalid, what


def both(eng, m64, case, inputs=None, **kw):
    out = []
    for entry, real, eps in ((eng, np.float32, mr.EPS32), (m64, np.float64, mr.EPS64)):
        if inputs is None:
            r = mr.case_reference(case, eps)
        else:
            frames, boxes, idx1, idx2, lab1, lab2 = inputs
            r = mr.reference(frames, boxes, np.arange(case.n1) if idx1 is None else idx1, idx2, lab1, lab2, case.G1, case.G2, case.pbc, case.same, case.excl,
                             mr.CUTOFF, eps, **kw)
        got = call(entry, case, real, inputs=inputs)
        check(got, r, f"{case.name} {np.dtype(real).name}")
        out.append(got)
    return out


def same_bits(a, b, names=ALL):
    for n in names:
        x, y = getattr(a, n), getattr(b, n)
        if x is None or y is None:
            continue
        x, y = np.asarray(x), np.asarray(y)
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), n


def test_the_shapes_cross_every_size_of_the_plan():
    from molar_amd import api
    _, rw, rb, ct, cs, fb = api.mindist_plan(5, 600, 3 * CT, want=ALL)
    assert (rw, rb, ct, cs, fb) == (RW, RB, CT, COL_SPLITS, FRAME_BLOCK)
    assert [api.mindist_plan(1, 10, n2)[4] for n2 in (CT - 1, CT, CT + 1, 2 * CT, 2 * CT + 1, 5 * CT)] == [1, 1, 2, 2, 3, 3]
    n1s, n2s = {a for a, _ in SIZES}, {b for _, b in SIZES}
    assert 1 in n1s
    for edge in (64, rw, rb):
        assert {edge - 1, edge, edge + 1} <= n1s, edge
    assert {1, ct - 1, ct, ct + 1, 2 * ct, 2 * ct + 1} <= n2s
    assert sorted(c.F for c in FRAME_CASES) == [1, fb, fb + 1, 2 * fb + 1]
    assert all(c.F * c.n1 * c.n2 <= 2 * 10 ** 5 for c in ALL_CASES)


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_every_output_within_its_bound(eng, m64, case):
    both(eng, m64, case)


def test_inside_one_set_is_symmetric_and_is_the_two_set_call_without_its_diagonal(m64):
    for name in ("same", "same_excl", "same_nolabels"):
        case = next(c for c in mr.CASES if c.name == name)
        frames, boxes, idx1, _, lab1, _ = mr.case_inputs(case)
        got = call(m64, case, np.float64)
        for mat in (got.mat, got.mat_mean[None], got.mat_min[None], got.mat_freq[None]):
            assert np.array_equal(mat, mat.transpose(0, 2, 1), equal_nan=mat.dtype.kind == "f"), name
        if case.excl:
            assert np.all(np.isposinf(got.mat[:, np.arange(case.G1), np.arange(case.G1)]))
            continue
        # a two-set call on the same atoms sees d(i, i) = 0 first: the reference of that call, with the diagonal of its matrix of
        # distances taken out by hand, is what the single-set call must give
        ref = mr.reference(frames, boxes, np.arange(case.n1), np.arange(case.n1), lab1, lab1, case.G1, case.G1, case.pbc, False, False, mr.CUTOFF, check=False)
        D = np.where(np.eye(case.n1, dtype=bool)[None], np.inf, ref.D.astype(np.float64))
        a1 = np.asarray(got.atom1)
        assert np.all(np.abs(a1 - D.min(axis=2)) <= np.take_along_axis(ref.B, D.argmin(axis=2)[..., None], axis=2)[..., 0] + mr.U * a1), name
        assert np.array_equal(np.asarray(got.near1), D.argmin(axis=2).astype(np.uint64)), name


def test_each_output_alone_equals_all_together(eng, m64):
    case = next(c for c in mr.CASES if c.name == "groups")
    for entry, real in ((eng, np.float32), (m64, np.float64)):
        full = call(entry, case, real)
        for name in ALL:
            one = call(entry, case, real, want=(name,))
            assert all(getattr(one, n) is None for n in ALL if n != name)
            same_bits(one, full, (name,))
        same_bits(call(entry, case, real, want=("dist", "pair", "atom2")), full, ("dist", "pair", "atom2"))       # dist from the pass over set 2


def test_frame_stride_and_row_strides(m64):
    case = next(c for c in mr.CASES if c.name == "groups")
    frames, boxes, idx1, idx2, lab1, lab2 = mr.case_inputs(case)
    full = call(m64, case, np.float64)
    wide = np.full((case.F, case.natoms + 7, 3), 1e30)
    wide[:, :case.natoms] = frames
    strided = wide[:, :case.natoms]
    a1 = np.full((case.F, case.n1 + 5), -1.0)
    n1 = np.full((case.F, case.n1 + 5), 7, np.uint64)
    a2 = np.full((case.F, case.n2 + 3), -1.0)
    out = [None, None, a1[:, :case.n1], n1[:, :case.n1], a2[:, :case.n2]] + [None] * 6
    got = call(m64, case, np.float64, want=("atom1", "near1", "atom2"), inputs=(strided, boxes, idx1, idx2, lab1, lab2), out=out)
    same_bits(got, full, ("atom1", "near1", "atom2"))
    assert np.all(a1[:, case.n1:] == -1.0) and np.all(n1[:, case.n1:] == 7) and np.all(a2[:, case.n2:] == -1.0), "the rest of a row is not touched"


def test_device_memory_on_both_sides(eng, m64):
    import torch
    case = next(c for c in mr.CASES if c.name == "groups_tric")
    frames, boxes, idx1, idx2, lab1, lab2 = mr.case_inputs(case)
    for entry, real in ((eng, np.float32), (m64, np.float64)):
        host = call(entry, case, real)
        t = lambda x, dt: None if x is None else torch.as_tensor(np.asarray(x).astype(dt)).cuda()
        dev = entry.min_distances(torch.as_tensor(np.asarray(frames, real)).cuda(), idx1=t(idx1, np.int64), idx2=t(idx2, np.int64), labels1=t(lab1, np.int32),
                                  labels2=t(lab2, np.int32), ngroups1=case.G1, ngroups2=case.G2, boxes=t(boxes, real), pbc=case.pbc, cutoff=mr.CUTOFF,
                                  want=ALL)
        eng.synchronize()
        for n in ALL:
            x, y = getattr(dev, n).cpu().numpy(), np.asarray(getattr(host, n))
            assert np.array_equal(x.view(y.dtype) if x.dtype != y.dtype else x, y, equal_nan=y.dtype.kind == "f"), n


def test_a_frame_that_is_not_finite_is_nan_and_changes_no_other(m64):
    case = next(c for c in mr.CASES if c.name == "bad")
    clean = case._replace(bad=())
    got, ref = call(m64, case, np.float64), call(m64, clean, np.float64)
    good = np.array([f not in case.bad for f in range(case.F)])
    assert np.array_equal(got.frame_ok, good.astype(np.uint32)) and int(got.nvalid[0]) == good.sum()
    for n in ("dist", "pair", "atom1", "near1", "atom2", "mat"):
        assert np.array_equal(np.asarray(getattr(got, n))[good], np.asarray(getattr(ref, n))[good]), n
    for n in ("dist", "atom1", "atom2", "mat"):
        assert np.all(np.isnan(np.asarray(getattr(got, n))[~good])), n
    assert np.all(np.asarray(got.pair)[~good] == mr.NONE) and np.all(np.asarray(got.near1)[~good] == mr.NONE)
    # a refused box does the same
    frames, boxes, idx1, idx2, lab1, lab2 = mr.case_inputs(clean)
    boxes = boxes.copy()
    boxes[2, 3:6] = 0.0
    got2 = call(m64, clean, np.float64, inputs=(frames, boxes, idx1, idx2, lab1, lab2))
    assert list(got2.frame_ok) == [1, 1, 0, 1] and np.all(np.isnan(got2.dist[2])) and np.array_equal(got2.dist[[0, 1, 3]], ref.dist[[0, 1, 3]])


def test_same_call_same_bits_whatever_the_frame_block(eng, m64, monkeypatch):
    case = next(c for c in ALL_CASES if c.name == "F5")
    for entry, real in ((eng, np.float32), (m64, np.float64)):
        first = call(entry, case, real)
        same_bits(call(entry, case, real), first)
        for fb in (1, 3, 5, 64):
            same_bits(call(entry, case, real, frame_block=fb), first)
        monkeypatch.setenv("MOLAR_HIP_MINDIST_COL_SPLITS", "1")
        same_bits(call(entry, case, real), first)
        monkeypatch.setenv("MOLAR_HIP_MINDIST_COL_SPLITS", str(COL_SPLITS))


@pytest.mark.parametrize("name", ["none", "ortho_idx", "frames", "tric", "tricframes", "mask3_ortho", "mask5_tric", "same"])
def test_dist_is_bit_equal_to_internal_coords_on_the_reported_pair(eng, m64, name):
    case = next(c for c in mr.CASES if c.name == name)
    frames, boxes, idx1, idx2, lab1, lab2 = mr.case_inputs(case)
    i1 = np.arange(case.n1, dtype=np.uint64) if idx1 is None else idx1
    i2 = i1 if case.same else idx2
    for entry, real in ((eng, np.float32), (m64, np.float64)):
        got = call(entry, case, real, want=("dist", "pair", "atom1", "near1"))
        tuples = np.stack([i1[got.pair[:, 0].astype(np.int64)], i2[got.pair[:, 1].astype(np.int64)]], axis=1).astype(np.uint64)
        ic = entry.internal_coords(np.asarray(frames, real), tuples, boxes=None if boxes is None else np.asarray(boxes, real), pbc=case.pbc, want=("values",))
        assert np.array_equal(np.diagonal(np.asarray(ic.values)), got.dist), (name, real)
        # and every atom's distance on its nearest atom, frame 0
        t1 = np.stack([i1, i2[got.near1[0].astype(np.int64)]], axis=1).astype(np.uint64)
        ic1 = entry.internal_coords(np.asarray(frames[:1], real), t1, boxes=None if boxes is None else np.asarray(boxes if boxes.ndim == 1 else boxes[:1], real),
                                    pbc=case.pbc, want=("values",))
        assert np.array_equal(np.asarray(ic1.values)[0], got.atom1[0]), (name, real)


def test_known_answer_two_lattices_across_the_cell_boundary(m64):
    # a 4 x 4 x 4 lattice of spacing 1 in a cube of edge 4, and its copy displaced by (3.75, 0.25, 0) - which is (-0.25, 0.25, 0)
    # through the boundary: every atom's nearest copy is sqrt(0.125) away, a power of two under the root: exact
    g = np.arange(4.0)
    a = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + 0.125
    b = a + np.array([3.75, 0.25, 0.0])
    frames = np.concatenate([a, b])[None]
    box = np.diag([4.0, 4.0, 4.0]).reshape(9)
    got = m64.min_distances(frames, idx1=np.arange(64), idx2=np.arange(64, 128), boxes=box, want=("dist", "atom1", "atom2", "near1"))
    want = np.sqrt(0.125)
    assert np.all(got.atom1 == want) and np.all(got.atom2 == want) and got.dist[0] == want
    assert np.array_equal(np.asarray(got.near1[0]), np.arange(64, dtype=np.uint64)), "the nearest atom of lattice site i is its own copy"
    plain = m64.min_distances(frames, idx1=np.arange(64), idx2=np.arange(64, 128), boxes=None, want=("dist",))
    assert plain.dist[0] > 0.7, "without the box the copy is far"


def test_exact_ties_give_the_lowest_pair(eng, m64):
    # coordinates that are duplicates bit for bit: atoms 3, 7 and 12 of set 2 sit on one point, atoms 5 and 9 of set 1 on another;
    # every other atom is far.  Labels out of order, so the sorted order of the kernels is not the order of the sets.
    rng = np.random.default_rng(5)
    n1, n2 = 140, 150
    x1 = mr.f32_exact(rng.uniform(0.0, 1.0, (n1, 3)))
    x2 = mr.f32_exact(rng.uniform(2.0, 3.0, (n2, 3)))
    x1[[5, 9]] = mr.f32_exact([1.25, 1.5, 1.75])
    x2[[3, 7, 12]] = mr.f32_exact([1.5, 1.5, 1.75])
    frames = np.concatenate([x1, x2])[None]
    lab1 = (np.arange(n1)[::-1] % 5).astype(np.uint32)
    lab2 = (np.arange(n2)[::-1] % 7).astype(np.uint32)
    for entry, real in ((eng, np.float32), (m64, np.float64)):
        for labels in (False, True):
            got = entry.min_distances(np.asarray(frames, real), idx1=np.arange(n1), idx2=np.arange(n1, n1 + n2), labels1=lab1 if labels else None,
                                      labels2=lab2 if labels else None, ngroups1=5, ngroups2=7, boxes=None, want=("dist", "pair", "near1", "atom1"))
            assert got.dist[0] == 0.25 and list(got.pair[0]) == [5, 3], (real, labels, got.pair)
            assert got.near1[0][5] == 3 and got.near1[0][9] == 3 and got.atom1[0][9] == 0.25
            swapped = entry.min_distances(np.asarray(frames, real), idx1=np.arange(n1), idx2=np.arange(n1, n1 + n2), labels1=lab1 if labels else None,
                                          labels2=lab2 if labels else None, ngroups1=5, ngroups2=7, boxes=None, want=("dist", "pair", "atom2"))
            assert list(swapped.pair[0]) == [5, 3] and swapped.atom2[0][12] == 0.25
    # inside one set: (i, j) and (j, i) tie by symmetry
    got = m64.min_distances(np.asarray(frames[:, :n1]), same=True, boxes=None, want=("pair", "near1"))
    assert list(got.pair[0]) == [5, 9] and got.near1[0][9] == 5


def test_an_index_or_label_out_of_range_in_device_memory_touches_no_output(m64):
    import torch
    from molar_amd import api
    case = next(c for c in mr.CASES if c.name == "groups")
    frames, boxes, idx1, idx2, lab1, lab2 = mr.case_inputs(case)
    fr = torch.as_tensor(frames).cuda()
    i2 = torch.as_tensor(idx2.astype(np.int64)).cuda()
    l1 = torch.as_tensor(lab1.astype(np.int32)).cuda()
    l2 = torch.as_tensor(lab2.astype(np.int32)).cuda()
    bad_i2, bad_l1 = i2.clone(), l1.clone()
    bad_i2[11] = case.natoms
    bad_l1[3] = case.G1
    shapes = {"dist": (case.F,), "atom1": (case.F, case.n1), "mat": (case.F, case.G1, case.G2), "mat_mean": (case.G1, case.G2)}
    for kw in (dict(idx2=bad_i2, labels1=l1), dict(idx2=i2, labels1=bad_l1)):
        out = [torch.full(shapes[n], -7.0, dtype=torch.float64, device="cuda") if n in shapes else None for n in ALL]
        with pytest.raises(api.MolarHipError) as e:
            m64.min_distances(fr, labels2=l2, ngroups1=case.G1, ngroups2=case.G2, boxes=torch.as_tensor(boxes).cuda(), want=tuple(shapes), out=out,
                              n1=case.n1, **kw)
        assert e.value.code == mr.ERR_INVALID
        m64.eng.synchronize()
        assert all(bool((o == -7.0).all()) for o in out if o is not None)


def test_bound_report():
    """Prints the largest used fraction of each bound over this file's cases (run with -s; the numbers are in profiles/mindist.txt)."""
    assert FRACTIONS, "runs after the comparisons"
    for name, frac in sorted(FRACTIONS.items()):
        print(f"mindist bound use: {name} {frac:.3f}")
        assert frac <= 1.0
