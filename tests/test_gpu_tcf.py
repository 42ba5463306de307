"""Time correlation functions of vectors on the GPU (molar_hip_tcf / _f64: the vector stage, the fold, the register-blocked lag
stage, the finish) against the numpy reference of tests/tcf_ref.py, output by output within the bounds derived there.  Both
entries see the same numbers (f32 frames and boxes, cast to f64 for the f64 entry), so one reference serves both; every
reference is computed once per module.  The shapes stand either side of every size molar_hip_tcf_plan reports.  The largest
used fraction of each bound is printed by the last test."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tcf_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu
mr = tr.mr
ALL = ("c1", "c2", "c1_vec", "c2_vec", "nvalid", "mean", "s2", "bad_frames")
P2 = ("c2", "c2_vec", "s2")


@pytest.fixture(scope="module")
def eng():
    from molar_amd import api
    return api.Engine()


@pytest.fixture(scope="module")
def m64(eng):
    from molar_amd import api
    return api.MeasureF64(eng)


def plan(F=258, V=2, **kw):
    """(frame_chunk, vec_chunk, lag_block, lags_per_lane, segment, window) of the plan entry."""
    from molar_amd import api
    return api.tcf_plan(F, V, **kw)[1:]


FC, _, LB, R, SEG, WIN = plan()


def f32box(b):
    return np.asarray(b, np.float64).astype(np.float32).astype(np.float64)


ORTHO, TRIC = f32box(tr.ORTHO), f32box(tr.TRICLINIC)
_CASES, _REFS = {}, {}


def case(F, V, kind, seed, box=None):
    """frames and tuples of tr.make_case, made once; box: None, "ortho", "tric" or "scaled" (per-frame boxes)."""
    key = (F, V, kind, seed, box)
    if key not in _CASES:
        boxes = f32box(mr.scaled_boxes(F, 3)) if box == "scaled" else None
        box9 = TRIC if box == "tric" else ORTHO if box else None
        fr, tp = tr.make_case(F, V, kind, seed, box9=box9, boxes=boxes)
        _CASES[key] = (fr, tp, boxes if box == "scaled" else box9)
    fr, tp, bx = _CASES[key]
    return fr.copy(), tp.copy(), bx


def freeze(kw):
    return tuple(sorted((k, v.tobytes() + str(v.shape).encode() if isinstance(v, np.ndarray) else v) for k, v in kw.items()))


def reference(frames, tuples, **kw):
    key = (frames.tobytes(), frames.shape, tuples.tobytes(), freeze(kw))
    if key not in _REFS:
        _REFS[key] = tr.tcf(frames, tuples, **kw)
    return _REFS[key]


def names_of(mode):
    return tuple(n for n in ALL if mode == tr.UNIT or n not in P2)


def call(entry, frames, tuples, real, want=None, **kw):
    kw = dict(kw)
    kw.pop("bad", None)
    mode = kw.pop("mode", tr.UNIT)
    if kw.get("boxes") is not None:
        kw["boxes"] = np.asarray(kw["boxes"], real)
    return entry.vector_correlations(np.asarray(frames, real), tuples, mode=mode, want=names_of(mode) if want is None else want, **kw)


def both(eng, m64, frames, tuples, what, **kw):
    """The f32 and the f64 entry on the same numbers against one reference; returns the two results and the reference."""
    assert frames.dtype == np.float32
    if kw.get("boxes") is None:
        kw.pop("boxes", None)
        kw["pbc"] = 0
    ref = reference(frames, tuples, **kw)
    out = []
    for entry, real, eps in ((eng, np.float32, tr.EPS32), (m64, np.float64, tr.EPS64)):
        got = call(entry, frames, tuples, real, **kw)
        tr.check(got, ref, eps, what=f"{what} {np.dtype(real).name}")
        assert np.array_equal(got.lags, ref["n"])
        out.append(got)
    return out, ref


def same_bits(a, b, names=ALL):
    for n in names:
        x, y = getattr(a, n), getattr(b, n)
        if x is None and y is None:
            continue
        assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=np.asarray(x).dtype.kind == "f"), n


def test_plan_shape():
    assert FC == 64 and LB == 64 * R and WIN == SEG + LB and SEG % (2 * R) == 0


# Frames either side of the chunk of the vector stage, of the segment of origins and of the window they reach, two and three
# segments, and (with the segment a multiple of 2 R) every count of origins the last two-step turn of the blocked loop is left.
FRAMES = sorted({1, 2, 3, FC - 1, FC, FC + 1, SEG - 1, SEG, SEG + 1, SEG + 2, SEG + 3, SEG + 4, SEG + 5, SEG + 2 * R - 1, WIN - 1, WIN, WIN + 1, 2 * SEG - 1,
                 2 * SEG, 2 * SEG + 1, 3 * SEG + 1})


@pytest.mark.parametrize("F", FRAMES)
def test_frames(eng, m64, F):
    fr, tp, bx = case(F, 3, 2, 1000 + F, "ortho")
    both(eng, m64, fr, tp, f"F={F}", boxes=bx)


@pytest.mark.parametrize("L", [0, 1])
def test_max_lag(eng, m64, L):
    fr, tp, bx = case(66, 3, 2, 7)
    (g32, g64), ref = both(eng, m64, fr, tp, f"max_lag={L}", max_lag=L)
    assert g32.c1.shape == (1, L + 1) and g64.c2_vec.shape == (3, L + 1)


# lags either side of a whole block, a number of lags that no lane width divides, the last block narrower than the others
# (one, two and four lags per lane), and two whole blocks
@pytest.mark.parametrize("lags", sorted({LB - 1, LB, LB + 1, LB + 63, LB + 64, LB + 65, LB + 128, LB + 129, LB + 131, 2 * LB, 2 * LB + 1, 3, 63, 65, 127, 130}))
def test_lag_block_edges(eng, m64, lags):
    F = max(lags, 2 * LB + 2)
    fr, tp, bx = case(F, 2, 2, 8)
    both(eng, m64, fr, tp, f"lags={lags}", max_lag=lags - 1)


@pytest.mark.parametrize("stride", [1, 2, 3, 7, SEG + 2, 10 ** 6])
def test_origin_stride(eng, m64, stride):
    """strides that do not divide the segment, one that leaves whole segments without an origin, one beyond the block"""
    fr, tp, bx = case(3 * SEG + 1, 3, 3, 11)
    both(eng, m64, fr, tp, f"origin_stride={stride}", origin_stride=stride)
    both(eng, m64, fr, tp, f"origin_stride={stride} max_lag=70", origin_stride=stride, max_lag=70)


@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 255, 256, 257])
def test_vectors(eng, m64, V):
    fr, tp, bx = case(10, V, 2, 20 + V, "ortho")
    both(eng, m64, fr, tp, f"V={V}", boxes=bx)


@pytest.mark.parametrize("V,last", [(32768, 0), (32769, 1), (32771, 3)])
def test_vec_chunk_edges(eng, m64, V, last):
    """Four vectors per workgroup of the lag kernel (the plan says so); the last workgroup holds vec_chunk, 1 and vec_chunk - 1;
    label runs of 6 cross the chunks, unsorted."""
    chunk = plan(3, V)[1]
    assert chunk == 4 and V % chunk == last
    fr, tp, bx = case(3, V, 1, 30)
    labels = ((np.arange(V) // 6) * 7 % 5).astype(np.uint32)
    both(eng, m64, fr, tp, f"V={V}", labels=labels, ngroups=5)


def test_labels(eng, m64):
    fr, tp, bx = case(40, 65, 2, 41, "ortho")
    V = 65
    both(eng, m64, fr, tp, "G=V", boxes=bx, labels=np.arange(V, dtype=np.uint32)[::-1].copy(), ngroups=V)
    rng = np.random.default_rng(3)
    both(eng, m64, fr, tp, "unsorted labels", boxes=bx, labels=rng.integers(0, 4, size=V).astype(np.uint32), ngroups=4)
    # group 2 has no vector at all, group 1 only a bad one: NaN rows, nvalid 0
    labels = np.zeros(V, np.uint32)
    labels[5] = 1
    labels[7:] = 3
    tr.make_bad(fr, tp, 5, 20)
    (g32, g64), ref = both(eng, m64, fr, tp, "empty groups", boxes=bx, labels=labels, ngroups=4, bad=(5,))
    assert list(g32.nvalid) == [6, 0, 0, 58] and np.all(np.isnan(g64.c1[1:3])) and not np.any(np.isnan(g64.c1[[0, 3]]))


@pytest.mark.parametrize("kind", [1, 2, 3])
@pytest.mark.parametrize("mode", [tr.UNIT, tr.RAW])
@pytest.mark.parametrize("dims", [7, 3, 4])
def test_kinds_modes_masks(eng, m64, kind, mode, dims):
    fr, tp, bx = case(70, 5, kind, 50 + kind)
    both(eng, m64, fr, tp, f"kind={kind} mode={mode} dims={dims}", mode=mode, dims=dims, max_lag=40)


@pytest.mark.parametrize("kind", [2, 3])
@pytest.mark.parametrize("box,pbc", [(None, 0), ("ortho", 7), ("tric", 7), ("ortho", 3), ("scaled", 7), ("scaled", 5)])
def test_boxes(eng, m64, kind, box, pbc):
    fr, tp, bx = case(30, 9, kind, 60 + kind, box)
    (g32, g64), ref = both(eng, m64, fr, tp, f"kind={kind} box={box} pbc={pbc}", boxes=bx, pbc=pbc)
    if box == "ortho" and pbc == 7:
        # the boundary does cut bonds: without the image the answer is another one
        raw = call(eng, fr, tp, np.float32, boxes=None, pbc=0)
        assert np.abs(raw.c1_vec - g32.c1_vec).max() > 0.1


def test_kind_1_reads_no_box(eng, m64):
    fr, tp, bx = case(20, 4, 1, 70)
    a = call(eng, fr, tp, np.float32)
    b = call(eng, fr, tp, np.float32, boxes=np.full(9, np.nan), pbc=7)
    same_bits(a, b)


BAD = [("frame 0", 0, "zero"), ("a middle frame", 35, "zero"), ("the last frame", 69, "zero"), ("a NaN coordinate", 64, "nan")]


@pytest.mark.parametrize("kind", [1, 2, 3])
@pytest.mark.parametrize("what,f,how", BAD)
def test_bad_vectors(eng, m64, kind, what, f, how):
    """The bad vector is NaN in its own rows and counted; every other vector's rows are, bit for bit, those of the call in which
    a good tuple takes its place; the group rows follow the reference."""
    fr, tp, bx = case(70, 6, kind, 80 + kind, "ortho" if kind > 1 else None)
    labels = np.array([0, 1, 0, 1, 0, 1], np.uint32)
    good = [call(e, fr, tp, real, boxes=bx, labels=labels, ngroups=2) for e, real in ((eng, np.float32), (m64, np.float64))]
    tr.make_bad(fr, tp, 2, f, how)
    (b32, b64), ref = both(eng, m64, fr, tp, f"kind={kind} bad in {what}", boxes=bx, labels=labels, ngroups=2, bad=(2,))
    others = [0, 1, 3, 4, 5]
    for g, b in zip(good, (b32, b64)):
        assert b.bad_frames[2] == 1 and np.all(np.isnan(b.c1_vec[2])) and np.all(np.isnan(b.c2_vec[2])) and np.isnan(b.s2[2]) and np.all(np.isnan(b.mean[2]))
        for n in ("c1_vec", "c2_vec", "mean", "s2", "bad_frames"):
            assert np.array_equal(getattr(g, n)[others], getattr(b, n)[others]), n
        assert np.array_equal(g.c1[1], b.c1[1]) and np.array_equal(g.c2[1], b.c2[1])       # the group the bad vector is not in
        assert list(b.nvalid) == [2, 3]


def test_collinear_triple_and_equal_atoms(eng, m64):
    # kind 3 without a box: C - A = 2 (B - A) on the grid, a cross product of exactly zero
    fr, tp, bx = case(20, 4, 3, 90)
    a, b, c = (int(k) for k in tp[1])
    fr[7, c] = fr[7, a] + 2 * (fr[7, b] - fr[7, a])
    (g32, g64), ref = both(eng, m64, fr, tp, "collinear triple", bad=(1,))
    assert g32.bad_frames[1] == 1
    # kind 2 with A == B: bad in every frame in UNIT mode, valid zeros in RAW mode
    fr, tp, bx = case(20, 4, 2, 91, "ortho")
    tp[3, 1] = tp[3, 0]
    (g32, g64), ref = both(eng, m64, fr, tp, "A == B, UNIT", boxes=bx, bad=(3,))
    assert g64.bad_frames[3] == 20 and g64.nvalid[0] == 3
    (g32, g64), ref = both(eng, m64, fr, tp, "A == B, RAW", boxes=bx, mode=tr.RAW)
    assert g64.bad_frames[3] == 0 and np.all(g64.c1_vec[3] == 0) and g64.nvalid[0] == 4


def test_host_and_device_memory(eng, m64):
    torch = pytest.importorskip("torch")
    fr, tp, bx = case(2 * SEG + 5, 7, 3, 95, "scaled")
    labels = np.array([1, 0, 1, 1, 0, 2, 1], np.uint32)
    for entry, real in ((eng, np.float32), (m64, np.float64)):
        host = call(entry, fr, tp, real, boxes=bx, labels=labels, ngroups=3, origin_stride=1)
        dev = entry.vector_correlations(torch.as_tensor(fr.astype(real)).cuda(), torch.as_tensor(tp.astype(np.int64)).cuda(),
                                        labels=torch.as_tensor(labels.astype(np.int32)).cuda(), ngroups=3, boxes=torch.as_tensor(bx.astype(real)).cuda(), want=ALL)
        eng.synchronize()
        for n in ALL:
            assert np.array_equal(np.asarray(getattr(host, n)).astype(np.float64), getattr(dev, n).cpu().numpy().astype(np.float64), equal_nan=True), n


def test_layout(eng, m64):
    """a frame stride above 3 natoms, and ld > L + 1 with a sentinel behind each row left untouched"""
    fr, tp, bx = case(SEG + 3, 5, 2, 96, "ortho")
    F, natoms = fr.shape[:2]
    L = 20
    for entry, real in ((eng, np.float32), (m64, np.float64)):
        dense = call(entry, fr, tp, real, boxes=bx, max_lag=L)
        wide = np.full((F, natoms + 3, 3), np.nan, real)
        wide[:, :natoms] = fr
        rows = [np.full((5, L + 4), -7.0, real) for _ in range(2)]
        out = (None, None, rows[0][:, :L + 1], rows[1][:, :L + 1], None, None, None, None)
        got = entry.vector_correlations(wide[:, :natoms], tp, boxes=bx.astype(real), max_lag=L, want=ALL, out=out)
        same_bits(dense, got)
        assert all(np.all(r[:, L + 1:] == -7.0) for r in rows) and np.array_equal(rows[0][:, :L + 1], dense.c1_vec)


def test_single_outputs_and_repeatability(eng, m64):
    fr, tp, bx = case(WIN + 1, 6, 2, 97, "ortho")
    labels = np.array([0, 1, 1, 0, 2, 1], np.uint32)
    tr.make_bad(fr, tp, 4, 3)
    for entry, real in ((eng, np.float32), (m64, np.float64)):
        every = call(entry, fr, tp, real, boxes=bx, labels=labels, ngroups=3)
        same_bits(every, call(entry, fr, tp, real, boxes=bx, labels=labels, ngroups=3))
        for n in ALL:
            one = call(entry, fr, tp, real, boxes=bx, labels=labels, ngroups=3, want=(n,))
            assert all(getattr(one, m) is None for m in ALL if m != n)
            same_bits(every, one, (n,))
        # P1 alone: the kernel without the d^2 sums gives the same c1
        same_bits(every, call(entry, fr, tp, real, boxes=bx, labels=labels, ngroups=3, want=("c1", "c1_vec")), ("c1", "c1_vec"))


def test_errors_touch_no_output(eng, m64):
    torch = pytest.importorskip("torch")
    from molar_amd import _lib
    lib = _lib.load()
    fr = np.ones((4, 5, 3))
    for entry, fn, real in ((eng, lib.molar_hip_tcf, np.float32), (m64, lib.molar_hip_tcf_f64, np.float64)):
        ctx = entry.ctx
        for what, want, got in tr.argument_errors(fn, ctx, real):
            assert got == want, (what, want, got, lib.molar_hip_last_error())
        outs = dict(c1=np.full((2, 2), -7.0, real), c2=np.full((2, 2), -7.0, real), c1_vec=np.full((1, 2), -7.0, real), c2_vec=np.full((1, 2), -7.0, real),
                    nvalid=np.full(2, 77, np.uint64), mean=np.full((1, 3), -7.0, real), s2=np.full(1, -7.0, real), bad_frames=np.full(1, 77, np.uint32))
        rows = [("an index not below natoms", tr.ERR_INVALID, dict(tuples=[[0, 5]])),
                ("a label not below ngroups", tr.ERR_INVALID, dict(labels=[2], G=2)),
                ("a box vector of zero length", tr.ERR_ZERO_LENGTH, dict(boxes=[1, 0, 0, 0, 0, 0, 0, 0, 1], pbc=7)),
                ("a box without an inverse", tr.ERR_INVERSE, dict(boxes=[1, 0, 0, 1, 0, 0, 0, 0, 1], pbc=7))]
        for what, want, kw in rows:
            assert tr.raw_tcf(fn, ctx, fr, real, **{**dict(L=1, ld=2, G=2, labels=[0]), **kw, **outs}) == want, (what, lib.molar_hip_last_error())
            assert all(np.all(o == (77 if o.dtype.kind == "u" else -7.0)) for o in outs.values()), what
        # a bad index and a bad label in DEVICE memory: judged there, nothing written
        for bad_tuples, bad_labels in (([[0, 5]], [0]), ([[0, 1]], [3])):
            t = torch.as_tensor(np.asarray(bad_tuples, np.int64)).cuda()
            lab = torch.as_tensor(np.asarray(bad_labels, np.int32)).cuda()
            c1 = torch.full((2, 2), -7.0, dtype=torch.float32 if real == np.float32 else torch.float64, device="cuda")
            nv = torch.full((2,), 77, dtype=torch.int64, device="cuda")
            sp = _lib.TcfSpec(2, 0, 7, 0)
            frr = np.ascontiguousarray(fr, real)
            torch.cuda.synchronize()
            st = fn(ctx, frr.ctypes.data, 4, 15, 5, t.data_ptr(), 1, lab.data_ptr(), 2, None, 0, 0, C.addressof(sp), 1, 1, c1.data_ptr(), None, None, None, 0,
                    nv.data_ptr(), None, None, None)
            assert st == tr.ERR_INVALID, lib.molar_hip_last_error()
            eng.synchronize()
            assert bool((c1 == -7.0).all()) and bool((nv == 77).all())


def test_workspace_that_cannot_be_allocated(eng, m64):
    """One atom taken as 200 000 vectors over 100 000 frames: 1.2 MB of frames, 480 GB of f64 vectors.  The workspace is the first
    thing the call asks the device for, before any launch; its byte count is in the message."""
    from molar_amd import api
    F, V, L = 100000, 200000, 10
    want = api.tcf_plan(F, V, 1, L)[0]
    assert want > 24 * F * V
    for fn, real in ((eng.lib.molar_hip_tcf, np.float32), (eng.lib.molar_hip_tcf_f64, np.float64)):
        out = np.full((1, L + 1), -7.0, real)
        assert tr.raw_tcf(fn, eng.ctx, np.ones((F, 1, 3), real), real, tuples=np.zeros((V, 1), np.uint64), L=L, c1=out) == tr.ERR_TOO_LARGE
        assert str(want) in eng.lib.molar_hip_last_error().decode(), eng.lib.molar_hip_last_error()
        assert np.all(out == -7.0)
    fr, tp, bx = case(6, 5, 1, 99)
    assert not np.any(np.isnan(eng.vector_correlations(fr, tp).c1))              # the engine still works afterwards


def test_report(eng):
    """Not a test of its own: the largest used fraction of every bound over this module, for profiles/tcf.txt."""
    assert tr.REPORT, "the tests above ran"
    for key in sorted(tr.REPORT):
        print(f"tcf bound used, largest: {key} {tr.REPORT[key]:.3g}")
        assert tr.REPORT[key] < 1.0
