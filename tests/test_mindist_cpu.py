"""Minimum distances, everything that needs no GPU: the ABI of the three entries on every side, the arithmetic of
molar_hip_mindist_plan, the argument errors the library reports before it touches the context, the host helpers of api.py, and
the reference of tests/mindist_ref.py checked against itself - another route on orthorhombic boxes, known answers, and its own
assertions on every case the GPU tests use."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mindist_ref as mr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("molar_hip_mindist_plan", "molar_hip_mindist", "molar_hip_mindist_f64")


def test_abi_of_the_three_entries():
    from molar_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "molar_hip.h")).read())
    ffi = open(os.path.join(ROOT, "rust", "molar_hip", "src", "ffi.rs")).read()
    for name in NAMES:
        assert f"int {name}(" in header, name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert f'b"{name}\\0"' in ffi, name
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_ffi as gen
    funcs = {name: params for name, _, params in gen.c_functions(open(gen.HEADER).read())}
    assert len(funcs["molar_hip_mindist_plan"]) == len(_lib.SYMBOLS["molar_hip_mindist_plan"][1]) == 13
    assert len(funcs["molar_hip_mindist"]) == len(_lib.SYMBOLS["molar_hip_mindist"][1]) == 29
    assert len(funcs["molar_hip_mindist_f64"]) == len(_lib.SYMBOLS["molar_hip_mindist_f64"][1]) == 29
    # mat_mean is double in both entries
    f32, f64 = [t for t, _ in funcs["molar_hip_mindist"]], [t for t, _ in funcs["molar_hip_mindist_f64"]]
    assert [t for k, t in enumerate(f32) if k != 24] == [t.replace("double", "float") for k, t in enumerate(f64) if k != 24]
    assert "double" in f32[24] and f32[24] == f64[24]
    assert open(gen.OUT).read() == gen.render(gen.c_functions(open(gen.HEADER).read())), "run python tools/gen_rust_ffi.py"
    # the spec: the same fields on every side, 24 bytes
    fields = ["pbc", "same", "exclude_same_group", "frame_block", "cutoff"]
    assert C.sizeof(_lib.MindistSpec) == 24 and [f[0] for f in _lib.MindistSpec._fields_] == fields
    assert re.search(r"typedef struct \{ uint32_t pbc; uint32_t same; uint32_t exclude_same_group; uint32_t frame_block; double cutoff; \} molar_hip_mindist_spec;",
                     header)
    types_rs = open(os.path.join(ROOT, "rust", "molar_hip", "src", "types.rs")).read()
    assert re.search(r"pub struct MolarHipMindistSpec \{\s*pub pbc: u32,\s*pub same: u32,\s*pub exclude_same_group: u32,\s*pub frame_block: u32,\s*pub cutoff: f64,\s*\}",
                     types_rs)
    hpp = open(os.path.join(ROOT, "include", "molar_hip.hpp")).read()
    assert "min_distances(" in hpp and "min_distances_f64(" in hpp and "(molar_hip_mindist," in hpp and "(molar_hip_mindist_f64," in hpp
    lib_rs = open(os.path.join(ROOT, "rust", "molar_hip", "src", "lib.rs")).read()
    assert "pub fn min_distances(" in lib_rs and "pub fn min_distances_plan(" in lib_rs
    assert "mindist.hip" in build.SOURCES


def test_plan_needs_no_gpu_is_monotone_and_honours_the_overrides(monkeypatch):
    from molar_amd import api
    monkeypatch.delenv("MOLAR_HIP_MINDIST_COL_SPLITS", raising=False)
    monkeypatch.delenv("MOLAR_HIP_MINDIST_FRAME_BLOCK", raising=False)
    everything = ("dist", "atom1", "atom2", "mat")
    ws, rw, rb, ct, cs, fb = api.mindist_plan(1, 5000, 5000, want=everything)
    assert (rw, rb, ct) == (mr.ROWS_WAVE, mr.ROWS_BLOCK, mr.COL_TILE) and rb == 4 * rw and fb == 1
    # 79 column tiles, 10 workgroups of rows: 64 splits at the most, whole tiles each: 2 tiles per split, 40 splits
    assert cs == 40
    # enough frames fill the device without a split; one tile of columns is never split
    assert api.mindist_plan(1024, 5000, 5000)[4] == 1 and api.mindist_plan(1, 100, ct)[4] == 1 and api.mindist_plan(1, 100, ct + 1)[4] == 2
    assert api.mindist_plan(1024, 5000, 5000)[5] == 256, "256 frames at once at the most"
    # nothing asked for but the flags: no pass, a small workspace; every output adds to it
    sizes = [api.mindist_plan(8, 700, 900, 5, 6, want=w)[0] for w in (("frame_ok",), ("dist",), ("dist", "atom1"), ("dist", "atom1", "atom2"), everything)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[1] < sizes[-1]
    # never smaller for a larger argument
    base = api.mindist_plan(8, 700, 900, 5, 6, want=everything)[0]
    for args in ((9, 700, 900, 5, 6), (8, 701, 900, 5, 6), (8, 700, 901, 5, 6), (8, 700, 900, 6, 6), (8, 700, 900, 5, 7), (2000, 700, 900, 5, 6)):
        assert api.mindist_plan(*args, want=everything)[0] >= base, args
    # a workspace of a block above a gibibyte per frame still holds one frame
    big = api.mindist_plan(4, 200000, 200000, want=("atom1",))
    assert big[5] >= 1 and big[0] > 0
    # the same set: n2 and ngroups2 are not read
    assert api.mindist_plan(3, 400, None, 7, 1, want=("mat",), same=True) == api.mindist_plan(3, 400, 12345, 7, 99, want=("mat",), same=True)
    assert api.mindist_plan(0, 400, 400)[0] == 0 and api.mindist_plan(3, 0, 400)[0] == 0
    # frame_block of the spec, then the variable, both capped by the frames
    assert api.mindist_plan(100, 50, 50, frame_block=7)[5] == 7 and api.mindist_plan(5, 50, 50, frame_block=7)[5] == 5
    monkeypatch.setenv("MOLAR_HIP_MINDIST_FRAME_BLOCK", "3")
    monkeypatch.setenv("MOLAR_HIP_MINDIST_COL_SPLITS", "2")
    assert api.mindist_plan(100, 50, 5000)[4:] == (2, 3) and api.mindist_plan(100, 50, 5000, frame_block=9)[5] == 9
    assert api.mindist_plan(100, 50, 10)[4] == 1
    with pytest.raises(api.MolarHipError) as e:
        api.mindist_plan(1, 1 << 31, 5)
    assert e.value.code == mr.ERR_TOO_LARGE
    with pytest.raises(api.MolarHipError) as e:
        api.mindist_plan(1, 100, 100, 1 << 16, 1 << 16, want=("mat",))
    assert e.value.code == mr.ERR_TOO_LARGE


def raw_call(fn, ctx, real, F=2, natoms=10, stride=None, idx1=None, n1=4, lab1=None, G1=1, idx2=None, n2=5, lab2=None, G2=1, boxes=None, box_stride=0, spec=None,
             null_spec=False, want=("dist",), ld1=None, ld2=None, pbc=7, same=0, excl=0, cutoff=0.5, null_frames=False):
    """One call through ctypes with host arrays; the status."""
    from molar_amd import _lib
    frames = np.zeros((F, natoms, 3), real)
    keep = []

    def ptr(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dt)
        keep.append(a)
        return a.ctypes.data
    sp = _lib.MindistSpec(pbc, same, excl, 0, cutoff) if spec is None else spec
    n2e = n1 if same else n2
    G2e = G1 if same else G2
    shapes = {"dist": ((F,), real), "pair": ((F, 2), np.uint64), "atom1": ((F, n1), real), "near1": ((F, n1), np.uint64), "atom2": ((F, n2e), real),
              "mat": ((F, G1, G2e), real), "mat_mean": ((G1, G2e), np.float64), "mat_min": ((G1, G2e), real), "mat_freq": ((G1, G2e), np.uint32),
              "frame_ok": ((F,), np.uint32), "nvalid": ((1,), np.uint64)}
    outs = {k: (np.zeros(*shapes[k]) if k in want else None) for k in shapes}
    o = {k: (None if v is None else v.ctypes.data) for k, v in outs.items()}
    return fn(ctx, None if null_frames else frames.ctypes.data, F, 3 * natoms if stride is None else stride, natoms, ptr(idx1, np.uint64), n1, ptr(lab1, np.uint32), G1,
              ptr(idx2, np.uint64), n2, ptr(lab2, np.uint32), G2, ptr(boxes, real), box_stride, None if null_spec else C.addressof(sp), o["dist"], o["pair"],
              o["atom1"], o["near1"], n1 if ld1 is None else ld1, o["atom2"], n2e if ld2 is None else ld2, o["mat"], o["mat_mean"], o["mat_min"], o["mat_freq"],
              o["frame_ok"], o["nvalid"])


def test_argument_errors_need_no_device():
    from molar_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    ctx = C.create_string_buffer(1 << 16)                    # never read: the arguments are judged before the context is used
    S, I, L = mr.ERR_SIZES, mr.ERR_INVALID, mr.ERR_TOO_LARGE
    errors = [
        ("a null spec", I, dict(null_spec=True)),
        ("pbc above 7", I, dict(pbc=8)),
        ("same = 2", I, dict(same=2)),
        ("exclude_same_group without same", I, dict(excl=1)),
        ("a cutoff that is NaN", I, dict(cutoff=float("nan"))),
        ("same with a second index", I, dict(same=1, idx2=[0, 1, 2, 3])),
        ("same with second labels", I, dict(same=1, lab2=[0, 0, 0, 0])),
        ("same with atom2", I, dict(same=1, want=("atom2",))),
        ("n1 = 0", S, dict(n1=0)),
        ("n2 = 0", S, dict(n2=0)),
        ("labels with ngroups = 0", S, dict(lab1=[0, 0, 0, 0], G1=0)),
        ("box_stride = 3", I, dict(boxes=np.eye(3).reshape(9), box_stride=3)),
        ("natoms = 0", I, dict(natoms=0)),
        ("n1 above natoms without an index", I, dict(n1=11)),
        ("n2 above natoms without an index", I, dict(n2=11)),
        ("a stride below 3 natoms", I, dict(stride=29)),
        ("ld1 below n1", I, dict(want=("atom1",), ld1=3)),
        ("ld2 below n2", I, dict(want=("atom2",), ld2=4)),
        ("an index not below natoms", I, dict(idx1=[0, 1, 2, 10])),
        ("a second index not below natoms", I, dict(idx2=[0, 1, 2, 3, 10])),
        ("a label not below ngroups1", I, dict(lab1=[0, 1, 2, 1], G1=2)),
        ("a label not below ngroups2", I, dict(lab2=[0, 1, 3, 1, 0], G2=3)),
        ("null frames", I, dict(null_frames=True)),
        ("2^31 cells", L, dict(idx1=np.zeros(4), lab1=[0, 0, 0, 0], G1=1 << 16, idx2=np.zeros(5), lab2=[0] * 5, G2=1 << 16, want=())),
    ]
    for fn, real in ((lib.molar_hip_mindist, np.float32), (lib.molar_hip_mindist_f64, np.float64)):
        for what, want, kw in errors:
            got = raw_call(fn, C.addressof(ctx), real, **kw)
            assert got == want, (what, want, got, lib.molar_hip_last_error())
        assert raw_call(fn, C.addressof(ctx), real, F=0) == 0, "nframes == 0 is a successful no-op"
        assert raw_call(fn, None, real) == mr.ERR_INVALID, "a null context"


def test_host_helpers():
    from molar_amd import api
    resids = np.array([1, 1, 1, 2, 2, 3, 99999, 1, 1, 2])                  # the column wraps: the second 1 is another residue
    lab, G = api.mindist_groups_from_resindex(resids)
    assert lab.dtype == np.uint32 and list(lab) == [0, 0, 0, 1, 1, 2, 3, 4, 4, 5] and G == 6
    lab, G = api.mindist_groups_from_resindex(resids, idx=[8, 0, 4, 9])    # the residues the selection touches, in file order
    assert list(lab) == [2, 0, 1, 3] and G == 4
    lab, G = api.mindist_groups_from_resindex([])
    assert lab.shape == (0,) and G == 0
    assert api.MinDistances._fields == ("dist", "pair", "atom1", "near1", "atom2", "mat", "mat_mean", "mat_min", "mat_freq", "frame_ok", "nvalid")
    assert (api.MINDIST_DIST, api.MINDIST_ATOM1, api.MINDIST_ATOM2, api.MINDIST_MAT) == (1, 2, 4, 8)


# ---------------------------------------------------------------- the reference against itself

def test_box_record_as_the_library_forms_it():
    ortho = mr.box_from_matrix(mr.ORTHO)
    assert ortho.shifts.shape == (0, 3) and np.array_equal(ortho.inv[[0, 4, 8]], 1.0 / mr.ORTHO[[0, 4, 8]]) and np.all(ortho.inv[[1, 2, 3, 5, 6, 7]] == 0.0)
    tric = mr.box_from_matrix(mr.TRIC)
    assert tric.shifts.shape[0] > 0, "the sheared cell has correction shifts"
    m = tric.m.reshape(3, 3).T
    assert np.allclose(tric.inv.reshape(3, 3).T @ m, np.eye(3), atol=1e-14)
    # every shift is a lattice vector, and the set is symmetric
    k = np.linalg.solve(m, tric.shifts.T).T
    assert np.allclose(k, np.round(k), atol=1e-12) and {tuple(r) for r in np.round(k)} == {tuple(-r) for r in np.round(k)}
    assert mr.box_from_matrix([1, 0, 0, 0, 0, 0, 0, 0, 1]) is None and mr.box_from_matrix([1, 0, 0, 2, 0, 0, 0, 0, 1]) is None


@pytest.mark.parametrize("pbc", [0, 1, 2, 3, 4, 5, 6, 7])
def test_shortest_vector_against_the_image_enumeration(pbc):
    rng = np.random.default_rng(pbc)
    box = mr.box_from_matrix(mr.ORTHO)
    v = (rng.uniform(-2.2, 2.2, (4000, 3)) * mr.ORTHO[[0, 4, 8]]).astype(mr.LD)
    best, _, _ = mr.shortest_vector(box, v, pbc)
    d = np.sqrt((best * best).sum(axis=-1))
    e = mr.image_enumeration(mr.ORTHO[[0, 4, 8]], v, pbc)
    # the two routes differ by the f64 rounding of 1 / L alone: L (1 / L) v against v
    assert np.max(np.abs(d - e)) <= 4.0 * mr.U * np.max(np.abs(v).astype(np.float64)) * np.sqrt(3.0)
    # under the sheared cell with the shifts no lattice translate is shorter
    tric = mr.box_from_matrix(mr.TRIC)
    w = v[:400]
    best, _, _ = mr.shortest_vector(tric, w, 7)
    n2 = (best * best).sum(axis=-1)
    m = tric.m.reshape(3, 3).T.astype(mr.LD)
    for i in range(-2, 3):
        for j in range(-2, 3):
            for k in range(-2, 3):
                t = best + (m @ np.array([i, j, k], mr.LD))
                assert np.all((t * t).sum(axis=-1) >= n2 * (1 - 1e-15))


def test_reference_known_answers():
    # two atoms through the boundary of a cube; a frame that is not finite; an empty group and an excluded diagonal
    frames = np.array([[[0.25, 0.5, 0.5], [3.75, 0.5, 0.5], [2.0, 2.0, 2.0]],
                       [[0.25, 0.5, 0.5], [np.nan, 0.5, 0.5], [2.0, 2.0, 2.0]],
                       [[0.5, 0.5, 0.5], [3.75, 0.5, 0.5], [2.0, 2.0, 2.0]]])
    box = np.diag([4.0, 4.0, 4.0]).reshape(9)
    r = mr.reference(frames, box, [0], [1, 2], None, [0, 2], 1, 3, cutoff=0.6)
    assert list(r.frame_ok) == [1, 0, 1] and r.nvalid == 2
    assert r.dist[0] == 0.5 and np.isnan(r.dist[1]) and r.dist[2] == 0.75
    assert r.pair.tolist() == [[0, 0], [int(mr.NONE)] * 2, [0, 0]] and r.near1[1, 0] == mr.NONE
    assert r.atom2[0].tolist() == [0.5, 2.75] and np.all(np.isnan(r.atom2[1]))
    assert r.mat.shape == (3, 1, 3) and np.all(np.isposinf(r.mat[[0, 2], 0, 1])) and np.all(np.isnan(r.mat[1]))
    assert r.mat_mean[0, 0] == 0.625 and np.isposinf(r.mat_mean[0, 1]) and r.mat_min[0, 0] == 0.5 and list(r.mat_freq[0]) == [1, 0, 0]
    plain = mr.reference(frames[:1], None, [0], [1, 2], cutoff=0.6)
    assert plain.dist[0] == 2.75 and plain.pair.tolist() == [[0, 1]]
    s = mr.reference(frames[[2]], box, [0, 1, 2], None, [0, 0, 1], None, 2, None, same=True, exclude_same_group=True, cutoff=0.6)
    assert np.all(np.isposinf(s.mat[:, [0, 1], [0, 1]])) and np.array_equal(s.mat, s.mat.transpose(0, 2, 1)) and s.pair.tolist() == [[0, 2]]
    one = mr.reference(frames[:1], box, [0], None, same=True)
    assert np.isposinf(one.dist[0]) and one.pair[0, 0] == mr.NONE and np.isposinf(one.mat_mean[0, 0])
    nothing = mr.reference(frames[1:2], box, [0], [1, 2])
    assert nothing.nvalid == 0 and np.isnan(nothing.mat_mean[0, 0]) and np.isposinf(nothing.mat_min[0, 0])


def test_reference_refuses_inputs_it_cannot_decide():
    base = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 3.0, 0.0]]])
    with pytest.raises(AssertionError, match="argmin"):
        mr.reference(base, None, [0], [1, 2])                                # two atoms at the same distance
    near = base.copy()
    near[0, 2, 0] = -1.0 - 1e-15
    with pytest.raises(AssertionError, match="argmin"):
        mr.reference(near, None, [0], [1, 2])                                # apart, but by less than the bounds
    mr.reference(base, None, [0], [1, 2], check=False)
    with pytest.raises(AssertionError, match="cutoff"):
        mr.reference(base, None, [0], [1, 3], cutoff=1.0)                    # a group distance on the cutoff
    # a fractional coordinate on one half under the sheared cell
    tric = mr.box_from_matrix(mr.TRIC)
    half = (tric.m.reshape(3, 3).T @ np.array([0.5, 0.1, 0.2]))
    frames = np.array([[[0.0, 0.0, 0.0], half, [0.3, 0.1, 0.0]]])
    with pytest.raises(AssertionError, match="flip"):
        mr.reference(frames, mr.TRIC, [1], [0])
    mr.reference(frames, mr.TRIC, [2], [0])


@pytest.mark.parametrize("case", mr.ALL_CASES, ids=lambda c: c.name)
def test_every_committed_case_passes_the_reference_assertions(case):
    r = mr.case_reference(case, mr.EPS32)
    good = r.frame_ok.astype(bool)
    assert r.nvalid == good.sum() and (len(case.bad) == 0) == bool(good.all())
    assert np.all(np.isfinite(r.atom1[good])) or case.same
    assert np.all(r.b_atom1[good] < 1e-6) and np.all(r.b_atom1[good] > 0.0)
    if case.G1 > 2:
        assert np.all(np.isposinf(r.mat[good][:, 1, :])), "group 1 stays empty"
