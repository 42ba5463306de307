"""The time correlation functions of vectors without a GPU: the ABI of the three entries, the plan entry (a pure host function),
the errors of the arguments alone, the numpy reference (tests/tcf_ref.py) against itself and against known answers, the
kernels' summation order restated in numpy against the acceptance bounds of the GPU tests, and the host helpers."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tcf_ref as tr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("molar_hip_tcf_plan", "molar_hip_tcf", "molar_hip_tcf_f64")
mr = tr.mr


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
    assert len(funcs["molar_hip_tcf_plan"]) == len(_lib.SYMBOLS["molar_hip_tcf_plan"][1]) == 14
    assert len(funcs["molar_hip_tcf"]) == len(_lib.SYMBOLS["molar_hip_tcf"][1]) == 24
    assert len(funcs["molar_hip_tcf_f64"]) == len(_lib.SYMBOLS["molar_hip_tcf_f64"][1]) == 24
    assert [t for t, _ in funcs["molar_hip_tcf"]] == [t.replace("double", "float") for t, _ in funcs["molar_hip_tcf_f64"]]
    assert open(gen.OUT).read() == gen.render(gen.c_functions(open(gen.HEADER).read())), "run python tools/gen_rust_ffi.py"
    # the spec struct: the same four words on every side
    assert C.sizeof(_lib.TcfSpec) == 16 and [f[0] for f in _lib.TcfSpec._fields_] == ["kind", "mode", "dims", "reserved"]
    assert re.search(r"typedef struct \{ uint32_t kind; uint32_t mode; uint32_t dims; uint32_t reserved; \} molar_hip_tcf_spec;", header)
    types_rs = open(os.path.join(ROOT, "rust", "molar_hip", "src", "types.rs")).read()
    assert re.search(r"pub struct MolarHipTcfSpec \{\s*pub kind: u32,\s*pub mode: u32,\s*pub dims: u32,\s*pub reserved: u32,\s*\}", types_rs)
    assert "MOLAR_HIP_TCF_UNIT = 0, MOLAR_HIP_TCF_RAW = 1" in header and "TCF_UNIT: u32 = 0" in types_rs and "TCF_RAW: u32 = 1" in types_rs
    hpp = open(os.path.join(ROOT, "include", "molar_hip.hpp")).read()
    assert "vector_correlations(" in hpp and "vector_correlations_f64(" in hpp and "(molar_hip_tcf," in hpp and "(molar_hip_tcf_f64," in hpp
    lib_rs = open(os.path.join(ROOT, "rust", "molar_hip", "src", "lib.rs")).read()
    assert "pub fn vector_correlations(" in lib_rs and "pub fn vector_correlations_plan(" in lib_rs
    assert "tcf.hip" in build.SOURCES


def test_plan_needs_no_gpu_and_is_monotone():
    from molar_amd import api, build
    build.build_library()
    assert api.tcf_plan(0, 100)[0] == 0 and api.tcf_plan(100, 0)[0] == 0
    sizes_f = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 384, 1000, 4096, 65536]
    sizes_v = [1, 2, 63, 64, 65, 256, 257, 8191, 8192, 8193, 16384, 16385, 100000]

    def ws(F, V, **kw):
        w, fc, vc, lb, R, seg, win = api.tcf_plan(F, V, **kw)
        assert fc == 64 and 1 <= vc <= 64 and R in (1, 2, 4) and lb == 64 * R and seg % (2 * R) == 0 and win == seg + lb
        return w

    for V in sizes_v:
        last = 0
        for F in sizes_f:                                    # max_lag = F - 1 grows with F
            w = ws(F, V)
            assert w >= last and w >= 24 * V * F, (F, V)     # the f64 vectors alone
            last = w
    for F in sizes_f:
        for L in sorted({0, 1, F // 2, F - 1}):
            last = 0
            for V in sizes_v:
                w = ws(F, V, max_lag=L)
                assert w >= last, (F, V, L)
                last = w
        for V in (1, 64, 8193):
            seq = [ws(F, V, max_lag=L) for L in sorted({0, 1, F // 2, F - 1})]
            assert seq == sorted(seq)
            assert ws(F, V, ngroups=1) <= ws(F, V, ngroups=2) <= ws(F, V, ngroups=50)
            assert ws(F, V) <= ws(F, V, per_frame_boxes=True)
            # only mean / s2 / bad_frames: nothing for the lag stage; per-vector curves only: no group partials
            assert ws(F, V, want_lags=False) + 24 * V * F <= ws(F, V, want_groups=False) <= ws(F, V)
            assert ws(F, V, want_lags=False) == ws(F, V, want_lags=False, max_lag=0)
    # the launch-shape edges of the GPU tests: more than one vector per workgroup once vectors x lag blocks pass 2 x 8192
    assert api.tcf_plan(3, 16384)[2] == 2 and api.tcf_plan(3, 16383)[2] == 1 and api.tcf_plan(3, 100)[2] == 1


def test_argument_errors_need_no_device():
    from molar_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    ctx = C.create_string_buffer(1 << 16)                    # never read: the arguments are judged before the context is used
    for fn, real in ((lib.molar_hip_tcf, np.float32), (lib.molar_hip_tcf_f64, np.float64)):
        for what, want, got in tr.argument_errors(fn, C.addressof(ctx), real):
            assert got == want, (what, want, got, lib.molar_hip_last_error())
        assert tr.raw_tcf(fn, C.addressof(ctx), np.zeros((0, 5, 3), real), F=0) == 0, "nframes == 0 is a successful no-op"
        assert tr.raw_tcf(fn, None, np.ones((2, 5, 3), real)) == tr.ERR_INVALID
        # kind 1 reads neither boxes nor pbc: no ERR_NO_PBC before the context is needed (F = 0 ends the call there)
        assert tr.raw_tcf(fn, C.addressof(ctx), np.zeros((0, 5, 3), real), F=0, tuples=[[0]], pbc=7) == 0


def test_reference_image_routes_agree():
    fr, tp = tr.make_case(12, 9, 3, 5, box9=tr.ORTHO)
    a = tr.tcf(fr, tp, boxes=tr.ORTHO, route="round")
    b = tr.tcf(fr, tp, boxes=tr.ORTHO, route="brute")
    for name in ("c1", "c2", "c1_vec", "c2_vec", "mean", "s2"):
        assert float(np.abs(a[name] - b[name]).max()) <= 1e-16, name
    # the boundary did cut bonds: without the image the answer is another one altogether
    c = tr.tcf(fr, tp, boxes=None, pbc=0)
    assert float(np.abs(a["c1_vec"] - c["c1_vec"]).max()) > 0.1


def test_reference_asserts_on_ambiguous_input():
    fr = np.zeros((2, 2, 3), np.float32)
    fr[:, 1, 0] = 1.5                                        # half of the box along x
    for route in ("round", "brute"):
        with pytest.raises(AssertionError):
            tr.tcf(fr, [[0, 1]], boxes=tr.ORTHO, route=route)
    fr[:, 1, 0] = 2.0 ** -11                                 # neither zero nor long enough
    with pytest.raises(AssertionError):
        tr.tcf(fr, [[0, 1]])
    fr[:, 1, 0] = 0.0                                        # exactly zero, but not declared
    with pytest.raises(AssertionError):
        tr.tcf(fr, [[0, 1]])
    assert tr.tcf(fr, [[0, 1]], bad=[0])["bad_frames"][0] == 2
    assert tr.tcf(fr, [[0, 1]], mode=tr.RAW)["bad_frames"][0] == 0          # valid zeros in RAW mode


CASES = [dict(F=1, V=3, kind=2), dict(F=2, V=3, kind=1), dict(F=3, V=2, kind=3), dict(F=65, V=5, kind=2, chunk=2), dict(F=40, V=6, kind=2, os=7),
         dict(F=40, V=6, kind=3, dims=3, L=20), dict(F=30, V=7, kind=2, box="tric"), dict(F=30, V=7, kind=3, box="scaled", chunk=3, labels=True),
         dict(F=20, V=5, kind=2, box="ortho", pbc=3, dims=4), dict(F=24, V=6, kind=1, mode=tr.RAW, labels=True, chunk=4),
         dict(F=24, V=6, kind=2, box="ortho", bad=True, labels=True, chunk=2)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_kernel_route_in_numpy_stays_inside_half_of_the_bounds(case):
    F, V, kind = case["F"], case["V"], case["kind"]
    box = case.get("box")
    box9 = tr.TRICLINIC if box == "tric" else tr.ORTHO if box else None
    boxes = mr.scaled_boxes(F, 3) if box == "scaled" else box9
    fr, tp = tr.make_case(F, V, kind, 100 + F + V, box9=box9, boxes=boxes if box == "scaled" else None)
    bad = [1, 4] if case.get("bad") else []
    labels = np.array([2, 0, 0, 1, 0, 2, 2][:V]) if case.get("labels") else None
    kw = dict(boxes=boxes, pbc=case.get("pbc", 7) if box else 0, mode=case.get("mode", tr.UNIT), dims=case.get("dims", 7), max_lag=case.get("L"),
              origin_stride=case.get("os", 1), labels=labels, ngroups=4 if labels is not None else None)
    rng = np.random.default_rng(5)
    for frames in (fr.copy(), fr.astype(np.float64) + 1e-9 * rng.normal(size=fr.shape)):
        if bad:
            tr.make_bad(frames, tp, 1, F // 2)
            tr.make_bad(frames, tp, 4, 0, "nan")
        ref = tr.tcf(frames, tp, bad=bad, **kw)
        got = tr.kernel_route(frames, tp, vec_chunk=case.get("chunk", 1), **kw)
        for name, v in tr.check(got, ref, tr.EPS64, what=str(case)).items():
            assert v <= 0.5, (name, v)


def test_constant_vector_known_answer():
    fr = np.zeros((9, 2, 3), np.float32)
    fr[:, 1] = [0.25, -0.5, 1.0]
    ref = tr.tcf(fr, [[0, 1]])
    for name in ("c1", "c2", "c1_vec", "c2_vec", "s2"):
        assert np.abs(ref[name].astype(np.float64) - 1.0).max() <= 1e-15, name
    got = tr.kernel_route(fr, [[0, 1]])
    for name in ("c1", "c2", "c1_vec", "c2_vec", "s2"):
        assert np.abs(got[name] - 1.0).max() <= 64 * tr.U, name


def test_rotating_vector_known_answer():
    F, alpha = 64, 2 * np.pi / 64
    fr = np.zeros((F, 1, 3), np.float32)
    fr[:, 0, 0], fr[:, 0, 1] = np.cos(alpha * np.arange(F)), np.sin(alpha * np.arange(F))
    ref = tr.tcf(fr, [[0]])
    tau = np.arange(F)
    # the f32 rounding of a component (2^-24 relative, at most 2^-24 absolute) turns the unit vector by at most sqrt 2 2^-24;
    # the cosine of the angle between two of them moves by at most twice that, P2 by three times the move of the cosine
    # (|dP2/dx| <= 3), a second moment by twice the move of a component: margin 2^-21 for each
    margin = 2.0 ** -21
    assert np.abs(ref["c1"][0].astype(np.float64) - np.cos(alpha * tau)).max() <= margin
    assert np.abs(ref["c2"][0].astype(np.float64) - (3 * np.cos(alpha * tau) ** 2 - 1) / 2).max() <= margin
    assert abs(float(ref["s2"][0]) - 0.25) <= margin and np.abs(ref["mean"].astype(np.float64)).max() <= margin
    got = tr.kernel_route(fr, [[0]])
    assert np.abs(got["c1"][0] - np.cos(alpha * tau)).max() <= margin and abs(got["s2"][0] - 0.25) <= margin


def test_raw_ramp_known_answer():
    # kind 1 / RAW on x(f) = (f, 0, 0) / 8: d = t (t + tau) / 64, c1[tau] = mean over t = 0 .. F - 1 - tau, exact in the reals
    F = 17
    fr = np.zeros((F, 1, 3), np.float32)
    fr[:, 0, 0] = np.arange(F) / 8.0
    ref = tr.tcf(fr, [[0]], mode=tr.RAW)
    want = np.array([np.mean([t * (t + tau) / 64.0 for t in range(F - tau)]) for tau in range(F)])
    assert np.abs(ref["c1"][0].astype(np.float64) - want).max() <= 1e-15 * want.max()
    assert ref["c2"] is None and ref["s2"] is None
    os3 = tr.tcf(fr, [[0]], mode=tr.RAW, origin_stride=3, max_lag=5)
    want3 = np.array([np.mean([t * (t + tau) / 64.0 for t in range(0, F - tau, 3)]) for tau in range(6)])
    assert np.abs(os3["c1"][0].astype(np.float64) - want3).max() <= 1e-15 * want3.max()


def test_host_helpers():
    from molar_amd import api
    assert np.array_equal(api.tcf_lags(10), np.arange(10, 0, -1))
    assert np.array_equal(api.tcf_lags(10, 4, 3), [4, 3, 3, 3, 2])
    assert np.array_equal(api.tcf_lags(10, 9, 100), np.ones(10))
    for F, L, os_ in ((1, 0, 1), (7, 6, 2), (40, 17, 7)):
        assert np.array_equal(api.tcf_lags(F, L, os_), tr.n_of_tau(F, L, os_))
    # exp(-t / T) sampled finely: the integral to the end
    dt, T = 0.01, 0.7
    y = np.exp(-np.arange(4000) * dt / T)
    assert abs(api.correlation_time(y, dt) - T * (1 - y[-1])) <= 1e-4 * T
    # a line through zero: the triangle up to the crossing, the rest is not counted
    assert abs(api.correlation_time(np.array([1.0, 0.5, 0.0, -0.5, 3.0]), 2.0) - 2.0) <= 1e-15
    assert abs(api.correlation_time(np.array([1.0, -1.0, 5.0]), 1.0) - 0.25) <= 1e-15
    assert api.correlation_time(np.array([0.0, 1.0]), 1.0) == 0.0 and api.correlation_time(np.array([2.0]), 1.0) == 0.0
    # angle_vectors: kind 1 / RAW of (cos, sin, 0) is the autocorrelation of the angle
    phi = np.random.default_rng(2).uniform(-np.pi, np.pi, size=(12, 3))
    block = api.angle_vectors(phi)
    assert block.shape == (12, 3, 3) and np.all(block[..., 2] == 0) and block.flags.c_contiguous
    ref = tr.tcf(block, [[0], [1], [2]], mode=tr.RAW)
    want = np.array([[np.mean(np.cos(phi[tau:, v] - phi[:12 - tau, v])) for tau in range(12)] for v in range(3)])
    assert np.abs(ref["c1_vec"].astype(np.float64) - want).max() <= 1e-14
    assert np.isnan(api.angle_vectors(np.array([[np.nan]]))[0, 0, 0])
