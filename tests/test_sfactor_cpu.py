"""The static structure factor without a GPU: the ABI of the three entries, the plan entry (a pure host function) and its
overrides, the errors of the arguments alone, the numpy reference (tests/sfactor_ref.py) against known answers and its own
assertion, the kernels' route restated in numpy float64 against the acceptance bounds of the GPU tests, and the host helpers."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sfactor_ref as sr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("molar_hip_sfactor_plan", "molar_hip_sfactor", "molar_hip_sfactor_f64")


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
    assert len(funcs["molar_hip_sfactor_plan"]) == len(_lib.SYMBOLS["molar_hip_sfactor_plan"][1]) == 11
    assert len(funcs["molar_hip_sfactor"]) == len(_lib.SYMBOLS["molar_hip_sfactor"][1]) == 20
    assert len(funcs["molar_hip_sfactor_f64"]) == len(_lib.SYMBOLS["molar_hip_sfactor_f64"][1]) == 20
    assert [t for t, _ in funcs["molar_hip_sfactor"]] == [t.replace("double", "float") for t, _ in funcs["molar_hip_sfactor_f64"]]
    assert open(gen.OUT).read() == gen.render(gen.c_functions(open(gen.HEADER).read())), "run python tools/gen_rust_ffi.py"
    # the grid struct: the same fields on every side, 40 bytes
    assert C.sizeof(_lib.SfactorGrid) == 40 and [f[0] for f in _lib.SfactorGrid._fields_] == ["hmax", "qmin", "dq", "nshells", "reserved"]
    assert re.search(r"typedef struct \{ uint32_t hmax\[3\]; double qmin, dq; uint32_t nshells; uint32_t reserved; \} molar_hip_sfactor_grid;", header)
    types_rs = open(os.path.join(ROOT, "rust", "molar_hip", "src", "types.rs")).read()
    assert re.search(r"pub struct MolarHipSfactorGrid \{\s*pub hmax: \[u32; 3\],\s*pub qmin: f64,\s*pub dq: f64,\s*pub nshells: u32,\s*pub reserved: u32,\s*\}", types_rs)
    hpp = open(os.path.join(ROOT, "include", "molar_hip.hpp")).read()
    assert "structure_factor(" in hpp and "structure_factor_f64(" in hpp and "(molar_hip_sfactor," in hpp and "(molar_hip_sfactor_f64," in hpp
    lib_rs = open(os.path.join(ROOT, "rust", "molar_hip", "src", "lib.rs")).read()
    assert "pub fn structure_factor(" in lib_rs and "pub fn structure_factor_plan(" in lib_rs
    assert "sfactor.hip" in build.SOURCES


def test_plan_needs_no_gpu_is_monotone_and_honours_the_overrides(monkeypatch):
    from molar_amd import api, build
    build.build_library()
    monkeypatch.delenv("MOLAR_HIP_SFACTOR_ATOM_CHUNK", raising=False)
    monkeypatch.delenv("MOLAR_HIP_SFACTOR_FRAME_BLOCK", raising=False)
    g = api.sfactor_grid((3, 3, 3), 0.0, 0.1, 8)
    assert api.sfactor_plan(0, 100, g)[0] == 0 and api.sfactor_plan(100, 0, g)[0] == 0
    ws, layout, rb, cb, ac, ks, fb = api.sfactor_plan(10, 5000, g)
    assert (layout, rb, cb) == (0, sr.ROW_BLOCK, sr.COL_BLOCK) and ac % 16 == 0 and ks == -(-5000 // ac) and fb == 10
    assert api.sfactor_plan(10, 100, api.sfactor_grid((3, 3, 0)))[1] == 1, "a lateral grid: rows k, columns h"
    assert api.sfactor_plan(10, 100, api.sfactor_grid((3, 0, 0)))[1] == 0, "K = L = 0 stays with layout 0"
    assert api.sfactor_plan(10, 100, api.sfactor_grid((0, 0, 3)))[1] == 0

    def w(F=64, n=1000, G=1, hmax=(3, 3, 3), ns=8):
        return api.sfactor_plan(F, n, api.sfactor_grid(hmax, 0.0, 0.1, ns), G)[0]

    for key, values in (("F", [1, 2, 3, 63, 64, 255, 256, 257, 1000, 4096, 100000]), ("n", [1, 3, 4, 5, 2047, 2048, 2049, 100000, 333333, 10 ** 6]),
                        ("G", [1, 2, 3, 7, 50]), ("ns", [0, 1, 8, 64, 1000])):
        for other in (dict(), dict(hmax=(16, 16, 16)), dict(hmax=(32, 32, 0)), dict(n=333333) if key != "n" else dict(F=3)):
            seq = [w(**{key: v}, **other) for v in values]
            assert seq == sorted(seq), (key, other, seq)
    for d in range(3):
        for other in (dict(), dict(F=1000, n=333333), dict(G=3)):
            seq = []
            for h in (0, 1, 2, 7, 8, 16, 31, 32, 63, 64, 100):
                hm = [4, 4, 4]
                hm[d] = h
                seq.append(w(hmax=tuple(hm), **other))
            assert seq == sorted(seq), (d, other, seq)
    # frame_block shrinks where one frame's regions are large, the workspace does not
    big = api.sfactor_plan(1000, 333333, api.sfactor_grid((16, 16, 16), 0.0, 0.1, 64))
    assert 1 <= big[6] < 256 and big[5] == -(-333333 // big[4])
    # the overrides, read by the plan as by the call
    monkeypatch.setenv("MOLAR_HIP_SFACTOR_ATOM_CHUNK", "64")
    monkeypatch.setenv("MOLAR_HIP_SFACTOR_FRAME_BLOCK", "2")
    p = api.sfactor_plan(10, 5000, g)
    assert p[4] == 64 and p[5] == -(-5000 // 64) and p[6] == 2
    monkeypatch.setenv("MOLAR_HIP_SFACTOR_ATOM_CHUNK", "70")
    assert api.sfactor_plan(10, 5000, g)[4] == 80, "rounded up to the 16 atoms staged at a time"
    monkeypatch.setenv("MOLAR_HIP_SFACTOR_FRAME_BLOCK", "50")
    assert api.sfactor_plan(10, 5000, g)[6] == 10, "never more than the frames"
    # what the plan refuses
    with pytest.raises(api.MolarHipError):
        api.sfactor_plan(10, 100, api.sfactor_grid((1024, 0, 0)))
    with pytest.raises(api.MolarHipError):
        api.sfactor_plan(10, 100, api.sfactor_grid((3, 3, 3), 0.0, 0.0, 4))
    with pytest.raises(api.MolarHipError):
        api.sfactor_plan(10, 100, api.sfactor_grid((1023, 1023, 1023)))


def test_argument_errors_need_no_device():
    from molar_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    ctx = C.create_string_buffer(1 << 16)                    # never read: the arguments are judged before the context is used
    for fn, real in ((lib.molar_hip_sfactor, np.float32), (lib.molar_hip_sfactor_f64, np.float64)):
        for what, want, got in sr.argument_errors(fn, C.addressof(ctx), real):
            assert got == want, (what, want, got, lib.molar_hip_last_error())
        assert sr.raw_sfactor(fn, C.addressof(ctx), real, F=0) == 0, "nframes == 0 is a successful no-op"
        assert sr.raw_sfactor(fn, None, real) == sr.ERR_INVALID


def test_reference_one_atom():
    p = np.array([[[0.7, -1.3, 5.1]]])
    w = np.array([-2.5])
    hmax = (2, 2, 1)
    r = sr.reference(p, sr.TRICLINIC32, None, w, None, 1, hmax)
    m, _ = sr.miller(hmax)
    s = np.linalg.solve(sr.box_matrix(sr.TRICLINIC32), p[0, 0])
    want = -2.5 * np.exp(-2j * np.pi * (m @ s))
    assert np.abs(r.rho[0, 0, :, 0] + 1j * r.rho[0, 0, :, 1] - want).max() < 1e-13
    assert np.abs(r.sab[0] - 6.25).max() < 1e-13, "|rho|^2 = w^2"
    assert np.abs(r.rho_mean - r.rho[0]).max() == 0.0 and r.frame_ok[0] == 1


def test_reference_cubic_lattice_and_two_species():
    c, hmax = 3, (6, 3, 4)
    m, _ = sr.miller(hmax)
    x = sr.cubic_lattice(c)[None]
    r = sr.reference(x, sr.ORTHO, None, None, None, 1, hmax)
    bragg = np.all(m % c == 0, axis=1)
    rho = r.rho[0, 0, :, 0] + 1j * r.rho[0, 0, :, 1]
    assert np.abs(rho[bragg] - c ** 3).max() < 1e-12 and np.abs(rho[~bragg]).max() < 1e-12
    # a second species on the same lattice shifted by half a spacing: rho_b = rho_a exp(-i pi (h + k + l) / c), so at a Bragg
    # point S_ab = N^2 (-1)^((h + k + l) / c)
    both = np.concatenate([sr.cubic_lattice(c), sr.cubic_lattice(c, offset=0.5)])[None]
    labels = np.repeat([0, 1], c ** 3)
    r2 = sr.reference(both, sr.ORTHO, None, None, labels, 2, hmax)
    sign = np.where((m.sum(axis=1) // c) % 2 == 0, 1.0, -1.0)
    assert np.abs(r2.sab[0][bragg] - c ** 6).max() < 1e-9 and np.abs(r2.sab[2][bragg] - c ** 6).max() < 1e-9
    assert np.abs(r2.sab[1][bragg] - sign[bragg] * c ** 6).max() < 1e-9
    assert np.abs(r2.sab[:, ~bragg]).max() < 1e-9


def test_reference_asserts_on_a_q_on_a_shell_edge():
    m, canonical = sr.miller((2, 2, 2))
    q = sr.qnorm(sr.ORTHO, m)
    on_edge = float(q[canonical][3])
    with pytest.raises(AssertionError):
        sr.shell_bins(sr.ORTHO, m, canonical, on_edge - 2 * 0.37, 0.37, 6)
    # the edges the tests use pass for every box they use
    for case in sr.ALL_CASES:
        if case.nshells:
            boxes = np.asarray(sr.case_inputs(case)[1], np.float64).reshape(-1, 9)
            mm, cc = sr.miller(case.hmax)
            for b in boxes:
                sr.shell_bins(b, mm, cc, case.qmin, case.dq, case.nshells)


def test_reference_nan_frame_and_shells():
    case = sr.C("nan", 9, 3, (2, 2, 1), box="scaled", G=2, signed=True, nshells=6)
    frames, boxes, idx, weight, labels = sr.case_inputs(case)
    fr = frames.copy()
    fr[1, 4, 2] = np.nan
    r = sr.reference(fr, boxes, idx, weight, labels, 2, case.hmax, sr.QMIN, sr.DQ, 6)
    keep = sr.reference(fr[[0, 2]], np.asarray(boxes)[[0, 2]], idx, weight, labels, 2, case.hmax, sr.QMIN, sr.DQ, 6)
    assert list(r.frame_ok) == [1, 0, 1] and np.all(np.isnan(r.rho[1])) and not np.any(np.isnan(r.rho[[0, 2]]))
    assert np.array_equal(r.sab, keep.sab) and np.array_equal(r.shell, keep.shell, equal_nan=True) and np.array_equal(r.shell_count, keep.shell_count)
    m, canonical = sr.miller(case.hmax)
    assert int(r.shell_count.sum()) <= 2 * int(canonical.sum())
    none = sr.reference(np.full_like(fr, np.nan), boxes, idx, weight, labels, 2, case.hmax, sr.QMIN, sr.DQ, 6)
    assert not none.frame_ok.any() and np.all(np.isnan(none.sab)) and np.all(np.isnan(none.rho_mean)) and np.all(np.isnan(none.shell))
    assert not none.shell_count.any()


@pytest.mark.parametrize("case", sr.ALL_CASES, ids=lambda c: c.name)
def test_kernel_route_in_float64_stays_inside_half_of_the_bounds(case):
    frames, boxes, idx, weight, labels = sr.case_inputs(case)
    ref = sr.case_reference(case, sr.EPS64)
    got = sr.kernel_route(frames, boxes, idx, weight, labels, case.G, case.hmax)
    assert sr.fraction(got, ref.rho, ref.b_rho) <= 0.5


def test_host_helpers():
    from molar_amd import api
    hmax = (2, 1, 3)
    m, canonical = api.sfactor_miller(hmax)
    mm, cc = sr.miller(hmax)
    assert np.array_equal(m, mm) and np.array_equal(canonical, cc) and m.shape == (3 * 3 * 7, 3)
    H, K, L = hmax
    assert all(((h * (2 * K + 1) + (k + K)) * (2 * L + 1) + (l + L)) == i for i, (h, k, l) in enumerate(m))
    # of every pair m, -m inside the grid exactly one is canonical, and m = 0 is not
    inside = {tuple(v) for v in m}
    for v, c in zip(m, canonical):
        if tuple(-v) in inside and tuple(v) != (0, 0, 0):
            assert c != bool(canonical[[tuple(x) == tuple(-v) for x in m]][0])
    assert not canonical[list(map(tuple, m)).index((0, 0, 0))]
    q = api.sfactor_qvectors(sr.TRICLINIC32, hmax)
    assert q.shape == (63, 3) and np.abs(np.sqrt((q * q).sum(axis=1)) - np.asarray(sr.qnorm(sr.TRICLINIC32, m), np.float64)).max() < 1e-12
    M = sr.box_matrix(sr.TRICLINIC32)
    assert np.abs(q @ M - 2 * np.pi * m).max() < 1e-12, "q.a = 2 pi h, q.b = 2 pi k, q.c = 2 pi l"
    assert np.array_equal(api.sfactor_qvectors(M, hmax), q), "[3, 3] rows are the transposed [9]"
    boxes = np.stack([sr.TRICLINIC32, 1.1 * sr.TRICLINIC32])
    qf = api.sfactor_qvectors(boxes, hmax)
    assert qf.shape == (2, 63, 3) and np.array_equal(qf[0], q) and np.abs(qf[1] * 1.1 - q).max() < 1e-12
    g = api.sfactor_grid(hmax, 0.013, 0.37, 4)
    assert np.allclose(api.sfactor_shell_centres(g), 0.013 + 0.37 * (np.arange(4) + 0.5))
    assert np.array_equal(api.sfactor_pairs(3), [[0, 0], [0, 1], [0, 2], [1, 1], [1, 2], [2, 2]])
    # normalisation: by the atoms or by the sum of w^2 of the two groups
    labels = np.array([0, 2, 2, 0, 2])
    wts = np.array([1.0, -2.0, 0.5, 3.0, 1.0])
    sab = np.arange(6 * 4, dtype=np.float64).reshape(6, 4) + 1.0
    nn = api.sfactor_normalize(sab, labels=labels, ngroups=3, how="n")
    assert np.allclose(nn[0], sab[0] / 2) and np.allclose(nn[2], sab[2] / np.sqrt(6)) and np.allclose(nn[5], sab[5] / 3)
    assert np.all(np.isnan(nn[[1, 3, 4]])), "pairs with the empty group"
    w2 = api.sfactor_normalize(sab, weights=wts, labels=labels, ngroups=3, how="w2")
    assert np.allclose(w2[0], sab[0] / 10.0) and np.allclose(w2[5], sab[5] / 5.25) and np.allclose(w2[2], sab[2] / np.sqrt(52.5))
    assert np.allclose(api.sfactor_normalize(sab[:1], n=7), sab[:1] / 7)
    # intensity: the factor 2 for a != b, constant and q-dependent form factors
    s = np.array([[1.0, 2.0], [0.5, -1.0], [3.0, 1.0]])
    assert np.allclose(api.sfactor_intensity(s, [2.0, -1.0]), 4 * s[0] - 4 * s[1] + s[2])
    fq = np.array([[2.0, 1.0], [-1.0, 3.0]])
    assert np.allclose(api.sfactor_intensity(s, fq), fq[0] ** 2 * s[0] + 2 * fq[0] * fq[1] * s[1] + fq[1] ** 2 * s[2])
    # the series as a block of vectors
    rho = np.arange(2 * 3 * 5 * 2, dtype=np.float32).reshape(2, 3, 5, 2)
    v = api.sfactor_as_vectors(rho)
    assert v.shape == (2, 15, 3) and v.dtype == np.float32 and v.flags.c_contiguous
    assert np.array_equal(v[..., :2].reshape(2, 3, 5, 2), rho) and not v[..., 2].any()
