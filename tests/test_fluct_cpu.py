"""The trajectory fluctuations without a GPU: the ABI of the three entries, the plan entry (a pure host function), the numpy
reference (tests/fluct_ref.py) against answers known in closed form, the kernels' route restated in numpy against the
acceptance bounds of the GPU tests, and the cap on K_fit."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fluct_ref as fr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("molar_hip_fluct_plan", "molar_hip_fluct", "molar_hip_fluct_f64")


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
    assert len(funcs["molar_hip_fluct_plan"]) == len(_lib.SYMBOLS["molar_hip_fluct_plan"][1]) == 5
    assert len(funcs["molar_hip_fluct"]) == len(_lib.SYMBOLS["molar_hip_fluct"][1]) == 16
    assert len(funcs["molar_hip_fluct_f64"]) == len(_lib.SYMBOLS["molar_hip_fluct_f64"][1]) == 16
    assert open(gen.OUT).read() == gen.render(gen.c_functions(open(gen.HEADER).read())), "run python tools/gen_rust_ffi.py"
    hpp = open(os.path.join(ROOT, "include", "molar_hip.hpp")).read()
    assert "fluctuations(" in hpp and "fluctuations_f64(" in hpp and "molar_hip_fluct(" in hpp and "molar_hip_fluct_f64(" in hpp
    lib_rs = open(os.path.join(ROOT, "rust", "molar_hip", "src", "lib.rs")).read()
    assert "pub fn fluctuations(" in lib_rs and "pub fn fluct_plan(" in lib_rs
    assert "fluct.hip" in build.SOURCES


def test_plan_needs_no_gpu_and_is_monotone():
    from molar_amd import api, build
    build.build_library()
    for cov in (False, True):
        assert api.fluct_plan(0, 100, cov) == (0, 1)
        assert api.fluct_plan(100, 0, cov) == (0, 1)
    sizes_f = [1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 255, 256, 257, 511, 512, 1000, 1024, 4096, 10000, 65536]
    sizes_n = [1, 2, 5, 6, 21, 22, 43, 100, 1000, 1366, 4096, 4097, 5000, 100000]
    for cov in (False, True):
        for n in sizes_n:
            last = 0
            for F in sizes_f:
                ws, ks = api.fluct_plan(F, n, cov)
                assert ws >= last and ks >= 1, (F, n, cov, ws, last)
                assert cov or ks == 1
                if cov:
                    assert ws >= 8 * 3 * n * F               # the packed deviations alone
                last = ws
        for F in sizes_f:
            last = 0
            for n in sizes_n:
                ws, _ = api.fluct_plan(F, n, cov)
                assert ws >= last, (F, n, cov)
                last = ws
    for F in sizes_f:
        for n in sizes_n:
            assert api.fluct_plan(F, n, False)[0] <= api.fluct_plan(F, n, True)[0]
    # the two paths of the GPU tests: few coordinates and many frames split the frames, few frames do not
    assert api.fluct_plan(4096, 5, True)[1] > 1
    assert api.fluct_plan(64, 5, True)[1] == 1
    assert api.fluct_plan(256, 3000, True)[1] == 1


def test_reference_rigid_copies():
    """Rigid copies of one structure, fitted: mean = reference, cov = rmsf = 0, to the bound.  The copies themselves are rigid
    only to the f64 rounding of their construction (three products, two sums and the translation per coordinate: at most
    e_in = 8 u C, C the largest |coordinate|), which is data to the reference: the mean may be off by e_in and the variances
    by e_in^2 on top of the bounds."""
    base = fr.random_frames(1, 40, 1, sigma=0.0, rigid=False, dtype=np.float64)[0]
    rng = np.random.default_rng(2)
    frames = np.stack([base @ fr.random_rotation(rng).T + rng.normal(size=3) for _ in range(7)])
    ref = fr.fluct(frames, ref=base, fit=True)
    b_cov, b_mean, b_rmsf2, _, b_rmsd2 = fr.bounds(ref, fr.EPS64, fr.k_fit()[0])
    e_in = 8 * fr.U * np.abs(frames).max()
    assert np.all(np.abs(ref.mean - base) <= b_mean + e_in)
    assert np.all(np.abs(ref.cov) <= b_cov + e_in ** 2)
    assert np.all(ref.rmsf ** 2 <= b_rmsf2 + 3 * e_in ** 2)
    assert np.all(ref.rmsd ** 2 <= b_rmsd2 + 3 * e_in ** 2)


def test_reference_two_frames_without_fit():
    rng = np.random.default_rng(3)
    p = np.round(rng.normal(size=(9, 3)) * 64) / 64          # dyadic: p +- d and every product below are exact
    d = np.round(rng.normal(size=(9, 3)) * 16) / 64
    ref = fr.fluct(np.stack([p + d, p - d]), fit=False)
    assert np.array_equal(ref.mean, p)
    assert np.array_equal(ref.cov, np.outer(d.ravel(), d.ravel()))
    assert np.array_equal(ref.rmsf ** 2, (d * d).sum(-1)) or np.allclose(ref.rmsf, np.linalg.norm(d, axis=1), rtol=2e-16, atol=0)
    assert np.array_equal(ref.R[1], np.eye(3)) and np.all(ref.t == 0)
    assert np.allclose(ref.rmsd, [0.0, 2 * np.sqrt((d * d).sum() / 9)], rtol=1e-15)


def test_reference_cosine_displacement():
    F, a = 64, 0.25
    p = fr.random_frames(1, 5, 4, sigma=0.0, rigid=False, dtype=np.float64)[0]
    frames = np.repeat(p[None], F, axis=0)
    frames[:, 2, 1] += a * np.cos(2 * np.pi * np.arange(F) / F)
    ref = fr.fluct(frames, fit=False)
    assert abs(ref.cov[7, 7] - a * a / 2) < 1e-15
    assert abs(ref.rmsf[2] - a / np.sqrt(2)) < 1e-15
    assert np.all(np.abs(np.delete(ref.rmsf, 2)) < 1e-15)


def test_reference_rmsf_is_the_trace_of_the_diagonal_block():
    for fit in (False, True):
        ref = fr.fluct(fr.tile_case(17, 22, fit), fit=fit)
        tr = np.diag(ref.cov).reshape(-1, 3).sum(1)
        assert np.allclose(ref.rmsf ** 2, tr, rtol=1e-15, atol=0)
        assert np.array_equal(ref.cov, ref.cov.T)


def test_iterating_onto_the_mean_does_not_raise_the_sum_of_squares():
    """A property of the definition that the GPU test relies on: the mean of a pass is the minimiser of the summed squared
    distances for that pass's rotations, and refitting onto it can only lower them again."""
    kw = fr.named_inputs()["iterated"]
    first = fr.fluct(kw["frames"], fit=True, iterations=0)
    again = fr.fluct(kw["frames"], fit=True, iterations=2)
    to_mean = fr.fluct(kw["frames"], ref=again.mean, fit=True)
    assert (to_mean.rmsd ** 2).sum() <= (first.rmsd ** 2).sum()


def test_k_fit_stays_under_the_cap():
    k, units, where = fr.k_fit()
    print(f"K_fit = {k:.3g} (largest discrepancy of the two routes {units:.3g} u/g at {where})")
    assert 1.0 <= k <= 128.0, (k, units, where)


CASES = [(F, n, fit) for fit in (False, True) for n in (1, 2, 5, 22, 43, 257) for F in (1, 2, 5, 17, 260) if not (fit and n < 5)]


@pytest.mark.parametrize("F,n,fit", CASES)
def test_kernel_route_in_numpy_stays_inside_half_of_the_bounds(F, n, fit):
    """The bounds are derived, not measured; here the kernels' route in numpy f64 is held against half of them."""
    k = fr.k_fit()[0]
    rng = np.random.default_rng(1000 * n + F)
    for what, kw in {
        "plain": dict(),
        "masses": dict(mass=rng.uniform(0.5, 30.0, n)),
        "far from the origin": dict(offset=50.0),
    }.items():
        frames = fr.random_frames(F, n, seed=31 * n + F, sigma=0.05, rigid=fit).astype(np.float64)
        frames = (frames + kw.pop("offset", 0.0)).astype(np.float32)
        for iterations in ((0, 2) if fit and F > 2 else (0,)):
            ref = fr.fluct(frames, fit=fit, iterations=iterations, **kw)
            got = fr.kernel_route(frames, fit=fit, iterations=iterations, **kw)
            fr.check(got, ref, fr.EPS64, k, f"{what} F={F} n={n} fit={fit} it={iterations}", limit=0.5)
