"""Trajectory fluctuations on the GPU (molar_hip_fluct / _f64: mean structure, RMSF, positional covariance after an optional
fit) against the numpy reference of tests/fluct_ref.py, entry by entry within the bounds derived there.  Every reference is
computed once per module."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fluct_ref as fr  # noqa: E402

pytestmark = pytest.mark.gpu

U = fr.U


@pytest.fixture(scope="module")
def eng():
    from molar_amd import api
    return api.Engine()


@pytest.fixture(scope="module")
def m64(eng):
    from molar_amd import api
    return api.MeasureF64(eng)


def split_frames(n=5):
    return fr.split_frames(n)


def k_fit():
    return fr.k_fit()[0]


@functools.lru_cache(maxsize=None)
def tile_ref(F, n, fit):
    frames = fr.tile_case(F, n, fit)
    return frames, fr.fluct(frames, fit=fit)


@functools.lru_cache(maxsize=None)
def named_ref(name):
    kw = fr.named_inputs()[name]
    return kw, fr.fluct(fit=True, **kw)


def as64(kw):
    return {k: (v.astype(np.float64) if isinstance(v, np.ndarray) and v.dtype == np.float32 else v) for k, v in kw.items()}


def exact_symmetry(cov):
    assert np.array_equal(cov, cov.T), "not symmetric bit for bit"


def check_trace(got, ref, eps_out):
    """rmsf^2 equals the trace of its diagonal block of the covariance, to the sum of the two bounds."""
    b_cov, _, b_rmsf2, _, _ = fr.bounds(ref, eps_out, k_fit())
    tr = np.diag(got.cov.astype(np.float64)).reshape(-1, 3).sum(1)
    lim = b_rmsf2 + np.diag(b_cov).reshape(-1, 3).sum(1)
    assert fr.worst(np.abs(got.rmsf.astype(np.float64) ** 2 - tr), lim) <= 1.0


def proper(fit, eps):
    R = fit[:, :9].astype(np.float64).reshape(-1, 3, 3).transpose(0, 2, 1)
    assert np.all(np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)) <= 8 * eps), "R^T R is not the identity"
    assert np.all(np.linalg.det(R) > 0)
    return R


TILE = [(F, n, False) for n in fr.TILE_N_NOFIT for F in fr.TILE_F] + [(F, n, True) for n in fr.TILE_N_FIT for F in fr.TILE_F]


def tile_checks(call, frames, ref, F, n, fit, eps, what):
    got = call(frames, fit=fit, cov=True, fit_out=True)
    assert got.mean.shape == (n, 3) and got.rmsf.shape == (n,) and got.cov.shape == (3 * n, 3 * n) and got.fit.shape == (F, 13)
    exact_symmetry(got.cov)
    fr.check(got, ref, eps, k_fit(), what)
    check_trace(got, ref, eps)
    R = proper(got.fit, eps)
    if F == 1:
        assert np.all(got.cov == 0) and np.all(got.rmsf == 0), "one frame does not fluctuate"
        z = frames[0].astype(np.float64) @ R[0].T + got.fit[0, 9:12].astype(np.float64)
        assert np.allclose(got.mean, z, rtol=0, atol=(8 * eps + 64 * U) * (1 + np.abs(z).max()))
    if not fit:
        assert np.array_equal(R, np.broadcast_to(np.eye(3), R.shape)) and np.all(got.fit[:, 9:12] == 0)


@pytest.mark.parametrize("F,n,fit", TILE)
def test_tile_edges(eng, F, n, fit):
    frames, ref = tile_ref(F, n, fit)
    tile_checks(eng.fluctuations, frames, ref, F, n, fit, fr.EPS32, f"F={F} n={n} fit={fit}")


@pytest.mark.parametrize("F,n,fit", TILE)
def test_tile_edges_f64(m64, F, n, fit):
    frames, ref = tile_ref(F, n, fit)
    tile_checks(m64.fluctuations, frames.astype(np.float64), ref, F, n, fit, fr.EPS64, f"f64 F={F} n={n} fit={fit}")


@pytest.mark.parametrize("fit", [False, True])
def test_frame_split_and_fused_paths(eng, m64, fit):
    from molar_amd import api
    n = 5
    big, small = split_frames(n)
    assert api.fluct_plan(big, n, True)[1] > 1 and api.fluct_plan(small, n, True)[1] == 1
    frames = fr.split_case(big)
    for F in (big, small):
        ref = fr.fluct(frames[:F], fit=fit)
        got = eng.fluctuations(frames[:F], fit=fit, cov=True)
        exact_symmetry(got.cov)
        fr.check(got, ref, fr.EPS32, k_fit(), f"split F={F} fit={fit}")
        got64 = m64.fluctuations(frames[:F].astype(np.float64), fit=fit, cov=True)
        exact_symmetry(got64.cov)
        fr.check(got64, ref, fr.EPS64, k_fit(), f"split f64 F={F} fit={fit}")
        check_trace(got64, ref, fr.EPS64)
        again = m64.fluctuations(frames[:F].astype(np.float64), fit=fit, cov=True)
        assert all(np.array_equal(a, b) for a, b in zip(got64[:3], again[:3])), "the same call twice gives other bits"


def test_repeatability_and_cov_switch(eng):
    kw, _ = named_ref("gaps")
    a = eng.fluctuations(cov=True, fit_out=True, **kw)
    b = eng.fluctuations(cov=True, fit_out=True, **kw)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    c = eng.fluctuations(cov=False, **kw)
    assert c.cov is None and c.fit is None
    assert np.array_equal(c.mean, a.mean) and np.array_equal(c.rmsf, a.rmsf)


def test_selection_with_gaps_and_frame_stride(eng, m64):
    natoms, n, F = 300, 77, 19
    rng = np.random.default_rng(7)
    idx = np.sort(rng.choice(natoms, n, replace=False)).astype(np.uint64)
    body = fr.random_frames(F, natoms, seed=11, sigma=0.07)
    wide = rng.normal(size=(F, 3 * natoms + 5)).astype(np.float32)
    wide[:, :3 * natoms] = body.reshape(F, -1)
    frames = wide[:, :3 * natoms].reshape(F, natoms, 3)               # frame stride 3 natoms + 5, read in place
    assert frames.strides[0] == 4 * (3 * natoms + 5)
    mass = rng.uniform(1.0, 16.0, natoms).astype(np.float32)
    for fit in (True, False):
        ref = fr.fluct(frames, idx=idx, mass=mass, fit=fit)
        got = eng.fluctuations(frames, idx=idx, mass=mass, fit=fit, cov=True, fit_out=True)
        exact_symmetry(got.cov)
        fr.check(got, ref, fr.EPS32, k_fit() if fit else 1.0, f"gaps + stride fit={fit}")
        same = eng.fluctuations(np.ascontiguousarray(frames), idx=idx, mass=mass, fit=fit, cov=True, fit_out=True)
        assert all(np.array_equal(a, b) for a, b in zip(got, same)), "contiguous frames give other bits"


def test_device_memory_equals_host_memory(eng, m64):
    import torch
    kw, _ = named_ref("gaps")
    host = eng.fluctuations(cov=True, fit_out=True, iterations=1, **kw)
    dev = eng.fluctuations(torch.from_numpy(kw["frames"]).cuda(), idx=torch.from_numpy(kw["idx"].astype(np.int64)).cuda(),
                           mass=torch.from_numpy(kw["mass"]).cuda(), cov=True, fit_out=True, iterations=1)
    assert all(t.is_cuda and t.dtype == torch.float32 for t in dev)
    eng.synchronize()                                                 # device results are written on the engine's stream, not waited for
    assert all(np.array_equal(d.cpu().numpy(), h) for d, h in zip(dev, host))
    k64 = as64(kw)
    host64 = m64.fluctuations(cov=True, fit_out=True, **k64)
    ref_dev = torch.from_numpy(k64["frames"][0][k64["idx"].astype(np.int64)].copy()).cuda()
    dev64 = m64.fluctuations(torch.from_numpy(k64["frames"]).cuda(), idx=torch.from_numpy(kw["idx"].astype(np.int64)).cuda(),
                             mass=torch.from_numpy(k64["mass"]).cuda(), ref=ref_dev, cov=True, fit_out=True)
    eng.synchronize()
    assert all(np.array_equal(d.cpu().numpy(), h) for d, h in zip(dev64, host64))


def test_random_masses_with_zeros(eng, m64):
    kw, ref = named_ref("zero masses")
    assert np.count_nonzero(kw["mass"] == 0) == 12
    got = eng.fluctuations(cov=True, fit_out=True, **kw)
    fr.check(got, ref, fr.EPS32, k_fit(), "masses with zeros")
    light = kw["mass"] == 0
    assert np.all(got.rmsf[light] > 0) and np.all(np.diag(got.cov).reshape(-1, 3)[light] > 0)      # they still get their statistics
    got64 = m64.fluctuations(cov=True, fit_out=True, **as64(kw))
    fr.check(got64, ref, fr.EPS64, k_fit(), "masses with zeros f64")


def test_argument_errors(eng, m64):
    from molar_amd._lib import MolarHipError
    kw, _ = named_ref("zero masses")
    frames = kw["frames"]
    with pytest.raises(MolarHipError) as e:
        eng.fluctuations(frames, mass=np.zeros_like(kw["mass"]))
    assert e.value.code == 2                                          # MOLAR_HIP_ERR_ZERO_MASS
    with pytest.raises(MolarHipError) as e:
        m64.fluctuations(frames.astype(np.float64), mass=np.zeros(len(kw["mass"])))
    assert e.value.code == 2
    with pytest.raises(MolarHipError) as e:
        eng.fluctuations(frames, idx=np.array([1, frames.shape[1]], np.uint64))
    assert e.value.code == 50                                         # an index that is not below natoms
    with pytest.raises(MolarHipError) as e:
        eng.fluctuations(frames, idx=np.zeros(0, np.uint64))
    assert e.value.code == 1                                          # MOLAR_HIP_ERR_SIZES: n == 0
    # ld below 3n, through the C entry itself
    F, natoms = frames.shape[:2]
    fc = np.ascontiguousarray(frames)
    mean, rmsf, cov = np.zeros((natoms, 3), np.float32), np.zeros(natoms, np.float32), np.zeros((3 * natoms, 3 * natoms), np.float32)
    args = (eng.ctx, fc.ctypes.data, F, 3 * natoms, natoms, None, natoms, None, None, 1, 0, mean.ctypes.data, rmsf.ctypes.data, cov.ctypes.data)
    assert eng.lib.molar_hip_fluct(*args, C.c_size_t(3 * natoms - 1), None) == 1
    assert eng.lib.molar_hip_fluct(*args, C.c_size_t(3 * natoms), None) == 0
    empty = eng.fluctuations(frames[:0], cov=True, fit_out=True)      # no frames: a successful no-op
    assert empty.fit.shape == (0, 13)


def test_reference_argument(eng, m64):
    kw, ref = named_ref("given reference")
    got = eng.fluctuations(cov=True, fit_out=True, **kw)
    fr.check(got, ref, fr.EPS32, k_fit(), "given reference")
    frames = kw["frames"]
    a = eng.fluctuations(frames, cov=True, fit_out=True)
    b = eng.fluctuations(frames, ref=frames[0], cov=True, fit_out=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), "ref=None is not frame 0"
    idx = np.arange(1, 30, 2).astype(np.uint64)
    a = eng.fluctuations(frames, idx=idx, fit_out=True)
    b = eng.fluctuations(frames, idx=idx, ref=frames[0][idx.astype(np.int64)], fit_out=True)
    assert all(np.array_equal(x, y) for x, y in zip(a[:2] + a[3:], b[:2] + b[3:]))


def test_iterations(eng, m64):
    kw, _ = named_ref("iterated")
    frames = kw["frames"]
    ref = fr.fluct(frames, fit=True, iterations=2)
    got = eng.fluctuations(frames, iterations=2, cov=True, fit_out=True)
    fr.check(got, ref, fr.EPS32, k_fit(), "iterations=2")
    got64 = m64.fluctuations(frames.astype(np.float64), iterations=2, cov=True, fit_out=True)
    fr.check(got64, ref, fr.EPS64, k_fit(), "iterations=2 f64")
    # a property of the definition (checked on the reference by the CPU tests): refitting onto the mean lowers the summed squares
    first = m64.fluctuations(frames.astype(np.float64), fit_out=True)
    to_mean = m64.fluctuations(frames.astype(np.float64), ref=got64.mean, fit_out=True)
    assert (to_mean.fit[:, 12] ** 2).sum() <= (first.fit[:, 12] ** 2).sum()
    # without a fit the iterations are ignored
    a = eng.fluctuations(frames, fit=False, iterations=3, cov=True)
    b = eng.fluctuations(frames, fit=False, cov=True)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


@pytest.mark.parametrize("real", ["f32", "f64"])
def test_fit_records(eng, m64, real):
    kw, ref = named_ref("plain 257")
    eps = fr.EPS32 if real == "f32" else fr.EPS64
    got = eng.fluctuations(fit_out=True, **kw) if real == "f32" else m64.fluctuations(fit_out=True, **as64(kw))
    fr.check(got, ref, eps, k_fit(), f"records {real}")
    R = proper(got.fit, eps)
    # R p + t applied in numpy reproduces the mean
    z = np.einsum("fde,fke->fkd", R, kw["frames"].astype(np.float64)) + got.fit[:, None, 9:12].astype(np.float64)
    _, b_mean, _, b_R, _ = fr.bounds(ref, eps, k_fit())
    slack = b_mean + (b_R * np.sqrt(3.0) + 8 * eps) * (1 + np.abs(kw["frames"]).max())      # the records' own rounding, applied to |p|
    assert fr.worst(np.abs(z.mean(0) - got.mean), slack) <= 1.0


def test_two_atoms_with_fit(eng, m64):
    """The optimal rotation of two atoms is not unique: only the rmsd and the properness of R are checked."""
    frames = fr.random_frames(6, 2, seed=12, sigma=0.1)
    ref = fr.fluct(frames, fit=True)
    for call, fz, eps in ((eng.fluctuations, frames, fr.EPS32), (m64.fluctuations, frames.astype(np.float64), fr.EPS64)):
        got = call(fz, fit=True, cov=True, fit_out=True)
        proper(got.fit, eps)
        _, _, _, _, b_rmsd2 = fr.bounds(ref, eps, 1.0)
        assert fr.worst(np.abs(got.fit[:, 12].astype(np.float64) ** 2 - ref.rmsd ** 2), b_rmsd2) <= 1.0
        assert np.all(np.isfinite(got.mean)) and np.all(np.isfinite(got.cov))
        exact_symmetry(got.cov)


def test_non_finite_input(eng):
    kw, _ = named_ref("given reference")
    frames, ref = kw["frames"], kw["ref"]
    assert frames.shape[0] == 8
    clean = eng.fluctuations(frames, ref=ref, cov=True, fit_out=True)
    dirty = frames.copy()
    dirty[3, 11, 1] = np.nan
    got = eng.fluctuations(dirty, ref=ref, cov=True, fit_out=True)       # status 0: no exception
    assert np.all(np.isnan(got.fit[3]))
    keep = np.arange(8) != 3
    assert np.array_equal(got.fit[keep], clean.fit[keep])
    assert np.all(np.isnan(got.mean)) and np.all(np.isnan(got.rmsf)) and np.all(np.isnan(got.cov))     # the fitted frame enters all of them
    # without a fit the NaN enters one coordinate only
    got = eng.fluctuations(dirty, fit=False, cov=True)
    bad = np.zeros(3 * frames.shape[1], bool)
    bad[3 * 11 + 1] = True
    assert np.array_equal(np.isnan(got.mean.ravel()), bad)
    assert np.array_equal(np.isnan(got.rmsf), bad.reshape(-1, 3).any(1))
    assert np.array_equal(np.isnan(got.cov), bad[:, None] | bad[None, :])
    plain = eng.fluctuations(frames, fit=False, cov=True)
    assert np.array_equal(got.cov[~bad][:, ~bad], plain.cov[~bad][:, ~bad])
