"""The all-pairs RMSD matrix on the GPU (molar_hip_rmsd_matrix / _f64) against the numpy reference of
tests/rmsd_matrix_ref.py.  Unless said otherwise every entry is held to the bound derived there from f64 rounding,

    |got^2 - ref^2| <= (3 n + 16) 2^-53 (rg2_a + rg2_b) + 4 eps_out ref^2,    eps_out = 2^-24 (f32 entry) or 2^-53 (f64 entry).

The references are computed once per module and shared."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rmsd_matrix_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu

TILE_F = [1, 2, 15, 16, 17, 33, 48]
TILE_N = [1, 2, 3, 5, 63, 64, 65, 257]


@pytest.fixture(scope="module")
def eng():
    from molar_amd import api
    return api.Engine()


@pytest.fixture(scope="module")
def m64(eng):
    from molar_amd import api
    return api.MeasureF64(eng)


@pytest.fixture(scope="module")
def tile_refs():
    """One block of 48 frames per n; every F of the tile-edge cases is a leading part of it, and so is its reference."""
    refs = {}
    for n in TILE_N:
        frames = rr.random_frames(max(TILE_F), n, 100 + n)
        refs[n] = (frames, *rr.matrix(frames)[:2])
    return refs


def exact_symmetry(got):
    assert np.array_equal(got, got.T), "not symmetric bit for bit"
    assert np.all(np.diagonal(got) == 0), "diagonal not exactly zero"


@pytest.mark.parametrize("n", TILE_N)
@pytest.mark.parametrize("F", TILE_F)
def test_tile_edges(eng, tile_refs, F, n):
    frames, ref, rg = tile_refs[n]
    got = eng.rmsd_matrix(frames[:F])
    assert got.dtype == np.float32 and got.shape == (F, F)
    exact_symmetry(got)
    rr.check(got, ref[:F, :F], rg[:F], rg[:F], n, rr.EPS32, f"F={F} n={n}")


@pytest.mark.parametrize("n", TILE_N)
@pytest.mark.parametrize("F", TILE_F)
def test_tile_edges_f64(m64, tile_refs, F, n):
    frames, ref, rg = tile_refs[n]
    got = m64.rmsd_matrix(frames[:F].astype(np.float64))
    assert got.dtype == np.float64
    exact_symmetry(got)
    rr.check(got, ref[:F, :F], rg[:F], rg[:F], n, rr.EPS64, f"f64 F={F} n={n}")


def test_selection_with_gaps_and_frame_stride(eng):
    natoms, n, F = 500, 123, 19
    rng = np.random.default_rng(7)
    idx = np.sort(rng.choice(natoms, n, replace=False)).astype(np.uint64)
    wide = rng.normal(size=(F, 3 * natoms + 5)).astype(np.float32)
    frames = wide[:, :3 * natoms].reshape(F, natoms, 3)               # frame stride 3 natoms + 5, read in place
    assert frames.strides[0] == 4 * (3 * natoms + 5)
    ref, rg, _ = rr.matrix(frames, idx=idx)
    got = eng.rmsd_matrix(frames, idx=idx)
    exact_symmetry(got)
    rr.check(got, ref, rg, rg, n, rr.EPS32, "gaps + stride")
    assert np.array_equal(got, eng.rmsd_matrix(np.ascontiguousarray(frames), idx=idx))


@pytest.fixture(scope="module")
def mass_case():
    natoms, F = 211, 21
    rng = np.random.default_rng(8)
    frames = rr.random_frames(F, natoms, 9)
    mass = rng.uniform(1.0, 32.0, natoms)
    mass[rng.choice(natoms, 30, replace=False)] = 0.0
    mass = mass.astype(np.float32)
    return frames, mass, rr.matrix(frames, mass=mass)


def test_random_masses_with_zeros(eng, m64, mass_case):
    frames, mass, (ref, rg, _) = mass_case
    got = eng.rmsd_matrix(frames, mass=mass)
    exact_symmetry(got)
    rr.check(got, ref, rg, rg, frames.shape[1], rr.EPS32, "masses")
    got64 = m64.rmsd_matrix(frames.astype(np.float64), mass=mass.astype(np.float64))
    exact_symmetry(got64)
    rr.check(got64, ref, rg, rg, frames.shape[1], rr.EPS64, "masses f64")


def test_all_masses_zero_is_an_error(eng, m64, mass_case):
    from molar_amd._lib import MolarHipError
    frames, mass, _ = mass_case
    with pytest.raises(MolarHipError) as e:
        eng.rmsd_matrix(frames, mass=np.zeros_like(mass))
    assert e.value.code == 2                                          # MOLAR_HIP_ERR_ZERO_MASS
    with pytest.raises(MolarHipError) as e:
        m64.rmsd_matrix(frames.astype(np.float64), mass=np.zeros(len(mass)))
    assert e.value.code == 2


def test_rectangular(eng):
    n = 77
    f1, f2 = rr.random_frames(7, n, 11), rr.random_frames(19, n, 12)
    ref, rg1, rg2 = rr.matrix(f1, f2)
    out = np.full((7, 24), -7.0, np.float32)
    got = eng.rmsd_matrix(f1, frames2=f2, out=out)
    assert got is out and np.all(out[:, 19:] == -7.0), "padding touched"
    rr.check(out[:, :19], ref, rg1, rg2, n, rr.EPS32, "7 x 19")
    back = eng.rmsd_matrix(f2, frames2=f1)
    assert back.shape == (19, 7)
    rr.check(back, ref.T, rg2, rg1, n, rr.EPS32, "19 x 7")
    # the same block twice is still the rectangular form: the diagonal is computed, not forced
    ref11, _, _ = rr.matrix(f1)
    twice = eng.rmsd_matrix(f1, frames2=f1)
    rr.check(twice, ref11, rg1, rg1, n, rr.EPS32, "7 x 7 of one block")


@pytest.fixture(scope="module")
def rigid_case():
    frames = rr.rigid_copies(6, 1000, 13)                             # 50 nm from the origin
    mirror = frames[0] * np.array([1, 1, -1], np.float32)
    frames = np.concatenate([frames, mirror[None]])
    return frames, rr.matrix(frames)


def test_rigid_copies_and_a_mirror_image(eng, m64, rigid_case):
    frames, (ref, rg, _) = rigid_case
    got = eng.rmsd_matrix(frames)
    exact_symmetry(got)
    rr.check(got, ref, rg, rg, 1000, rr.EPS32, "rigid at 50 nm")
    assert np.all(got[:6, :6] < 1e-4) and np.all(got[6, :6] > 0.3), "a mirror image must not fit"
    got64 = m64.rmsd_matrix(frames.astype(np.float64))
    rr.check(got64, ref, rg, rg, 1000, rr.EPS64, "rigid at 50 nm f64")


@pytest.mark.parametrize("shape", ["planar", "collinear"])
def test_degenerate_selections(eng, shape):
    n, F = 150, 18
    rng = np.random.default_rng(14)
    frames = rr.rigid_copies(F, n, 15, offset=3.0).astype(np.float64)
    base = rng.normal(size=(n, 3))
    base[:, 2] = 0.0
    if shape == "collinear":
        base[:, 1] = 0.0
    for f in range(F):                                                # rigid images of the flat structure, some perturbed in it
        moved = base + (rng.normal(size=(n, 3)) * 0.05 * (base != 0) if f % 3 == 2 else 0.0)
        frames[f] = moved @ rr.random_rotation(rng).T + 3.0
    frames = frames.astype(np.float32)
    ref, rg, _ = rr.matrix(frames)
    got = eng.rmsd_matrix(frames)
    exact_symmetry(got)
    rr.check(got, ref, rg, rg, n, rr.EPS32, shape)


def test_no_fit_mode(eng, m64):
    n, F = 301, 20
    base = rr.random_frames(1, n, 16)[0].astype(np.float64) + 20.0
    shifts = np.random.default_rng(17).normal(size=(F, 3))
    shifts[0] = 0.0
    frames = (base[None] + shifts[:, None, :]).astype(np.float32)
    mass = np.random.default_rng(18).uniform(1, 16, n).astype(np.float32)
    ref, rg, _ = rr.matrix(frames, mass=mass, fit=False)
    got = eng.rmsd_matrix(frames, mass=mass, fit=False)
    exact_symmetry(got)
    rr.check(got, ref, rg, rg, n, rr.EPS32, "no fit")
    want = np.linalg.norm(shifts[:, None, :] - shifts[None, :, :], axis=-1)
    assert np.allclose(got, want, atol=1e-5)                          # translations: |t_a - t_b| up to the f32 inputs' rounding
    fitted = eng.rmsd_matrix(frames, mass=mass)
    assert np.all(fitted < 1e-5)
    other = rr.random_frames(F, n, 19)
    refo, rgo, _ = rr.matrix(other, fit=False)
    rr.check(eng.rmsd_matrix(other, fit=False), refo, rgo, rgo, n, rr.EPS32, "no fit, unrelated")
    rr.check(m64.rmsd_matrix(other.astype(np.float64), fit=False), refo, rgo, rgo, n, rr.EPS64, "no fit, f64")
    r1, r2 = other[:5], other[5:]
    refr, rg1, rg2 = rr.matrix(r1, r2, fit=False)
    rr.check(eng.rmsd_matrix(r1, frames2=r2, fit=False), refr, rg1, rg2, n, rr.EPS32, "no fit, rectangular")


@pytest.fixture(scope="module")
def split_case():
    frames = rr.random_frames(3, 3000, 20)
    return frames, rr.matrix(frames)


def test_k_split_path(eng, m64, split_case):
    from molar_amd import api
    frames, (ref, rg, _) = split_case
    assert api.rmsd_matrix_plan(3, 0, 3000)[1] > 1
    got = eng.rmsd_matrix(frames)
    exact_symmetry(got)
    rr.check(got, ref, rg, rg, 3000, rr.EPS32, "K split")
    got64 = m64.rmsd_matrix(frames.astype(np.float64))
    exact_symmetry(got64)
    rr.check(got64, ref, rg, rg, 3000, rr.EPS64, "K split f64")
    f2 = rr.random_frames(2, 3000, 21)
    assert api.rmsd_matrix_plan(3, 2, 3000)[1] > 1
    refr, rg1, rg2 = rr.matrix(frames, f2)
    rr.check(eng.rmsd_matrix(frames, frames2=f2), refr, rg1, rg2, 3000, rr.EPS32, "K split, rectangular")


def test_fused_path_with_forty_frames(eng):
    from molar_amd import api
    n = 100
    assert api.rmsd_matrix_plan(40, 0, n)[1] == 1
    frames = rr.random_frames(40, n, 22)
    ref, rg, _ = rr.matrix(frames)
    got = eng.rmsd_matrix(frames)
    exact_symmetry(got)
    rr.check(got, ref, rg, rg, n, rr.EPS32, "fused")


def test_mid_size(eng):
    """F = 200, n = 3000: 13 tiles a side, K split.  All 40 000 entries are held to the bound against the pairwise SVD reference."""
    from molar_amd import api
    F, n = 200, 3000
    base = rr.random_frames(1, n, 23)[0]
    frames = (base[None] + np.random.default_rng(24).normal(size=(F, n, 3)).astype(np.float32) * np.linspace(0.01, 1.0, F, dtype=np.float32)[:, None, None])
    ks = api.rmsd_matrix_plan(F, 0, n)[1]
    got = eng.rmsd_matrix(frames)
    exact_symmetry(got)
    ref, rg, _ = rr.matrix(frames)
    rr.check(got, ref, rg, rg, n, rr.EPS32, f"mid size (ksplits {ks})")


def test_single_frame_that_is_not_contiguous(eng):
    """A [1, natoms, 3] CUDA view with non-unit inner strides must be copied, not read as if it were contiguous."""
    import torch
    n = 50
    block = rr.random_frames(9, n, 30)
    one = np.ascontiguousarray(rr.random_frames(1, n, 31)[0].T)                  # [3, n] in memory
    view = torch.from_numpy(one).cuda().t().unsqueeze(0)                        # [1, n, 3] with strides (., 1, n)
    assert view.shape == (1, n, 3) and view.stride(2) != 1
    want = eng.rmsd_matrix(block, frames2=one.T[None])
    got = eng.rmsd_matrix(torch.from_numpy(block).cuda(), frames2=view)
    eng.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    back = eng.rmsd_matrix(view, frames2=torch.from_numpy(block).cuda())
    eng.synchronize()
    assert np.array_equal(back.cpu().numpy(), eng.rmsd_matrix(one.T[None], frames2=block))


def test_device_memory_equals_host_memory(eng, m64, mass_case):
    import torch
    frames, mass, _ = mass_case
    idx = np.arange(0, frames.shape[1], 2).astype(np.uint64)
    host = eng.rmsd_matrix(frames, idx=idx, mass=mass)
    dev = eng.rmsd_matrix(torch.from_numpy(frames).cuda(), idx=torch.from_numpy(idx.astype(np.int64)).cuda(), mass=torch.from_numpy(mass).cuda())
    assert dev.is_cuda and dev.dtype == torch.float32
    eng.synchronize()                                                 # a device result is written on the engine's stream, not waited for
    assert np.array_equal(dev.cpu().numpy(), host)
    f2 = frames[:5]
    hostr = eng.rmsd_matrix(frames, frames2=f2, fit=False)
    out = torch.full((frames.shape[0], 8), -1.0, device="cuda")
    devr = eng.rmsd_matrix(torch.from_numpy(frames).cuda(), frames2=torch.from_numpy(f2).cuda(), fit=False, out=out)
    eng.synchronize()
    assert np.array_equal(devr.cpu().numpy()[:, :5], hostr) and bool((out[:, 5:] == -1.0).all())
    host64 = m64.rmsd_matrix(frames.astype(np.float64))
    dev64 = m64.rmsd_matrix(torch.from_numpy(frames.astype(np.float64)).cuda())
    eng.synchronize()
    assert np.array_equal(dev64.cpu().numpy(), host64)


def test_repeatability(eng, split_case, mass_case):
    frames, _ = split_case
    assert np.array_equal(eng.rmsd_matrix(frames), eng.rmsd_matrix(frames))
    frames, mass, _ = mass_case
    assert np.array_equal(eng.rmsd_matrix(frames, mass=mass), eng.rmsd_matrix(frames, mass=mass))


@pytest.mark.parametrize("fit", [True, False])
def test_non_finite_input(eng, fit):
    n, F, bad = 90, 20, 17
    frames = rr.random_frames(F, n, 25)
    clean = eng.rmsd_matrix(frames, fit=fit)
    dirty = frames.copy()
    dirty[bad, 40, 1] = np.nan
    got = eng.rmsd_matrix(dirty, fit=fit)                               # status 0: no exception
    assert np.all(np.isnan(got[bad, :])) and np.all(np.isnan(got[:, bad]))
    keep = np.arange(F) != bad
    assert np.array_equal(got[np.ix_(keep, keep)], clean[np.ix_(keep, keep)])
    ref, rg, _ = rr.matrix(frames[keep], fit=fit)
    rr.check(got[np.ix_(keep, keep)], ref, rg, rg, n, rr.EPS32, "beside a NaN frame")
    # the frame that supplies the origin of the mode without a fit
    dirty = frames.copy()
    dirty[0, 3, 0] = np.inf
    got = eng.rmsd_matrix(dirty, fit=fit)
    assert np.all(np.isnan(got[0, :])) and np.all(np.isnan(got[:, 0]))
    ref, rg, _ = rr.matrix(frames[1:], fit=fit)
    rr.check(got[1:, 1:], ref, rg, rg, n, rr.EPS32, "beside a non-finite frame 0")


def test_argument_errors(eng):
    from molar_amd._lib import MolarHipError
    frames = rr.random_frames(4, 10, 26)
    with pytest.raises(MolarHipError) as e:
        eng.rmsd_matrix(frames, idx=np.zeros(0, np.uint64))
    assert e.value.code == 1                                          # MOLAR_HIP_ERR_SIZES: n == 0
    with pytest.raises(MolarHipError) as e:
        eng.rmsd_matrix(frames, out=np.zeros((4, 3), np.float32))
    assert e.value.code == 1                                          # ld below the column count
    with pytest.raises(MolarHipError) as e:
        eng.rmsd_matrix(frames, frames2=rr.random_frames(6, 10, 27), out=np.zeros((4, 5), np.float32))
    assert e.value.code == 1
    with pytest.raises(MolarHipError) as e:
        eng.rmsd_matrix(frames, idx=np.array([1, 10], np.uint64))
    assert e.value.code == 50                                         # an index that is not below natoms
    assert eng.rmsd_matrix(frames[:0]).shape == (0, 0)                # no frames: a successful no-op


def test_rows_equal_fit_rmsd_batch(eng):
    """With unit masses row a is what the product's own route gives: fit_rmsd_batch with frame a as the reference.  1e-5
    relative, the project's Measure tolerance, on top of the bound."""
    n, F = 400, 12
    frames = (rr.random_frames(1, n, 28) + rr.random_frames(F, n, 29, scale=0.2)).astype(np.float32)
    ref, rg, _ = rr.matrix(frames)
    got = eng.rmsd_matrix(frames)
    ones = np.ones(n, np.float32)
    lim = rr.bound(ref, rg, rg, n, rr.EPS32) / np.maximum(got + ref, 1e-300)      # the bound is on squares: |g - r| = |g^2 - r^2| / (g + r)
    for a in range(F):
        row = eng.fit_rmsd_batch(frames.copy(), ones, frames[a], apply=False)["rmsd"]
        others = np.arange(F) != a
        assert np.all(np.abs(got[a] - row)[others] <= 1e-5 * row[others] + lim[a][others]), a
        assert row[a] <= 1e-5 * np.sqrt(rg[a]) + 1e-6                 # its own route does not force the diagonal to zero
