"""The host-arithmetic f64 membrane entries (MolAR's `f64` feature; no GPU needed): compute_initial_normals
(molar_membrane/src/lib.rs:456-505) and smooth_curvature (:584-621) against numpy float64 restatements of the reference
loops, their argument checks, and the parts of an f64 Membrane that need no device."""
import ctypes as C

import numpy as np
import pytest

from molar_amd import api
from molar_amd import _lib
from molar_amd._lib import MolarHipError

ERR_INVALID_ARGUMENT = 50


def random_patches(rng, K, mean_len=6):
    lists = []
    for i in range(K):
        n = int(rng.integers(0, 2 * mean_len))
        lists.append([int(x) for x in rng.choice(K, size=min(n, K), replace=False) if x != i])
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    ids = np.array([x for l in lists for x in l], np.uint64)
    return lists, off, ids


def normals_loop64(head, tail, lists, valid):
    """lib.rs:456-505 in float64; pass 2 reads the normals it has already written (lipid order)"""
    K = len(head)

    def norm(v):
        return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])

    def within(a, b):
        n1, n2 = norm(a), norm(b)
        if n1 == 0 or n2 == 0:
            return True
        c = ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) / (n1 * n2)
        return np.arccos(min(max(c, -1.0), 1.0)) <= np.pi / 2

    thv = np.zeros((K, 3))
    for i in range(K):
        if valid[i]:
            d = head[i] - tail[i]
            thv[i] = d / norm(d)
    nv = np.zeros((K, 3))
    for p in range(2):
        src = thv if p == 0 else nv
        for i in range(K):
            if not valid[i]:
                continue
            s = np.zeros(3)
            for l in lists[i]:
                if within(src[l], src[i]):
                    s = s + src[l]
            s = s + src[i]
            nv[i] = s / norm(s)
    return nv


def shell(i, n, slot_off, nvert, neib):
    """n-th Voronoi neighbour shell of lipid i (lib.rs:562-583), ascending"""
    def direct(l):
        s0 = int(slot_off[l]) + 4 * l
        return set(int(x) for x in neib[s0:s0 + int(nvert[l])])
    members = direct(i)
    for _ in range(2, n):
        for l in list(members):
            members |= direct(l)
    return sorted(members)


def curvature_loop64(valid, slot_off, nvert, neib, n, mean, gauss):
    m_out, g_out = mean.copy(), gauss.copy()
    for i in range(len(valid)):
        if not valid[i]:
            continue
        sm, sg, cnt = 0.0, 0.0, 0
        for l in shell(i, n, slot_off, nvert, neib):
            if valid[l]:
                sm += mean[l]; sg += gauss[l]; cnt += 1
        m_out[i] = (mean[i] + sm) / (cnt + 1)
        g_out[i] = (gauss[i] + sg) / (cnt + 1)
    return m_out, g_out


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_initial_normals_f64_matches_the_loop(seed):
    rng = np.random.default_rng(seed)
    K = 120
    head = rng.normal(size=(K, 3)) + np.array([0, 0, 2.0])
    tail = rng.normal(size=(K, 3)) * 0.3
    lists, off, ids = random_patches(rng, K)
    valid = (rng.random(K) > 0.1).astype(np.uint8)
    got = api.membrane_initial_normals(head, tail, off, ids, valid=valid)
    assert got.dtype == np.float64
    want = normals_loop64(head, tail, lists, valid)
    ok = valid.astype(bool)
    assert np.allclose(got[ok], want[ok], rtol=1e-14, atol=1e-14)
    assert np.all(got[~ok] == 0.0)                     # invalid lipids: the normals passed in (zeros)
    # float32 input still takes the f32 entry
    assert api.membrane_initial_normals(head.astype(np.float32), tail.astype(np.float32), off, ids, valid=valid).dtype == np.float32


@pytest.mark.parametrize("n_shells", [1, 2, 3])
def test_smooth_curvature_f64_matches_the_loop(n_shells):
    rng = np.random.default_rng(10 + n_shells)
    K = 150
    plen = rng.integers(3, 9, size=K)
    off = np.concatenate([[0], np.cumsum(plen)]).astype(np.uint64)
    slot_off = off
    nvert = np.zeros(K, np.uint32)
    neib = np.zeros(int(off[-1]) + 4 * K, np.uint64)
    for i in range(K):
        nv = int(rng.integers(0, plen[i] + 4 + 1))
        nvert[i] = nv
        s0 = int(off[i]) + 4 * i
        neib[s0:s0 + nv] = rng.choice(K, size=nv, replace=False)
    valid = (rng.random(K) > 0.15).astype(np.uint8)
    mean = rng.normal(size=K) * 1e-3
    gauss = rng.normal(size=K) * 1e-6
    m, g = api.membrane_smooth_curvature(valid, off, nvert, neib, n_shells, mean, gauss)
    assert m.dtype == np.float64 and g.dtype == np.float64
    wm, wg = curvature_loop64(valid, slot_off, nvert, neib, n_shells, mean, gauss)
    assert np.allclose(m, wm, rtol=1e-14, atol=0) and np.allclose(g, wg, rtol=1e-14, atol=0)
    assert np.array_equal(m[valid == 0], mean[valid == 0])
    m0, g0 = api.membrane_smooth_curvature(valid, off, nvert, neib, 0, mean, gauss)
    assert np.array_equal(m0, mean) and np.array_equal(g0, gauss)


def test_f64_host_entries_reject_bad_arguments():
    lib = _lib.load()
    K = 3
    head = np.zeros((K, 3)); tail = np.ones((K, 3)); out = np.zeros((K, 3))
    off = np.array([0, 1, 2, 3], np.uint64); ids = np.array([1, 2, 0], np.uint64)
    P = lambda a: a.ctypes.data
    assert lib.molar_hip_membrane_initial_normals_f64(K, None, P(tail), P(off), P(ids), None, P(out)) == ERR_INVALID_ARGUMENT
    assert "null" in _lib.last_error()
    bad = np.array([1, 2, 7], np.uint64)
    assert lib.molar_hip_membrane_initial_normals_f64(K, P(head), P(tail), P(off), P(bad), None, P(out)) == ERR_INVALID_ARGUMENT
    assert "out of range" in _lib.last_error()
    with pytest.raises(MolarHipError):
        api.membrane_initial_normals(head, tail, off, bad)
    valid = np.ones(K, np.uint8); nvert = np.array([9, 0, 0], np.uint32); neib = np.zeros(int(off[-1]) + 4 * K, np.uint64)
    m = np.zeros(K); g = np.zeros(K)
    assert lib.molar_hip_membrane_smooth_curvature_f64(K, P(valid), P(off), P(nvert), P(neib), 1, P(m), P(g)) == ERR_INVALID_ARGUMENT
    assert "slots" in _lib.last_error()
    nvert[0] = 1
    assert lib.molar_hip_membrane_smooth_curvature_f64(K, P(valid), P(off), P(nvert), P(neib), 1, None, P(g)) == ERR_INVALID_ARGUMENT
    assert "null" in _lib.last_error()
    assert lib.molar_hip_membrane_smooth_curvature_f64(K, None, P(off), P(nvert), P(neib), 1, P(m), P(g)) == ERR_INVALID_ARGUMENT
    # the device entries check the context before anything else
    st = api.new_membrane_state(head, out, None, 3, dtype=np.float64)
    S = api._MembraneState(*[st[k].ctypes.data for k in api._MEMBRANE_FIELDS])
    Pp = api._MembranePatches(K, P(off), P(ids))
    box9 = np.eye(3).reshape(9) * 5.0
    assert lib.molar_hip_membrane_smooth_f64(None, C.byref(Pp), P(box9), C.byref(S)) == ERR_INVALID_ARGUMENT
    assert lib.molar_hip_center_batch_f64(None, P(head), K, P(ids), P(off), K, None, P(out)) == ERR_INVALID_ARGUMENT
    assert lib.molar_hip_unwrap_simple_batch_f64(None, P(head), K, P(ids), P(off), K, P(box9), 7) == ERR_INVALID_ARGUMENT


def test_new_membrane_state_dtypes():
    head = np.zeros((4, 3)); nrm = np.tile([0.0, 0.0, 1.0], (4, 1))
    s64 = api.new_membrane_state(head, nrm, None, 10, dtype=np.float64)
    s32 = api.new_membrane_state(head, nrm, None, 10)
    for k in ("head_markers", "normals", "quad_coefs", "mean_curv", "gauss_curv", "princ_curvs", "princ_dirs", "area",
              "voro_vertexes", "fitted_patch_points"):
        assert s64[k].dtype == np.float64 and s32[k].dtype == np.float32, k
        assert s64[k].shape == s32[k].shape
    assert s64["neib_ids"].dtype == np.uint64 and s64["nvert"].dtype == np.uint32
    with pytest.raises(TypeError):
        api.new_membrane_state(head, nrm, None, 10, dtype=np.int32)


def test_f64_membrane_without_a_device():
    from molar_amd import membrane as mb
    from molar_amd.membrane_stats import LipidGroup
    tpl = mb.pope_like_template()
    K = 4
    first = np.arange(K) * tpl.natoms
    natoms = K * tpl.natoms
    masses = np.ones(natoms)
    m = mb.Membrane(None, natoms, first, tpl, masses, mb.MembraneOptions(), precision="f64")
    assert m.fusable() is False and m.masses.dtype == np.float64
    with pytest.raises(TypeError):
        m.compute(np.zeros((natoms, 3), np.float32), np.eye(3))
    with pytest.raises(ValueError):
        m.compute_begin(np.zeros((natoms, 3)), np.eye(3))
    m32 = mb.Membrane(None, natoms, first, tpl, masses, mb.MembraneOptions())
    assert m32.fusable() is True and m32.masses.dtype == np.float32
    with pytest.raises(TypeError):
        m32.compute(np.zeros((natoms, 3), np.float64), np.eye(3))
    with pytest.raises(ValueError):
        mb.Membrane(None, natoms, first, tpl, masses, precision="f16")
    # groups accumulate in the membrane's precision
    m.add_ids_to_group("all", np.arange(K))
    g = m.groups["all"]
    assert isinstance(g, LipidGroup)
    st = g.per_species["LIP"]
    assert st.area.F is np.float64 and st.order[0].x.dtype == np.float64
    res = dict(valid=np.ones(K, np.uint8), patch_off=np.arange(K + 1, dtype=np.uint64), area=np.full(K, 0.6 + 1e-12),
               normals=np.tile([0.0, 0.0, 1.0], (K, 1)), mean_curv=np.full(K, 1e-12), gauss_curv=np.full(K, 1e-15),
               order=[np.full((K, l - 2), 0.25) for l in m.tail_lens], nvert=np.ones(K, np.uint32),
               neib_ids=np.zeros(K + 4 * K, np.uint64))
    g.frame_update(res, m.species_of_lipid, np.tile([0.0, 0.0, 1.0], (K, 1)))
    mean, _ = st.area.compute()
    assert mean == np.float64(0.6 + 1e-12)                 # not rounded to float32
    assert st.mean_curv.compute()[0] == np.float64(1e-12)
