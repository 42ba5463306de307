"""Membrane analysis for MolAR's `f64` feature on the GPU: the f64 smoothing pass (MeasureF64.membrane_smooth), the f64 batch
helpers and Membrane(precision="f64").compute against the same pipeline assembled from the f64 oracle's primitives
(molar_membrane/src/lib.rs:410-454 with Float = f64)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (state key, oracle key) of the float arrays a smoothing pass writes per lipid
FLOATS = (("quad_coefs", "coefs"), ("mean_curv", "mean_curv"), ("gauss_curv", "gauss_curv"), ("princ_curvs", "princ_curvs"),
          ("princ_dirs", "princ_dirs"), ("area", "area"), ("normals", "normals"), ("head_markers", "head"))
PER_LIPID = ("head_markers", "normals", "quad_coefs", "mean_curv", "gauss_curv", "princ_curvs", "princ_dirs", "area", "nvert")


@pytest.fixture(scope="module")
def eng():
    from molar_amd import build
    from molar_amd.api import Engine
    build.build_library()
    return Engine(0)


@pytest.fixture(scope="module")
def m64(eng):
    from molar_amd.api import MeasureF64
    return MeasureF64(eng)


def patches_from(o, ob, head, cutoff):
    r = o.search_single_pbc(cutoff, head, ob, 7)
    K = len(head)
    i = r["i"].astype(np.int64); j = r["j"].astype(np.int64)
    src = np.stack([i, j], 1).reshape(-1); dst = np.stack([j, i], 1).reshape(-1)
    order = np.argsort(src, kind="stable")
    return (np.concatenate([[0], np.cumsum(np.bincount(src, minlength=K))]).astype(np.uint64), dst[order].astype(np.uint64))


def sheet(tric):
    """the jittered undulating sheet of test_gpu_membrane.py::test_smooth_sheet_parity_and_geometry (float32 values)"""
    rng = np.random.default_rng(5)
    side = 40
    L = side * 0.8
    g = (np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2) + 0.5
         + 0.2 * rng.normal(size=(side * side, 2))) * L / side
    z = 5.0 + 0.3 * np.sin(2 * np.pi * g[:, 0] / L) * np.cos(2 * np.pi * g[:, 1] / L) + 0.02 * rng.normal(size=len(g))
    head = np.concatenate([g, z[:, None]], 1).astype(np.float32)
    box = np.diag([L, L, 12.0]).astype(np.float32)
    if tric:
        box[0, 1] = 0.3 * L
        head[:, 0] += 0.3 * head[:, 1]
    K = len(head)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (K, 1))
    nrm += 0.05 * rng.normal(size=nrm.shape).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return head, nrm, box


def sphere_cap():
    """the sphere cap of test_smooth_sphere_curvature_and_invalidation"""
    rng = np.random.default_rng(11)
    R, n = 10.0, 800
    th = np.arccos(1 - rng.random(n) * (1 - np.cos(0.6))); ph = rng.random(n) * 2 * np.pi
    c = np.array([25.0, 25.0, 10.0])
    pts = np.stack([R * np.sin(th) * np.cos(ph), R * np.sin(th) * np.sin(ph), R * np.cos(th)], 1) + c
    return pts, (pts - c) / R, np.diag([50.0, 50.0, 50.0])


def worst(got, want):
    """largest |got - want| relative to max(|want|, 1e-12 x the array's largest magnitude)"""
    got = np.asarray(got, np.float64); want = np.asarray(want, np.float64)
    if want.size == 0:
        return 0.0
    scale = max(float(np.abs(want).max()), 1e-300)
    return float((np.abs(got - want) / np.maximum(np.abs(want), 1e-12 * scale)).max())


def check_state(got, want, poff, K, entry=None, tol=1e-12, label=""):
    """f64 GPU state against the f64 oracle's: validity, vertex counts and Voronoi neighbour ids exactly, every float array
    to `tol` relative with an absolute floor of tol x the array's largest magnitude; lipids invalid on entry untouched."""
    assert np.array_equal(got["valid"], want["valid"])
    ok = want["valid"].astype(bool)
    assert np.array_equal(got["nvert"][ok], want["nvert"][ok])
    vg, vw, fg, fw = [], [], [], []
    for k in np.flatnonzero(ok):
        s0 = int(poff[k]) + 4 * k
        nv = int(want["nvert"][k])
        assert np.array_equal(got["neib_ids"][s0:s0 + nv], want["neib_ids"][s0:s0 + nv])
        vg.append(got["voro_vertexes"][s0:s0 + nv]); vw.append(want["voro"][s0:s0 + nv])
        a, b = int(poff[k]), int(poff[k + 1])
        fg.append(got["fitted_patch_points"][a:b]); fw.append(want["fitted"][a:b])
    pairs = [(g, got[g][ok], want[w][ok]) for g, w in FLOATS]
    pairs += [("voro_vertexes", np.concatenate(vg), np.concatenate(vw)), ("fitted_patch_points", np.concatenate(fg), np.concatenate(fw))]
    devs = {}
    for name, g, w in pairs:
        assert g.dtype == np.float64, name
        devs[name] = worst(g, w)
        scale = float(np.abs(w).max()) if w.size else 0.0
        assert np.allclose(g, w, rtol=tol, atol=tol * scale), (name, devs[name])
    print(label, "worst relative deviation:", {k: f"{v:.2e}" for k, v in devs.items()})
    if entry is not None:                                  # lipids invalid on entry keep their values, byte for byte
        off = entry["valid"] == 0
        for k in PER_LIPID:
            assert got[k][off].tobytes() == entry[k][off].tobytes(), k
    return devs


def run_pass(m64, orc64, head, nrm, box, poff, pids, valid=None, label=""):
    from molar_amd import api
    K = len(head)
    st = api.new_membrane_state(head, nrm, valid, len(pids), dtype=np.float64)
    entry = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in st.items()}
    m64.membrane_smooth(box, st, poff, pids)
    vin = np.ones(K, np.uint8) if valid is None else valid
    want = orc64.membrane_smooth(orc64.box_from_matrix(box), np.asarray(head, np.float64), np.asarray(nrm, np.float64), vin, poff, pids)
    devs = check_state(st, want, poff, K, entry=entry, label=label)
    return st, want, devs


@pytest.mark.parametrize("tric", [False, True])
def test_smooth_f64_sheet(m64, orc64, tric):
    head, nrm, box = sheet(tric)
    ob = orc64.box_from_matrix(box.astype(np.float64))
    poff, pids = patches_from(orc64, ob, head.astype(np.float64), 2.0)
    st, _, _ = run_pass(m64, orc64, head.astype(np.float64), nrm.astype(np.float64), box.astype(np.float64), poff, pids,
                        label=f"sheet tric={tric}")
    assert st["valid"].all() and 5.5 < st["nvert"].mean() < 6.5


def test_smooth_f64_sphere_cap_with_invalid_lipids(m64, orc64):
    pts, nrm, box = sphere_cap()
    n = len(pts)
    poff, pids = patches_from(orc64, orc64.box_from_matrix(box), pts, 2.5)
    valid = np.ones(n, np.uint8); valid[::17] = 0
    st, _, _ = run_pass(m64, orc64, pts, nrm, box, poff, pids, valid=valid, label="sphere cap")
    ok = st["valid"].astype(bool)
    assert 0.5 * n < ok.sum() < n - n // 17
    assert abs(st["mean_curv"][ok].mean() - 0.1) < 0.015
    assert np.all(st["princ_curvs"][ok, 0] >= st["princ_curvs"][ok, 1])


def test_smooth_f64_long_patches_take_the_hbm_slices(m64, orc64):
    """patches of more than 60 members: local points and cell vertices live in the lanes' HBM slices"""
    head, nrm, box = sheet(False)
    h = head.astype(np.float64); b = box.astype(np.float64)
    poff, pids = patches_from(orc64, orc64.box_from_matrix(b), h, 3.8)
    lens = np.diff(poff.astype(np.int64))
    assert (lens > 60).sum() > len(h) // 2
    run_pass(m64, orc64, h, nrm.astype(np.float64), b, poff, pids, label="long patches")


def test_f64_curvature_beats_f32_by_four_orders(eng, m64, orc64):
    """the point of the feature: on the sheet, the f64 pass's worst deviation from the f64 oracle in the curvatures is at
    least 1e4 times smaller than the f32 pass's on the same inputs"""
    from molar_amd import api
    head, nrm, box = sheet(False)
    ob64 = orc64.box_from_matrix(box.astype(np.float64))
    poff, pids = patches_from(orc64, ob64, head.astype(np.float64), 2.0)
    want = orc64.membrane_smooth(ob64, head.astype(np.float64), nrm.astype(np.float64), np.ones(len(head), np.uint8), poff, pids)
    s32 = api.new_membrane_state(head, nrm, None, len(pids))
    eng.membrane_smooth(box, s32, poff, pids)
    s64 = api.new_membrane_state(head.astype(np.float64), nrm.astype(np.float64), None, len(pids), dtype=np.float64)
    m64.membrane_smooth(box.astype(np.float64), s64, poff, pids)
    ok = want["valid"].astype(bool) & s32["valid"].astype(bool) & s64["valid"].astype(bool)
    assert ok.sum() == len(head)
    for k in ("mean_curv", "gauss_curv"):
        d32 = np.abs(s32[k][ok].astype(np.float64) - want[k][ok]).max()
        d64 = np.abs(s64[k][ok] - want[k][ok]).max()
        print(f"{k}: worst |f32 - oracle| {d32:.3e}, worst |f64 - oracle| {d64:.3e}")
        assert d32 > 0 and d64 <= 1e-4 * d32, (k, d32, d64)


def test_batch_helpers_f64(m64, orc64):
    from molar_amd import membrane as mb
    xyz, box, first, tpl, masses = mb.build_bilayer(200, 40000)
    x = xyz.astype(np.float64); b = box.astype(np.float64); ms = masses.astype(np.float64)
    m = mb.Membrane(None, len(x), first, tpl, ms, precision="f64")
    K, na = len(first), tpl.natoms
    ob = orc64.box_from_matrix(b)
    work = x.copy()
    m64.unwrap_simple_batch(work, m.lipid_idx, m.lipid_off, b)
    ref = x.copy()
    for k in range(K):
        f0 = int(first[k])
        ref[f0:f0 + na] = orc64.unwrap_simple_dim(ref[f0:f0 + na], ob, 7)
    assert np.array_equal(work, ref)
    assert not np.array_equal(work, x)                    # some lipids were split over the boundary
    got = m64.center_batch(work, m.marker_idx, m.marker_off, ms).reshape(K, 3, 3)
    cog = m64.center_batch(work, m.marker_idx, m.marker_off).reshape(K, 3, 3)
    for s, sub in enumerate((tpl.head, tpl.mid, tpl.tail_end)):
        for k in range(K):
            f0 = int(first[k])
            want = orc64.center_of_mass(work[f0:f0 + na], ms[f0:f0 + na], sub.astype(np.uint64))
            assert np.allclose(got[k, s], want, rtol=1e-14, atol=0)
            assert np.allclose(cog[k, s], orc64.center_of_geometry(work[f0:f0 + na], sub.astype(np.uint64)), rtol=1e-14, atol=0)


def normals_f64(head, tail, patch):
    """lib.rs:456-505 in float64, sequential second pass"""
    K = len(head)
    nrm = lambda v: np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    thv = np.array([(head[i] - tail[i]) / nrm(head[i] - tail[i]) for i in range(K)])

    def ok(a, b):
        n1, n2 = nrm(a), nrm(b)
        if n1 == 0 or n2 == 0:
            return True
        return np.arccos(np.clip(((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) / (n1 * n2), -1.0, 1.0)) <= np.pi / 2
    nv = np.zeros((K, 3))
    for p in range(2):
        src = thv if p == 0 else nv
        for i in range(K):
            s = np.zeros(3)
            for l in patch[i]:
                if ok(src[l], src[i]):
                    s = s + src[l]
            s = s + src[i]
            nv[i] = s / nrm(s)
    return nv


def oracle_pass(orc64, ob, st, poff, pids):
    """one orc64.membrane_smooth pass with the engine's IN/OUT state semantics (a lipid that is or becomes invalid keeps its
    values; the slotted arrays start from zero when the patch structure changes)"""
    K = len(st["valid"])
    w = orc64.membrane_smooth(ob, st["head_markers"], st["normals"], st["valid"], poff, pids)
    E = int(poff[-1]); S = E + 4 * K
    out = {k: v.copy() for k, v in st.items()}
    if out["neib_ids"].shape[0] != max(S, 1):
        out["neib_ids"] = np.zeros(max(S, 1), np.uint64); out["voro_vertexes"] = np.zeros((max(S, 1), 3))
        out["fitted_patch_points"] = np.zeros((max(E, 1), 3)); out["nvert"][:] = 0
    ok = w["valid"].astype(bool)
    for g, k in FLOATS + (("nvert", "nvert"),):
        out[g][ok] = w[k][ok]
    out["valid"] = w["valid"].copy()
    for i in np.flatnonzero(ok):
        s0 = int(poff[i]) + 4 * i
        nv = int(w["nvert"][i])
        out["neib_ids"][s0:s0 + nv] = w["neib_ids"][s0:s0 + nv]
        out["voro_vertexes"][s0:s0 + nv] = w["voro"][s0:s0 + nv]
        a, b = int(poff[i]), int(poff[i + 1])
        out["fitted_patch_points"][a:b] = w["fitted"][a:b]
    return out, w


def run_f64_pipeline_check(eng, orc64, per_leaflet, natoms, iters=1, nsp=0, nss=0):
    """Membrane(precision="f64").compute against the pipeline assembled from orc64 primitives (run_pipeline_check of
    test_gpu_membrane.py, in f64)."""
    from molar_amd import api
    from molar_amd import membrane as mb
    xyz, box, first, tpl, masses = mb.build_bilayer(per_leaflet, natoms)
    x = xyz.astype(np.float64); b = box.astype(np.float64); ms = masses.astype(np.float64)
    K, na = len(first), tpl.natoms
    m = mb.Membrane(eng, len(x), first, tpl, ms, mb.MembraneOptions(cutoff=1.5, order_type=1, max_smooth_iter=iters,
                                                                    n_shells_patch=nsp, n_shells_smoothing=nss), precision="f64")
    assert not m.fusable()
    work = x.copy()
    res = m.compute(work, b)
    ob = orc64.box_from_matrix(b)
    ref = x.copy()
    for k in range(K):
        f0 = int(first[k])
        ref[f0:f0 + na] = orc64.unwrap_simple_dim(ref[f0:f0 + na], ob, 7)
    assert np.array_equal(work, ref)
    for name, sub in (("head", tpl.head), ("mid", tpl.mid), ("tail", tpl.tail_end)):
        assert res[name].dtype == np.float64
        want = np.array([orc64.center_of_mass(ref[int(first[k]):int(first[k]) + na], ms[int(first[k]):int(first[k]) + na],
                                              sub.astype(np.uint64)) for k in range(K)])
        assert np.allclose(res[name], want, rtol=1e-14, atol=1e-14)
    r = orc64.search_single_pbc(1.5, res["head"], ob, 7)
    patch = [[] for _ in range(K)]
    for i, j in zip(r["i"].tolist(), r["j"].tolist()):
        patch[i].append(j); patch[j].append(i)
    poff = np.concatenate([[0], np.cumsum([len(p) for p in patch])]).astype(np.uint64)
    pids = np.array([x for p in patch for x in p], np.uint64)
    if nsp == 0:
        assert np.array_equal(res["patch_off"], poff) and np.array_equal(res["patch_ids"], pids)
    assert np.allclose(res["initial_normals"], normals_f64(res["head"], res["tail"], patch), rtol=0, atol=1e-14)
    # the smoothing passes, driven pass by pass through the oracle
    st = api.new_membrane_state(res["head"], res["initial_normals"], None, len(pids), dtype=np.float64)
    it = 0
    while True:
        if nsp > 0 and it == 0:
            st, _ = oracle_pass(orc64, ob, st, poff, pids)
            poff, pids = api.membrane_nth_shell_patches(st["valid"], poff, pids, st["nvert"], st["neib_ids"], nsp)
        st, w = oracle_pass(orc64, ob, st, poff, pids)
        it += 1
        if it >= iters:
            break
    if nss > 0:
        st["mean_curv"], st["gauss_curv"] = api.membrane_smooth_curvature(st["valid"], poff, st["nvert"], st["neib_ids"], nss,
                                                                          st["mean_curv"], st["gauss_curv"])
        w = dict(w, mean_curv=st["mean_curv"], gauss_curv=st["gauss_curv"])
    assert np.array_equal(res["patch_off"], poff) and np.array_equal(res["patch_ids"], pids)
    tol = 1e-12 if iters == 1 and nsp == 0 else 1e-10
    got = dict(res, head_markers=res["smoothed_head"])
    check_state(got, dict(w, head=st["head_markers"], normals=st["normals"]), poff, K, tol=tol,
                label=f"frame iters={iters} shells=({nsp},{nss})")
    for t, carbons in enumerate(tpl.tails):
        for k in range(0, K, 7):
            if not res["valid"][k]:
                continue
            f0 = int(first[k])
            want = orc64.lipid_tail_order(ref[f0:f0 + na], 1, res["normals"][k][None, :], tpl.bond_orders[t], idx=carbons.astype(np.uint64))
            assert np.allclose(res["order"][t][k], want, rtol=1e-12, atol=1e-12)
    return K, int(np.count_nonzero(res["valid"]))


@pytest.mark.parametrize("iters,nsp,nss", [(1, 0, 0), (3, 0, 0), (2, 2, 1)])
def test_membrane_f64_frame_matches_oracle(eng, orc64, iters, nsp, nss):
    K, nvalid = run_f64_pipeline_check(eng, orc64, 200, 40000, iters, nsp, nss)
    assert nvalid > (0.9 if nsp == 0 else 0.5) * K       # second-shell patches at 1.5 nm leave more rim cells open


@pytest.mark.timeout(1500)
def test_membrane_f64_frame_at_baseline_size(eng, orc64):
    K, nvalid = run_f64_pipeline_check(eng, orc64, 2000, 500_000)
    assert K == 4000 and nvalid > 3900


def test_membrane_f64_torch_frame_same_bits(eng):
    import torch
    from molar_amd import membrane as mb
    xyz, box, first, tpl, masses = mb.build_bilayer(200, 40000)
    x = xyz.astype(np.float64); b = box.astype(np.float64); ms = masses.astype(np.float64)
    opt = mb.MembraneOptions(cutoff=1.5, order_type=1)
    host = x.copy()
    r_np = mb.Membrane(eng, len(x), first, tpl, ms, opt, precision="f64").compute(host, b)
    dev = torch.from_numpy(x.copy()).to("cuda")
    r_t = mb.Membrane(eng, len(x), first, tpl, ms, opt, precision="f64").compute(dev, b)
    assert np.array_equal(dev.cpu().numpy(), host)
    for k, v in r_np.items():
        if k == "order":
            assert all(np.array_equal(a, c) for a, c in zip(v, r_t[k]))
        else:
            assert np.asarray(v).tobytes() == np.asarray(r_t[k]).tobytes(), k
    with pytest.raises(TypeError):
        mb.Membrane(eng, len(x), first, tpl, ms, opt, precision="f64").compute(dev.float(), b)
