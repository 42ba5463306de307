"""Every Measure reduction (measure.hip, measure_f64.hip) at the edges of its launch shape, f32 and f64: the grid cap and the
grid-stride trips of the single-call kernels, the finalisers' second trip, the batch shapes of fit_rmsd_batch (8 atoms per
thread, the 16-workgroup cap, whole and partial four-atom trips with mixed guards, the packed switch), the f64 batch cap, one
wave per CSR selection at 1, 2, 63, 64, 65 .. 1000 atoms, the lipid-order workgroups.  The inputs, the exact-sum references
and the bounds (a few ulps of the output type, derived in the module's docstring) are those of tests/measure_shape_cases.py;
tests/test_measure_shape_cases_cpu.py proves without a GPU that they reach the shapes and that every comparison sees one
atom.  Rotation-dependent outputs keep the project's tolerances against the f64 oracle, data movement is bit-exact.  The
last test prints what was exercised and the worst error / bound per entry (for information)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import measure_shape_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu

SEEN = {}       # kernel family -> set of launch-shape descriptions
WORST = {}      # entry -> worst error / bound


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


@pytest.fixture(scope="module")
def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def seen(family, **shape):
    SEEN.setdefault(family, set()).add(tuple(sorted(shape.items())))


def within(entry, got, ref_bound, what):
    """|got - ref| <= bound, elementwise; the worst ratio is kept for the summary"""
    ref, bound = ref_bound
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    ratio = float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)))) if err.size else 0.0
    WORST[entry] = max(WORST.get(entry, 0.0), ratio)
    assert (err <= bound).all(), f"{what} {entry}: engine {got}, reference {ref}, error {err}, bound {bound} (x{ratio:.3g})"


def dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).cuda()


def host(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else a


def tens6(t):
    return np.array([t[0, 0], t[1, 1], t[2, 2], t[0, 1], t[0, 2], t[1, 2]], np.float64)


def full3(t6):
    return np.array([[t6[0], t6[3], t6[4]], [t6[3], t6[1], t6[5]], [t6[4], t6[5], t6[2]]])


# ------------------------------------------------------------------------------------------------ single-call reductions

@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("with_idx", [True, False], ids=["gather", "all"])
@pytest.mark.parametrize("key", mc.SIZE_KEYS)           # largest first, then 1, then the rest: the partial buffers shrink and grow
def test_single_call_entries_at_every_shape(eng, m64, orc32, orc64, cus, prec, key, with_idx):
    n = mc.size_of(key, cus)
    s = mc.system(n, with_idx)
    ref = mc.single_reference(s, prec, cus)
    sh = mc.single_shape(cus, n)
    for fam in ("sums", "moments/central", "rmsd", "fit_sums/cov", "minmax", "apply", "translate"):
        seen(f"f{prec} {fam}", n=n, nb=sh["nb"], trips=sh["trips"], capped=sh["capped"], fin_trips=sh["fin_trips"])
    shp = mc.single_shape(cus, n, 1)
    for fam in ("sums_pbc", "unwrap"):
        seen(f"f{prec} {fam}", n=n, nb=shp["nb"], trips=shp["trips"], capped=shp["capped"], fin_trips=shp["fin_trips"])
    dt = np.float32 if prec == 32 else np.float64
    E, orc = (eng, orc32) if prec == 32 else (m64, orc64)
    what = f"n={n} {'gather' if with_idx else 'all'}"
    p = f"f{prec} "
    hx1, hx2, hxw = (mc.as_real(s[k], dt) for k in ("X1", "X2", "Xw"))
    hm = s["mass"].astype(dt)
    hi1, hi2 = mc.idx_arg(s), mc.idx_arg(s, "sel2")
    resident = n >= 4096 * cus                          # the three sizes that move tens of megabytes: one upload per case
    if resident:
        x1, x2, xw, m = dev(hx1), dev(hx2), dev(hxw), dev(hm)
        i1, i2 = (None, None) if hi1 is None else (dev(hi1, np.int64), dev(hi2, np.int64))
    else:
        x1, x2, xw, m, i1, i2 = hx1, hx2, hxw, hm, hi1, hi2

    def work(a):
        if not resident:
            return a.copy()
        import torch
        c = a.clone()
        torch.cuda.synchronize()            # the engine reads device tensors on its own stream: the copy has to be complete
        return c
    box = mc.BOX.astype(dt)
    ob = orc.box_from_matrix(box)

    within(p + "center_of_geometry", E.center_of_geometry(x1, i1), ref["cog"], what)
    within(p + "center_of_mass", E.center_of_mass(x1, m, i1), ref["com"], what)
    within(p + "gyration", E.gyration(x1, m, i1), ref["gyration"], what)
    within(p + "rmsd", E.rmsd(x1, x2, i1, i2), ref["rmsd"], what)
    within(p + "rmsd_mw", E.rmsd_mw(x1, m, x2, i1, i2), ref["rmsd_mw"], what)
    for dims in (7, 3):
        within(p + f"center_of_geometry_pbc dims {dims}", E.center_of_geometry_pbc(xw, box, dims, i1), ref[f"cog_pbc{dims}"], what)
        within(p + f"center_of_mass_pbc dims {dims}", E.center_of_mass_pbc(xw, m, box, dims, i1), ref[f"com_pbc{dims}"], what)
    gp = E.gyration(xw, m, i1, box) if prec == 32 else E.gyration_pbc(xw, m, box, i1)
    within(p + "gyration (box)", gp, ref["gyration_pbc"], what)
    lo, up = E.min_max(x1, i1)
    rlo, rup = orc.min_max(hx1, hi1)
    assert np.array_equal(lo, rlo) and np.array_equal(up, rup), what
    if n >= 3:
        atol_ax = (mc.AXES_RTOL32 if prec == 32 else mc.AXES_ATOL64)
        for bx, key_t, xx in ((None, "tensor", x1), (box, "tensor_pbc", xw)):
            mom, axes, tens = E.inertia(xx, m, i1, box=bx)
            within(p + "inertia tensor" + (" (box)" if bx is not None else ""), tens6(tens), ref[key_t], what)
            rt = full3(ref[key_t][0])
            eye_tol = 1e-5 if prec == 32 else 1e-13
            assert np.allclose(axes.T @ axes, np.eye(3), atol=eye_tol) and abs(np.linalg.det(axes) - 1.0) <= eye_tol, what
            assert np.allclose(axes.astype(np.float64) @ np.diag(mom.astype(np.float64)) @ axes.T.astype(np.float64), rt,
                               rtol=mc.AXES_RTOL32 if prec == 32 else 0, atol=atol_ax * np.abs(rt).max()), what
        scale = 64.0
        for at_origin in (False, True):
            R, t = E.fit_transform(x1, m, x2, m, i1, i2, at_origin=at_origin)
            Ro, to = (orc64.fit_transform_at_origin(hx1, hm, hx2, hi1, hi2) if at_origin
                      else orc64.fit_transform(hx1, hm, hx2, hm, hi1, hi2))
            if prec == 32:
                assert np.allclose(R, Ro, atol=mc.R_ATOL32), (what, at_origin, np.abs(R - Ro).max())
                assert np.allclose(t, to, rtol=mc.T_RTOL32, atol=mc.T_ATOL32), (what, at_origin, np.abs(t - to).max())
            else:
                assert np.allclose(R, Ro, rtol=0, atol=mc.RTOL_ROT64), (what, at_origin, np.abs(R - Ro).max())
                assert np.allclose(t, to, rtol=0, atol=mc.RTOL_ROT64 * scale * 10), (what, at_origin, np.abs(t - to).max())
            if at_origin:
                assert not np.asarray(t).any()
            else:
                Rt = (R, t)
    else:                                               # no unique fit below three atoms: a fixed transform for apply
        Rt = (np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], dt), np.array([1.0, -2.0, 3.0], dt))
    # data movement: bit for bit
    R, t = Rt
    w = work(x1)
    E.apply_transform(w, R, t, i1)
    assert np.array_equal(host(w), orc.apply_transform(hx1, R, t, hi1)), p + what + " apply_transform"
    w = work(x1)
    E.translate(w, [0.25, -1.5, 3.0], i1)
    assert np.array_equal(host(w), orc.translate(hx1, [0.25, -1.5, 3.0], hi1)), p + what + " translate"
    for dims in (7, 3):
        w = work(xw)
        E.unwrap_simple(w, box, dims, i1)
        assert np.array_equal(host(w), orc.unwrap_simple_dim(hxw, ob, dims, hi1)), p + what + f" unwrap_simple dims {dims}"


@pytest.mark.parametrize("prec", [32, 64])
def test_periodic_entries_in_a_triclinic_box(eng, m64, orc32, orc64, cus, prec):
    """One triclinic case per periodic entry at the project's tolerances against the f64 oracle (the exact-sum cases above
    are orthorhombic): 65 537 gathered atoms, two finaliser trips."""
    c = mc.triclinic_case(prec)
    E, orc = (eng, orc32) if prec == 32 else (m64, orc64)
    xyz, m, box, idx = c["xyz"], c["mass"], c["box"], c["idx"]
    b64 = orc64.box_from_matrix(box.astype(np.float64))
    ca, gr = ((1e-5, 1e-4) if prec == 32 else (1e-12, 1e-12))
    for dims in (7, 3):
        assert np.allclose(E.center_of_mass_pbc(xyz, m, box, dims, idx), orc64.center_of_mass_pbc_dims(xyz, m, b64, dims, idx),
                           rtol=1e-5 if prec == 32 else 0, atol=ca)
        assert np.allclose(E.center_of_geometry_pbc(xyz, box, dims, idx), orc64.center_of_geometry_pbc_dims(xyz, b64, dims, idx),
                           rtol=1e-5 if prec == 32 else 0, atol=ca)
    g = E.gyration(xyz, m, idx, box) if prec == 32 else E.gyration_pbc(xyz, m, box, idx)
    assert g == pytest.approx(orc64.gyration_pbc(xyz, m, b64, idx), rel=gr)
    mom, axes, tens = E.inertia(xyz, m, idx, box=box)
    rt = orc64.inertia_tensor(xyz, m, idx, box=b64)
    assert np.allclose(tens, rt, rtol=0, atol=(1e-5 if prec == 32 else 1e-11) * np.abs(rt).max())
    un = xyz.copy()
    E.unwrap_simple(un, box, 7, idx)
    assert np.array_equal(un, orc.unwrap_simple_dim(xyz, orc.box_from_matrix(box), 7, idx))


# ------------------------------------------------------------------------------------------------ fit_rmsd_batch

def _fit_inputs(fs, mode, dt):
    """frames, mass, reference, idx, ref_idx; mode "same": ref_idx == idx, "other": an index set of its own, "none": the
    selected atoms alone as whole frames (idx = ref_idx = None)"""
    sel, rsel = fs["sel"], fs["ref_sel"]
    if mode == "none":
        return (mc.as_real(fs["frames"][:, sel], dt), fs["mass"][sel].astype(dt), mc.as_real(fs["ref"][rsel], dt), None, None)
    ref = mc.as_real(fs["ref_same" if mode == "same" else "ref"], dt)
    return mc.as_real(fs["frames"], dt), fs["mass"].astype(dt), ref, sel.astype(np.uint64), (sel if mode == "same" else rsel).astype(np.uint64)


@pytest.mark.parametrize("mode", ["same", "other", "none"], ids=["ref_idx=idx", "ref_idx!=idx", "idx=None"])
@pytest.mark.parametrize("F,nkey", mc.FIT32_CASES)
def test_fit_rmsd_batch_shapes(eng, orc32, orc64, cus, F, nkey, mode):
    """Every frame against the per-frame reference (R, t, centre of mass and RMSD at the project's tolerances, the gyration
    radius at its exact-sum bound, the moved frame bit for bit), and the batch against per-frame engine calls bit for bit:
    the sums are exact, so they are the same numbers whatever the grouping of 4 or 8 atoms per thread."""
    n = mc.size_of(str(nkey), cus)
    fs = mc.fit_system(n, F)
    sh = mc.fit32_shape(cus, n, F)
    seen("f32 fit_rmsd_batch " + ("packed" if sh["packed"] else "unpacked"), F=F, n=n, nb=sh["nb"], per=sh["per"], capped=sh["capped"],
         whole_trips=sh["whole_trips"], mixed_guards=sh["mixed_guards"], fin_trips=sh["fin_trips"])
    frames, mass, ref, idx, ref_idx = _fit_inputs(fs, mode, np.float32)
    what = f"F={F} n={n} {mode}"
    resident = n >= 4096 * cus
    per_frame = []
    for f in range(F):
        R64, t64 = orc64.fit_transform(frames[f], mass, ref, mass, idx, ref_idx)
        per_frame.append((R64, t64, mc.fit_gyration_reference(fs, f, 32, None)))
    for apply in (False, True):
        if resident:
            work = dev(frames)
            di, dr = (None, None) if idx is None else (dev(idx, np.int64), dev(ref_idx, np.int64))
            out = eng.fit_rmsd_batch(work, dev(mass), dev(ref), idx=di, ref_idx=dr, apply=apply)
            work = host(work)
        else:
            work = frames.copy()
            out = eng.fit_rmsd_batch(work, mass, ref, idx=idx, ref_idx=ref_idx, apply=apply)
        for f in range(F):
            R64, t64, gyr = per_frame[f]
            assert np.allclose(out["R"][f], R64, atol=mc.R_ATOL32), (what, f, np.abs(out["R"][f] - R64).max())
            assert np.allclose(out["t"][f], t64, rtol=mc.T_RTOL32, atol=mc.T_ATOL32), (what, f)
            moved = orc32.apply_transform(frames[f], out["R"][f], out["t"][f], idx)
            assert np.array_equal(work[f], moved if apply else frames[f]), (what, f, apply)
            assert out["rmsd"][f] == pytest.approx(orc64.rmsd(moved, ref, idx, ref_idx), rel=mc.RMSD_FIT_RTOL32), (what, f)
            assert np.allclose(out["com"][f], orc64.center_of_mass(moved, mass, idx), rtol=mc.T_RTOL32, atol=mc.T_ATOL32), (what, f)
            within("fit_rmsd_batch gyration", out["gyration"][f], gyr, f"{what} frame {f}")
            w1 = frames[f:f + 1].copy()
            one = eng.fit_rmsd_batch(w1, mass, ref, idx=idx, ref_idx=ref_idx, apply=apply)
            for k in ("rmsd", "R", "t", "com", "gyration"):
                assert np.array_equal(out[k][f], one[k][0]), (what, apply, k, f)
            assert np.array_equal(work[f], w1[0]), (what, apply, f)


@pytest.mark.parametrize("F,n", mc.FIT64_CASES)
def test_fit_rmsd_batch_f64_shapes(m64, orc64, F, n):
    fs = mc.fit_system(n, F)
    sh = mc.fit64_shape(n)
    seen("f64 fit_rmsd_batch", F=F, n=n, nb=sh["nb"], trips=sh["trips"], capped=sh["capped"], fin_trips=sh["fin_trips"])
    for mode in ("same", "other", "none"):
        frames, mass, ref, idx, ref_idx = _fit_inputs(fs, mode, np.float64)
        what = f"f64 F={F} n={n} {mode}"
        for apply in (False, True):
            work = frames.copy()
            out = m64.fit_rmsd_batch(work, mass, ref, idx=idx, ref_idx=ref_idx, apply=apply)
            for f in range(F):
                within("fit_rmsd_batch_f64 gyration", out["gyration"][f], mc.fit_gyration_reference(fs, f, 64, sh), f"{what} frame {f}")
                R, t = out["R"][f], out["t"][f]
                assert np.allclose(R @ R.T, np.eye(3), atol=1e-13) and np.isfinite(out["rmsd"][f]), (what, f)
                moved = orc64.apply_transform(frames[f], R, t, idx)
                assert np.array_equal(work[f], moved if apply else frames[f]), (what, f, apply)
                assert np.allclose(out["com"][f], orc64.center_of_mass(moved, mass, idx), rtol=0, atol=mc.COM_FIT_ATOL64), (what, f)
                if n < 3:                   # the rotation is not unique: the fitted atom lies on its reference
                    assert out["rmsd"][f] <= 1e-12 and np.allclose(out["com"][f], ref[0 if ref_idx is None else int(ref_idx[0])], rtol=0, atol=1e-12), (what, f)
                    continue
                Ro, to = orc64.fit_transform(frames[f], mass, ref, mass, idx, ref_idx)
                assert np.allclose(R, Ro, rtol=0, atol=mc.RTOL_ROT64), (what, f, np.abs(R - Ro).max())
                assert np.allclose(t, to, rtol=0, atol=mc.RTOL_ROT64 * 64 * 10), (what, f)
                assert out["rmsd"][f] == pytest.approx(orc64.rmsd(moved, ref, idx, ref_idx), rel=mc.RMSD_FIT_RTOL64), (what, f)


# ------------------------------------------------------------------------------------------------ CSR batches

@pytest.mark.parametrize("nsel", mc.CSR_NSEL)
def test_csr_batches_one_wave_per_selection(eng, m64, orc32, orc64, nsel):
    """Selections of 1, 2, 3, 63, 64, 65, 127, 128, 129 and 1000 atoms in two orders, cut to nsel: every batched entry against
    the exact sums of each selection (centres, gyration, rmsd) or the per-selection oracle (fits, the periodic gyration,
    unwrap)."""
    cs = mc.csr_system()
    sizes = cs["sizes"][:nsel]
    shp = mc.csr_shape(sizes)
    seen("CSR batches", nsel=nsel, nb=shp["nb"], idle_waves=shp["idle_waves"], steps=tuple(sorted(set(shp["steps"]))))
    off = cs["off"][:nsel + 1].astype(np.uint64)
    last = int(off[-1])
    idx, idx2 = cs["idx"][:last].astype(np.uint64), cs["idx2"][:last].astype(np.uint64)
    sels = [idx[int(off[k]):int(off[k + 1])] for k in range(nsel)]
    x1, x2, x3, xw = (mc.as_real(cs[k], np.float32) for k in ("X1", "X2", "X3", "Xw"))
    mass = cs["mass"].astype(np.float32)
    box = mc.BOX.astype(np.float32)
    b64, b32 = orc64.box_from_matrix(mc.BOX), orc32.box_from_matrix(box)
    ref2 = [mc.csr_reference(cs, k, 32, "X2") for k in range(nsel)]
    ref3 = [mc.csr_reference(cs, k, 32, "X3") for k in range(nsel)]
    g = eng.gyration_batch(x1, idx, off, mass)
    gp = eng.gyration_batch(xw, idx, off, mass, box=box)
    r3, r3w = eng.rmsd_batch(x1, x3, idx, off), eng.rmsd_batch(x1, x3, idx, off, mass=mass)
    r2, r2w = eng.rmsd_batch(x1, x2, idx, off, idx2=idx2), eng.rmsd_batch(x1, x2, idx, off, mass=mass, idx2=idx2)
    cg, cm = eng.center_batch(x1, idx, off), eng.center_batch(x1, idx, off, mass=mass)
    for k in range(nsel):
        what = f"nsel={nsel} selection {k} of {int(sizes[k])}"
        within("gyration_batch", g[k], ref2[k]["gyration"], what)
        wp = orc64.gyration_pbc(xw, mass, b64, sels[k])
        assert abs(gp[k] - wp) <= mc.PBC_GYR_BATCH_RTOL32 * wp, (what, gp[k], wp)
        within("rmsd_batch", r3[k], ref3[k]["rmsd"], what)
        within("rmsd_batch (mass)", r3w[k], ref3[k]["rmsd_mw"], what)
        within("rmsd_batch (idx2)", r2[k], ref2[k]["rmsd"], what)
        within("rmsd_batch (mass, idx2)", r2w[k], ref2[k]["rmsd_mw"], what)
        within("center_batch", cg[k], ref2[k]["cog"], what)
        within("center_batch (mass)", cm[k], ref2[k]["com"], what)
    # fits: onto the same atoms of frame 3, and onto the second index set of frame 2
    for second, i2, x in (("X3", None, x3), ("X2", idx2, x2)):
        out = eng.fit_batch(x1, mass, x, idx, off, idx2=i2, mass2=None if i2 is None else mass, apply=False)
        if i2 is not None:              # one mass column: named twice or left out, it is read through idx2 for the second centre
            for k, v in eng.fit_batch(x1, mass, x, idx, off, idx2=i2, mass2=None, apply=False).items():
                assert np.array_equal(v, out[k]), k
        for k in range(nsel):
            what = f"nsel={nsel} fit onto {second}, selection {k} of {int(sizes[k])}"
            s2 = sels[k] if i2 is None else i2[int(off[k]):int(off[k + 1])]
            for v in out.values():
                assert np.isfinite(v[k]).all(), what
            within("fit_batch gyration", out["gyration"][k], (ref2 if second == "X2" else ref3)[k]["gyration"], what)
            assert np.allclose(out["com"][k], orc64.center_of_mass(x, mass, s2), atol=mc.CSR_T_ATOL32), what      # lands on cm2
            if sizes[k] < 3:
                continue
            R, t = orc64.fit_transform(x1, mass, x, mass, sels[k], s2)
            assert np.allclose(out["R"][k], R, atol=mc.CSR_R_ATOL32), (what, np.abs(out["R"][k] - R).max())
            assert np.allclose(out["t"][k], t, atol=mc.CSR_T_ATOL32), what
            w = orc64.rmsd(orc64.apply_transform(x1, R, t, sels[k]), x, sels[k], s2)
            assert abs(out["rmsd"][k] - w) <= mc.CSR_RMSD_RTOL32 * max(w, 1e-3), (what, out["rmsd"][k], w)
    # a second frame longer than the one mass column, read through its own index: refused, mass2 has to be given
    from molar_amd._lib import MolarHipError
    longer = np.concatenate([x2, x2[:7]])
    with pytest.raises(MolarHipError) as e:
        eng.fit_batch(x1, mass, longer, idx, off, idx2=idx2)
    assert e.value.code == 50
    # apply: the selections are disjoint; atoms outside them are untouched bit for bit
    z = x1.copy()
    out = eng.fit_batch(z, mass, x3, idx, off, apply=True)
    rest = np.ones(cs["natoms"], bool)
    rest[idx.astype(np.int64)] = False
    assert np.array_equal(z[rest], x1[rest])
    for k in range(nsel):
        sk = sels[k].astype(np.int64)
        if sizes[k] >= 3:
            R, t = orc64.fit_transform(x1, mass, x3, mass, sels[k], sels[k])
            assert np.abs(z[sk] - orc64.apply_transform(x1, R, t, sels[k])[sk]).max() < 2e-4, k
        elif sizes[k] == 1:
            assert np.abs(z[sk] - x3[sk]).max() < 2e-4, k
        assert np.array_equal(z[sk], orc32.apply_transform(x1, out["R"][k], out["t"][k], sels[k])[sk]), k
    # unwrap, per selection, in both precisions; the f64 centres
    want32, want64 = xw.copy(), xw.astype(np.float64)
    for k in range(nsel):
        want32 = orc32.unwrap_simple_dim(want32, b32, 7, sels[k])
        want64 = orc64.unwrap_simple_dim(want64, b64, 7, sels[k])
    un = xw.copy()
    eng.unwrap_simple_batch(un, idx, off, box, 7)
    assert np.array_equal(un, want32)
    un = xw.astype(np.float64)
    m64.unwrap_simple_batch(un, idx, off, mc.BOX, 7)
    assert np.array_equal(un, want64)
    d1, dm = mc.as_real(cs["X1"], np.float64), cs["mass"].astype(np.float64)
    cg, cm = m64.center_batch(d1, idx, off), m64.center_batch(d1, idx, off, mass=dm)
    for k in range(nsel):
        r = mc.csr_reference(cs, k, 64)
        within("center_batch_f64", cg[k], r["cog"], f"nsel={nsel} selection {k}")
        within("center_batch_f64 (mass)", cm[k], r["com"], f"nsel={nsel} selection {k}")


# ------------------------------------------------------------------------------------------------ lipid order

@pytest.mark.parametrize("order_type", [0, 1, 2])
@pytest.mark.parametrize("ntails", mc.LIPID_NTAILS[32])
def test_lipid_tail_order_workgroup_edges(eng, orc32, orc64, ntails, order_type):
    """16 tails per workgroup: 1, 15, 16, 17, 33 tails of 3, 4 and 18 carbons, at the tolerances of the existing tests"""
    seen("f32 lipid_order", ntails=ntails, **mc.lipid_shape(ntails, 16))
    xyz, tails, bonds, normals = mc.lipid_tails(ntails, np.float32)
    got = eng.lipid_tail_order(xyz, tails, order_type, normals, bonds)
    for t in range(ntails):
        want32 = orc32.lipid_tail_order(xyz, order_type, normals[t], bonds[t], idx=tails[t])
        want = orc64.lipid_tail_order(xyz, order_type, normals[t], bonds[t], idx=tails[t])
        assert got[t].shape == want.shape == (len(tails[t]) - 2,)
        assert np.allclose(got[t], want32, atol=2e-5), (t, got[t], want32)
        assert np.allclose(got[t], want, atol=2e-4), (t, got[t], want)


@pytest.mark.parametrize("order_type", [0, 1, 2])
@pytest.mark.parametrize("ntails", mc.LIPID_NTAILS[64])
def test_lipid_tail_order_f64_workgroup_edges(m64, orc64, ntails, order_type):
    seen("f64 lipid_order", ntails=ntails, **mc.lipid_shape(ntails, 64))
    xyz, tails, bonds, normals = mc.lipid_tails(ntails, np.float64)
    got = m64.lipid_tail_order(xyz, tails, order_type, normals, bonds)
    for t in range(ntails):
        want = orc64.lipid_tail_order(xyz, order_type, normals[t], bonds[t], tails[t])
        assert got[t].shape == want.shape
        assert np.allclose(got[t], want, rtol=0, atol=1e-12, equal_nan=True), (t, got[t], want)


# ------------------------------------------------------------------------------------------------ what was exercised

def test_summary_of_exercised_shapes(cus):
    """Printed for the record (run with -s): the launch shapes every kernel family met in this session and the worst error /
    bound per entry.  The shapes are those of the module's mirror of the launch arithmetic at this card's compute-unit count
    (the library reports no grid sizes); that the sweep's sizes reach the grid cap, trips beyond the four a thread makes
    below the cap, and the finalisers' second trip on THIS card is asserted here from the mirror itself, whatever subset of
    the sweep ran."""
    shapes = [mc.single_shape(cus, mc.size_of(key, cus)) for key in mc.SIZE_KEYS]
    assert any(s["capped"] for s in shapes) and max(s["trips"] for s in shapes) == 9 and any(s["trips"] == 5 for s in shapes)
    assert any(s["fin_trips"] >= 2 and not s["capped"] for s in shapes)
    assert any(mc.fit64_shape(n)["capped"] for _, n in mc.FIT64_CASES)
    assert any(mc.fit32_shape(cus, mc.size_of(str(k), cus), F)["capped"] for F, k in mc.FIT32_CASES if F >= 64)
    print(f"\ncompute units: {cus}; C-dependent sizes: 4096C = {4096 * cus}, 4096C+1 = {4096 * cus + 1}, "
          f"2*4096C+257 = {2 * 4096 * cus + 257}")
    for fam in sorted(SEEN):
        recorded = sorted(SEEN[fam], key=lambda t: str(t))
        print(f"{fam}: {len(recorded)} shapes")
        for sh in recorded:
            print("    " + ", ".join(f"{k}={v}" for k, v in sh))
    print("worst error / bound per entry (information, not a threshold):")
    for entry in sorted(WORST):
        print(f"    {entry}: {WORST[entry]:.3f}")
