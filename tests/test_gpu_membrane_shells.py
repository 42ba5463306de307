"""The neighbour-shell options in the chained frame (molar_hip_membrane_plan_set_shells): patches rebuilt as the n-th
Voronoi shell after a first smoothing pass, and curvatures averaged over the n-th shell, on the device inside one
begin / end pair.  The yardstick is the stage-by-stage branch of Membrane.compute (fused=False), which
tests/test_gpu_membrane.py compares with the CPU checker: every array has to agree bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARRAYS = ("head", "mid", "tail", "patch_off", "patch_ids", "initial_normals", "valid", "smoothed_head", "normals", "quad_coefs",
          "mean_curv", "gauss_curv", "princ_curvs", "princ_dirs", "area", "nvert", "neib_ids", "voro_vertexes", "fitted_patch_points")
SHELLS = [(1, 0), (2, 0), (3, 2), (0, 1), (0, 3), (4, 3)]


@pytest.fixture(scope="module")
def eng():
    from molar_amd import build
    from molar_amd.api import Engine
    build.build_library()
    return Engine(0)


def same_bits(a, b, what):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    if a.tobytes() != b.tobytes():
        u = lambda x: x.reshape(-1).view(np.uint8 if x.dtype.itemsize == 1 else f"u{x.dtype.itemsize}")
        bad = np.flatnonzero(u(a) != u(b))
        raise AssertionError(f"{what}: {len(bad)} of {a.size} elements differ, first at {bad[:5]}: {a.reshape(-1)[bad[:5]]} vs {b.reshape(-1)[bad[:5]]}")


def same_result(got, want, what=""):
    E = len(want["patch_ids"])
    for k in ARRAYS:
        a, b = got[k], want[k]
        if k == "fitted_patch_points":      # (the stage-by-stage state keeps one padding row when there is no patch entry at all)
            a, b = a[:E], b[:E]
        same_bits(a, b, f"{what}{k}")
    assert len(got["order"]) == len(want["order"])
    for t, (a, b) in enumerate(zip(got["order"], want["order"])):
        same_bits(a, b, f"{what}order[{t}]")


def bilayer(per_leaflet, natoms, seed=20240607, shear=None):
    from molar_amd import membrane as mb
    xyz, box, first, tpl, masses = mb.build_bilayer(per_leaflet, natoms, seed=seed)
    if shear is not None:
        s = np.eye(3)
        s[0, 1], s[0, 2], s[1, 2] = shear
        xyz = (xyz.astype(np.float64) @ s.T).astype(np.float32)
        box = (s @ box.astype(np.float64)).astype(np.float32)
    return xyz, box, first, tpl, masses


def pair(eng, system, **opts):
    from molar_amd import membrane as mb
    xyz, box, first, tpl, masses = system
    mk = lambda fused: mb.Membrane(eng, len(xyz), first, tpl, masses, mb.MembraneOptions(fused=fused, **opts))
    return mk(True), mk(False)


def frames_of(xyz, n, seed=5, sigma=0.02):
    rng = np.random.default_rng(seed)
    return [(xyz + rng.normal(0, sigma, xyz.shape)).astype(np.float32) for _ in range(n)]


def search_entries(m, ticket):
    """Entries of the frame's search patches (two per marker pair), from the chained plan's view."""
    return 2 * int(m._plan_obj._views[ticket].npairs)


def chained(m, frame, box):
    t = m.compute_begin(frame, box)
    return m.compute_end(t), search_entries(m, t)


def check_frame(got, want, E, shp, what):
    same_result(got, want, what)
    if shp:     # the staged path re-slots only when the slot count changes: never let the comparison depend on that
        assert int(got["patch_off"][-1]) != E, f"{what}shell entries equal the search entries ({E})"


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("shells", SHELLS)
def test_chained_shells_equal_the_stages(eng, shells, iters):
    k = SHELLS.index(shells) + 3 * (iters == 3)
    opts = dict(cutoff=1.5 if k % 2 else 2.0, order_type=k % 3, max_smooth_iter=iters, n_shells_patch=shells[0], n_shells_smoothing=shells[1])
    if k % 4 == 1:
        opts["unwrap"] = False
    if k % 4 == 2:
        opts["global_normal"] = (0.0, 0.0, 1.0)
    system = bilayer(150, 30000)
    fused, staged = pair(eng, system, **opts)
    assert fused.fusable() and not staged.fusable()
    off = np.array([3, 77, 150, 151, 298])
    for m in (fused, staged):
        m.valid[off] = 0                                  # switched off by the caller (set_valid)
    kept = []
    for f, frame in enumerate(frames_of(system[0], 3, seed=11 + k)):
        a, b = frame.copy(), frame.copy()
        (got, E), want = chained(fused, a, system[1]), staged.compute(b, system[1])
        same_bits(a, b, "unwrapped frame")
        check_frame(got, want, E, shells[0], f"frame {f}: ")
        assert not got["valid"][off].any()
        assert np.array_equal(fused.valid, staged.valid)
        kept.append(int(np.count_nonzero(got["valid"])))
    # (a first-shell patch holds about six points for the six coefficients of the quadric: with several passes most such fits
    # are dropped as the frames go on, so only the first frame is asked to keep a good part of the bilayer)
    assert kept[0] > 10, kept


@pytest.mark.parametrize("shells", [(3, 2), (4, 3)])
def test_sheared_box_noisy_frames_two_in_flight(eng, shells):
    """A triclinic box, noisy frames with a defect that drops lipids (the flags carry over), two frames in flight."""
    system = bilayer(160, 32000, seed=7, shear=(0.3, -0.2, 0.25))
    xyz, box = system[0], system[1]
    fused, staged = pair(eng, system, cutoff=1.6, order_type=2, max_smooth_iter=2, n_shells_patch=shells[0], n_shells_smoothing=shells[1])
    fr = frames_of(xyz, 5, seed=3, sigma=0.03)
    bad = fr[1].copy()
    bad[40 * 52: 40 * 52 + 12, 2] += 1.5
    fr[1] = bad
    want = [staged.compute(f.copy(), box) for f in fr]
    bufs = [f.copy() for f in fr]
    got = []
    t_prev = fused.compute_begin(bufs[0], box)
    for k in range(1, len(fr)):
        t = fused.compute_begin(bufs[k], box)
        got.append((fused.compute_end(t_prev), search_entries(fused, t_prev)))
        t_prev = t
    got.append((fused.compute_end(t_prev), search_entries(fused, t_prev)))
    for f, ((g, E), w) in enumerate(zip(got, want)):
        check_frame(g, w, E, shells[0], f"frame {f}: ")
    assert np.array_equal(fused.valid, staged.valid)
    assert np.count_nonzero(fused.valid == 0) > 0


def test_resident_coordinates(eng):
    import torch
    system = bilayer(120, 20000)
    fused, staged = pair(eng, system, cutoff=1.5, order_type=1, n_shells_patch=3, n_shells_smoothing=2)
    for frame in frames_of(system[0], 2):
        d = torch.from_numpy(frame).cuda()
        b = frame.copy()
        (got, E), want = chained(fused, d, system[1]), staged.compute(b, system[1])
        same_bits(d.cpu().numpy(), b, "unwrapped frame")
        check_frame(got, want, E, 3, "")


def test_shell_capacity_outgrown_then_back_to_no_shells(eng):
    """(1,0) frames provision the shell arrays for about six entries a lipid; (4,0) needs about 37, so its first frames are
    repeated inside _end (with two frames in flight: both of them).  Going back to (0,0) gives the bits of a plan that never
    had shells."""
    system = bilayer(150, 30000)
    xyz, box = system[0], system[1]
    fused, staged = pair(eng, system, cutoff=2.0, order_type=1, n_shells_patch=1)
    plain, _ = pair(eng, system, cutoff=2.0, order_type=1)
    fr = frames_of(xyz, 7, seed=9)
    for f in fr[:2]:
        (got, E), want = chained(fused, f.copy(), box), staged.compute(f.copy(), box)
        check_frame(got, want, E, 1, "(1,0): ")
    small = int(got["patch_off"][-1])
    K = len(system[2])
    assert small < 8 * K + 1024 < 4 * small        # what (1,0) provisions; (4,0) needs several times as much
    for m in (fused, staged):
        m.opt.n_shells_patch = 4
    want = [staged.compute(f.copy(), box) for f in fr[2:5]]
    bufs = [f.copy() for f in fr[2:5]]
    t0 = fused.compute_begin(bufs[0], box)
    t1 = fused.compute_begin(bufs[1], box)
    got = [(fused.compute_end(t0), search_entries(fused, t0))]
    t2 = fused.compute_begin(bufs[2], box)
    got.append((fused.compute_end(t1), search_entries(fused, t1)))
    got.append((fused.compute_end(t2), search_entries(fused, t2)))
    for f, ((g, E), w) in enumerate(zip(got, want)):
        check_frame(g, w, E, 4, f"(4,0) frame {f}: ")
        assert int(g["patch_off"][-1]) > 8 * K + 1024
    for m in (fused, staged):
        m.opt.n_shells_patch = 0
    plain.valid[:] = fused.valid
    for f in fr[5:]:
        got, want, base = fused.compute(f.copy(), box), staged.compute(f.copy(), box), plain.compute(f.copy(), box)
        same_result(got, want, "(0,0): ")
        same_result(got, base, "(0,0) vs never shells: ")


def test_set_shells_with_a_frame_in_flight_is_refused(eng):
    from molar_amd.api import MolarHipError
    system = bilayer(100, 15000)
    xyz, box = system[0], system[1]
    fused, _ = pair(eng, system, cutoff=1.5, order_type=1)
    plain, _ = pair(eng, system, cutoff=1.5, order_type=1)
    plan = fused._plan()
    t = fused.compute_begin(xyz.copy(), box)
    with pytest.raises(MolarHipError):
        plan.set_shells(3, 2)
    got = fused.compute_end(t)
    same_result(got, plain.compute(xyz.copy(), box), "refused set_shells: ")
    # and the plan still has no shells for the next frame
    f = frames_of(xyz, 1)[0]
    same_result(fused.compute(f.copy(), box), plain.compute(f.copy(), box), "next frame: ")
    # Membrane: options changed between two begins of a pipelined trajectory are refused, not silently left for later
    t = fused.compute_begin(f.copy(), box)
    fused.opt.n_shells_patch = 3
    with pytest.raises(ValueError):
        fused.compute_begin(f.copy(), box)
    same_result(fused.compute_end(t), plain.compute(f.copy(), box), "frame begun before the change: ")


def test_large_n_takes_the_fallback(eng):
    """n = 12 on a 2 x 196 lipid bilayer: every shell is a whole leaflet (more than the 128 members the LDS path holds)."""
    system = bilayer(196, 24000)
    fused, staged = pair(eng, system, cutoff=1.5, order_type=0, max_smooth_iter=2, n_shells_patch=12, n_shells_smoothing=12)
    for f, frame in enumerate(frames_of(system[0], 2)):
        (got, E), want = chained(fused, frame.copy(), system[1]), staged.compute(frame.copy(), system[1])
        check_frame(got, want, E, 12, f"frame {f}: ")
        sizes = np.diff(got["patch_off"].astype(np.int64))[got["valid"].astype(bool)]
        assert sizes.max() > 128


def test_ten_thousand_lipids(eng):
    system = bilayer(5300, 560_000)
    fused, staged = pair(eng, system, cutoff=1.5, order_type=1, n_shells_patch=3, n_shells_smoothing=2)
    a, b = system[0].copy(), system[0].copy()
    (got, E), want = chained(fused, a, system[1]), staged.compute(b, system[1])
    same_bits(a, b, "unwrapped frame")
    check_frame(got, want, E, 3, "")
    assert np.count_nonzero(got["valid"]) > 10000
