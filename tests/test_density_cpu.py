"""The density calls without a GPU: the ABI of the three entries, the plan entry (a pure host function), the errors of the
arguments alone, the numpy reference (tests/density_ref.py) against known answers, and the host helpers."""
import ctypes as C
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import density_ref as dr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("molar_hip_density_plan", "molar_hip_density", "molar_hip_density_f64")


def test_abi_of_the_three_entries():
    from molar_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    raw = open(os.path.join(ROOT, "include", "molar_hip.h")).read()
    header = re.sub(r"\s+", " ", raw)
    ffi = open(os.path.join(ROOT, "rust", "molar_hip", "src", "ffi.rs")).read()
    for name in NAMES:
        assert f"int {name}(" in header, name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert f'b"{name}\\0"' in ffi, name
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_ffi as gen
    funcs = {name: params for name, _, params in gen.c_functions(open(gen.HEADER).read())}
    assert len(funcs["molar_hip_density_plan"]) == len(_lib.SYMBOLS["molar_hip_density_plan"][1]) == 8
    assert len(funcs["molar_hip_density"]) == len(_lib.SYMBOLS["molar_hip_density"][1]) == 23
    assert len(funcs["molar_hip_density_f64"]) == len(_lib.SYMBOLS["molar_hip_density_f64"][1]) == 23
    assert [t for t, _ in funcs["molar_hip_density"]] == [t.replace("double", "float") for t, _ in funcs["molar_hip_density_f64"]]
    assert open(gen.OUT).read() == gen.render(gen.c_functions(open(gen.HEADER).read())), "run python tools/gen_rust_ffi.py"
    # the grid: the header's fields, the ctypes mirror and the #[repr(C)] struct, in the same order and of the same size
    body = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*molar_hip_density_grid\s*;", gen.strip_comments(raw)).group(1)
    cfields = [re.search(r"(\w+)\s*(\[[^\]]*\])?\s*$", part.strip()).group(1) for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert cfields == ["mode", "nbins", "lo", "hi", "centre_dims"] == [f for f, _ in _lib.DensityGrid._fields_]
    assert C.sizeof(_lib.DensityGrid) == 72                                   # 4 + 12 | 24 | 24 | 4 and the tail padding of a double's alignment
    rs = open(os.path.join(ROOT, "rust", "molar_hip", "src", "types.rs")).read()
    rbody = re.search(r"#\[repr\(C\)\]\n#\[derive\([^)]*\)\]\npub struct MolarHipDensityGrid\s*\{(.*?)\n\}", rs, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): ([^,]+),", rbody) == [("mode", "u32"), ("nbins", "[u32; 3]"), ("lo", "[f64; 3]"), ("hi", "[f64; 3]"), ("centre_dims", "u32")]
    hpp = open(os.path.join(ROOT, "include", "molar_hip.hpp")).read()
    assert "inline Density density(" in hpp and "density_f64(" in hpp and "molar_hip_density(" in hpp and "molar_hip_density_f64(" in hpp
    lib_rs = open(os.path.join(ROOT, "rust", "molar_hip", "src", "lib.rs")).read()
    assert "pub fn density(" in lib_rs and "pub fn density_plan(" in lib_rs
    assert "density.hip" in build.SOURCES


def test_plan_needs_no_gpu_and_is_monotone():
    from molar_amd import api, build
    build.build_library()
    prof = api.profile_grid(2, 200)
    assert api.density_plan(0, 100, prof)[0] == 0 and api.density_plan(100, 0, prof)[0] == 0
    ws, fc, ac, lc = api.density_plan(256, 500000, prof, 5)
    assert fc >= 1 and ac >= 256 and lc >= 1000
    sizes_f = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 4096, 65536]
    sizes_b = [1, 2, 63, 64, 65, 200, 4095, 4096, 4097, 16384, 100000, 524287, 524288, 524289, 699051, 2097152, 33554431, 33554432, 33554433, 40000000]
    for G in (1, 2, 5):
        for nb in sizes_b:
            if G * nb >= 2 ** 31:
                continue
            last = 0
            for F in sizes_f:
                w, chunk, atoms, cells = api.density_plan(F, 1000, api.profile_grid(2, nb), G)
                assert (atoms, cells) == (ac, lc) and chunk >= 1
                assert w >= last and w >= 8 * G * nb * (min(F, chunk) + 3), (F, G, nb)     # the frames' bins, the sums, count, density
                last = w
    for F in sizes_f:
        for G in (1, 2, 5):
            seq = [api.density_plan(F, 1000, api.profile_grid(2, nb), G)[0] for nb in sizes_b if G * nb < 2 ** 31]
            assert seq == sorted(seq), (F, G)
        for nb in (200, 16384, 2097152):
            seq = [api.density_plan(F, 1000, api.profile_grid(2, nb), G)[0] for G in (1, 2, 3, 5, 8, 64)]
            assert seq == sorted(seq), (F, nb)
            assert api.density_plan(F, 10, api.profile_grid(2, nb))[0] <= api.density_plan(F, 10 ** 7, api.profile_grid(2, nb))[0]
    # the chunk of frames shrinks as the grid grows and never reaches zero
    chunks = [api.density_plan(100, 10, api.profile_grid(2, nb))[1] for nb in sizes_b]
    assert chunks == sorted(chunks, reverse=True) and chunks[0] > 1 and chunks[-1] == 1
    # the three shapes give the same plan for the same number of bins
    assert api.density_plan(7, 9, api.map_grid((16, 8)))[0] == api.density_plan(7, 9, api.volume_grid((0, 0, 0), (1, 1, 1), (2, 8, 8)))[0]


def test_argument_errors_need_no_device():
    from molar_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    ctx = C.create_string_buffer(1 << 16)                    # never read: the arguments are judged before the context is used
    for fn, real in ((lib.molar_hip_density, np.float32), (lib.molar_hip_density_f64, np.float64)):
        for what, want, got in dr.argument_errors(fn, C.addressof(ctx), real):
            assert got == want, (what, want, got, lib.molar_hip_last_error())
        g = dr.grid(dr.BOX, (1, 1, 4))
        assert dr.raw_density(fn, C.addressof(ctx), np.zeros((0, 5, 3), real), g, real, F=0, boxes=dr.ORTHO)[0] == 0, "nframes == 0 is a successful no-op"
        assert dr.raw_density(fn, None, np.zeros((2, 5, 3), real), g, real, boxes=dr.ORTHO)[0] == dr.ERR_INVALID
    # the plan entry judges its grid too
    bad = _lib.DensityGrid()
    bad.mode = 1
    assert lib.molar_hip_density_plan(1, 1, 1, C.addressof(bad), None, None, None, None) == dr.ERR_INVALID
    assert lib.molar_hip_density_plan(1, 1, 1, None, None, None, None, None) == dr.ERR_INVALID


def test_reference_lattice_counts_one_everywhere():
    nb = (4, 3, 5)
    F = 2
    # one atom at the centre of every cell of the fractional lattice of a skewed box
    u = np.stack(np.meshgrid(*[(np.arange(k) + 0.5) / k for k in nb], indexing="ij"), -1).reshape(-1, 3)
    fr = np.stack([u @ dr.box_of(dr.TRICLINIC, 0).T] * F).astype(np.float32)
    ref = dr.density(fr, dr.grid(dr.BOX, nb), boxes=dr.TRICLINIC)
    dr.margin_ok(ref)
    assert (ref["count"] == F).all() and (ref["I"] == 1).all() and (ref["outside"] == 0).all() and ref["S"] == 0
    # ... and the number density is one atom per bin volume
    assert np.abs(ref["density"] * ref["binvol"][0] - 1).max() < 1e-18
    # the same lattice in lab coordinates
    lo, hi = (-1.0, 0.0, 2.0), (1.0, 3.0, 4.5)
    x = np.asarray(lo) + u * (np.asarray(hi) - np.asarray(lo))
    ref = dr.density(x[None].astype(np.float32), dr.grid(dr.LAB, nb, lo, hi))
    dr.margin_ok(ref)
    assert (ref["count"] == 1).all() and (ref["outside"] == 0).all()


def test_reference_conserves_the_kept_weights():
    F, n, nb = 5, 300, (3, 4, 6)
    boxes = dr.mr.scaled_boxes(F, 2, dr.TRICLINIC)
    fr = dr.scatter_box(3, F, n, nb, boxes, pbc=3)
    rng = np.random.default_rng(4)
    w = rng.uniform(-2, 2, n)
    labels = rng.integers(0, 3, n)
    ref = dr.density(fr, dr.grid(dr.BOX, nb), weight=w, labels=labels, ngroups=3, boxes=boxes, pbc=3)
    dr.margin_ok(ref)
    assert ref["outside"].min() > 0 and ref["outside"].max() < n
    # with nothing outside, the sum over the bins of density * binvol * F is the sum of the weights as they were quantised
    q = np.array([int(np.rint(v * 2.0 ** ref["S"])) for v in w])
    one =dr.density(fr, dr.grid(dr.BOX, nb), weight=w, boxes=dr.TRICLINIC, pbc=7)
    assert (one["outside"] == 0).all()
    total = float((one["density"] * one["binvol"][0]).sum() * F)
    assert abs(total - F * float(q.sum()) * 2.0 ** -one["S"]) <= 1e-15 * F * float(np.abs(q).sum()) * 2.0 ** -one["S"]
    assert int(one["count"].sum()) == F * n and int(ref["count"].sum()) == F * n - int(ref["outside"].sum())


def test_reference_centres_a_split_slab():
    F, npairs, nz = 4, 40, 20
    z0 = np.array([0.02, 0.5, 0.97, 0.3])                      # the first and third slab straddle the cell boundary
    g = dr.grid(dr.BOX, (1, 1, nz), centre_dims=4)
    fr = dr.slab(5, F, npairs, nz, z0)
    ids = np.arange(2 * npairs)
    ref = dr.density(fr, g, boxes=dr.ORTHO, centre_idx=ids)
    dr.margin_ok(ref)
    assert ref["resultant"] > 0.1
    assert np.abs(ref["centre"][:, 2].astype(np.float64) - z0).max() < 1e-6 and (ref["centre"][:, :2] == 0).all()
    # every frame gives the same histogram, symmetric about the middle, and empty far from it
    assert all((ref["I"][f] == ref["I"][0]).all() for f in range(F))
    assert (ref["I"][0, 0] == ref["I"][0, 0][::-1]).all() and ref["I"][0, 0, 0] == 0 and ref["I"][0].sum() == 2 * npairs
    # the plain mean of the wrapped coordinates is somewhere else for a split slab
    plain = (fr[0, :, 2].astype(np.float64) / 4.0 % 1.0).mean()
    assert abs(plain - z0[0]) > 0.1


def test_weight_scale_of_the_reference():
    assert dr.weight_scale(np.arange(1.0, 251.0), 250) == 62 - 8 - 8          # 250 < 2^8 weights, the largest 250 < 2^8
    assert dr.weight_scale(np.array([1.0]), 1) == 52                           # 62 - 0 - 1, clamped
    assert dr.weight_scale(np.array([0.25, -0.7]), 2 ** 20) == 62 - 20 - 0     # |w| < 1 = 2^0
    assert dr.weight_scale(np.array([256.0]), 257) == 62 - 9 - 9               # a power of two needs the next exponent
    assert dr.weight_scale(np.zeros(3), 3) == 52


def test_host_helpers():
    from molar_amd import api
    g = api.profile_grid(2, 8)
    assert g.nbins == (1, 1, 8) and g.mode == api.DENSITY_BOX and g.centre_dims == 0 and api.profile_grid(0, 3, centre=True).centre_dims == 1
    assert api.map_grid((5, 7)).nbins == (5, 7, 1)
    v = api.volume_grid((0, 0, -1), (1, 2, 1), (2, 4, 8))
    assert v.mode == api.DENSITY_LAB and v.nbins == (2, 4, 8)
    assert np.array_equal(api.density_axis(v, 2), -1 + (np.arange(8) + 0.5) * 0.25)
    assert np.array_equal(api.density_axis(g, 2), (np.arange(8) + 0.5) / 8)
    assert np.allclose(api.density_axis(g, 2, box=dr.ORTHO), (np.arange(8) + 0.5) / 8 * 4.0, rtol=0, atol=1e-15)
    assert np.allclose(api.density_axis(g, 2, box=np.diag([3.0, 3.5, 4.0])), (np.arange(8) + 0.5) / 8 * 4.0, rtol=0, atol=1e-15)
    c = api.profile_grid(2, 8, centre=True)
    assert np.array_equal(api.density_axis(c, 2), (np.arange(8) + 0.5) / 8 - 0.5)
    # symmetrising a symmetric profile is the identity; an antisymmetric one vanishes; groups are kept apart
    sym = np.array([[1.0, 2.0, 5.0, 5.0, 2.0, 1.0], [0.0, 3.0, 4.0, 4.0, 3.0, 0.0]])
    g6 = api.profile_grid(2, 6)
    assert np.array_equal(api.density_symmetrize(sym, g6, 2), sym)
    assert np.array_equal(api.density_symmetrize(sym.reshape(2, 1, 1, 6), g6, 2), sym.reshape(2, 1, 1, 6))
    assert np.array_equal(api.density_symmetrize(np.array([-2.0, -1.0, 0.0, 1.0, 2.0]), api.profile_grid(0, 5), 0), np.zeros(5))
    m = np.arange(12.0).reshape(3, 4)
    assert np.array_equal(api.density_symmetrize(m.ravel(), api.map_grid((3, 4)), 1), (0.5 * (m + m[:, ::-1])).ravel())
