"""The cases of tests/measure_shape_cases.py, checked without a GPU: every case reaches the launch shape it claims (for 64 and
for 256 compute units, through the module's mirror of the launch arithmetic), its terms are exact in f32, its selections
are real gathers, and its comparison sees ONE atom: removing any probed element from the reference, or counting it twice,
moves an output of every kernel family by at least 16 of the bounds the module derives."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import measure_shape_cases as mc  # noqa: E402

CUS = (64, 256)


# ------------------------------------------------------------------------------------------------ the mirror itself

def test_mirror_reproduces_the_figures_read_off_the_launch_code():
    """blocks_for / blocks64 at 256 compute units: 1024 atoms per workgroup, the cap of 1024 workgroups beyond 1 048 576 atoms,
    the finalisers' second trip beyond 64 workgroups; the batch rules of both precisions."""
    assert mc.single_shape(256, 50_000)["nb"] == 49 and mc.single_shape(256, 50_000)["fin_trips"] == 1
    assert mc.single_shape(256, 65_536)["fin_trips"] == 1 and mc.single_shape(256, 65_537)["fin_trips"] == 2
    assert not mc.single_shape(256, 1_048_576)["capped"] and mc.single_shape(256, 1_048_577)["capped"]
    assert mc.single_shape(256, 1_048_577) == dict(nb=1024, capped=True, stride=262144, trips=5, fin_trips=16)
    assert mc.fit32_shape(256, 20_000, 7)["per"] == 4 and mc.fit32_shape(256, 20_000, 8)["per"] == 8
    assert not mc.fit32_shape(256, 4099, 3)["packed"] and mc.fit32_shape(256, 4099, 4)["packed"]
    assert mc.fit32_shape(256, 10 ** 6, 63)["nb"] == 489 and mc.fit32_shape(256, 10 ** 6, 64)["nb"] == 16
    assert mc.fit64_shape(100_000)["nb"] == 49 and not mc.fit64_shape(131_072)["capped"] and mc.fit64_shape(131_073)["capped"]
    assert mc.csr_shape([3, 64, 65, 1000, 1]) == dict(nb=2, idle_waves=3, steps=[1, 1, 2, 16, 1])
    assert mc.lipid_shape(17, 16) == dict(nb=2, idle=15) and mc.lipid_shape(64, 64) == dict(nb=1, idle=0)


def test_probes_are_the_edges_of_every_range():
    for n in (1, 2, 255, 256, 257, 1025):
        p = set(mc.stride_probes(n).tolist())
        assert n - 1 in p and 0 in p
        for b in range(0, n, 256):
            assert b in p and min(b + 256, n) - 1 in p
        q = set(mc.stride_probes(n, 1).tolist())
        assert n - 1 in q
        for b in range(1, n, 256):
            assert b in q and min(b + 256, n) - 1 in q
    assert mc.csr_probes(1).tolist() == [0] and mc.csr_probes(65).tolist() == [0, 63, 64]
    assert mc.csr_probes(129).tolist() == [0, 63, 64, 127, 128] and mc.csr_probes(128).tolist() == [0, 63, 64, 127]
    # every workgroup's range in every grid-stride segment, and every four-atom trip, starts and ends on a probe
    for C, n, F in ((64, 36865, 65), (256, 2 * 4096 * 64 + 257, 1)):
        sh = mc.fit32_shape(C, n, F)
        p = set(mc.stride_probes(n).tolist())
        for seg in range(0, n, sh["stride"]):
            for b in range(seg, min(seg + sh["stride"], n), 256):
                assert b in p and min(b + 256, n) - 1 in p


# ------------------------------------------------------------------------------------------------ single-call reductions

def claimed_single_shape(key, C):
    """what the size is there for"""
    small = {"1": (1, 1), "2": (1, 1), "63": (1, 1), "64": (1, 1), "65": (1, 1), "255": (1, 1), "256": (1, 1), "257": (1, 2),
             "1023": (1, 4), "1024": (1, 4), "1025": (2, 3), "65536": (64, 4), "65537": (65, 4)}
    if key in small:
        nb, trips = small[key]
        return dict(nb=nb, capped=False, stride=nb * 256, trips=trips, fin_trips=2 if key == "65537" else 1)
    trips, capped = {"4096C": (4, False), "4096C+1": (5, True), "2*4096C+257": (9, True)}[key]
    return dict(nb=4 * C, capped=capped, stride=1024 * C, trips=trips, fin_trips=C // 16)


@pytest.mark.parametrize("C", CUS)
@pytest.mark.parametrize("key", mc.SIZE_KEYS)
def test_single_call_cases_reach_their_shape_and_see_one_atom(key, C):
    n = mc.size_of(key, C)
    assert mc.single_shape(C, n) == claimed_single_shape(key, C)
    if key == "2*4096C+257":            # the last segment is a partial one that ends inside its second workgroup
        assert n % (1024 * C) == 257
    if C == 256 and key.endswith("C"):
        assert n == 1_048_576
    for with_idx in (True, False):
        s = mc.system(n, with_idx)
        if with_idx:                    # real gathers: gaps, no prefix, a second index set of its own
            assert s["natoms"] > n and (np.diff(s["sel"]) > 0).all()
            assert n < 3 or (np.diff(s["sel"]) > 1).any()
            assert not np.array_equal(s["sel"], np.arange(n)) and (n < 3 or not np.array_equal(s["sel"], s["sel2"]))
        else:
            assert s["natoms"] == n
        sel = s["sel"]
        assert n - 1 in s["probes"] and (n == 1 or n - 1 in s["pbc_probes"])
        assert (s["mass"][sel[s["probes"]]] == mc.SENT_MASS).all() and (np.abs(s["X1"][sel[s["probes"]]]) == mc.XMAX).all()
        assert np.abs(s["X1"][sel]).max() <= mc.XMAX and 1 <= s["mass"].min() and s["mass"].max() <= 32
        assert 0 <= s["Xw"].min() and s["Xw"].max() < mc.BOX_EDGE * mc.UNIT
        assert mc.exact_in_f32(s)
        assert np.abs(mc.term_sums(np.abs(s["X1"][sel]), s["mass"][sel], s["X2"][s["sel2"]] + 2 * np.abs(s["X1"][sel]))).max() < 2 ** 52    # exact in f64, any order
        if n == 1:
            continue                    # one atom: nothing to remove, and counting it twice changes no ratio
        for prec in (32, 64):
            for family, ratio in mc.single_sensitivities(s, prec, C).items():
                assert ratio >= mc.SENS, (key, C, with_idx, prec, family, ratio)


def test_the_bounds_are_ulps_not_tolerances():
    """the derived bounds stay within 5 ulps of the output type in f32 (8 for the periodic gyration) and 40 in f64 (the stated
    depth of additions), so they cannot hide what the old 1e-5 hid"""
    for key in ("65537", "2*4096C+257"):
        s = mc.system(mc.size_of(key, 64), True)
        for prec, ulp in ((32, 2.0 ** -23), (64, 2.0 ** -52)):
            ref = mc.single_reference(s, prec, 64)
            for name in ("cog", "com", "rmsd", "rmsd_mw", "gyration", "gyration_pbc", "cog_pbc7", "com_pbc7"):
                v, b = ref[name]
                rel = np.max(np.asarray(b) / np.maximum(np.abs(v), 1e-300))
                # (the periodic gyration adds the data's own difference error e_d: 7 f32 ulps here, 32 f64 ulps at 256 CUs)
                limit = (8 if name == "gyration_pbc" else 5) if prec == 32 else 40
                assert rel <= limit * ulp, (key, prec, name, rel)


@pytest.mark.parametrize("n,with_idx", [(2, True), (257, True), (1025, False), (65537, True)])
def test_exact_sum_references_agree_with_the_f64_oracle(orc64, n, with_idx):
    """The references are formulas over integer sums (the periodic ones with the reference's centre quirk and the images
    taken by hand): the f64 oracle, which walks the atoms one by one, must give the same numbers up to its own serial
    summation noise, n * 2^-53 of the largest term sum."""
    s = mc.system(n, with_idx)
    ref = mc.single_reference(s, 64, 256)
    x1, x2, xw = (mc.as_real(s[k], np.float64) for k in ("X1", "X2", "Xw"))
    m = s["mass"].astype(np.float64)
    i1, i2 = mc.idx_arg(s), mc.idx_arg(s, "sel2")
    box = orc64.box_from_matrix(mc.BOX)
    got = dict(cog=orc64.center_of_geometry(x1, i1), com=orc64.center_of_mass(x1, m, i1), gyration=orc64.gyration(x1, m, i1),
               rmsd=orc64.rmsd(x1, x2, i1, i2), rmsd_mw=orc64.rmsd_mw(x1, m, x2, i1, i2), gyration_pbc=orc64.gyration_pbc(xw, m, box, i1))
    for dims in (7, 3):
        got[f"cog_pbc{dims}"] = orc64.center_of_geometry_pbc_dims(xw, box, dims, i1)
        got[f"com_pbc{dims}"] = orc64.center_of_mass_pbc_dims(xw, m, box, dims, i1)
    if n >= 3:
        for key, t in (("tensor", orc64.inertia_tensor(x1, m, i1)), ("tensor_pbc", orc64.inertia_tensor(xw, m, i1, box=box))):
            got[key] = np.array([t[0, 0], t[1, 1], t[2, 2], t[0, 1], t[0, 2], t[1, 2]])
    for key, g in got.items():
        v, b = ref[key]
        slack = n * mc.U64 * np.max(np.abs(v))
        assert (np.abs(np.asarray(g) - v) <= b + slack).all(), (key, g, v)


# ------------------------------------------------------------------------------------------------ fit_rmsd_batch

def claimed_fit32(F, n, C):
    if n in (16384, 16385, 32768, 32769, 36865):
        nb, capped, whole, partial, mixed = {16384: (8, False, 2, False, False), 16385: (9, False, 1, True, True),
                                             32768: (16, False, 2, False, False), 32769: (16, True, 2, True, True),
                                             36865: (16, True, 2, True, True)}[n]
        return dict(nb=nb, capped=capped, cap16=True, per=8, packed=True, whole_trips=whole, partial_trip=partial, mixed_guards=mixed)
    if n in (1023, 1025, 2047, 2049):
        per = 8 if F >= 8 else 4
        # 8 atoms per thread, four per trip: from 1025 atoms on a whole trip precedes the partial one
        return dict(nb=-(-n // (256 * per)), capped=False, cap16=F >= 64, per=per, packed=F >= 4,
                    whole_trips=1 if per == 8 and n > 1024 else 0, partial_trip=True, mixed_guards=True)
    if n == 65537:
        return dict(nb=65, capped=False, per=4, packed=F >= 4, fin_trips=2)
    return dict(nb=4 * C, capped=True, per=4, packed=F >= 4, fin_trips=C // 16, whole_trips=1, partial_trip=True, mixed_guards=True)


@pytest.mark.parametrize("C", CUS)
def test_fit32_cases_reach_their_shape(C):
    seen = set()
    for F, key in mc.FIT32_CASES:
        n = mc.size_of(str(key), C)
        sh = mc.fit32_shape(C, n, F)
        for k, v in claimed_fit32(F, n, C).items():
            assert sh[k] == v, (F, n, k, sh)
        seen.add((sh["per"], sh["cap16"], sh["packed"], sh["capped"], sh["mixed_guards"], sh["whole_trips"] > 1, sh["fin_trips"] > 1))
    # both atoms-per-thread rules, the 16-workgroup cap reached and not, packed and not, whole trips followed by a mixed one
    assert {(4, False, False), (4, False, True), (8, False, True), (8, True, True)} <= {(p, c, k) for p, c, k, *_ in seen}
    assert any(c16 and cap and mixed and whole for _, c16, _, cap, mixed, whole, _ in seen)
    assert any(fin for *_, fin in seen)


def test_fit64_cases_reach_their_shape():
    want = {1: (1, False, 1), 2047: (1, False, 8), 2048: (1, False, 8), 2049: (2, False, 5), 131072: (64, False, 8),
            131073: (64, True, 9), 262444: (64, True, 17)}
    for F, n in mc.FIT64_CASES:
        sh = mc.fit64_shape(n)
        assert (sh["nb"], sh["capped"], sh["trips"]) == want[n], (n, sh)


FIT_SENS_CASES = (sorted({(32, F, mc.size_of(str(key), C)) for F, key in mc.FIT32_CASES for C in CUS})
                  + [(64, F, n) for F, n in mc.FIT64_CASES])


@pytest.mark.parametrize("prec,F,n", FIT_SENS_CASES)
def test_fit_gyration_sees_one_atom(prec, F, n):
    """Every case of FIT32_CASES (at 64 and at 256 compute units) and of FIT64_CASES: the fitted selection's gyration radius
    (the sharp output of a fit) moves by 16 of its bounds for the first and the last frame - the f64 bound with the depth
    of that case's own launch shape.  One atom (FIT64_CASES, n = 1) is exempt as everywhere."""
    fs = mc.fit_system(n, F)
    assert fs["natoms"] > n and not np.array_equal(fs["sel"], np.arange(n))
    assert n < 3 or not np.array_equal(fs["sel"], fs["ref_sel"])
    assert (fs["mass"][fs["sel"][fs["probes"]]] == mc.SENT_MASS).all() and n - 1 in fs["probes"]
    for f in {0, F - 1}:
        assert (np.abs(fs["frames"][f][fs["sel"][fs["probes"]]]).min(1) >= mc.XMAX - 26).all()      # corners stay corners
        if n == 1:
            continue
        r = mc.fit_gyration_sensitivity(fs, f, prec, mc.fit64_shape(n))
        assert r >= mc.SENS, (prec, F, n, f, r)


# ------------------------------------------------------------------------------------------------ CSR batches

def test_csr_cases_reach_every_wave_step_edge_and_see_one_atom():
    cs = mc.csr_system()
    sizes = cs["sizes"]
    assert sorted(sizes[:10]) == sorted(sizes[10:]) == sorted(mc.CSR_SIZES) and list(sizes[:10]) != list(sizes[10:])
    assert len(np.unique(cs["idx"])) == len(cs["idx"]) and len(np.unique(cs["idx2"])) == len(cs["idx2"])   # disjoint: apply is defined
    assert cs["natoms"] > len(cs["idx"])
    for nsel in mc.CSR_NSEL:
        sh = mc.csr_shape(sizes[:nsel])
        assert sh["nb"] == -(-nsel // 4) and sh["idle_waves"] == (-nsel) % 4
    assert {mc.csr_shape(sizes[:n])["idle_waves"] for n in mc.CSR_NSEL} == {0, 1, 3}
    assert {1, 2, 3, 16} <= set(mc.csr_shape(sizes)["steps"])
    for k in range(len(sizes)):
        a, b = int(cs["off"][k]), int(cs["off"][k + 1])
        # both ends of every selection are sentinels: a wave that reads one element into its neighbour meets one
        assert cs["mass"][cs["idx"][a]] == mc.SENT_MASS and cs["mass"][cs["idx"][b - 1]] == mc.SENT_MASS
        if b - a == 1:
            continue
        for prec in (32, 64):
            sens = mc.csr_sensitivity(cs, k, prec)
            for family in (("sums", "moments", "rmsd") if prec == 32 else ("sums",)):
                assert sens[family] >= mc.SENS, (k, int(sizes[k]), prec, family, sens[family])
        # the periodic gyration keeps a tolerance (f32 terms about an f32 centre): it still sees one atom
        ref, rel = mc.csr_pbc_gyration(cs, k)
        assert rel >= mc.SENS * mc.PBC_GYR_BATCH_RTOL32, (k, int(sizes[k]), rel)


def test_lipid_cases_fill_and_overflow_a_workgroup():
    for prec, per in ((32, 16), (64, 64)):
        shapes = [mc.lipid_shape(t, per) for t in mc.LIPID_NTAILS[prec]]
        assert [s["nb"] for s in shapes] == ([1, 1, 1, 2, 3] if prec == 32 else [1, 1, 1, 2])
        assert 0 in [s["idle"] for s in shapes] and 1 in [s["idle"] for s in shapes]
    xyz, tails, bonds, normals = mc.lipid_tails(33, np.float32)
    assert sorted({len(t) for t in tails}) == [3, 4, 18]
    assert any((b == 2).any() for b in bonds) and {len(n) for n in normals} >= {1, 2, 16}
