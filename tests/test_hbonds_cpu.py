"""Hydrogen bonds, the part that needs no GPU: the C ABI's declarations and their mirrors, the reference of the GPU tests
(tests/hbonds_ref.py) against an all-images brute force, the CONDITION of the GPU tests - no candidate of any case inside a
band - and the host helpers of the Python layer."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hbonds_ref as hr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["molar_hip_hbonds_count", "molar_hip_hbonds_fill", "molar_hip_hbonds_counts", "molar_hip_hbonds_frames",
         "molar_hip_hbonds_frames_fill"]


def header_functions():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_ffi as g
    return {name: params for name, _, params in g.c_functions(open(g.HEADER).read())}


def test_symbols_in_header_and_rust_ffi():
    funcs = header_functions()
    ffi = open(os.path.join(ROOT, "rust", "molar_hip", "src", "ffi.rs")).read()
    for name in NAMES:
        assert name in funcs, name
        assert re.search(r"pub %s: unsafe extern" % name[len("molar_hip_"):], ffi), name
    header = open(os.path.join(ROOT, "include", "molar_hip.h")).read()
    assert "MOLAR_HIP_HBOND_DHA_MIN = 0" in header and "MOLAR_HIP_HBOND_HDA_MAX = 1" in header
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_ctypes_signatures():
    import ctypes as C

    from molar_amd._lib import SYMBOLS
    funcs = header_functions()
    kinds = {"double": C.c_double, "size_t": C.c_size_t, "int32_t": C.c_int32}
    for name in NAMES:
        restype, argtypes = SYMBOLS[name]
        assert restype is C.c_int
        assert len(argtypes) == len(funcs[name]), name
        for (ctype, pname), at in zip(funcs[name], argtypes):
            want = C.c_void_p if "*" in ctype else kinds[ctype.strip()]
            assert at is want, (name, pname, ctype)


def test_angle_kinds_match_the_header():
    from molar_amd import api
    assert (api.HBOND_DHA_MIN, api.HBOND_HDA_MAX) == (hr.DHA, hr.HDA) == (0, 1)


# ---------------------------------------------------------------- the reference against brute force

@pytest.mark.parametrize("boxname,pbc,kind,angle,max_ha", [
    ("box_ortho", 7, hr.DHA, 150.0, 0.0),
    ("box_a", 7, hr.DHA, 150.0, 0.0),
    ("box_a", 7, hr.HDA, 30.0, 0.25),
    ("box_ortho", 3, hr.DHA, 120.0, 0.0),
])
def test_reference_agrees_with_all_images_brute_force(orc32, boxname, pbc, kind, angle, max_ha):
    from molar_amd import synth
    nw = 60
    box = getattr(synth, boxname)(3 * nw)
    don, off, hidx, acc = hr.water_topology(nw, ragged=(kind == hr.HDA))
    c = dict(xyz=hr.waters(nw, box, 5, wrap_dims=pbc), box=box, pbc=pbc, donors=don, hoff=off, hidx=hidx, acceptors=acc, kind=kind,
             angle=angle, max_ha=max_ha, cutoff=0.35)
    ref = hr.reference_from_list(c, *hr.oracle_list(orc32, c))
    brute = hr.reference_from_list(c, *hr.brute_list(c))
    assert ref["n_candidates"] == brute["n_candidates"] > 0
    assert len(ref["triples"]) > 0
    assert np.array_equal(ref["triples"], brute["triples"])
    assert np.array_equal(ref["angle"], brute["angle"])
    # the order: donor position, then hydrogen-table position, then acceptor position
    pos = ref["pos"]
    assert np.array_equal(np.lexsort((pos[:, 2], pos[:, 1], pos[:, 0])), np.arange(len(pos)))


def test_reference_by_hand():
    """one straight and one bent trio, no box: the numbers of the definition"""
    xyz, _ = hr.trios(2, nbent=1)
    c = dict(xyz=xyz, box=None, pbc=0, donors=np.array([0, 3], np.uint64), hoff=np.array([0, 1, 2], np.uint64), hidx=np.array([1, 4], np.uint64),
             acceptors=np.array([2, 5], np.uint64), kind=hr.DHA, angle=150.0, max_ha=0.0, cutoff=0.35)
    ref = hr.reference_from_list(c, np.array([0, 1, 0]), np.array([0, 1, 0]))      # the list with a duplicate
    assert ref["triples"].tolist() == [[0, 1, 2]]
    want = 180.0 - np.degrees(np.arctan2(0.02, 0.19))
    assert abs(ref["angle"][0] - want) < 1e-5            # (f32 coordinates)
    assert abs(ref["dist_ha"][0] - np.hypot(0.19, 0.02)) < 1e-6
    c["kind"], c["angle"] = hr.HDA, 30.0
    ref = hr.reference_from_list(c, np.array([0, 1]), np.array([0, 1]))
    assert ref["triples"].tolist() == [[0, 1, 2]]       # H-D-A of the bent trio is about 40 degrees


# ---------------------------------------------------------------- the condition of the GPU tests

@pytest.mark.parametrize("name", sorted(hr.CASES))
def test_no_candidate_inside_a_band(orc32, name):
    ref = hr.reference(orc32, name)
    assert ref["n_candidates"] > 0
    assert ref["n_list"] > ref["n_unique"], "the oracle's list of this case has no duplicates"
    assert float(ref["clearance"].min()) > 1.0
    # the bounds of the columns are roundings, not tolerances
    if len(ref["triples"]):
        assert ref["bound_angle"].max() < 1e-9 and ref["bound_da"].max() < 1e-12


@pytest.mark.parametrize("name", sorted(hr.FRAMES))
def test_no_candidate_inside_a_band_frames(orc32, name):
    block = hr.frames_case(name)
    counts = []
    for f in range(block["frames"].shape[0]):
        ref = hr.reference(orc32, (name, f), hr.frame_of(block, f))
        if ref["n_candidates"]:
            assert float(ref["clearance"].min()) > 1.0
        counts.append(len(ref["triples"]))
    assert counts.count(0) == 1 and counts[-2] == 0          # the one empty frame


def test_trios_are_what_they_say(orc32):
    xyz, box = hr.trios(65, nbent=3, nfar=2)
    t = np.arange(65, dtype=np.uint64) * 3
    c = dict(xyz=xyz, box=box, pbc=7, donors=t, hoff=np.arange(66, dtype=np.uint64), hidx=t + 1, acceptors=t + 2, kind=hr.DHA, angle=150.0,
             max_ha=0.0, cutoff=0.35)
    ref = hr.reference_from_list(c, *hr.oracle_list(orc32, c))
    assert ref["n_candidates"] == 63 and len(ref["triples"]) == 60
    assert float(ref["clearance"].min()) > 1.0


# ---------------------------------------------------------------- host helpers of the Python layer

def test_hydrogens_three_forms():
    from molar_amd.api import hydrogens_csr
    off, idx = hydrogens_csr(np.array([4, 7, 9]), 3)
    assert off.dtype == idx.dtype == np.uint64
    assert off.tolist() == [0, 1, 2, 3] and idx.tolist() == [4, 7, 9]
    off, idx = hydrogens_csr([4, 7, 9], 3)
    assert off.tolist() == [0, 1, 2, 3] and idx.tolist() == [4, 7, 9]
    off, idx = hydrogens_csr([[1, 2], [], [5, 6, 8]], 3)
    assert off.tolist() == [0, 2, 2, 5] and idx.tolist() == [1, 2, 5, 6, 8]
    off, idx = hydrogens_csr([[], [], []], 3)
    assert off.tolist() == [0, 0, 0, 0] and idx.shape == (0,) and idx.dtype == np.uint64
    off, idx = hydrogens_csr((np.array([0, 2, 2, 5]), [1, 2, 5, 6, 8]), 3)
    assert off.dtype == np.uint64 and off.tolist() == [0, 2, 2, 5] and idx.tolist() == [1, 2, 5, 6, 8]
    for bad, n in (([1, 2], 3), ((np.array([0, 1]), [1]), 3), ((1, 2, 3), 3), (np.zeros((3, 2), np.uint64), 3)):
        with pytest.raises(ValueError):
            hydrogens_csr(bad, n)


@pytest.mark.parametrize("wrapped", [False, True])
def test_hbond_donors_finds_the_generators_topology(orc32, wrapped):
    from molar_amd import api, synth
    nw = 120
    box = synth.box_a(3 * nw)
    xyz = hr.waters(nw, box, 11, wrap_dims=7 if wrapped else 0)
    ox, off, hidx, _ = hr.water_topology(nw)
    top = api.Topology(np.ones(3 * nw, np.float32))
    state = api.State(xyz, box=object() if wrapped else None)         # (the box itself is the stand-in search's business)
    heavy = api.Sel(top, state, ox)
    hyd = api.Sel(top, state, np.setdiff1d(np.arange(3 * nw), ox.astype(np.int64)))

    def search(cutoff, s1, s2, dims):
        p1, p2 = xyz[s1.index.astype(np.int64)], xyz[s2.index.astype(np.int64)]
        if api.pbc_mask(dims):
            r = orc32.search_double_pbc(cutoff, p1, p2, orc32.box_from_matrix(box), api.pbc_mask(dims))
        else:
            r = orc32.search_double(cutoff, p1, p2)
        return np.stack([s1.index[r["i"].astype(np.int64)], s2.index[r["j"].astype(np.int64)]], 1), r["d"]

    got_off, got_idx = api.hbond_donors(heavy, hyd, search=search)
    assert got_off.dtype == got_idx.dtype == np.uint64
    assert np.array_equal(got_off, off) and np.array_equal(got_idx, hidx)


def test_hbond_donors_nearest_heavy_atom_wins():
    from molar_amd.api import _donors_csr
    heavy = np.array([10, 20, 30], np.uint64)
    pairs = np.array([[10, 1], [20, 1], [20, 1], [30, 2], [10, 3], [30, 3]], np.uint64)       # (a duplicate of the list among them)
    dist = np.array([0.11, 0.10, 0.10, 0.09, 0.10, 0.10])
    off, idx = _donors_csr(heavy, pairs, dist)
    assert off.tolist() == [0, 1, 2, 3] and idx.tolist() == [3, 1, 2]       # the tie of hydrogen 3 goes to the atom listed first
