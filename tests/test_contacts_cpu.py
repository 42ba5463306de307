"""Contact counts without a GPU: the ABI of the two entries, and the numpy folding of the oracle's list
(tests/contacts_ref.py) against an O(N^2) minimum-image brute force, with its invariants."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contacts_ref as cr  # noqa: E402

from molar_amd import synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("molar_hip_search_contacts", "molar_hip_search_contacts_frames")


def test_abi_of_the_two_entries():
    from molar_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "molar_hip.h")).read())
    ffi = open(os.path.join(ROOT, "rust", "molar_hip", "src", "ffi.rs")).read()
    for name in NAMES:
        assert f"int {name}(" in header, name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert f'b"{name}\\0"' in ffi, name
    assert "} molar_hip_contact_groups;" in header
    assert len(_lib.SYMBOLS["molar_hip_search_contacts"][1]) == 7
    assert len(_lib.SYMBOLS["molar_hip_search_contacts_frames"][1]) == 11
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_ffi as gen
    funcs = {name: params for name, _, params in gen.c_functions(open(gen.HEADER).read())}
    assert len(funcs["molar_hip_search_contacts"]) == 7 and len(funcs["molar_hip_search_contacts_frames"]) == 11
    assert open(gen.OUT).read() == gen.render(gen.c_functions(open(gen.HEADER).read())), "run python tools/gen_rust_ffi.py"
    hpp = open(os.path.join(ROOT, "include", "molar_hip.hpp")).read()
    assert "struct ContactMap" in hpp and "molar_hip_search_contacts_frames(" in hpp
    # the repr(C) struct of the Rust shim has the header's fields, in order
    rs = open(os.path.join(ROOT, "rust", "molar_hip", "src", "types.rs")).read()
    body = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*molar_hip_contact_groups\s*;", gen.strip_comments(open(gen.HEADER).read())).group(1)
    cfields = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    rbody = re.search(r"#\[repr\(C\)\]\n#\[derive\(Clone, Copy\)\]\npub struct MolarHipContactGroups\s*\{(.*?)\n\}", rs, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):", rbody) == cfields == ["group1", "ngroups1", "group2", "ngroups2"]
    lib_rs = open(os.path.join(ROOT, "rust", "molar_hip", "src", "lib.rs")).read()
    assert "pub fn contacts_single(" in lib_rs and "pub fn contacts_double(" in lib_rs
    import ctypes as C
    assert C.sizeof(_lib.ContactGroups) == 4 * C.sizeof(C.c_void_p)


N, CUTOFF = 600, 0.45


@pytest.fixture(scope="module")
def frame():
    box = synth.box_ortho(N)                    # L = 1.817 nm: 4 cells per dimension at 0.45, a complete grid, no duplicates
    return box, synth.frame(N, box, 1)          # (frame 0 has a pair 7.5e-7 nm from the cutoff: see brute_pairs)


def brute_pairs(pos1, pos2, L, same):
    """Minimum-image pairs of an orthorhombic box in double precision.  The list decides in f32: a coordinate difference, the
    box products of a wrapped pair and the sum of squares each carry a few 2^-24 relative errors on lengths of up to the box
    edge (1.8 nm), some 5e-7 nm on a distance - a pair closer than 1e-6 nm to the cutoff would make the comparison meaningless."""
    d = pos2[None, :, :].astype(np.float64) - pos1[:, None, :].astype(np.float64)
    d -= L * np.round(d / L)
    r = np.sqrt((d * d).sum(-1))
    if same:
        r[np.tril_indices(len(pos1))] = np.inf
    assert not np.any(np.abs(r - CUTOFF) < 1e-6), "a pair sits on the cutoff: the f32 list and the f64 brute force may differ"
    return np.nonzero(r <= CUTOFF)


def test_single_folding_is_the_brute_force(orc32, frame):
    box, pos = frame
    ref = orc32.search_single_pbc(CUTOFF, pos, orc32.box_from_matrix(box), 7)
    assert min(ref["dims"]) >= 3
    g = (np.arange(N) // 3).astype(np.uint32)
    G = int(g.max()) + 1
    count, deg, m = cr.single(ref, N, g, G)
    bi, bj = brute_pairs(pos, pos, float(box[0, 0]), True)
    assert count == len(bi) > 0
    bdeg = np.bincount(bi, minlength=N) + np.bincount(bj, minlength=N)
    assert np.array_equal(deg, bdeg.astype(np.uint64))
    bm = np.zeros((G, G), np.uint64)
    np.add.at(bm, (g[bi].astype(np.int64), g[bj].astype(np.int64)), 1)          # bi < bj and labels ascend: already [min][max]
    assert np.array_equal(m, bm)
    assert deg.sum() == 2 * count and m.sum() == count
    assert not np.any(np.tril(m, -1))


def test_double_folding_is_the_brute_force(orc32, frame):
    box, pos = frame
    i1, i2 = np.arange(0, 350), np.arange(250, N)
    ref = orc32.search_double_pbc(CUTOFF, pos[i1], pos[i2], orc32.box_from_matrix(box), 7)
    g1, G1 = cr.ragged_labels(len(i1), seed=3)
    g2, G2 = cr.ragged_labels(len(i2), seed=4)
    count, deg1, deg2, m = cr.double(ref, len(i1), len(i2), g1, G1, g2, G2)
    bi, bj = brute_pairs(pos[i1], pos[i2], float(box[0, 0]), False)
    # the two-set list repeats cross pairs of atoms that share a cell (both halves of the entry find them); the atoms the two
    # selections share are at distance 0 of themselves, and everything the brute force finds is in the list at least once
    got = set(zip(ref["i"].tolist(), ref["j"].tolist()))
    assert got == set(zip(bi.tolist(), bj.tolist()))
    assert deg1.sum() == count and deg2.sum() == count and m.sum() == count
    assert count >= len(bi)
    occ = cr.occupancy([m, np.zeros_like(m), m])
    assert np.array_equal(occ, 2 * (m > 0))
