"""Connected components without a GPU: the ABI of the two entries, the scipy folding of the oracle's list
(tests/clusters_ref.py) against an O(N^2) minimum-image brute force with a union-find of its own, and - on the reference
alone - the conditions that make the cases of tests/test_gpu_clusters.py worth comparing: a GPU test cannot pass there on a
trivial partition."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clusters_ref as cl  # noqa: E402

from molar_amd import synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("molar_hip_search_clusters", "molar_hip_search_clusters_frames")


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
    assert len(_lib.SYMBOLS["molar_hip_search_clusters"][1]) == 8
    assert len(_lib.SYMBOLS["molar_hip_search_clusters_frames"][1]) == 10
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_ffi as gen
    funcs = {name: params for name, _, params in gen.c_functions(open(gen.HEADER).read())}
    assert len(funcs["molar_hip_search_clusters"]) == 8 and len(funcs["molar_hip_search_clusters_frames"]) == 10
    assert open(gen.OUT).read() == gen.render(gen.c_functions(open(gen.HEADER).read())), "run python tools/gen_rust_ffi.py"
    hpp = open(os.path.join(ROOT, "include", "molar_hip.hpp")).read()
    assert "inline Clusters clusters(" in hpp and "inline void clusters_frames(" in hpp
    assert "molar_hip_search_clusters(" in hpp and "molar_hip_search_clusters_frames(" in hpp
    lib_rs = open(os.path.join(ROOT, "rust", "molar_hip", "src", "lib.rs")).read()
    assert "pub fn clusters(" in lib_rs and "fns.search_clusters)" in lib_rs
    import molar_amd.api as a
    assert hasattr(a.Engine, "search_clusters") and hasattr(a.Engine, "search_clusters_frames")
    assert hasattr(a, "clusters") and hasattr(a.Sel, "split_clusters") and hasattr(a.Clusters, "split")


# ---------------------------------------------------------------- the folding against a brute force

def brute_components(pos, L, cutoff, g=None, G=0):
    """comp_of by an O(N^2) minimum-image adjacency (orthorhombic box, double precision) and a plain union-find"""
    d = pos[None, :, :].astype(np.float64) - pos[:, None, :].astype(np.float64)
    d -= L * np.round(d / L)
    r = np.sqrt((d * d).sum(-1))
    r[np.tril_indices(len(pos))] = np.inf
    assert not np.any(np.abs(r - cutoff) < 1e-6), "a pair sits on the cutoff: the f32 list and the f64 brute force may differ"
    P = len(pos) if g is None else G
    parent = list(range(P))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i, j in zip(*np.nonzero(r <= cutoff)):
        a, b = (int(i), int(j)) if g is None else (int(g[i]), int(g[j]))
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return cl.canonical([find(p) for p in range(P)])


@pytest.mark.parametrize("cutoff", [0.21, 0.45])
def test_folding_is_the_brute_force(orc32, cutoff):
    n = 600
    box = synth.box_ortho(n)
    pos = synth.frame(n, box, 1)
    ref = orc32.search_single_pbc(cutoff, pos, orc32.box_from_matrix(box), 7)
    C, comp_of, sizes, offsets, members = cl.components(ref, n)
    want = brute_components(pos, float(box[0, 0]), cutoff)
    assert np.array_equal(comp_of, want) and C == int(want.max()) + 1
    assert cutoff != 0.21 or 8 < C < n          # structure at the small cutoff (one component at the large one)
    assert int(sizes.sum()) == n and np.array_equal(sizes, np.bincount(comp_of))
    assert offsets[0] == 0 and np.array_equal(np.diff(offsets.astype(np.int64)), sizes)
    for k in range(C):
        assert np.array_equal(members[int(offsets[k]):int(offsets[k + 1])], np.nonzero(comp_of == k)[0])
    first = [int(members[int(offsets[k])]) for k in range(C)]
    assert first == sorted(first) and first[0] == 0
    # groups: ragged labels, and more groups than labels (the empty ones are singletons at the end)
    g = (np.arange(n) // 3).astype(np.uint32)
    G = int(g.max()) + 1 + 5
    Cg, comp_g, sizes_g, _, _ = cl.components(ref, n, g, G)
    assert np.array_equal(comp_g, brute_components(pos, float(box[0, 0]), cutoff, g, G))
    assert np.array_equal(comp_g[-5:], np.arange(Cg - 5, Cg)) and np.all(sizes_g[-5:] == 1)


# ---------------------------------------------------------------- the inputs of the GPU tests, on the reference alone

@pytest.mark.parametrize("case", cl.CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[3]}")
def test_structured_cases_have_structure(orc32, case):
    boxname, n, _, cutoff, pbc = case
    pos, _, ref = cl.case_ref(orc32, case)
    many, singles, largest, across = cl.conditions(pos, ref, n, cutoff)
    assert many >= 8 and singles >= 1 and largest >= 65, (many, singles, largest)
    if pbc:
        assert across >= 1, across


def test_blob_frame_is_what_it_was_built_to_be(orc32):
    pos, box, lab = cl.blob_frame()
    assert len(pos) <= 600
    ref = orc32.search_single_pbc(cl.BLOB_CUTOFF, pos, orc32.box_from_matrix(box), 7)
    assert max(ref["dims"]) <= 3
    C, comp_of, sizes, _, _ = cl.components(ref, len(pos))
    assert C == 6 and np.array_equal(comp_of, cl.canonical(lab))
    assert sorted(sizes.tolist()) == [60, 60, 60, 60, 122, 123]
    # blobs 2 and 3 hang together only through the bridge across the face z = 0
    i, j = ref["i"].astype(np.int64), ref["j"].astype(np.int64)
    inside = np.linalg.norm(pos[i].astype(np.float64) - pos[j].astype(np.float64), axis=1) <= cl.BLOB_CUTOFF * 1.001
    assert cl.components((i[inside], j[inside]), len(pos))[0] > C


def test_chains_are_what_they_were_built_to_be(orc32):
    box = np.diag(cl.CHAIN_BOX).astype(np.float32)
    ob = orc32.box_from_matrix(box)
    whole = cl.chain()
    assert whole.shape == (cl.CHAIN_N, 3)
    ref = orc32.search_single_pbc(cl.CHAIN_CUTOFF, whole, ob, 7)
    C, _, _, _, _ = cl.components(ref, cl.CHAIN_N)
    assert C == 1 and len(ref["i"]) == cl.CHAIN_N - 1         # the bonds and nothing else: the graph is a path
    cut = cl.chain(cut_from=64)
    C, _, sizes, _, _ = cl.components(orc32.search_single_pbc(cl.CHAIN_CUTOFF, cut, ob, 7), cl.CHAIN_N)
    assert C >= 8 and np.any(sizes == 64) and np.any(sizes == 65) and np.any(sizes > 65), sizes      # both sides of the wave width


def test_lattice_has_no_pair(orc32):
    pos, box = cl.lattice()
    ref = orc32.search_single_pbc(0.3, pos, orc32.box_from_matrix(box), 7)
    assert len(ref["i"]) == 0
