"""What molar_hip_search_contacts has to give, folded by numpy from the ORACLE's pair list (ids = positions in the
selections).  Nothing here touches the code under test.

    single(ref, n, g, G)            -> count, deg[n], map[G, G] (upper triangle)
    double(ref, n1, n2, g1, G1, g2, G2) -> count, deg1[n1], deg2[n2], map[G1, G2]
    occupancy(maps)                 -> frames in which each entry of the per-frame maps is non-zero

`ref` is what Oracle.search_single(_pbc) / search_double(_pbc) return: {"i": ..., "j": ...}.  The list keeps the
reference's duplicates (same-cell cross pairs of the two-set search, repeated cell pairs of tiny periodic grids), and so do
these counts.
"""
import numpy as np


def single(ref, n, g=None, G=0):
    i = ref["i"].astype(np.int64)
    j = ref["j"].astype(np.int64)
    count = len(i)
    deg = (np.bincount(i, minlength=n) + np.bincount(j, minlength=n)).astype(np.uint64)
    m = None
    if g is not None:
        g = np.asarray(g, np.int64)
        gi, gj = g[i], g[j]
        m = np.zeros((G, G), np.uint64)
        np.add.at(m, (np.minimum(gi, gj), np.maximum(gi, gj)), 1)
    return count, deg, m


def double(ref, n1, n2, g1=None, G1=0, g2=None, G2=0):
    i = ref["i"].astype(np.int64)
    j = ref["j"].astype(np.int64)
    count = len(i)
    deg1 = np.bincount(i, minlength=n1).astype(np.uint64)
    deg2 = np.bincount(j, minlength=n2).astype(np.uint64)
    m = None
    if g1 is not None:
        g1 = np.asarray(g1, np.int64)
        g2 = np.asarray(g2, np.int64)
        m = np.zeros((G1, G2), np.uint64)
        np.add.at(m, (g1[i], g2[j]), 1)
    return count, deg1, deg2, m


def occupancy(maps):
    occ = np.zeros(maps[0].shape, np.uint32)
    for m in maps:
        occ += (m > 0).astype(np.uint32)
    return occ


def ragged_labels(n, seed=7, lo=1, hi=40):
    """Labels of consecutive groups of ragged sizes lo..hi; returns (labels[n] uint32, number of groups)."""
    rng = np.random.default_rng(seed)
    sizes = []
    while sum(sizes) < n:
        sizes.append(int(rng.integers(lo, hi + 1)))
    lab = np.repeat(np.arange(len(sizes)), sizes)[:n].astype(np.uint32)
    return lab, int(lab.max()) + 1
