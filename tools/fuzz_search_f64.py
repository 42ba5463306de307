#!/usr/bin/env python
"""Randomised differential test of the f64 drivers (search_f64.hip: grid by stable radix sort, plan, bounding-box row pruning,
adjacent-image classification of entries across the boundary, LDS output queue) against the f64 build of the CPU oracle: random
boxes (orthorhombic, sheared, strongly triclinic, flat, tiny, large with >= 4 cells per dimension), cutoffs, densities,
periodicity masks, selections, all four kinds, coordinates from host arrays or resident in HBM, atoms outside the cell, pairs
planted at the cutoff edge across the periodic boundary, local ids, NaN and (with a box) infinite coordinates, NaN radii, empty
selections, cells of more than 256 atoms.  Every case must be bit-identical (ids, order, distances).
run(ncases, seed) returns the counts of cases, failures, cases skipped because the oracle refuses the box, and cases with full
periodicity and >= 4 cells in every dimension (where entries across the boundary are classified by the adjacent image).
Usage: python tools/fuzz_search_f64.py [ncases] [seed]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def random_box(rng):
    kind = rng.integers(0, 7)
    L = rng.uniform(1.5, 6.0, 3)
    if kind == 0:
        m = np.diag(L)
    elif kind == 1:
        m = np.diag(L); m[0, 2] = -rng.uniform(0, 0.3) * L[0]; m[1, 2] = -rng.uniform(0, 0.3) * L[1]
    elif kind == 2:
        m = np.diag(L); m[0, 1] = rng.uniform(-0.5, 0.5) * L[0]; m[0, 2] = rng.uniform(-0.5, 0.5) * L[0]; m[1, 2] = rng.uniform(-0.5, 0.5) * L[1]
    elif kind == 3:
        m = np.diag(L) + rng.uniform(-0.3, 0.3, (3, 3)) * L.min()
    elif kind == 4:
        m = np.diag([L[0] * 2, L[1] * 2, rng.uniform(0.6, 1.2)])
    elif kind == 5:
        m = np.diag(rng.uniform(0.7, 1.6, 3))
    else:                                             # roomy: several cells per dimension even at large cutoffs
        m = np.diag(rng.uniform(5.0, 9.0, 3)); m[0, 1] = rng.uniform(-0.3, 0.3) * m[0, 0]; m[1, 2] = rng.uniform(-0.3, 0.3) * m[1, 1]
    return m.astype(np.float64)


def first_difference(got, ref):
    """Index of the first entry in which two (i, j, d) lists differ (the shorter length if one is a prefix of the other)."""
    n = min(len(got[0]), len(ref[0]))
    bad = np.zeros(n, bool)
    for g, r in zip(got, ref):
        bad |= ~((g[:n] == r[:n]) | ((g[:n] != g[:n]) & (r[:n] != r[:n])))
    return int(np.argmax(bad)) if bad.any() else n


def run(ncases=200, seed=1, eng=None, verbose=True):
    """`eng`: an Engine (made here if None).  An object with `host_only = True` gets numpy inputs only (a stand-in for the
    engine in a test of the generator itself)."""
    from oracle.oracle import Oracle
    if eng is None:
        from molar_amd import api, build
        build.build_library()
        eng = api.Engine(0)
    host_only = bool(getattr(eng, "host_only", False))
    SINGLE, DOUBLE, WITHIN, VDW = 0, 1, 2, 3                      # molar_amd.api.SEARCH_*
    o = Oracle("f64")
    rng = np.random.default_rng(seed)
    stats = {"cases": ncases, "fails": 0, "skipped": 0, "full_pbc_4cells": 0, "cells_above_256": 0, "empty": 0}

    def fail(what, tag, *more):
        stats["fails"] += 1
        print(what, tag, *more)
    for case in range(ncases):
        box = random_box(rng)
        vol = abs(np.linalg.det(box))
        dens = rng.choice([20.0, 60.0, 100.0, 300.0, 800.0])      # 800: cells of more than 256 atoms (the chunk loop)
        n = int(min(max(vol * dens, 30), 8000))
        pos = rng.random((n, 3)) @ box.T + rng.normal(0, rng.choice([0.0, 0.05, 0.5]), (n, 3))
        rc = float(rng.uniform(0.25, 0.9 if dens == 800.0 else 1.3))
        if rng.random() < 0.4 and n >= 200:
            # pairs planted at rc * (1 +- 1e-16 .. 1e-8) around atoms next to the faces of the cell
            k = n // 5
            frac = rng.random((k, 3))
            frac[np.arange(k), rng.integers(0, 3, k)] = rng.choice([0.0, 1.0], k) + rng.normal(0, 0.01, k)
            pa = frac @ box.T
            u = rng.normal(size=(k, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
            e = 10.0 ** rng.uniform(-16.0, -8.0, k) * rng.choice([-1.0, 1.0], k)
            pos[:k] = pa
            pos[k:2 * k] = pa + rc * (1.0 + e)[:, None] * u
        pbc = int(rng.choice([7, 7, 7, 0, 1, 2, 3, 4, 5, 6]))
        kind = int(rng.choice([SINGLE, SINGLE, SINGLE, DOUBLE, DOUBLE, WITHIN, VDW]))
        if rng.random() < 0.1:
            pos[rng.integers(0, n)] = np.nan                      # an atom that pairs with nothing
        if rng.random() < 0.1 and pbc:                            # (without a box an infinite coordinate makes the zero-seeded
            pos[rng.integers(0, n), rng.integers(0, 3)] = rng.choice([np.inf, -np.inf])      # bounding box, so the grid, infinite)
        resident = bool(rng.random() < 0.5) and not host_only
        local = bool(rng.random() < 0.25)
        empty = int(rng.choice([0, 0, 0, 0, 0, 0, 0, 0, 1, 2]))  # 1 / 2: the first / second selection is empty (not for vdW:
        nan_radii = bool(rng.random() < 0.3)                      # the reference unwrap()s the maximum of no radii)
        try:
            ob = o.box_from_matrix(box)
        except Exception:
            stats["skipped"] += 1
            continue
        tag = (f"case {case}: kind {kind} n {n} rc {rc!r} pbc {pbc} resident {resident} ids_local {local} empty {empty} "
               f"box {box.tolist()}")
        if resident:
            import torch
        xyz = torch.from_numpy(pos).cuda() if resident else pos

        def dev(a):
            if not resident or a is None:
                return a
            return torch.from_numpy(a.astype(np.int64) if a.dtype == np.uint64 else a).cuda()

        def ref_ids(idx):                                         # local ids: the reference's own numbering of a selection
            return None if local else idx
        try:
            kw = dict(box=box, pbc=pbc) if pbc else {}
            if kind == SINGLE:
                idx = None if rng.random() < 0.5 else np.sort(rng.choice(n, max(n // 2, 2), replace=False)).astype(np.uint64)
                if empty:
                    idx = np.zeros(0, np.uint64)
                p = pos if idx is None else pos[idx.astype(int)]
                ref = o.search_single_pbc(rc, p, ob, pbc, ids=ref_ids(idx), nthreads=4) if pbc else o.search_single(rc, p, ids=ref_ids(idx), nthreads=4)
                got = eng.search_f64(SINGLE, rc, xyz, dev(idx), ids_local=local, **kw)
            elif kind in (DOUBLE, VDW):
                perm = rng.permutation(n)
                i1 = np.sort(perm[: n // 3]).astype(np.uint64); i2 = np.sort(perm[n // 3:]).astype(np.uint64)
                if kind == DOUBLE and empty == 1:
                    i1 = np.zeros(0, np.uint64)
                if kind == DOUBLE and empty == 2:
                    i2 = np.zeros(0, np.uint64)
                p1, p2 = pos[i1.astype(int)], pos[i2.astype(int)]
                if kind == DOUBLE:
                    ref = o.search_double_pbc(rc, p1, p2, ob, pbc, ids1=ref_ids(i1), ids2=ref_ids(i2), nthreads=4) if pbc \
                        else o.search_double(rc, p1, p2, ids1=ref_ids(i1), ids2=ref_ids(i2), nthreads=4)
                    got = eng.search_f64(DOUBLE, rc, xyz, dev(i1), xyz, dev(i2), ids_local=local, **kw)
                else:
                    v1 = rng.uniform(0.1, 0.25, len(i1)); v2 = rng.uniform(0.1, 0.25, len(i2))
                    if nan_radii:                                 # ignored by the maximum that sizes the grid; never a hit
                        v1[rng.random(len(v1)) < 0.05] = np.nan
                        v2[::64] = np.nan
                        v1[-1] = v2[-1] = 0.2
                    ref = o.search_double_vdw_pbc(p1, p2, v1, v2, ob, pbc, nthreads=4) if pbc else o.search_double_vdw(p1, p2, v1, v2, nthreads=4)
                    got = eng.search_f64(VDW, None, xyz, dev(i1), xyz, dev(i2), vdw1=dev(v1), vdw2=dev(v2), **kw)
            else:
                i1 = np.arange(n, dtype=np.uint64); i2 = np.sort(rng.choice(n, max(n // 20, 1), replace=False)).astype(np.uint64)
                if empty == 1:
                    i1 = np.zeros(0, np.uint64)
                if empty == 2:
                    i2 = np.zeros(0, np.uint64)
                p1, p2 = pos[i1.astype(int)], pos[i2.astype(int)]
                if pbc:
                    ref = o.search_within_pbc(rc, p1, p2, ob, pbc, ref_ids(i1), ref_ids(i2), nthreads=4)
                    ids = eng.search_f64(WITHIN, rc, xyz, dev(i1), xyz, dev(i2), box=box, pbc=pbc, ids_local=local)
                else:
                    fin = pos[np.isfinite(pos).all(1)]
                    lo = np.minimum(fin.min(0), 0.0) - (rc + 2.220446049250313e-16); up = np.maximum(fin.max(0), 0.0) + (rc + 2.220446049250313e-16)
                    ref = o.search_within(rc, p1, p2, lo, up, ref_ids(i1), ref_ids(i2), nthreads=4)
                    ids = eng.search_f64(WITHIN, rc, xyz, dev(i1), xyz, dev(i2), lower=lo, upper=up, ids_local=local)
                got = (ids,)
            want = (ref["i"],) if kind == WITHIN else (ref["i"], ref["j"], ref["d"])
            if pbc == 7 and min(ref["dims"]) >= 4:
                stats["full_pbc_4cells"] += 1
            stats["cells_above_256"] += int(n / float(np.prod(ref["dims"])) > 256.0)
            stats["empty"] += int(len(ref["i"]) == 0)
            ok = len(got[0]) == len(want[0]) and all(np.array_equal(g, w) for g, w in zip(got, want))
            if not ok:
                fail("MISMATCH", tag, len(got[0]), len(want[0]), "first difference at", first_difference(got, want), "dims", ref["dims"])
        except Exception as exc:      # an engine error on a case the oracle accepts is a failure too
            fail("ERROR", tag, repr(exc))
    if verbose:
        print(f"{ncases} cases, {stats['fails']} failures, {stats['skipped']} skipped, {stats['full_pbc_4cells']} with full periodicity "
              f"and >= 4 cells per dimension, {stats['cells_above_256']} with more than 256 atoms per cell, {stats['empty']} empty results")
    return stats


def main():
    ncases = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    return 1 if run(ncases, seed)["fails"] else 0


if __name__ == "__main__":
    sys.exit(main())
