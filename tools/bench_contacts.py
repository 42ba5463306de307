#!/usr/bin/env python
"""The fused contact counts (molar_hip_search_contacts / _frames) against the route a caller had before them: the resident
pair list (molar_hip_search_resident with the (i, j) plane only, local ids), torch.bincount of both columns for the degrees
and a torch.bincount of g[i] * G + g[j] for the map.  Inputs and outputs stay in device memory.  Beside each row: the fused
histogram of the same frame (what the bare fused pair loop costs).

Shapes, all box A:  (a) 250k atoms, rc 1.2, degrees only;  (b) a 60k-atom selection of that frame, rc 0.8, labels pos // 15
(4000 groups), degrees and map;  (c) two disjoint 60k-atom selections, same labels, two-set search;  (d) 64 frames of (b)
through the frames form with occupancy, against 64 runs of the list route plus the same fold;  (e) 1M atoms, rc 1.2, degrees.

Timing: a warm-up, then `reps` repetitions, each bracketed by a pair of events on torch's stream - the first recorded after a
device-wide synchronisation, the second after the engine's stream has been waited for - median and minimum in ms.
The results of the two routes are compared before anything is timed.  One JSON line per shape.
Usage: python tools/bench_contacts.py [reps] [shapes, e.g. abc]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from molar_amd import api, build, synth
    build.build_library()
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    shapes = sys.argv[2] if len(sys.argv) > 2 else "abcde"
    eng = api.Engine(0)
    eng.search_resident_planes(False)

    def timeit(fn, n=reps):
        fn()                                        # warm-up (buffers grow here)
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            eng.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            eng.synchronize()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts = np.array(ts)
        return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(ts.min()), 4), "max_ms": round(float(ts.max()), 4)}

    def list_route(kind, rc, x1, i1, x2, i2, box, n1, n2, g1, g2, G):
        """degrees (and the map) out of the resident list; returns (count, deg1, deg2 or None, map or None)"""
        cnt, pa, _ = eng.search_resident(kind, rc, x1, i1, x2, i2, box=box, pbc=7, ids_local=True)
        p = api.device_view(pa, (cnt, 2), torch.int32)
        i, j = p[:, 0], p[:, 1]
        if kind == api.SEARCH_SINGLE:
            deg1, deg2 = torch.bincount(i, minlength=n1) + torch.bincount(j, minlength=n1), None
        else:
            deg1, deg2 = torch.bincount(i, minlength=n1), torch.bincount(j, minlength=n2)
        m = None
        if g1 is not None:
            a, b = g1[i.long()], g2[j.long()]
            if kind == api.SEARCH_SINGLE:
                a, b = torch.minimum(a, b), torch.maximum(a, b)
            m = torch.bincount(a * G + b, minlength=G * G).view(G, G)
        return cnt, deg1, deg2, m

    def hist_time(kind, rc, x1, i1, x2, i2, box):
        bins = torch.zeros(1200, dtype=torch.int64, device="cuda")
        return timeit(lambda: eng.search_histogram(kind, rc, 0.0, rc, 1200, x1, i1, x2, i2, box=box, pbc=7, bins=bins, want_count=False))

    def one_frame(tag, n, rc, kind, sel1, sel2, labels):
        box = synth.box_a(n)
        x = torch.from_numpy(synth.frame(n, box)).cuda()
        i1 = None if sel1 is None else torch.from_numpy(sel1.astype(np.int64)).cuda()
        i2 = None if sel2 is None else torch.from_numpy(sel2.astype(np.int64)).cuda()
        n1 = n if sel1 is None else len(sel1)
        n2 = 0 if sel2 is None else len(sel2)
        two = kind == api.SEARCH_DOUBLE
        x2 = x if two else None
        G = 0
        g32 = g64 = None
        if labels:
            G = (max(n1, n2) + 14) // 15
            g64 = (torch.arange(max(n1, n2), device="cuda") // 15)
            g32 = g64.to(torch.int32)
        deg1 = torch.zeros(n1, dtype=torch.int64, device="cuda")
        deg2 = torch.zeros(n2, dtype=torch.int64, device="cuda") if two else None
        cmap = torch.zeros((G, G), dtype=torch.int64, device="cuda") if labels else None

        def fused():
            eng.search_contacts(kind, rc, x, i1, x2, i2, box=box, pbc=7, group1=None if g32 is None else g32[:n1], ngroups1=G,
                                group2=None if (g32 is None or not two) else g32[:n2], ngroups2=G, deg1=deg1, deg2=deg2, cmap=cmap,
                                want_map=labels, want_count=False)

        def lists():
            return list_route(kind, rc, x, i1, x2, i2, box, n1, n2, None if g64 is None else g64[:n1], None if g64 is None else g64[:max(n2, n1)], G)

        fused()
        eng.synchronize()
        cnt, l1, l2, lm = lists()
        same = bool(torch.equal(deg1, l1)) and (l2 is None or bool(torch.equal(deg2, l2))) and (lm is None or bool(torch.equal(cmap, lm)))
        row = {"shape": tag, "atoms": n, "n1": n1, "n2": n2, "cutoff": rc, "groups": G, "entries": int(cnt), "results_equal": same,
               "fused": timeit(fused), "list_route": timeit(lists), "fused_histogram": hist_time(kind, rc, x, i1, x2, i2, box)}
        row["speedup_median"] = round(row["list_route"]["median_ms"] / row["fused"]["median_ms"], 3)
        print(json.dumps(row), flush=True)

    rng = np.random.default_rng(5)
    n = 250_000
    perm = rng.permutation(n)
    selb = np.sort(perm[:60_000])
    selc = np.sort(perm[60_000:120_000])
    if "a" in shapes:
        one_frame("a", n, 1.2, api.SEARCH_SINGLE, None, None, False)
    if "b" in shapes:
        one_frame("b", n, 0.8, api.SEARCH_SINGLE, selb, None, True)
    if "c" in shapes:
        one_frame("c", n, 0.8, api.SEARCH_DOUBLE, selb, selc, True)
    if "d" in shapes:
        nf, rc = 64, 0.8
        box = synth.box_a(n)
        frames = torch.from_numpy(np.stack([synth.frame(n, box, f) for f in range(nf)])).cuda()
        i1 = torch.from_numpy(selb.astype(np.int64)).cuda()
        n1 = len(selb)
        G = (n1 + 14) // 15
        g64 = torch.arange(n1, device="cuda") // 15
        g32 = g64.to(torch.int32)
        deg = torch.zeros(n1, dtype=torch.int64, device="cuda")
        cmap = torch.zeros((G, G), dtype=torch.int64, device="cuda")
        occ = torch.zeros((G, G), dtype=torch.int32, device="cuda")

        def fused():
            eng.search_contacts_frames(api.SEARCH_SINGLE, rc, frames, idx1=i1, box=box, pbc=7, group1=g32, ngroups1=G, deg1=deg, cmap=cmap, occupancy=occ)

        def lists():
            d = torch.zeros(n1, dtype=torch.int64, device="cuda")
            m = torch.zeros((G, G), dtype=torch.int64, device="cuda")
            o = torch.zeros((G, G), dtype=torch.int32, device="cuda")
            for f in range(nf):
                _, d1, _, mf = list_route(api.SEARCH_SINGLE, rc, frames[f], i1, None, None, box, n1, 0, g64, g64, G)
                d += d1
                m += mf
                o += (mf > 0).to(torch.int32)
            return d, m, o

        fused()
        eng.synchronize()
        d, m, o = lists()
        same = bool(torch.equal(deg, d) and torch.equal(cmap, m) and torch.equal(occ, o))
        hb = torch.zeros(1200, dtype=torch.int64, device="cuda")
        row = {"shape": "d", "atoms": n, "n1": n1, "frames": nf, "cutoff": rc, "groups": G, "entries": int(m.sum()), "results_equal": same,
               "fused": timeit(fused, max(reps // 4, 5)), "list_route": timeit(lists, max(reps // 4, 5)),
               "fused_histogram": timeit(lambda: eng.search_histogram_frames(api.SEARCH_SINGLE, rc, 0.0, rc, 1200, frames, idx1=i1, box=box, pbc=7, bins=hb),
                                         max(reps // 4, 5))}
        row["speedup_median"] = round(row["list_route"]["median_ms"] / row["fused"]["median_ms"], 3)
        print(json.dumps(row), flush=True)
        del frames
    if "e" in shapes:
        one_frame("e", 1_000_000, 1.2, api.SEARCH_SINGLE, None, None, False)


if __name__ == "__main__":
    main()
