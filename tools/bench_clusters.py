#!/usr/bin/env python
"""Connected components of the contact graph (molar_hip_search_clusters / _frames) against the two routes a caller had before:
  (a) the resident pair list (molar_hip_search_resident, (i, j) plane only, local ids), then min-label propagation in torch:
      labels = arange(P); every round takes, per particle, the smallest label among itself and its neighbours
      (scatter_reduce amin over both columns) and jumps pointers (labels = labels[labels]) until nothing changes;
  (b) the resident list copied to the host, then scipy.sparse.csgraph.connected_components.
Inputs stay in device memory; route (b) ends on the host by its nature.  The three routes are run in turn inside every
repetition (alternated), after a warm-up; median, minimum and maximum of `reps` repetitions in ms.  The partitions of the
three routes are compared before anything is timed.  Beside each row: the contacts call of the same request with no output but
the count (the same pair loop with "add one" in place of "unite"), and the union-find's counters per hit of the pair loop
(molar_hip_search_clusters_counters: hits that reach the forest, compare-and-swaps, path-shortening atomic minima).

Shapes, all box A at 100 atoms / nm^3:  (a) 1M atoms, rc 0.35: one giant component;  (b) 16 % of those atoms (the density at
which rc 0.35 has the mean degree of rc 0.19 at full density: the percolation threshold, components of every size);
(c) 200k atoms of a 500k-atom frame as 4000 groups of 50 atoms that sit together (lipid-like), rc 0.6;  (d) 64 frames of 100k
atoms, rc 0.19, through the frames form, against 64 runs of each other route.
One JSON line per shape.  Usage: python tools/bench_clusters.py [reps] [shapes, e.g. abc]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from molar_amd import api, build, synth
    build.build_library()
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    shapes = sys.argv[2] if len(sys.argv) > 2 else "abcd"
    eng = api.Engine(0)
    eng.search_resident_planes(False)

    def alternated(routes, n=reps):
        """{name: fn} -> {name: stats}; one repetition runs every route once, in turn.  The host-side route leaves the device
        idle for tenths of a second and whatever is timed next would pay for its clocks coming back up: an untimed run of the
        first route goes in front of every timed call."""
        for fn in routes.values():
            fn()                                    # warm-up (buffers grow here)
        wake = next(iter(routes.values()))
        ts = {k: [] for k in routes}
        for _ in range(n):
            for k, fn in routes.items():
                wake()
                torch.cuda.synchronize()
                eng.synchronize()
                t0 = time.perf_counter()
                fn()
                eng.synchronize()
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        return {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4), "max_ms": round(float(np.max(v)), 4)}
                for k, v in ts.items()}

    def pair_list(rc, x, idx, box):
        cnt, pa, _ = eng.search_resident(api.SEARCH_SINGLE, rc, x, idx, box=box, pbc=7, ids_local=True)
        p = api.device_view(pa, (cnt, 2), torch.int32)
        return p[:, 0].long(), p[:, 1].long()

    def torch_route(rc, x, idx, box, P, g):
        i, j = pair_list(rc, x, idx, box)
        if g is not None:
            i, j = g[i], g[j]
        lab = torch.arange(P, device="cuda")
        while True:
            new = lab.scatter_reduce(0, i, lab[j], "amin").scatter_reduce(0, j, lab[i], "amin")
            new = new[new]
            if torch.equal(new, lab):
                return lab
            lab = new

    def scipy_route(rc, x, idx, box, P, g):
        i, j = pair_list(rc, x, idx, box)
        i, j = i.cpu().numpy(), j.cpu().numpy()
        if g is not None:
            gh = g.cpu().numpy()
            i, j = gh[i], gh[j]
        return connected_components(coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(P, P)), directed=False)

    def canonical_roots(comp_of):
        """smallest member of every particle's component, from the engine's comp_of"""
        comp_of = comp_of.long()
        first = torch.full((int(comp_of.max()) + 1,), comp_of.numel(), device="cuda", dtype=torch.long)
        first = first.scatter_reduce(0, comp_of, torch.arange(comp_of.numel(), device="cuda"), "amin")
        return first[comp_of]

    def one_frame(tag, n, rc, sel, group_size):
        box = synth.box_a(n)
        pos = synth.frame(n, box)
        x = torch.from_numpy(pos).cuda()
        idx = None if sel is None else torch.from_numpy(sel.astype(np.int64)).cuda()
        nsel = n if sel is None else len(sel)
        g32 = g64 = None
        P = nsel
        if group_size:
            P = (nsel + group_size - 1) // group_size
            g64 = torch.arange(nsel, device="cuda") // group_size
            g32 = g64.to(torch.int32)

        def fused():
            return eng.search_clusters(rc, x, idx, box=box, pbc=7, group=g32, ngroups=P, want_members=False)

        c = fused()
        want = torch_route(rc, x, idx, box, P, g64)                  # min-label propagation ends at the smallest member
        C_scipy, _ = scipy_route(rc, x, idx, box, P, g64)
        same = bool(torch.equal(canonical_roots(c.comp_of), want)) and C_scipy == c.ncomponents
        eng.clusters_counters(True)
        fused()
        hits, reach, cas, amin = eng.clusters_counters(False)
        row = {"shape": tag, "atoms": n, "selected": nsel, "particles": P, "cutoff": rc, "components": c.ncomponents,
               "largest": int(c.sizes.max()), "results_equal": same, "hits": hits,
               "per_hit": {"reach_forest": round(reach / max(hits, 1), 5), "cas": round(cas / max(hits, 1), 5), "atomic_min": round(amin / max(hits, 1), 5)}}
        row.update(alternated({
            "fused": fused,
            "list_torch": lambda: torch_route(rc, x, idx, box, P, g64),
            "list_scipy": lambda: scipy_route(rc, x, idx, box, P, g64),
            "contacts_count_only": lambda: eng.search_contacts(api.SEARCH_SINGLE, rc, x, idx, box=box, pbc=7, want_deg=False, want_map=False),
        }))
        row["speedup_vs_torch"] = round(row["list_torch"]["median_ms"] / row["fused"]["median_ms"], 3)
        row["speedup_vs_scipy"] = round(row["list_scipy"]["median_ms"] / row["fused"]["median_ms"], 3)
        print(json.dumps(row), flush=True)

    rng = np.random.default_rng(5)
    if "a" in shapes:
        one_frame("a", 1_000_000, 0.35, None, 0)
    if "b" in shapes:
        one_frame("b", 1_000_000, 0.35, np.sort(rng.permutation(1_000_000)[:160_000]), 0)
    if "c" in shapes:
        # 200k atoms ordered along a coarse grid, so that 50 consecutive ones sit together like the atoms of a lipid
        n = 500_000
        pos = synth.frame(n, synth.box_a(n))
        pick = rng.permutation(n)[:200_000]
        cell = np.floor(pos[pick] / 1.2).astype(np.int64)
        sel = pick[np.lexsort((pos[pick, 2], cell[:, 1], cell[:, 0]))]
        one_frame("c", n, 0.6, sel, 50)          # (an unsorted index: positions in the selection are what the labels go by)
    if "d" in shapes:
        n, nf, rc = 100_000, 64, 0.19
        box = synth.box_a(n)
        frames = torch.from_numpy(np.stack([synth.frame(n, box, f) for f in range(nf)])).cuda()
        hist = torch.zeros(n + 1, dtype=torch.int64, device="cuda")

        def fused():
            return eng.search_clusters_frames(rc, frames, box=box, pbc=7, size_hist=hist)

        b = fused()
        ncomp = [int(torch.unique(torch_route(rc, frames[f], None, box, n, None)).numel()) for f in range(4)]
        same = ncomp == b.ncomponents[:4].tolist()
        row = {"shape": "d", "atoms": n, "frames": nf, "cutoff": rc, "components_frame0": int(b.ncomponents[0]), "largest_frame0": int(b.largest[0]),
               "results_equal": same}
        row.update(alternated({
            "fused": fused,
            "list_torch": lambda: [torch_route(rc, frames[f], None, box, n, None) for f in range(nf)],
            "list_scipy": lambda: [scipy_route(rc, frames[f], None, box, n, None) for f in range(nf)],
        }, max(reps // 4, 5)))
        row["speedup_vs_torch"] = round(row["list_torch"]["median_ms"] / row["fused"]["median_ms"], 3)
        row["speedup_vs_scipy"] = round(row["list_scipy"]["median_ms"] / row["fused"]["median_ms"], 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
