#!/usr/bin/env python
"""Hydrogen bonds (molar_hip_hbonds_counts + _fill, molar_hip_hbonds_frames) against the route a caller had before them: the
resident two-set list ((i, j) plane, local ids), torch f64 gathers of D, H and A for every hydrogen of the donor, minimum
image in the orthorhombic cell, the angle by atan2, the threshold, and torch.unique over the keys (hydrogen << 32 | acceptor).
Everything stays in device memory; the two routes are alternated repetition by repetition.

Shapes (rigid three-site waters on a jittered lattice at water density, orthorhombic cell, rc 0.35, DHA 150):
  (a) 1M atoms, every oxygen donor and acceptor;
  (b) the oxygens of the first 3334 waters (a 10k-atom solute's worth) as donors against all oxygens of the 1M-atom frame;
  (c) the reverse: all oxygens as donors, those 3334 as acceptors;
  (d) 64 frames of 100k atoms through the frames form with the bond table, against 64 runs of the list route plus
      torch.unique(return_inverse, return_counts) over the block.
Timing: a warm-up, then `reps` repetitions of each route in turn, each bracketed by events on torch's stream (the first after
a device-wide synchronisation, the second after the engine's stream has been waited for); median / min / max in ms.  The routes'
results are compared before anything is timed.  One JSON line per shape.
Usage: python tools/bench_hbonds.py [reps] [shapes, e.g. abcd] [--write[=PATH]] [--fused-only]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import hbonds_ref as hr
    from molar_amd import api, build, synth
    build.build_library()
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 20
    shapes = args[1] if len(args) > 1 else "abcd"
    fused_only = "--fused-only" in sys.argv
    write = [a for a in sys.argv[1:] if a.startswith("--write")]
    eng = api.Engine(0)
    eng.search_resident_planes(False)
    RC, ANGLE = 0.35, 150.0

    def span(fn):
        torch.cuda.synchronize()
        eng.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        eng.synchronize()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def stats(ts):
        ts = np.array(ts)
        return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(ts.min()), 4), "max_ms": round(float(ts.max()), 4)}

    def alternate(routes):
        for fn in routes.values():
            fn()                                    # warm-up (buffers grow here)
        ts = {k: [] for k in routes}
        for _ in range(reps):
            for k, fn in routes.items():
                ts[k].append(span(fn))
        return {k: stats(v) for k, v in ts.items()}

    def torch_keys(xyz, don, acc, hoff2, hidx, L):
        """the unique keys of one frame by the list route; hydrogens: exactly two per donor (hoff2 = 2 * position)"""
        cnt, pa, _ = eng.search_resident(api.SEARCH_DOUBLE, RC, xyz, don, xyz, acc, box=np.diag([L] * 3), pbc=7, ids_local=True)
        p = api.device_view(pa, (cnt, 2), torch.int32).long()
        i, j = p[:, 0].repeat_interleave(2), p[:, 1].repeat_interleave(2)
        h = 2 * i + torch.arange(2, device="cuda").repeat(cnt)
        D, H, A = don[i], hidx[h], acc[j]
        x = xyz.double()
        mi = lambda v: v - L * torch.round(v / L)
        u, v = mi(x[D] - x[H]), mi(x[A] - x[H])
        ang = torch.rad2deg(torch.atan2(torch.linalg.cross(u, v).norm(dim=1), (u * v).sum(1)))
        ok = (ang >= ANGLE) & (D != A)
        return torch.unique(h[ok] << 32 | j[ok])

    def frame(nw, seed):
        box = synth.box_ortho(3 * nw)
        return hr.waters(nw, box, seed, 7), float(box[0, 0])

    out = []
    for s in shapes:
        if s in "abc":
            nw = 333334
            xyz_h, L = frame(nw, 1)
            xyz = torch.from_numpy(xyz_h).cuda()
            ox = torch.arange(nw, device="cuda") * 3
            part = ox[:3334].contiguous()
            don, acc = (ox, ox) if s == "a" else (part, ox) if s == "b" else (ox, part)
            hidx = torch.stack([don + 1, don + 2], 1).reshape(-1).contiguous()
            hoff = torch.arange(len(don) + 1, device="cuda") * 2
            box = np.diag([L] * 3).astype(np.float32)
            fused = lambda: eng.hbonds(xyz, don, (hoff, hidx), acc, box=box, pbc=7, cutoff=RC, angle=ANGLE)
            r = fused()
            row = {"shape": s, "atoms": 3 * nw, "donors": len(don), "acceptors": len(acc), "bonds": r.count}
            search = lambda: eng.search_resident(api.SEARCH_DOUBLE, RC, xyz, don, xyz, acc, box=box, pbc=7, ids_local=True)
            row["list_entries"] = search()[0]
            routes = {"fused": fused, "search_alone": search}
            if not fused_only:
                keys = torch_keys(xyz, don, acc, hoff, hidx, L)
                mine = (torch.searchsorted(hidx, r.triples[:, 1].long()) << 32) | torch.searchsorted(acc, r.triples[:, 2].long())
                row["routes_agree"] = bool(torch.equal(keys, mine))
                routes["torch_route"] = lambda: torch_keys(xyz, don, acc, hoff, hidx, L)
            row.update(alternate(routes))
        else:
            nw, F = 33334, 64
            fr = [frame(nw, 100 + f) for f in range(F)]
            L = fr[0][1]
            frames = torch.from_numpy(np.stack([x for x, _ in fr])).cuda()
            ox = torch.arange(nw, device="cuda") * 3
            hidx = torch.stack([ox + 1, ox + 2], 1).reshape(-1).contiguous()
            hoff = torch.arange(nw + 1, device="cuda") * 2
            box = np.diag([L] * 3).astype(np.float32)
            fused = lambda: eng.hbonds_frames(frames, ox, (hoff, hidx), ox, box=box, pbc=7, cutoff=RC, angle=ANGLE)
            r = fused()
            row = {"shape": s, "atoms": 3 * nw, "frames": F, "entries": int(r.per_frame.sum()), "table_rows": int(r.table.shape[0])}
            routes = {"fused": fused}
            if not fused_only:
                def block():
                    keys = torch.cat([torch_keys(frames[f], ox, ox, hoff, hidx, L) for f in range(F)])
                    return torch.unique(keys, return_inverse=True, return_counts=True)
                u, inv, cnt = block()
                row["routes_agree"] = bool(len(u) == r.table.shape[0] and torch.equal(inv.int(), r.bond_of_entry)
                                           and torch.equal(cnt.int(), r.occupancy))
                routes["torch_route"] = block
            row.update(alternate(routes))
        if "torch_route" in row:
            row["torch_median_over_fused_median"] = round(row["torch_route"]["median_ms"] / row["fused"]["median_ms"], 2)
        if "search_alone" in row:
            row["stages_behind_the_search_ms"] = round(row["fused"]["median_ms"] - row["search_alone"]["median_ms"], 4)
        print(json.dumps(row), flush=True)
        out.append(row)
    if write:
        path = write[0].split("=", 1)[1] if "=" in write[0] else os.path.join(ROOT, "profiles", "hbonds.txt")
        with open(path, "w") as f:
            f.write(f"# python tools/bench_hbonds.py {reps} {shapes} --write\n")
            for row in out:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
