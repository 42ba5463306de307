#!/usr/bin/env python
"""The density call (molar_hip_density: fractional or lab coordinates, per-frame centring, integer bins per frame, the fold over
the frames) against the same arithmetic written in torch f64 with everything resident on the device: a batched
`frames @ inv.T`, the circular-mean centre, wrap, floor, and ONE `torch.bincount(weights=...)` over the flattened
(frame, group, bin) index, then the division by the frames' bin volumes and the mean over the frames.  The torch route adds
floating-point weights with atomics in arrival order: it is NOT reproducible bit for bit, the fused call is.

Shapes:  (p) a z profile of a bilayer system: 500 000 atoms x 256 frames, 5 groups x 200 bins, mass weighted, centred on the
lipids (a fifth of the atoms), per-frame boxes;  (m) a lateral map: 128 x 128 of 4000 phosphates x 4096 frames, number density,
per-frame boxes;  (v) a volume map: 128^3 of 330 000 water oxygens x 64 frames in lab coordinates.  Frames are f32.

Before anything is timed the two routes are compared: the counts must be equal wherever no atom sits within 1e-9 of a bin
edge in the torch route's own coordinates (reported: bins that differ), the densities to the rounding of the fused call's f32 output, relative to the
largest entry (reported).  Timing: a warm-up, then `reps` repetitions (default 20), the routes taking turns, each bracketed by a pair of events -
the first recorded after a device-wide synchronisation, the second after the engine's stream has been waited for; median,
minimum and maximum in ms.  No ratio is fixed in advance: the line says which route won.

Also per shape: the bytes of selected coordinates read (12 per atom and frame), that over the fused call's median as GB/s, and
the same as a fraction of the device-to-device copy rate measured in the same run on a buffer of the frames' size (read + write
counted once each: the rate a kernel that only read the coordinates could reach).  Kernel times proper need a trace run:
`rocprofv3 --kernel-trace --stats -- python tools/bench_density.py --fused-only 5 p` (profiles/density_kernels.txt).
One JSON line per shape; the lines go to stdout and, with --write[=PATH], to profiles/density.txt (or PATH).
Usage: python tools/bench_density.py [reps] [shapes, e.g. pmv] [--fused-only] [--write[=PATH]]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BOX = (12.0, 12.5, 9.0)
# atoms, frames, groups, nbins, mode, centred, weighted
SHAPES = {"p": (500000, 256, 5, (1, 1, 200), "box", True, True), "m": (4000, 4096, 1, (128, 128, 1), "box", False, False),
          "v": (330000, 64, 1, (128, 128, 128), "lab", False, False)}
LAB_LO, LAB_HI = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0)


def make_case(torch, key):
    n, F, G, nbins, mode, centred, weighted = SHAPES[key]
    gen = torch.Generator(device="cuda").manual_seed(ord(key))
    scale = 1.0 + 0.02 * (2 * torch.rand((F, 1), device="cuda", dtype=torch.float64, generator=gen) - 1)
    boxes = torch.zeros((F, 9), device="cuda", dtype=torch.float64)
    for d in range(3):
        boxes[:, 4 * d] = BOX[d] * scale[:, 0]
    boxes = boxes.float()
    frames = torch.empty((F, n, 3), device="cuda", dtype=torch.float32)
    blen = boxes[:, [0, 4, 8]]
    for f0 in range(0, F, 64):
        u = torch.rand((min(64, F - f0), n, 3), device="cuda", dtype=torch.float32, generator=gen)
        if mode == "box":
            if centred:                                    # a bilayer: the first fifth of the atoms in a slab that drifts across the cell
                nl = n // 5
                z0 = ((f0 + torch.arange(u.shape[0], device="cuda")) * 0.013 % 1.0).float()[:, None]
                u[:, :nl, 2] = (z0 + 0.12 * (2 * u[:, :nl, 2] - 1)) % 1.0
            frames[f0:f0 + 64] = u * blen[f0:f0 + 64, None, :]
        else:
            frames[f0:f0 + 64] = 3.0 * torch.randn(u.shape, device="cuda", dtype=torch.float32, generator=gen)     # most of them outside the map, as the water of a large system is
    labels = (torch.arange(n, device="cuda") * G // n).int() if G > 1 else None
    weight = (1.0 + 15.0 * torch.rand(n, device="cuda", dtype=torch.float32, generator=gen)) if weighted else None
    centre_idx = torch.arange(n // 5, device="cuda") if centred else None
    return dict(frames=frames, boxes=boxes, labels=labels, weight=weight, centre_idx=centre_idx, G=G, nbins=nbins, mode=mode)


def grid_of(api, case):
    if case["mode"] == "lab":
        return api.volume_grid(LAB_LO, LAB_HI, case["nbins"])
    nb = case["nbins"]
    if nb[0] == 1 and nb[1] == 1:
        return api.profile_grid(2, nb[2], centre=case["centre_idx"] is not None)
    return api.map_grid(nb[:2])


def torch_route(torch, case):
    """(density [G, nb] f64, count [G, nb] int64, closest distance of a bin coordinate to an integer)."""
    fr, G, nbins = case["frames"], case["G"], case["nbins"]
    F, n = fr.shape[:2]
    nbt = torch.tensor(nbins, device="cuda", dtype=torch.float64)
    nb = int(np.prod(nbins))
    x = fr.double()
    if case["mode"] == "box":
        M = case["boxes"].double().reshape(F, 3, 3).transpose(1, 2)                  # column-major rows -> M[f][r][c]
        inv = torch.linalg.inv(M)
        s = torch.bmm(x, inv.transpose(1, 2))
        if case["centre_idx"] is not None:
            w = case["weight"].double()[case["centre_idx"]] if case["weight"] is not None else torch.ones(len(case["centre_idx"]), device="cuda", dtype=torch.float64)
            th = 2 * np.pi * s[:, case["centre_idx"], 2]
            c = torch.atan2(-(w * torch.sin(th)).sum(1), -(w * torch.cos(th)).sum(1)) / (2 * np.pi) + 0.5
            s[:, :, 2] += (0.5 - c)[:, None]
        u = s - torch.floor(s)
        keep = None
        binvol = torch.linalg.det(M).abs() / nb
    else:
        lo, hi = (torch.tensor(v, device="cuda", dtype=torch.float64) for v in (LAB_LO, LAB_HI))
        u = (x - lo) * (1.0 / (hi - lo))
        keep = ((u >= 0) & (u < 1)).all(-1)
        binvol = torch.full((F,), float(torch.prod((hi - lo) / nbt)), device="cuda", dtype=torch.float64)
    xb = u * nbt
    b = torch.minimum(torch.floor(xb), nbt - 1).long()
    near = (xb - torch.round(xb)).abs()
    cell = (b[..., 0] * nbins[1] + b[..., 1]) * nbins[2] + b[..., 2]
    g = case["labels"].long()[None, :] if case["labels"] is not None else 0
    flat = (torch.arange(F, device="cuda")[:, None] * G + g) * nb + cell
    wts = case["weight"].double()[None, :].expand(F, n) if case["weight"] is not None else None
    if keep is not None:
        flat, near = flat[keep], near[keep]
        wts = wts[keep] if wts is not None else None
    hist = torch.bincount(flat.reshape(-1), weights=None if wts is None else wts.reshape(-1), minlength=F * G * nb).reshape(F, G, nb)
    count = hist.sum(0) if wts is None else torch.bincount(flat.reshape(-1) % (G * nb), minlength=G * nb).reshape(G, nb)
    dens = (hist.double() / binvol[:, None, None]).mean(0)
    return dens, count, float(near.min())


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 20
    shapes = args[1] if len(args) > 1 else "pmv"
    fused_only = "--fused-only" in sys.argv
    write = next((a for a in sys.argv[1:] if a.startswith("--write")), None)
    import torch
    from molar_amd import api
    eng = api.Engine()
    lines = []
    for key in shapes:
        case = make_case(torch, key)
        grd = grid_of(api, case)
        fr = case["frames"]
        F, n = fr.shape[:2]
        kw = dict(weight=case["weight"], labels=case["labels"], ngroups=case["G"], boxes=case["boxes"] if case["mode"] == "box" else None,
                  centre_idx=case["centre_idx"], centre_weight=case["weight"] if case["centre_idx"] is not None else None)
        out = eng.density(fr, grd, **kw)
        eng.synchronize()

        def fused():
            eng.density(fr, grd, out=out, **kw)

        def timed(fn):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            eng.synchronize()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b)

        rec = dict(shape=key, atoms=n, frames=F, groups=case["G"], nbins=list(case["nbins"]), mode=case["mode"], centred=case["centre_idx"] is not None,
                   weighted=case["weight"] is not None, plan=dict(zip(("workspace_bytes", "frame_chunk", "atom_chunk", "lds_cells"), api.density_plan(F, n, grd, case["G"]))),
                   weight_scale_log2=out.weight_scale_log2, outside_fraction=float(out.outside.sum()) / (F * n))
        if fused_only:
            for _ in range(reps):
                fused()
            eng.synchronize()
            print(json.dumps(rec))
            continue
        dens_t, count_t, near = torch_route(torch, case)
        G, nb = dens_t.shape
        differ = int((out.count.reshape(G, nb) != count_t).sum())
        scale = float(dens_t.abs().max())
        rec.update(count_bins_that_differ=differ, torch_closest_to_an_edge=near, count_total=int(out.count.sum()), count_total_torch=int(count_t.sum()),
                   density_max_rel_diff=float((out.density.reshape(G, nb).double() - dens_t).abs().max()) / scale)
        del dens_t, count_t
        tf, tt = [], []
        timed(fused)
        timed(lambda: torch_route(torch, case))
        for _ in range(reps):
            tf.append(timed(fused))
            tt.append(timed(lambda: torch_route(torch, case)))
        copy = []
        dst = torch.empty_like(fr)
        for _ in range(5):
            copy.append(timed(lambda: dst.copy_(fr)))
        del dst
        nbytes = 12.0 * n * F
        med = float(np.median(tf))
        rec.update(fused_ms=dict(median=med, min=min(tf), max=max(tf)), torch_ms=dict(median=float(np.median(tt)), min=min(tt), max=max(tt)),
                   winner="fused" if med < float(np.median(tt)) else "torch", coordinate_bytes=nbytes, fused_GBps=nbytes / med * 1e-6,
                   copy_GBps_read_plus_write=2 * nbytes / float(np.median(copy)) * 1e-6)
        rec["fraction_of_copy_rate"] = rec["fused_GBps"] / rec["copy_GBps_read_plus_write"]
        print(json.dumps(rec))
        lines.append(json.dumps(rec))
        del case, fr, out
        torch.cuda.empty_cache()
    if write and lines:
        path = write.split("=", 1)[1] if "=" in write else os.path.join(ROOT, "profiles", "density.txt")
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
