#!/usr/bin/env python
"""The internal-coordinate call (molar_hip_intcoord: bond vectors, minimum images, atan2, on-chip integer histograms, chunk
partials folded in order) against the same arithmetic written in torch f64 with everything resident on the device: index
gathers, `torch.linalg.cross`, `atan2`, ONE `torch.bincount` per histogram, and sums of cos / sin (or of v and v^2) over the
frames.  The torch route walks the block in slices of at most 4096 frames so that its f64 temporaries fit beside the frames.

Shapes:  (r) a 1000-residue protein, 16 000 atoms x 65 536 frames, no box: the phi / psi / omega series (2994 dihedrals), their
histograms in three groups, the statistics and the 72 x 72 Ramachandran map;  (l) 4000 lipids x 28 tail dihedrals on
500 000-atom frames x 256 frames under per-frame boxes: histogram and circular statistics only, no series;  (w) a
1 000 000-atom water box x 64 frames under per-frame boxes: 333 333 HOH angles, series, histogram and statistics.  Frames are
f32, the coordinates random (the arithmetic does not care; a dihedral of random points is as costly as a real one).

Before anything is timed the two routes are compared: the histogram and the map bin by bin (reported: the bins that differ -
random coordinates do put a value within a rounding of an edge now and then - and the totals), the series to the rounding of
the fused call's f32 output (reported).  Timing: a warm-up, then `reps` repetitions (default 20), the routes taking turns, each
bracketed by a pair of events - the first recorded after a device-wide synchronisation, the second after the engine's stream
has been waited for; median, minimum and maximum in ms.  No ratio is fixed in advance: the line says which route won.

Also per shape: the bytes of coordinates the tuples gather (12 per atom of a tuple and frame), that over the fused call's
median as GB/s, and the same as a fraction of the device-to-device copy rate measured in the same run on the frames (read +
write counted once each).  Kernel times proper need a trace run:
`rocprofv3 --kernel-trace --stats -- python tools/bench_intcoord.py --fused-only 5 r` (profiles/intcoord_kernels.txt).
One JSON line per shape; the lines go to stdout and, with --write[=PATH], to profiles/intcoord.txt (or PATH).
Usage: python tools/bench_intcoord.py [reps] [shapes, e.g. rlw] [--fused-only] [--write[=PATH]]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BOX = (12.0, 12.5, 9.0)
SLICE = 4096
# atoms, frames, kind, boxes, series wanted, nbins, map_bins
SHAPES = {"r": (16000, 65536, 4, False, True, 72, 72), "l": (500000, 256, 4, True, False, 72, 0), "w": (1000000, 64, 3, True, True, 90, 0)}


def make_case(torch, key):
    n, F, kind, boxed, series, nbins, mb = SHAPES[key]
    gen = torch.Generator(device="cuda").manual_seed(ord(key))
    frames = torch.empty((F, n, 3), device="cuda", dtype=torch.float32)
    blen = torch.tensor(BOX, device="cuda", dtype=torch.float32)
    for f0 in range(0, F, 64):
        frames[f0:f0 + 64] = torch.rand((min(64, F - f0), n, 3), device="cuda", dtype=torch.float32, generator=gen) * blen
    boxes = None
    if boxed:
        scale = 1.0 + 0.02 * (2 * torch.rand((F, 1), device="cuda", dtype=torch.float64, generator=gen) - 1)
        boxes = torch.zeros((F, 9), device="cuda", dtype=torch.float64)
        for d in range(3):
            boxes[:, 4 * d] = BOX[d] * scale[:, 0]
        boxes = boxes.float()
    labels = pairs = None
    if key == "r":                                               # 16 atoms per residue: N, CA, C are its atoms 0, 2, 14
        res = np.arange(1, 1000)
        N, CA, C = 16 * res, 16 * res + 2, 16 * res + 14
        phi = np.stack([C - 16, N, CA, C], 1)[:-1]
        psi = np.stack([N, CA, C, N + 16], 1)[:-1]
        omega = np.stack([CA, C, N + 16, CA + 16], 1)[:-1]
        tuples = np.concatenate([phi, psi, omega])
        labels = np.repeat([0, 1, 2], len(phi))
        pairs = np.stack([np.arange(len(phi)), len(phi) + np.arange(len(phi))], 1)
    elif key == "l":                                             # 125 atoms per lipid, two tails of 17 carbons from atoms 40 and 80
        first = (125 * np.arange(4000))[:, None, None] + np.array([40, 80])[None, :, None] + np.arange(14)[None, None, :]
        tuples = (first.reshape(-1, 1) + np.arange(4)[None, :])
        labels = np.tile(np.arange(28), 4000)
    else:                                                        # O H H
        o = 3 * np.arange(n // 3)
        tuples = np.stack([o + 1, o, o + 2], 1)
    dev = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()
    return dict(frames=frames, boxes=boxes, tuples=dev(tuples, np.int64), labels=dev(labels, np.int32), pairs=dev(pairs, np.int64), kind=kind, series=series,
                nbins=nbins, map_bins=mb, G=1 if labels is None else int(labels.max()) + 1)


def torch_route(torch, case):
    """(values [F, T] f64 or None, hist [G, nbins], map or None, mean [T], spread [T])"""
    fr, tu, kind, nbins, mb, G = case["frames"], case["tuples"], case["kind"], case["nbins"], case["map_bins"], case["G"]
    F, T = fr.shape[0], tu.shape[0]
    lab = case["labels"].long() if case["labels"] is not None else torch.zeros(T, device="cuda", dtype=torch.long)
    hist = torch.zeros(G * nbins, device="cuda", dtype=torch.long)
    hmap = torch.zeros(mb * mb, device="cuda", dtype=torch.long) if mb else None
    s1 = torch.zeros(T, device="cuda", dtype=torch.float64)
    s2 = torch.zeros(T, device="cuda", dtype=torch.float64)
    vals = [] if case["series"] else None
    for f0 in range(0, F, SLICE):
        x = fr[f0:f0 + SLICE]
        p = [x[:, tu[:, j]].double() for j in range(kind)]
        b = [p[0] - p[1], p[2] - p[1]] if kind == 3 else [p[j + 1] - p[j] for j in range(kind - 1)]
        if case["boxes"] is not None:
            L = case["boxes"][f0:f0 + SLICE][:, [0, 4, 8]].double()[:, None, :]
            b = [d - L * torch.round(d / L) for d in b]
        if kind == 3:
            v = torch.atan2(torch.linalg.cross(b[0], b[1]).norm(dim=-1), (b[0] * b[1]).sum(-1))
            bins = torch.clamp(torch.floor(v / np.pi * nbins).long(), max=nbins - 1)
            s1 += v.sum(0)
            s2 += (v * v).sum(0)
        else:
            n1, n2 = torch.linalg.cross(b[0], b[1]), torch.linalg.cross(b[1], b[2])
            v = torch.atan2(b[1].norm(dim=-1) * (b[0] * n2).sum(-1), (n1 * n2).sum(-1))
            bins = torch.floor((v + np.pi) / (2 * np.pi) * nbins).long() % nbins
            s1 += torch.cos(v).sum(0)
            s2 += torch.sin(v).sum(0)
        hist += torch.bincount((lab[None, :] * nbins + bins).reshape(-1), minlength=G * nbins)
        if mb:
            mbin = torch.floor((v + np.pi) / (2 * np.pi) * mb).long() % mb
            pr = case["pairs"]
            hmap += torch.bincount((mbin[:, pr[:, 0]] * mb + mbin[:, pr[:, 1]]).reshape(-1), minlength=mb * mb)
        if vals is not None:
            vals.append(v)
    if kind == 3:
        mean = s1 / F
        spread = torch.sqrt(torch.clamp(s2 / F - mean * mean, min=0))
    else:
        mean = torch.atan2(s2, s1)
        spread = 1 - torch.hypot(s1, s2) / F
    return (torch.cat(vals) if vals is not None else None), hist.reshape(G, nbins), hmap, mean, spread


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 20
    shapes = args[1] if len(args) > 1 else "rlw"
    fused_only = "--fused-only" in sys.argv
    write = next((a for a in sys.argv[1:] if a.startswith("--write")), None)
    import torch
    from molar_amd import api
    eng = api.Engine()
    lines = []
    for key in shapes:
        case = make_case(torch, key)
        fr, tu = case["frames"], case["tuples"]
        F, n = fr.shape[:2]
        T, kind = tu.shape
        want = (("values",) if case["series"] else ()) + ("hist", "mean", "spread", "valid") + (("map",) if case["map_bins"] else ())
        kw = dict(labels=case["labels"], ngroups=case["G"], boxes=case["boxes"], nbins=case["nbins"], pairs=case["pairs"], map_bins=case["map_bins"], want=want)
        out = eng.internal_coords(fr, tu, **kw)
        eng.synchronize()

        def fused():
            eng.internal_coords(fr, tu, out=out, **kw)

        def timed(fn):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            eng.synchronize()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b)

        npairs = 0 if case["pairs"] is None else int(case["pairs"].shape[0])
        rec = dict(shape=key, atoms=n, frames=F, tuples=T, kind=kind, groups=case["G"], nbins=case["nbins"], map_bins=case["map_bins"], pairs=npairs,
                   boxes=case["boxes"] is not None, series=case["series"],
                   plan=dict(zip(("workspace_bytes", "frame_chunk", "tuple_chunk", "lds_cells"),
                                 api.intcoord_plan(F, T, kind, case["G"], npairs, 1, case["nbins"], None, case["map_bins"]))),
                   valid_fraction=float(out.valid.sum()) / (F * T))
        if fused_only:
            for _ in range(reps):
                fused()
            eng.synchronize()
            print(json.dumps(rec))
            continue
        v_t, h_t, m_t, mean_t, spread_t = torch_route(torch, case)
        rec.update(hist_bins_that_differ=int((out.hist != h_t).sum()), hist_total=int(out.hist.sum()), hist_total_torch=int(h_t.sum()),
                   mean_max_diff=float((out.mean.double() - mean_t).abs().max()), spread_max_diff=float((out.spread.double() - spread_t).abs().max()))
        if m_t is not None:
            rec.update(map_bins_that_differ=int((out.map.reshape(-1) != m_t).sum()), map_total=int(out.map.sum()), map_total_torch=int(m_t.sum()))
        if v_t is not None:
            rec.update(values_max_diff=float((out.values.double() - v_t).abs().max()))
        del v_t, h_t, m_t, mean_t, spread_t
        torch.cuda.empty_cache()
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
        gathered = 12.0 * T * kind * F * (2 if case["map_bins"] else 1)      # the map kernel gathers its tuples again
        med = float(np.median(tf))
        rec.update(fused_ms=dict(median=med, min=min(tf), max=max(tf)), torch_ms=dict(median=float(np.median(tt)), min=min(tt), max=max(tt)),
                   winner="fused" if med < float(np.median(tt)) else "torch", gathered_bytes=gathered, frames_bytes=12.0 * n * F,
                   fused_GBps=gathered / med * 1e-6, copy_GBps_read_plus_write=2 * 12.0 * n * F / float(np.median(copy)) * 1e-6)
        rec["fraction_of_copy_rate"] = rec["fused_GBps"] / rec["copy_GBps_read_plus_write"]
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        del case, fr, out
        torch.cuda.empty_cache()
    if write and lines:
        path = write.split("=", 1)[1] if "=" in write else os.path.join(ROOT, "profiles", "intcoord.txt")
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
