#!/usr/bin/env python
"""Minimum distances (molar_hip_mindist: every pair of two selections under each frame's own box in f64, the column atoms in
scalar registers; minima per frame, per atom and per pair of groups, and the time reductions of the group matrix) against the
route a caller had before it, written here in torch f64 on the device:

  (B) fractional coordinates of both sets once per frame, then per chunk of rows (capped at 1 GB of extra memory) the fractional
      differences, round, back-transform by the box matrix, squared norms; `amin` / `min` over the other set for the per-atom
      results, `scatter_reduce(amin)` by label along both axes for the group matrix; mean, minimum and count below the cutoff
      accumulated over the frames.  It does not search the correction shifts of a triclinic cell (torch has no minimum image;
      the bench's cells are sheared so mildly that the rounded vector is the shortest, and the routes are compared first).
  Route (B) is timed on `--frames-timed` frames and scaled by F / frames timed; the scaling is in the output.

Shapes:  (a) a 5000-atom protein against itself, 330 residue groups, exclude_same_group, x 1024 frames, one orthorhombic box:
mat_mean, mat_min, mat_freq;  (b) the same protein against 100 000 water oxygens x 256 frames: dist, pair, atom2;  (c) 4000
phosphorus atoms against a 2000-atom peptide under per-frame triclinic boxes x 4096 frames: atom1, near1.  Frames are random f32
positions resident on the device (the cost does not depend on the values).

Timing: a warm-up, then `reps` repetitions, the routes taking turns, each bracketed by a pair of events - the first recorded
after a device-wide synchronisation, the second after the engine's stream has been waited for; median, minimum and maximum in
ms.  Per shape also the plan, the pairs asked for and evaluated per second (the group pass of a single set evaluates both
halves of the matrix), and the evaluated pairs times the 20 f64 operations an orthorhombic pair costs (3 sub, 3 mul, 3 round,
3 sub, 3 mul, 3 mul, 2 add) as a fraction of the v_fma_f64 issue rate measured in the same run, before the engine opens the
device, by profiles/microbench/fma_f64_rate.  Kernel times proper need a trace run (tools/prof_mindist.py).
One JSON line per shape; the lines go to stdout and, with --write[=PATH], to profiles/mindist.txt (or PATH).
Usage: python tools/bench_mindist.py [reps] [shapes, e.g. ac] [--frames-timed=N (default: F / 64, at least 4)] [--fused-only] [--write[=PATH]]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
BOX = (9.0, 9.5, 10.0)
CUTOFF = 0.45
OPS_PER_PAIR = 20
# n1, n2 (0: the same set), groups, F, per-frame triclinic boxes, outputs
SHAPES = {"a": (5000, 0, 330, 1024, False, ("mat_mean", "mat_min", "mat_freq", "nvalid")),
          "b": (5000, 100000, 0, 256, False, ("dist", "pair", "atom2")),
          "c": (4000, 2000, 0, 4096, True, ("atom1", "near1"))}


def make_case(torch, n1, n2, G, F, tric, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    natoms = n1 + n2
    box = torch.tensor(BOX, device="cuda", dtype=torch.float32)
    frames = torch.empty((F, natoms, 3), device="cuda", dtype=torch.float32)
    for f0 in range(0, F, 64):
        n = min(64, F - f0)
        frames[f0:f0 + n] = torch.rand((n, natoms, 3), device="cuda", generator=gen) * box
    b9 = torch.zeros(9, device="cuda", dtype=torch.float32)
    b9[[0, 4, 8]] = box
    boxes = b9
    if tric:
        b9[3], b9[6], b9[7] = 0.6, -0.4, 0.5                # columns b and c lean a little: a sheared cell with correction shifts
        boxes = (b9[None, :] * (1.0 + 0.02 * (torch.rand((F, 1), device="cuda", generator=gen) - 0.5))).contiguous()
    labels = None
    if G:
        labels = (torch.arange(n1, device="cuda") * G // n1).to(torch.int32)          # residues: runs of 15 or 16 atoms
        labels = labels[torch.randperm(n1, device="cuda", generator=gen)]             # the atoms of the selection in any order
    idx1 = torch.arange(n1, device="cuda", dtype=torch.int64)
    idx2 = torch.arange(n1, natoms, device="cuda", dtype=torch.int64) if n2 else None
    return frames, boxes, idx1, idx2, labels


def route_torch(torch, frames, boxes, idx1, idx2, labels, G, want, cap=1 << 30):
    """The results `want` names, by route (B)."""
    F = frames.shape[0]
    same = idx2 is None
    n1 = idx1.shape[0]
    n2 = n1 if same else idx2.shape[0]
    rows = max(1, cap // (n2 * 3 * 8 * 3))
    out = {}
    lab = labels.long() if labels is not None else None
    if "mat_mean" in want:
        acc_sum = torch.zeros((G, G), device="cuda", dtype=torch.float64)
        acc_min = torch.full((G, G), float("inf"), device="cuda", dtype=torch.float64)
        acc_freq = torch.zeros((G, G), device="cuda", dtype=torch.int64)
    if "dist" in want:
        out["dist"] = torch.empty(F, device="cuda", dtype=torch.float64)
        out["atom2"] = torch.empty((F, n2), device="cuda", dtype=torch.float64)
    if "atom1" in want:
        out["atom1"] = torch.empty((F, n1), device="cuda", dtype=torch.float64)
        out["near1"] = torch.empty((F, n1), device="cuda", dtype=torch.int64)
    for f in range(F):
        m = (boxes if boxes.ndim == 1 else boxes[f]).double().reshape(3, 3).T               # columns a, b, c
        inv = torch.linalg.inv(m)
        s1 = frames[f][idx1].double() @ inv.T
        s2 = s1 if same else frames[f][idx2].double() @ inv.T
        if "mat_mean" in want:
            mat = torch.full((G, G), float("inf"), device="cuda", dtype=torch.float64)
        if "dist" in want:
            col = torch.full((n2,), float("inf"), device="cuda", dtype=torch.float64)
        for r0 in range(0, n1, rows):
            ds = s2[None, :, :] - s1[r0:r0 + rows, None, :]
            ds -= torch.round(ds)
            v = ds @ m.T
            d2 = (v * v).sum(dim=-1)
            if "mat_mean" in want:
                l1 = lab[r0:r0 + rows]
                d2 = torch.where(l1[:, None] == lab[None, :], float("inf"), d2)              # the diagonal and every pair inside a group
                part = torch.full((d2.shape[0], G), float("inf"), device="cuda", dtype=torch.float64)
                part.scatter_reduce_(1, lab[None, :].expand(d2.shape[0], -1), d2, reduce="amin")
                mat.scatter_reduce_(0, l1[:, None].expand(-1, G), part, reduce="amin")
            if "dist" in want:
                col = torch.minimum(col, d2.amin(dim=0))
            if "atom1" in want:
                val, arg = d2.min(dim=1)
                out["atom1"][f, r0:r0 + rows] = torch.sqrt(val)
                out["near1"][f, r0:r0 + rows] = arg
        if "mat_mean" in want:
            d = torch.sqrt(mat)
            acc_sum += d
            acc_min = torch.minimum(acc_min, d)
            acc_freq += d < CUTOFF
        if "dist" in want:
            out["atom2"][f] = torch.sqrt(col)
            out["dist"][f] = out["atom2"][f].min()
    if "mat_mean" in want:
        out.update(mat_mean=acc_sum / F, mat_min=acc_min, mat_freq=acc_freq)
    return out


def timed(torch, eng, fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    eng.synchronize()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    return dict(median=round(float(np.median(ts)), 3), min=round(min(ts), 3), max=round(max(ts), 3))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opts = dict(a[2:].split("=", 1) if "=" in a else (a[2:], "") for a in sys.argv[1:] if a.startswith("--"))
    reps = int(args[0]) if args else 20
    shapes = args[1] if len(args) > 1 else "abc"
    fused_only = "fused-only" in opts
    lines = []
    roof = 0.0
    if not fused_only:
        from bench_tcf import microbench
        text = microbench("fma_f64_rate")            # a child process of its own, before this one opens the device
        rows = [dict(zip(ln.split()[0::2], ln.split()[1::2])) for ln in text.splitlines() if ln.startswith("waves_per_simd")]
        roof = max(float(r["tfma"]) for r in rows)
        lines.append(json.dumps({"v_fma_f64_roof_tera_lane_fma_per_s": roof, "microbench": text.strip().splitlines()}))
        print(lines[0], flush=True)
    import torch
    from molar_amd import api
    eng = api.Engine()
    for key in shapes:
        n1, n2, G, F, tric, want = SHAPES[key]
        frames, boxes, idx1, idx2, labels = make_case(torch, n1, n2, G, F, tric, 23)
        same = n2 == 0
        kw = dict(idx1=idx1, idx2=idx2, labels1=labels, ngroups1=G if G else None, same=same, exclude_same_group=same, cutoff=CUTOFF, want=want)
        fused = lambda fr=frames, bx=boxes: eng.min_distances(fr, boxes=bx, **kw)
        ws, rw, rb, ct, cs, fb = api.mindist_plan(F, n1, n1 if same else n2, G or 1, G or 1, want=[w for w in want if w != "nvalid"], same=same)
        asked = F * (n1 * (n1 - 1) // 2 if same else n1 * n2)
        evaluated = F * n1 * (n1 if same else n2)
        res = dict(shape=key, n1=n1, n2=n1 if same else n2, groups=G, frames=F, triclinic_per_frame_boxes=tric, outputs=want, workspace_MB=round(ws / 2 ** 20, 1),
                   rows_per_wave=rw, rows_per_block=rb, cols_per_tile=ct, col_splits=cs, frame_block=fb, pairs_asked=asked, pairs_evaluated=evaluated)
        if not fused_only:
            Ft = min(F, int(opts["frames-timed"]) if "frames-timed" in opts else max(4, F // 64))
            sub, bsub = frames[:Ft], boxes if boxes.ndim == 1 else boxes[:Ft].contiguous()
            got = fused(sub, bsub)
            eng.synchronize()
            ref = route_torch(torch, sub, bsub, idx1, idx2, labels, G, want)
            for name in ("dist", "atom1", "atom2", "mat_mean", "mat_min"):
                if name in want:
                    a, b = getattr(got, name).double(), ref[name]
                    fin = torch.isfinite(b)
                    assert bool((torch.isfinite(a) == fin).all()), name
                    res[f"diff_{name}"] = float((a[fin] - b[fin]).abs().max())
                    assert res[f"diff_{name}"] < 1e-5, (name, res)             # f32 results: about 1e-7 of a nanometre-sized number
            if "near1" in want:
                res["near1_equal"] = f"{int((got.near1 == ref['near1']).sum())} of {ref['near1'].numel()}"
            if "mat_freq" in want:
                res["mat_freq_equal"] = f"{int((got.mat_freq.long() == ref['mat_freq']).sum())} of {ref['mat_freq'].numel()}"
            ts = {"torch": [], "fused_on_frames_timed": []}
            for _ in range(reps):
                ts["fused_on_frames_timed"].append(timed(torch, eng, lambda: fused(sub, bsub)))
                ts["torch"].append(timed(torch, eng, lambda: route_torch(torch, sub, bsub, idx1, idx2, labels, G, want)))
            res["frames_timed"] = Ft
            for name, t in ts.items():
                res[f"ms_{name}"] = stats(t)
            res["ms_torch_scaled_to_F"] = round(res["ms_torch"]["median"] * F / Ft, 1)
        fused()
        eng.synchronize()
        res["ms_fused"] = stats([timed(torch, eng, fused) for _ in range(reps)])
        sec = res["ms_fused"]["median"] * 1e-3
        res["pairs_asked_per_s"] = float("%.4g" % (asked / sec))
        res["pairs_evaluated_per_s"] = float("%.4g" % (evaluated / sec))
        if not fused_only:
            res["fraction_of_fma_issue_rate"] = round(evaluated * OPS_PER_PAIR / sec / (roof * 1e12), 3)
            res["torch_over_fused"] = round(res["ms_torch_scaled_to_F"] / res["ms_fused"]["median"], 2)
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        del frames
        torch.cuda.empty_cache()
    if "write" in opts:
        path = opts["write"] or os.path.join(ROOT, "profiles", "mindist.txt")
        with open(path, "w") as f:
            f.write("# python tools/bench_mindist.py %d %s --write\n" % (reps, shapes))
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
