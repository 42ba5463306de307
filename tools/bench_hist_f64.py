#!/usr/bin/env python
"""The radial distance histogram of BASELINE config 4 for MolAR's `f64` feature: box A, 250k atoms, rc 1.2 nm, 1200 bins of
0.001 nm, full periodicity, frames resident in HBM as float64.  Three routes over the same frames, bins in HBM:
  1. the f64 fused histogram (molar_hip_search_histogram_f64): single calls, and the frames form;
  2. the f64 route without it: search_count_f64 + search_fill_f64 into device columns + a GPU bincount of the f64 formula;
  3. the f32 fused histogram (frames rounded to f32): single calls and the frames form, for reference.
Prints one JSON line: ms per frame and frames/s of each route, and whether routes 1 and 2 give the same bins.

    python tools/bench_hist_f64.py [--natoms 250000] [--frames 8] [--reps 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def per_frame(fn, sync, nframes, reps):
    """Best of `reps` timed passes over all frames (after one warm-up pass), in ms per frame."""
    fn()
    sync()
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        t = (time.perf_counter() - t0) / nframes * 1e3
        best = t if best is None else min(best, t)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--natoms", type=int, default=250_000)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cutoff", type=float, default=1.2)
    ap.add_argument("--nbins", type=int, default=1200)
    args = ap.parse_args()
    import torch
    from molar_amd import api, build, synth
    build.build_library()
    eng = api.Engine(0)
    n, nf, rc, nbins = args.natoms, args.frames, args.cutoff, args.nbins
    box = synth.box_a(n).astype(np.float64)
    rng = np.random.default_rng(1)
    frames = np.stack([synth.frame(n, synth.box_a(n), k).astype(np.float64) + rng.normal(0, 1e-9, (n, 3)) for k in range(nf)])
    d64 = torch.from_numpy(frames).cuda()
    d32 = torch.from_numpy(frames.astype(np.float32)).cuda()
    torch.cuda.synchronize()

    def sync():
        eng.synchronize()
        torch.cuda.synchronize()
    b_fused = torch.zeros(nbins, dtype=torch.int64, device="cuda")

    def fused_single():
        for k in range(nf):
            eng.search_histogram_f64(api.SEARCH_SINGLE, rc, 0.0, rc, nbins, d64[k], box=box, pbc=7, bins=b_fused, want_count=False)

    def fused_frames():
        eng.search_histogram_frames_f64(api.SEARCH_SINGLE, rc, 0.0, rc, nbins, d64, box=box, pbc=7, bins=b_fused)
    b_ref = torch.zeros(nbins, dtype=torch.int64, device="cuda")
    npairs = eng.search_histogram_f64(api.SEARCH_SINGLE, rc, 0.0, rc, nbins, d64[0], box=box, pbc=7)[1]
    cap = int(npairs * 1.05) + 1024
    outs = (torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.int64, device="cuda"),
            torch.empty(cap, dtype=torch.float64, device="cuda"))          # the caller's result columns, allocated once

    def count_fill_bincount():
        for k in range(nf):
            _, _, dist = eng.search_f64(api.SEARCH_SINGLE, rc, d64[k], box=box, pbc=7, device_out=True, out=outs)
            b = torch.floor(float(nbins) * (dist - 0.0) / (rc - 0.0))           # Histogram1D::add_one in f64
            ok = (b >= 0) & (b < nbins)
            b_ref.add_(torch.bincount(b[ok].to(torch.int64), minlength=nbins))
    b32 = torch.zeros(nbins, dtype=torch.int64, device="cuda")
    box32 = box.astype(np.float32)

    def f32_single():
        for k in range(nf):
            eng.search_histogram(api.SEARCH_SINGLE, rc, 0.0, rc, nbins, d32[k], box=box32, pbc=7, bins=b32, want_count=False)

    def f32_frames():
        eng.search_histogram_frames(api.SEARCH_SINGLE, rc, 0.0, rc, nbins, d32, box=box32, pbc=7, bins=b32)

    reps = args.reps
    line = {"workload": f"radial distance histogram, f64, {n} atoms, triclinic box A, rc {rc} nm, {nbins} bins, pbc 7, "
                        f"{nf} frames resident in HBM", "natoms": n, "frames": nf, "pairs_frame0": int(npairs)}
    line["f64_fused_ms"] = per_frame(fused_single, sync, nf, reps)
    line["f64_fused_frames_ms"] = per_frame(fused_frames, sync, nf, reps)
    line["f64_count_fill_bincount_ms"] = per_frame(count_fill_bincount, sync, nf, reps)
    line["f32_fused_ms"] = per_frame(f32_single, sync, nf, reps)
    line["f32_fused_frames_ms"] = per_frame(f32_frames, sync, nf, reps)
    for k in [x for x in line if x.endswith("_ms")]:
        line[k.replace("_ms", "_fps")] = 1e3 / line[k]
    # one pass of each f64 route from zero: the same integer bins
    b_fused.zero_(); b_ref.zero_()
    sync()
    fused_single(); count_fill_bincount()
    sync()
    line["f64_fused_equals_count_fill_bincount"] = bool(torch.equal(b_fused, b_ref))
    line["speedup_f64_fused_vs_count_fill"] = line["f64_count_fill_bincount_ms"] / line["f64_fused_ms"]
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
