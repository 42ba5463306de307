#!/usr/bin/env python
"""The neighbour-shell options at C5 size (BASELINE.json configs[4]: 500k atoms, 4000 lipids, frames resident in HBM, one
context): the chained frame without shells, with (n_shells_patch, n_shells_smoothing) = (2,0) and (3,2) - two frames in
flight - and the stage-by-stage path with the same two shell options.  Prints one JSON line per variant.
Usage: python tools/bench_membrane_shells.py   (FRAMES=200 timed frames per variant, after warm-up)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from molar_amd import api, build
    from molar_amd import membrane as mb
    build.build_library()
    eng = api.Engine(0)
    xyz, box, first, tpl, masses = mb.build_bilayer(2000, 500_000)
    rng = np.random.default_rng(0)
    frames = [torch.from_numpy((xyz + rng.normal(0, 0.02, xyz.shape)).astype(np.float32)).cuda() for _ in range(4)]
    K = int(os.environ.get("FRAMES", "200"))
    pbox = api.PeriodicBox.from_matrix(box)
    work = [f.clone() for f in frames for _ in range((K + 3) // 4)]

    def run(m, fused):
        bufs = [w.clone() for w in work[:K]]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if fused:
            plan = m._plan()
            prev = plan.begin(bufs[0], pbox)
            for k in range(1, K):
                t = plan.begin(bufs[k], pbox)
                plan.end(prev)
                prev = t
            plan.end(prev)
        else:
            for k in range(K):
                m.compute(bufs[k], pbox)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / K

    variants = (((0, 0), True), ((2, 0), True), ((2, 0), False), ((3, 2), True), ((3, 2), False))
    pick = os.environ.get("VARIANTS")                       # e.g. VARIANTS=1,3: only those legs (for a profiler run)
    if pick:
        variants = [variants[int(k)] for k in pick.split(",")]
    for shells, fused in variants:
        m = mb.Membrane(eng, len(xyz), first, tpl, masses, mb.MembraneOptions(cutoff=2.5, order_type=1, n_shells_patch=shells[0],
                                                                               n_shells_smoothing=shells[1], fused=fused))
        for _ in range(3):                                  # warm-up (the chained plan provisions its buffers here)
            m.compute(frames[0].clone(), pbox)
        dt = min(run(m, fused) for _ in range(3))
        how = "chained frame, two in flight" if fused else "stage-by-stage calls"
        print(json.dumps({"workload": f"C5 500k-atom bilayer, 4000 lipids, frames resident; shells {shells}, {how}",
                          "n_shells_patch": shells[0], "n_shells_smoothing": shells[1], "fused": fused, "frames": K,
                          "frames_per_s": round(1.0 / dt, 1), "ms_per_frame": round(dt * 1e3, 4)}), flush=True)


if __name__ == "__main__":
    main()
