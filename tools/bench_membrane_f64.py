#!/usr/bin/env python
"""The f64 membrane pass at C5 size (BASELINE.json configs[4]: build_bilayer(2000, 500_000), 4000 lipids, frames resident in
HBM, one context): Membrane(precision="f64").compute (the staged loop, MolAR's `f64` feature) beside the f32 staged and
chained forms in the same run, for the default options and the (n_shells_patch, n_shells_smoothing) = (2,0) and (3,2)
shells.  Prints one JSON line per variant.  Kernel times (k_membrane_fit<double> and k_membrane_average<double> beside their f32 instances and k_membrane_fit_lanes) come from a
run under the tracer:
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/bench_membrane_f64.py
Usage: python tools/bench_membrane_f64.py   (FRAMES=20 timed frames per variant after two warm-up frames)"""
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
    base = [(xyz + rng.normal(0, 0.02, xyz.shape)).astype(np.float32) for _ in range(4)]
    n = int(os.environ.get("FRAMES", "20"))
    pbox = api.PeriodicBox.from_matrix(box)

    def run(precision, fused, shells):
        real = np.float64 if precision == "f64" else np.float32
        opt = mb.MembraneOptions(cutoff=2.5, order_type=1, fused=fused, n_shells_patch=shells[0], n_shells_smoothing=shells[1])
        m = mb.Membrane(eng, len(xyz), first, tpl, masses.astype(real), opt, precision=precision)
        bufs = [torch.from_numpy(base[k % 4].astype(real)).cuda() for k in range(n + 2)]
        b = box.astype(real) if precision == "f64" else pbox
        for k in range(2):                                  # warm-up: library state, buffers, kernel attributes
            m.compute(bufs[k], b)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if fused:
            prev = m.compute_begin(bufs[2], b)
            for k in range(3, n + 2):
                t = m.compute_begin(bufs[k], b)
                m.compute_end(prev)
                prev = t
            res = m.compute_end(prev)
        else:
            for k in range(2, n + 2):
                res = m.compute(bufs[k], b)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ok = res["valid"].astype(bool)
        return dict(variant=f"{precision} {'chained' if fused else 'staged'}", shells=list(shells), frames=n,
                    ms_per_frame=round(1e3 * dt / n, 3), frames_per_s=round(n / dt, 2), valid=int(ok.sum()),
                    mean_gauss_curv=float(np.abs(res["gauss_curv"][ok]).mean()))

    for shells in ((0, 0), (2, 0), (3, 2)):
        for precision, fused in (("f64", False), ("f32", False), ("f32", True)):
            print(json.dumps(run(precision, fused, shells)), flush=True)


if __name__ == "__main__":
    main()
