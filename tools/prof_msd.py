#!/usr/bin/env python
"""One shape of tools/bench_msd.py, the fused call only, for a kernel trace of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/prof_msd.py a 5

The per-kernel times of the stats file (msd_box / msd_unwrap / msd_pieces / msd_lag / msd_finish) say what part of the call's
time each stage takes; bench_msd.py itself times whole calls.  No counters in that run.
Usage: prof_msd.py SHAPE [reps]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    import torch
    from bench_msd import BOX, SHAPES, make_frames
    from molar_amd import api, build
    build.build_library()
    P, per, F, L, dims, drift, os_ = SHAPES[sys.argv[1]]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    eng = api.Engine(0)
    frames = make_frames(torch, P, per, F, 4321 + ord(sys.argv[1]))
    n = P * per
    box9 = torch.tensor(np.diag(BOX).reshape(9), device="cuda", dtype=torch.float32)
    groups = torch.arange(0, n + 1, per, device="cuda", dtype=torch.int64) if per > 1 else None
    refset = torch.arange(n, device="cuda", dtype=torch.int64) if drift else None
    out = api.Msd(torch.zeros(L + 1, device="cuda"), torch.zeros(L + 1, device="cuda"), None, None)
    for _ in range(reps + 1):
        eng.msd(frames, boxes=box9, groups=groups, ref_idx=refset, max_lag=L, origin_stride=os_, dims=dims, out=out)
    eng.synchronize()
    print(f"shape {sys.argv[1]}: {reps + 1} calls")


if __name__ == "__main__":
    main()
