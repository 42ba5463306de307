#!/usr/bin/env python
"""One shape of tools/bench_fluct.py, the fused call only, for a kernel trace of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/prof_fluct.py b 10

The per-kernel times of the stats file (tb_centre / fl_fit_sums / fl_rotation / fl_sums / fl_mean / fl_rmsf / fl_pack / fl_cov /
fl_cov_finish) say what part of the call's time each stage takes; bench_fluct.py itself only times the whole call.
Usage: prof_fluct.py SHAPE [reps]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    import torch
    from bench_fluct import SHAPES, make_frames
    from molar_amd import api, build
    build.build_library()
    F, n, want_cov = SHAPES[sys.argv[1]]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    eng = api.Engine(0)
    frames = make_frames(torch, sys.argv[1])
    out = api.Fluctuations(torch.zeros((n, 3), device="cuda"), torch.zeros(n, device="cuda"),
                           torch.zeros((3 * n, 3 * n), device="cuda") if want_cov else None, None)
    for _ in range(reps + 1):
        eng.fluctuations(frames, cov=want_cov, out=out)
    eng.synchronize()
    print(f"shape {sys.argv[1]}: {reps + 1} calls")


if __name__ == "__main__":
    main()
