#!/usr/bin/env python
"""One shape of tools/bench_rmsd_matrix.py, the fused call only, for a kernel trace of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/prof_rmsd_matrix.py a 10

The per-kernel times of the stats file (tb_centre / rm_pack / rm_g / rm_gram / rm_finish) say what part of the call's time
each stage takes; bench_rmsd_matrix.py itself only times the whole call.  Usage: prof_rmsd_matrix.py SHAPE [reps]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    import torch
    from bench_rmsd_matrix import SHAPES
    from molar_amd import api, build
    build.build_library()
    F1, F2, n = SHAPES[sys.argv[1]]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    eng = api.Engine(0)
    gen = torch.Generator(device="cuda").manual_seed(1234 + ord(sys.argv[1]))
    base = torch.randn((1, n, 3), device="cuda", generator=gen) * 2.0
    fr1 = (base + 0.3 * torch.randn((F1, n, 3), device="cuda", generator=gen)).contiguous()
    fr2 = (base + 0.3 * torch.randn((F2, n, 3), device="cuda", generator=gen)).contiguous() if F2 else None
    out = torch.zeros((F1, F2 or F1), device="cuda")
    for _ in range(reps + 1):
        eng.rmsd_matrix(fr1, frames2=fr2, out=out)
    eng.synchronize()
    print(f"shape {sys.argv[1]}: {reps + 1} calls")


if __name__ == "__main__":
    main()
