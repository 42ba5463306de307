#!/usr/bin/env python
"""One shape of tools/bench_mindist.py, the fused call only, for a kernel trace of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/prof_mindist.py a 5

The per-kernel times of the stats file (md_rows / md_groups / md_gather / md_rowfold / md_framefold / md_timefold and the partition's kernels)
say what part of the call's time each stage takes; the pair kernels' time against the pairs they evaluate (bench_mindist.py prints
them) is their fraction of the v_fma_f64 issue rate.  bench_mindist.py itself times whole calls.  No counters in that run.
Usage: prof_mindist.py SHAPE [reps]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    import bench_mindist
    shape, reps = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "5"
    sys.argv = [sys.argv[0], reps, shape, "--fused-only"]
    bench_mindist.main()
    print(f"shape {shape}: {reps} calls")


if __name__ == "__main__":
    main()
