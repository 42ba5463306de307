#!/usr/bin/env python
"""One shape of tools/bench_sfactor.py, the fused call only, for a kernel trace of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/prof_sfactor.py a 5

The per-kernel times of the stats file (sf_gram / sf_finish / sf_products / sf_bins / sf_shell_* and the partition's kernels)
say what part of the call's time each stage takes; the gram kernel's time against the flop it issues (bench_sfactor.py prints
them) is its fraction of the f64 MFMA roof.  bench_sfactor.py itself times whole calls.  No counters in that run.
Usage: prof_sfactor.py SHAPE [reps]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    import bench_sfactor
    shape, reps = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "5"
    sys.argv = [sys.argv[0], reps, shape, "--fused-only"]
    bench_sfactor.main()
    print(f"shape {shape}: {reps} calls")


if __name__ == "__main__":
    main()
