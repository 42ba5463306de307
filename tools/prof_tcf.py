#!/usr/bin/env python
"""One shape of tools/bench_tcf.py, the fused call only, for a kernel trace of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/prof_tcf.py a 5

The per-kernel times of the stats file (tcf_box / tcf_vector / tcf_fold / tcf_lag / tcf_finish) say what part of the call's time
each stage takes; bench_tcf.py itself times whole calls.  No counters in that run.
Usage: prof_tcf.py SHAPE [reps]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    import bench_tcf
    shape, reps = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "5"
    sys.argv = [sys.argv[0], reps, shape, "--fused-only"]
    bench_tcf.main()
    print(f"shape {shape}: {reps} calls")


if __name__ == "__main__":
    main()
