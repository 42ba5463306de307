#!/usr/bin/env python
"""One shape of tools/bench_vanhove.py, the fused call only, for a kernel trace of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/prof_vanhove.py a 5

The per-kernel times of the stats file (vh_check / the sort's kernels / vh_gather / vh_fold / vh_pair) say what part of the
call's time the prep pass and the pair pass take; the flushes are part of vh_pair (the A/B of bench_vanhove.py --ab against the
in-memory route bounds them).  bench_vanhove.py itself times whole calls.  No counters in that run.
Usage: prof_vanhove.py SHAPE [reps]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    import bench_vanhove
    shape, reps = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "5"
    sys.argv = [sys.argv[0], reps, shape, "--fused-only"]
    bench_vanhove.main()
    print(f"shape {shape}: {reps} calls")


if __name__ == "__main__":
    main()
