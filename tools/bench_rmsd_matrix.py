#!/usr/bin/env python
"""The all-pairs RMSD matrix (molar_hip_rmsd_matrix) against the route a caller had before it: one fit_rmsd_batch call with
apply=False per reference frame, each of which reads the whole block again.  Everything is resident in device memory.

Shapes:  (a) F = 256, n = 100 000;  (b) F = 1024, n = 10 000;  (c) F = 4096, n = 1000 (output-bound);  (d) 256 x 1024
rectangular, n = 10 000.  Frames are a random structure plus per-frame noise, unit masses, identity selection.

Before anything is timed the two routes are compared on the columns the baseline computes (the f32 route's own rounding:
1e-4 relative is asserted, the figure is in the row).  Timing: a warm-up, then `reps` repetitions, each bracketed by a pair of events on torch's stream - the first
recorded after a device-wide synchronisation, the second after the engine's stream has been waited for; median, minimum
and maximum in ms.  The baseline runs `BASE_ROWS` reference frames per repetition where all F would take minutes; its time is
scaled by F / BASE_ROWS and the row says so ("baseline_scaled_from").

Also per shape: the END-TO-END f64 FLOP/s - the Gram product's work (2 * 9 * n * pairs, pairs = F (F + 1) / 2 in the symmetric
form) over the time of the WHOLE call: centres, pack, G, the early 16-byte wait, Gram, finish and the launches - and that figure
as a fraction of the back-to-back issue rate of v_mfma_f64_16x16x4_f64 measured in the same run, before the engine opens the
device, by profiles/microbench/mfma_f64_rate (compiled on first use).  It is a lower bound of what the Gram kernel alone
reaches; kernel times need a trace run of their own.  Then the algorithmic HBM bytes 8 * 3 * n * (F1 + F2) + 4 * F1 * F2, and
the bytes the call moves by its own layout (f32 frames read twice, packed f64 operands written once and read by the tiles).
One JSON line per shape; the lines go to stdout and, with --write[=PATH], to profiles/rmsd_matrix.txt (or PATH).
Usage: python tools/bench_rmsd_matrix.py [reps] [shapes, e.g. abd] [--write[=PATH]]"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BASE_ROWS = 16
SHAPES = {"a": (256, 0, 100000), "b": (1024, 0, 10000), "c": (4096, 0, 1000), "d": (256, 1024, 10000)}


def mfma_roof():
    """TFLOP/s of back-to-back f64 MFMAs, one wave per SIMD with independent accumulators (the best row of the microbenchmark)."""
    src = os.path.join(ROOT, "profiles", "microbench", "mfma_f64_rate.hip")
    exe = src[:-4]
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", src, "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, check=True).stdout
    rows = [dict(zip(ln.split()[0::2], ln.split()[1::2])) for ln in out.splitlines() if ln.startswith("waves_per_simd")]
    one = [float(r["tflops"]) for r in rows if r["waves_per_simd"] == "1"]
    return max(one), out


def main():
    import torch
    from molar_amd import api, build
    build.build_library()
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 20
    shapes = args[1] if len(args) > 1 else "abcd"
    roof, roof_text = mfma_roof()                   # a child process of its own, before this one opens the device
    eng = api.Engine(0)
    lines = [json.dumps({"mfma_f64_16x16x4_roof_tflops": roof, "microbench": roof_text.strip().splitlines()})]
    print(lines[0], flush=True)

    def timeit(fn, n=reps):
        fn()                                        # warm-up (buffers grow here)
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            eng.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            eng.synchronize()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts = np.array(ts)
        return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(ts.min()), 4), "max_ms": round(float(ts.max()), 4)}

    for key in shapes:
        F1, F2, n = SHAPES[key]
        gen = torch.Generator(device="cuda").manual_seed(1234 + ord(key))
        base = torch.randn((1, n, 3), device="cuda", generator=gen) * 2.0
        fr1 = (base + 0.3 * torch.randn((F1, n, 3), device="cuda", generator=gen)).contiguous()
        fr2 = (base + 0.3 * torch.randn((F2, n, 3), device="cuda", generator=gen)).contiguous() if F2 else None
        cols = F2 or F1
        out = torch.zeros((F1, cols), device="cuda")
        ones = torch.ones(n, device="cuda")
        targets = fr2 if F2 else fr1                # the baseline fits the ROW block onto one reference frame: a column of the matrix
        rows = min(BASE_ROWS, cols)

        def fused():
            eng.rmsd_matrix(fr1, frames2=fr2, out=out)

        def baseline(nref=rows):
            res = []
            for b in range(nref):
                res.append(eng.fit_rmsd_batch(fr1, ones, targets[b], apply=False)["rmsd"])
            return res

        fused()
        eng.synchronize()
        got = out.cpu().numpy()
        want = np.stack(baseline(), axis=1)
        scale = np.maximum(want, 1e-3)
        worst = float(np.max(np.abs(got[:, :rows] - want) / scale))
        assert worst < 1e-4, f"shape {key}: the two routes differ by {worst:.3g} relative"
        tf = timeit(fused)
        tb = timeit(baseline, max(3, reps // 4))
        factor = cols / rows
        pairs = F1 * (F1 + 1) // 2 if not F2 else F1 * F2
        flop = 2.0 * 9 * n * pairs
        ws, ks = api.rmsd_matrix_plan(F1, F2, n)
        row = {
            "shape": key, "F1": F1, "F2": F2, "n": n, "ksplits": ks, "workspace_MB": round(ws / 2 ** 20, 1),
            "fused": tf, "baseline_per_call_ms": round(tb["median_ms"] / rows, 4), "baseline_scaled_from": rows,
            "baseline_ms": {k: round(v * factor, 2) for k, v in tb.items()},
            "baseline_over_fused": round(tb["median_ms"] * factor / tf["median_ms"], 1),
            "baseline_min_over_fused_max": round(tb["min_ms"] * factor / tf["max_ms"], 1),
            "routes_differ_rel": worst,
            "end_to_end_tflops": round(flop / (tf["median_ms"] * 1e-3) / 1e12, 2),
            "end_to_end_fraction_of_mfma_roof": round(flop / (tf["median_ms"] * 1e-3) / 1e12 / roof, 3),
            "algorithmic_MB": round((8 * 3 * n * (F1 + F2) + 4 * F1 * cols) / 1e6, 1),
            "layout_MB": round((2 * 4 * 3 * n * (F1 + F2) + 8 * 3 * n * (F1 + F2) + 4 * F1 * cols) / 1e6, 1),
            "operand_reads_MB_if_nothing_hit_cache": round(8 * 3 * n * 16 * (pairs / 256.0) * (1 + 0.5) / 1e6, 1),
        }
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        del fr1, fr2, out
        torch.cuda.empty_cache()
    write = [a for a in sys.argv[1:] if a.startswith("--write")]
    if write:
        dst = write[0].split("=", 1)[1] if "=" in write[0] else os.path.join(ROOT, "profiles", "rmsd_matrix.txt")
        with open(dst, "w") as f:
            f.write("# python tools/bench_rmsd_matrix.py %d %s --write\n" % (reps, shapes))
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
