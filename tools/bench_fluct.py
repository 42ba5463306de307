#!/usr/bin/env python
"""The trajectory fluctuations (molar_hip_fluct: mean structure, RMSF, positional covariance after a fit) against the route a
caller had before it: fit_rmsd_batch(apply=True) on a COPY of the block, torch.mean / torch.var over the frames and, for the
covariance, (X - m)^T (X - m) / F in f64 through torch.matmul.  Everything is resident in device memory; the selection is
the identity, so the baseline needs no gather.

Shapes:  (a) RMSF only, F = 1024, n = 100 000;  (b) PCA of C-alpha, F = 10 000, n = 1000;  (c) F = 2048, n = 5000;
(d) F = 256, n = 3000.  (b) - (d) ask for the covariance.  Frames are a random structure plus per-frame noise under a random
rotation per frame, unit masses, the reference is frame 0.

Before anything is timed the two routes are compared (the baseline rounds the fitted frames to f32 before its statistics are
formed: that difference is the baseline's own, the figures are in the row).  Timing: a warm-up, then `reps` repetitions of
each route, the two ALTERNATED, each bracketed by a pair of events on torch's stream - the first recorded after a device-wide
synchronisation, the second after the engine's stream has been waited for; median, minimum and maximum in ms.

Also per shape: for the covariance shapes the END-TO-END f64 FLOP/s - the product's work 2 * (3n)(3n + 16)/2 * F over the time
of the WHOLE call - and that figure as a fraction of the back-to-back issue rate of v_mfma_f64_16x16x4_f64 measured in the same
run, before the engine opens the device, by profiles/microbench/mfma_f64_rate (kernel times need a trace run of their own:
tools/prof_fluct.py); for the RMSF-only shape the bytes of its four sweeps over the frames (4 * 12 F n) over the time of the
whole call.  One JSON line per shape; the lines go to stdout and, with --write[=PATH], to profiles/fluct.txt (or PATH).
Usage: python tools/bench_fluct.py [reps] [shapes, e.g. abd] [--write[=PATH]]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
SHAPES = {"a": (1024, 100000, False), "b": (10000, 1000, True), "c": (2048, 5000, True), "d": (256, 3000, True)}


def make_frames(torch, key):
    """The block of a shape on the device: a structure of ~2 nm plus 0.1 nm of noise, every frame turned by a random rotation."""
    F, n, _ = SHAPES[key]
    gen = torch.Generator(device="cuda").manual_seed(4321 + ord(key))
    base = torch.randn((1, n, 3), device="cuda", generator=gen) * 2.0
    q = torch.randn((F, 4), device="cuda", generator=gen)
    q = q / q.norm(dim=1, keepdim=True)
    a, b, c, d = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c),
                     2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b),
                     2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d], dim=1).reshape(F, 3, 3)
    R[0] = torch.eye(3, device="cuda")
    out = torch.empty((F, n, 3), device="cuda")
    for f0 in range(0, F, 128):                     # in slabs: the noise of the largest shape is 1.2 GB
        noisy = base + 0.1 * torch.randn((min(128, F - f0), n, 3), device="cuda", generator=gen)
        out[f0:f0 + 128] = torch.einsum("fde,fke->fkd", R[f0:f0 + 128], noisy)
    return out.contiguous()


def main():
    import torch
    from bench_rmsd_matrix import mfma_roof
    from molar_amd import api, build
    build.build_library()
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 20
    shapes = args[1] if len(args) > 1 else "abcd"
    roof, roof_text = mfma_roof()                   # a child process of its own, before this one opens the device
    eng = api.Engine(0)
    lines = [json.dumps({"mfma_f64_16x16x4_roof_tflops": roof, "microbench": roof_text.strip().splitlines()})]
    print(lines[0], flush=True)

    def bracket(fn):
        torch.cuda.synchronize()
        eng.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        eng.synchronize()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def stats(ts):
        ts = np.array(ts)
        return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(ts.min()), 4), "max_ms": round(float(ts.max()), 4)}

    for key in shapes:
        F, n, want_cov = SHAPES[key]
        frames = make_frames(torch, key)
        ones = torch.ones(n, device="cuda")
        ref0 = frames[0].clone()
        out = api.Fluctuations(torch.zeros((n, 3), device="cuda"), torch.zeros(n, device="cuda"),
                               torch.zeros((3 * n, 3 * n), device="cuda") if want_cov else None, None)
        keep = {}

        def fused():
            keep["fused"] = eng.fluctuations(frames, cov=want_cov, out=out)

        def baseline():
            work = frames.clone()                                          # fit_rmsd_batch(apply) moves the frames it is given
            eng.fit_rmsd_batch(work, ones, ref0, apply=True)
            mean = work.mean(dim=0)
            rmsf = work.var(dim=0, unbiased=False).sum(dim=1).sqrt()
            cov = None
            if want_cov:
                X = (work - mean).reshape(F, 3 * n).double()
                cov = torch.matmul(X.T, X) / F
            keep["base"] = (mean, rmsf, cov)

        fused()
        eng.synchronize()
        baseline()
        torch.cuda.synchronize()
        got, (bm, br, bc) = keep["fused"], keep["base"]
        diff = {"mean_abs": float((got.mean - bm).abs().max()), "rmsf_abs": float((got.rmsf - br).abs().max()),
                "rmsf_scale": float(br.max())}
        if want_cov:
            diff["cov_abs"] = float((got.cov.double() - bc).abs().max())
            diff["cov_scale"] = float(bc.diagonal().max())
            del bc
        keep.clear()
        torch.cuda.empty_cache()
        tf, tb = [], []
        for _ in range(reps):                                              # the two routes take turns
            tf.append(bracket(fused))
            tb.append(bracket(baseline))
            keep.clear()
        tf, tb = stats(tf), stats(tb)
        ws, ks = api.fluct_plan(F, n, want_cov)
        row = {"shape": key, "F": F, "n": n, "cov": want_cov, "ksplits": ks, "workspace_MB": round(ws / 2 ** 20, 1), "fused": tf, "baseline": tb,
               "baseline_over_fused": round(tb["median_ms"] / tf["median_ms"], 2), "routes_differ": diff}
        if want_cov:
            flop = 2.0 * (3 * n) * (3 * n + 16) / 2 * F
            row["end_to_end_tflops"] = round(flop / (tf["median_ms"] * 1e-3) / 1e12, 2)
            row["end_to_end_fraction_of_mfma_roof"] = round(flop / (tf["median_ms"] * 1e-3) / 1e12 / roof, 3)
        else:
            row["sweep_bytes_MB"] = round(4 * 12 * F * n / 1e6, 1)
            row["end_to_end_sweep_TB_per_s"] = round(4 * 12 * F * n / (tf["median_ms"] * 1e-3) / 1e12, 3)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        del frames, out, ref0
        torch.cuda.empty_cache()
    write = [a for a in sys.argv[1:] if a.startswith("--write")]
    if write:
        dst = write[0].split("=", 1)[1] if "=" in write[0] else os.path.join(ROOT, "profiles", "fluct.txt")
        with open(dst, "w") as f:
            f.write("# python tools/bench_fluct.py %d %s --write\n" % (reps, shapes))
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
