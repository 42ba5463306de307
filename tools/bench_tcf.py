#!/usr/bin/env python
"""The time correlation functions of vectors (molar_hip_tcf: a vector per tuple and frame, P1 and P2 of u(t) . u(t + tau) over
all time origins) against the two routes a caller had before it, both written here in torch f64 on the device:

  (B) the same arithmetic launch by launch: index gathers, the minimum image by `round`, the normalisation, then ONE PAIR OF
      SLICE OPS PER LAG: d = (u[tau::os] * u[:F - tau:os]).sum(-1), its mean and the mean of its square per group.  Timed on
      `--lags-timed` lags spread evenly over 0 .. max_lag and scaled by (L + 1) / lags timed; the scaling is in the output;
  (C) the Wiener-Khinchin route: torch.fft.rfft of the zero-padded components - 3 transforms for P1, the 6 products u_a u_b
      (weights 1, 1, 1, 2, 2, 2) for P2 - in slabs of vectors, every origin and every lag up to F - 1 (no origin stride), its peak
      extra device memory reported.

Shapes:  (a) water: 200 000 O-H vectors x 1024 frames x 257 lags, one group, P1 + P2;  (b) NMR: 1000 N-H vectors x 65 536 frames
x 8193 lags, per-vector curves and s2;  (c) lipids: 8000 tail vectors in 2 groups x 8192 frames x 4097 lags under per-frame
boxes;  (e) as (c) with origin_stride 16;  (d) velocity autocorrelation, kind 1 / RAW: 100 000 atoms x 2048 frames x 513 lags.
Frames are random f32 numbers resident on the device (the cost does not depend on the values).

Before anything is timed the routes are compared with the fused call's outputs on the lags route (B) computes and (os = 1) on
all lags of route (C).  Timing: a warm-up, then `reps` repetitions, the routes taking turns, each bracketed by a pair of events
- the first recorded after a device-wide synchronisation, the second after the engine's stream has been waited for; median,
minimum and maximum in ms.

Also per shape: the pair evaluations, the lag stage's time as the difference between the full call and the same call asked for
the mean alone (which runs the vector stage and the fold but does not store the f64 vectors: the difference charges that
store to the lag stage; kernel times proper need a trace run, tools/prof_tcf.py), the pair rate over that time and over the
whole call, that rate times the operations per pair (5, 4 without P2) as a fraction of the back-to-back v_fma_f64 issue rate
measured in the same run, before the engine opens the device, by profiles/microbench/fma_f64_rate; the same call with
MOLAR_HIP_TCF_R = 2 and 1 (lags per lane; 1 is the plain one-lag-per-lane form); and the yardstick: molar_hip_msd's lag stage
(msd_lag_kernel, unchanged) on the same (particles, frames, lags), its triple rate times its 8 operations per triple (3 x (sub,
fma) + 2) as a fraction of the same roof.  The measured effect of a scalar-register operand on v_fma_f64
(profiles/microbench/fma_f64_sgpr) goes first.  One JSON line per shape; the lines go to stdout and, with --write[=PATH], to
profiles/tcf.txt (or PATH).
Usage: python tools/bench_tcf.py [reps] [shapes, e.g. acd] [--lags-timed=64] [--fused-only] [--write[=PATH]]"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
BOX = (6.0, 6.5, 7.0)
# vectors, kind, mode, F, max_lag, groups, per-frame boxes, origin stride, per-vector outputs
SHAPES = {"a": (200000, 2, "unit", 1024, 256, 1, False, 1, False), "b": (1000, 2, "unit", 65536, 8192, 1, False, 1, True),
          "c": (8000, 2, "unit", 8192, 4096, 2, True, 1, False), "e": (8000, 2, "unit", 8192, 4096, 2, True, 16, False),
          "d": (100000, 1, "raw", 2048, 512, 1, False, 1, False)}


def microbench(name):
    src = os.path.join(ROOT, "profiles", "microbench", name + ".hip")
    exe = src[:-4]
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", src, "-o", exe], check=True, timeout=300)
    return subprocess.run([exe], capture_output=True, text=True, timeout=120, check=True).stdout


def fma_roof():
    """1e12 lane FMAs per second of back-to-back v_fma_f64 (the best row of the microbenchmark), and the scalar-operand rows."""
    out = microbench("fma_f64_rate")
    rows = [dict(zip(ln.split()[0::2], ln.split()[1::2])) for ln in out.splitlines() if ln.startswith("waves_per_simd")]
    sg = microbench("fma_f64_sgpr")
    return max(float(r["tfma"]) for r in rows), out, sg


def make_frames(torch, V, kind, F, seed):
    """f32 [F, V * kind, 3]: atom A anywhere in the box, B within +-0.2 nm of A (wrapped into the box on its own)."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    box = torch.tensor(BOX, device="cuda", dtype=torch.float32)
    out = torch.empty((F, V * kind, 3), device="cuda", dtype=torch.float32)
    for f0 in range(0, F, 256):
        n = min(256, F - f0)
        a = torch.rand((n, V, 3), device="cuda", generator=gen) * box
        if kind == 1:
            out[f0:f0 + n] = a - 0.5 * box                   # velocities: both signs
        else:
            b = a + (torch.rand((n, V, 3), device="cuda", generator=gen) * 0.4 - 0.2)
            out[f0:f0 + n, 0::2] = a
            out[f0:f0 + n, 1::2] = b - box * torch.floor(b / box)
    return out


def vectors_torch(torch, frames, kind, unit, boxes):
    """u [F, V, 3] in f64, as the call forms it (orthorhombic minimum image by round)."""
    if kind == 1:
        w = frames.double()
    else:
        w = frames[:, 1::2].double() - frames[:, 0::2].double()
        edge = boxes.double()[..., [0, 4, 8]]
        edge = edge if edge.ndim == 1 else edge[:, None, :]
        w -= edge * torch.round(w / edge)
    if unit:
        w /= torch.sqrt((w * w).sum(-1, keepdim=True))
    return w


def lags_slices(torch, u, taus, os_, labels, G, p2):
    F = u.shape[0]
    c1 = torch.zeros((G, len(taus)), device="cuda", dtype=torch.float64)
    c2 = torch.zeros((G, len(taus)), device="cuda", dtype=torch.float64)
    for k, tau in enumerate(taus):
        d = (u[tau::os_] * u[:F - tau:os_]).sum(-1)                        # [origins, V]
        for g in range(G):
            dg = d if labels is None else d[:, labels == g]
            c1[g, k] = dg.mean()
            if p2:
                c2[g, k] = 1.5 * (dg * dg).mean() - 0.5
    return c1, c2


def lags_fft(torch, u, L, p2, per_vector, labels, G, slab=8192):
    """(c1, c2) over all origins: [G, L + 1] (per_vector: [V, L + 1]), by rfft of the zero-padded series in slabs of vectors."""
    F, V = u.shape[:2]
    cnt = torch.arange(F, F - L - 1, -1, device="cuda", dtype=torch.float64)
    rows = V if per_vector else G
    c1 = torch.zeros((rows, L + 1), device="cuda", dtype=torch.float64)
    c2 = torch.zeros((rows, L + 1), device="cuda", dtype=torch.float64)
    nv = torch.zeros(G, device="cuda", dtype=torch.float64)
    pairs = ((0, 0, 1.0), (1, 1, 1.0), (2, 2, 1.0), (0, 1, 2.0), (0, 2, 2.0), (1, 2, 2.0))
    for v0 in range(0, V, slab):
        x = u[:, v0:v0 + slab].permute(1, 2, 0).contiguous()               # [v, 3, F]
        f = torch.fft.rfft(x, n=2 * F, dim=-1)
        s1 = torch.fft.irfft(f * f.conj(), n=2 * F, dim=-1)[..., :L + 1].sum(1)
        del f
        s2 = None
        if p2:
            s2 = torch.zeros_like(s1)
            for a, b, wgt in pairs:
                f = torch.fft.rfft(x[:, a] * x[:, b], n=2 * F, dim=-1)
                s2 += wgt * torch.fft.irfft(f * f.conj(), n=2 * F, dim=-1)[..., :L + 1]
                del f
        if per_vector:
            c1[v0:v0 + slab] = s1 / cnt
            if p2:
                c2[v0:v0 + slab] = 1.5 * s2 / cnt - 0.5
        else:
            lab = torch.zeros(x.shape[0], device="cuda", dtype=torch.int64) if labels is None else labels[v0:v0 + slab].long()
            c1.index_add_(0, lab, s1)
            if p2:
                c2.index_add_(0, lab, s2)
            nv.index_add_(0, lab, torch.ones_like(lab, dtype=torch.float64))
    if not per_vector:
        c1 = c1 / (nv[:, None] * cnt)
        c2 = 1.5 * c2 / (nv[:, None] * cnt) - 0.5
    return c1, c2


def main():
    import torch
    from molar_amd import api, build
    build.build_library()
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    reps = int(args[0]) if args else 20
    shapes = args[1] if len(args) > 1 else "abced"
    lags_timed = next((int(a.split("=")[1]) for a in flags if a.startswith("--lags-timed=")), 64)
    fused_only = "--fused-only" in flags
    lines = []
    roof = None
    if not fused_only:
        roof, roof_text, sgpr_text = fma_roof()             # child processes of their own, before this one opens the device
        lines.append(json.dumps({"v_fma_f64_roof_tera_lane_fma_per_s": roof, "microbench": roof_text.strip().splitlines(),
                                 "scalar_operand": sgpr_text.strip().splitlines()}))
        print(lines[0], flush=True)
    eng = api.Engine(0)

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
        return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(ts.min()), 3), "max_ms": round(float(ts.max()), 3)}

    for key in shapes:
        V, kind, mode, F, L, G, pfb, os_, per_vector = SHAPES[key]
        unit = mode == "unit"
        frames = make_frames(torch, V, kind, F, 4321 + ord(key))
        tuples = torch.arange(V * kind, device="cuda", dtype=torch.int64).reshape(V, kind)
        labels = (torch.arange(V, device="cuda", dtype=torch.int32) % G).contiguous() if G > 1 else None
        box9 = torch.tensor(np.diag(BOX).reshape(9), device="cuda", dtype=torch.float32)
        boxes = (box9[None] * (1 + 0.01 * torch.rand((F, 1), device="cuda"))).contiguous() if pfb else box9
        if kind == 1:
            boxes = None
        want = (("c1_vec", "c2_vec", "s2") if per_vector else ("c1", "c2", "nvalid")) if unit else ("c1", "nvalid")
        rows = V if per_vector else G
        mk = lambda: torch.zeros((rows, L + 1), device="cuda")
        out = [None] * 8
        for nm in want:
            i = api.VectorCorrelations._fields.index(nm)
            out[i] = mk() if nm[:2] in ("c1", "c2") else torch.zeros(V if nm == "s2" else G, device="cuda", dtype=torch.int64 if nm == "nvalid" else torch.float32)
        mean_out = [None] * 5 + [torch.zeros((V, 3), device="cuda")] + [None] * 2
        keep = {}

        def fused():
            keep["fused"] = eng.vector_correlations(frames, tuples, labels=labels, ngroups=G, boxes=boxes, mode=mode, max_lag=L, origin_stride=os_, want=want, out=out)

        def mean_only():
            eng.vector_correlations(frames, tuples, labels=labels, ngroups=G, boxes=boxes, mode=mode, max_lag=L, origin_stride=os_, want=("mean",), out=mean_out)

        if fused_only:
            for _ in range(reps):
                fused()
            eng.synchronize()
            continue
        taus = sorted(set(np.linspace(0, L, lags_timed).astype(int).tolist()))
        tt = torch.tensor(taus, device="cuda")

        def route_b():
            keep["b"] = lags_slices(torch, vectors_torch(torch, frames, kind, unit, boxes), taus, os_, labels, 1 if per_vector else G, unit)

        def route_c():
            keep["c"] = lags_fft(torch, vectors_torch(torch, frames, kind, unit, boxes), L, unit, per_vector, labels, G)

        fused()
        eng.synchronize()
        mean_only()
        eng.synchronize()
        got = keep["fused"]
        diff = {}
        if per_vector:                                      # route (B) gives the mean over the vectors: compare with the mean of the rows
            route_b()
            diff["B_c1_abs"] = float((got.c1_vec.double().mean(0)[tt] - keep["b"][0][0]).abs().max())
            diff["B_c2_abs"] = float((got.c2_vec.double().mean(0)[tt] - keep["b"][1][0]).abs().max())
        else:
            route_b()
            diff["B_c1_abs"] = float((got.c1.double()[:, tt] - keep["b"][0]).abs().max())
            if unit:
                diff["B_c2_abs"] = float((got.c2.double()[:, tt] - keep["b"][1]).abs().max())
        keep.pop("b")
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        route_c()
        torch.cuda.synchronize()
        c_peak = torch.cuda.max_memory_allocated() - base
        if os_ == 1:
            g1, g2 = (got.c1_vec, got.c2_vec) if per_vector else (got.c1, got.c2)
            diff["C_c1_abs"] = float((g1.double() - keep["c"][0]).abs().max())
            if unit:
                diff["C_c2_abs"] = float((g2.double() - keep["c"][1]).abs().max())
        keep.clear()
        torch.cuda.empty_cache()
        tf, tm, tb, tc = [], [], [], []
        for _ in range(reps):                                              # the routes take turns
            tf.append(bracket(fused))
            tm.append(bracket(mean_only))
            tb.append(bracket(route_b))
            keep.clear()
            tc.append(bracket(route_c))
            keep.clear()
        tf, tm, tb, tc = stats(tf), stats(tm), stats(tb), stats(tc)
        # lags per lane: the same call with R = 2 and R = 1
        by_r = {}
        for r in ("2", "1"):
            os.environ["MOLAR_HIP_TCF_R"] = r
            fused()
            by_r["R=" + r] = stats([bracket(fused) for _ in range(max(3, reps // 4))])
        del os.environ["MOLAR_HIP_TCF_R"]
        # the yardstick: msd_lag_kernel on the same particles, frames and lags (kind-1 view of the first atom of every tuple)
        mo = api.Msd(torch.zeros(L + 1, device="cuda"), torch.zeros(L + 1, device="cuda"), None, None)
        do = api.Msd(None, None, None, torch.zeros((F, V, 3), device="cuda"))
        idx = torch.arange(V, device="cuda", dtype=torch.int64) * kind

        def msd_full():
            eng.msd(frames, idx=idx, max_lag=L, origin_stride=os_, out=mo)

        def msd_disp():
            eng.msd(frames, idx=idx, max_lag=L, origin_stride=os_, msd=False, m4=False, disp=True, out=do)

        msd_full(); msd_disp()
        n_y = max(3, reps // 4)
        ty = stats([bracket(msd_full) for _ in range(n_y)])
        tyd = stats([bracket(msd_disp) for _ in range(n_y)])
        del mo, do
        ws = api.tcf_plan(F, V, G, L, pfb, True, not per_vector)
        n_tau = api.tcf_lags(F, L, os_)
        pairs = float(V) * float(n_tau.sum())
        ops = 5 if unit else 4
        lag_ms = tf["median_ms"] - tm["median_ms"]
        msd_lag_ms = ty["median_ms"] - tyd["median_ms"]
        scale = (L + 1) / len(taus)
        row = {"shape": key, "vectors": V, "kind": kind, "mode": mode, "F": F, "max_lag": L, "groups": G, "per_frame_boxes": pfb, "origin_stride": os_,
               "outputs": list(want), "workspace_MB": round(ws[0] / 2 ** 20, 1), "plan": dict(zip(("frame_chunk", "vec_chunk", "lag_block", "lags_per_lane", "segment", "window"), ws[1:])),
               "fused": tf, "fused_mean_only": tm, "fused_other_lags_per_lane": by_r,
               "route_B_slices_timed": tb, "route_B_lags_timed": len(taus), "route_B_scaled_to_all_lags_ms": round(tb["median_ms"] * scale, 1),
               "route_B_scaling": "median x (max_lag + 1) / lags timed; the vectors are formed once per run, so the scaling overstates that part",
               "route_C_fft": tc, "route_C_note": "every origin and every lag up to F - 1" + (" (cannot use origin_stride)" if os_ > 1 else ""),
               "route_C_peak_extra_MB": round(c_peak / 2 ** 20, 1),
               "B_scaled_over_fused_median": round(tb["median_ms"] * scale / tf["median_ms"], 2), "C_median_over_fused_median": round(tc["median_ms"] / tf["median_ms"], 2),
               "routes_differ": diff, "pairs": pairs, "lag_stage_ms_by_difference": round(lag_ms, 3),
               "lag_stage_gpairs_per_s": round(pairs / (lag_ms * 1e-3) / 1e9, 1) if lag_ms > 0 else None,
               "end_to_end_gpairs_per_s": round(pairs / (tf["median_ms"] * 1e-3) / 1e9, 1),
               "lag_stage_fraction_of_fma_roof": round(pairs * ops / (lag_ms * 1e-3) / 1e12 / roof, 3) if lag_ms > 0 else None,
               "yardstick_msd": {"full": ty, "disp_only": tyd, "lag_stage_ms_by_difference": round(msd_lag_ms, 3),
                                 "lag_stage_fraction_of_fma_roof": round(pairs * 8 / (msd_lag_ms * 1e-3) / 1e12 / roof, 3) if msd_lag_ms > 0 else None}}
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        del frames, out, mean_out
        torch.cuda.empty_cache()
    write = [a for a in flags if a.startswith("--write")]
    if write:
        dst = write[0].split("=", 1)[1] if "=" in write[0] else os.path.join(ROOT, "profiles", "tcf.txt")
        with open(dst, "w") as f:
            f.write("# python tools/bench_tcf.py %d %s --lags-timed=%d --write\n" % (reps, shapes, lags_timed))
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
