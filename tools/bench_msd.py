#!/usr/bin/env python
"""The mean-squared displacement (molar_hip_msd: no-jump unwrap, particle displacements, drift removal, the lag sums over all
time origins) against the two routes a caller had before it, both written here in torch f64 on the device:

  (B) unwrap by a minimum-imaged `diff` + `cumsum`, groups by `index_add_`, the drift by a weighted mean, then ONE PAIR OF SLICE
      OPS PER LAG: ((U[tau::os] - U[:F - tau:os])^2).sum(-1), its mean and the mean of its square;
  (C) the same unwrap, then the FFT identity msd = (S1 - 2 S2) / (F - tau) with S2 the autocorrelation through torch.fft.rfft of
      the zero-padded block and S1 by the usual recursion (no origin stride, every lag up to F - 1 computed, no fourth moment).

Shapes:  (a) lipids: P = 4096 single-atom particles, F = 8192, max_lag = 4096, lateral (xy), drift removal over all of them;
(b) water: 300 000 atoms in 100 000 groups of three, F = 1024, max_lag = 512;  (c) ions: P = 256, F = 65 536, max_lag = 1024;
(d) as (a) with origin_stride = 16.  Frames are random walks wrapped into an orthorhombic box, f32, resident on the device.

Before anything is timed the routes are compared with the fused call's outputs (largest relative difference of msd over the
lags > 0; of m4 for route B).  Timing: a warm-up, then `reps` repetitions, the routes taking turns, each bracketed by a pair of
events - the first recorded after a device-wide synchronisation, the second after the engine's stream has been waited for;
median, minimum and maximum in ms.  GATE: the fused call's median is below route (B)'s MINIMUM.  Route (C) is reported, not
gated: its time, its peak extra device memory and its largest relative deviation from the longdouble reference of
tests/msd_ref.py on a scaled-down copy of the shape (as is the fused call's, beside it).

Also per shape: the particle-origin-lag triples, the lag stage's time as the difference between the full call and the same call
asked for `disp` only (kernel times proper need a trace run: tools/prof_msd.py), the triple rate over that time and over the
whole call, that rate times the FMAs per triple (components + 1) as a fraction of the back-to-back v_fma_f64 issue rate measured
in the same run, before the engine opens the device, by profiles/microbench/fma_f64_rate, and the workspace from msd_plan.
One JSON line per shape; the lines go to stdout and, with --write[=PATH], to profiles/msd.txt (or PATH).
Usage: python tools/bench_msd.py [reps] [shapes, e.g. acd] [--write[=PATH]]"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
BOX = (6.0, 6.5, 7.0)
# P, atoms per particle, F, max_lag, dims, drift removal, origin stride
SHAPES = {"a": (4096, 1, 8192, 4096, 3, True, 1), "b": (100000, 3, 1024, 512, 7, False, 1), "c": (256, 1, 65536, 1024, 7, False, 1),
          "d": (4096, 1, 8192, 4096, 3, True, 16)}


def fma_roof():
    """1e12 lane FMAs per second of back-to-back v_fma_f64 (the best row of the microbenchmark)."""
    src = os.path.join(ROOT, "profiles", "microbench", "fma_f64_rate.hip")
    exe = src[:-4]
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", src, "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, check=True).stdout
    rows = [dict(zip(ln.split()[0::2], ln.split()[1::2])) for ln in out.splitlines() if ln.startswith("waves_per_simd")]
    return max(float(r["tfma"]) for r in rows), out


def make_frames(torch, P, per, F, seed, step=0.2):
    """A wrapped f32 walk [F, P * per, 3] on the device: the atoms of a particle share its steps (uniform in +-step of the box),
    sit 0.1 nm apart and jitter by 0.01 nm."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    box = torch.tensor(BOX, device="cuda", dtype=torch.float64)
    pos = (torch.rand((F, P, 1, 3), device="cuda", dtype=torch.float64, generator=gen) * 2 - 1) * step * box
    pos[0] = torch.rand((P, 1, 3), device="cuda", dtype=torch.float64, generator=gen) * box
    pos = torch.cumsum(pos, dim=0)
    offs = 0.1 * torch.randn((1, P, per, 3), device="cuda", dtype=torch.float64, generator=gen)
    out = torch.empty((F, P * per, 3), device="cuda", dtype=torch.float32)
    for f0 in range(0, F, 256):                     # in slabs: the jitter of the largest shape is 7 GB
        x = pos[f0:f0 + 256] + offs
        x = (x + 0.01 * torch.randn(x.shape, device="cuda", dtype=torch.float64, generator=gen)).reshape(x.shape[0], P * per, 3)
        out[f0:f0 + 256] = (x - box * torch.floor(x / box)).float()
    return out


def unwrap_torch(torch, frames, box, per, ref_all):
    """U [F, P, 3] in f64: minimum-imaged diff + cumsum, groups by index_add_ (unit weights), the drift of all atoms removed."""
    x = frames.double()
    d = x[1:] - x[:-1]
    d -= box * torch.round(d / box)
    u = torch.zeros_like(x)
    torch.cumsum(d, dim=0, out=u[1:])
    del x, d
    if ref_all:
        drift = u.mean(dim=1, keepdim=True)
    if per > 1:
        P = u.shape[1] // per
        g = torch.arange(P, device="cuda").repeat_interleave(per)
        U = torch.zeros((u.shape[0], P, 3), device="cuda", dtype=torch.float64)
        U.index_add_(1, g, u)
        U /= per
    else:
        U = u
    if ref_all:
        U = U - drift
    return U


def lags_slices(torch, U, L, os_, comp):
    F = U.shape[0]
    msd = torch.zeros(L + 1, device="cuda", dtype=torch.float64)
    m4 = torch.zeros(L + 1, device="cuda", dtype=torch.float64)
    V = U[..., comp]
    for tau in range(L + 1):
        r2 = ((V[tau::os_] - V[:F - tau:os_]) ** 2).sum(-1)
        msd[tau] = r2.mean()
        m4[tau] = (r2 * r2).mean()
    return msd, m4


def lags_fft(torch, U, L, comp):
    F = U.shape[0]
    V = U[..., comp].permute(1, 2, 0).contiguous()                 # [P, nd, F]
    sq = (V * V).sum(1)                                            # [P, F]
    f = torch.fft.rfft(V, n=2 * F, dim=-1)
    s2 = torch.fft.irfft(f * f.conj(), n=2 * F, dim=-1)[..., :F].sum(1)        # [P, F]
    del f
    # S1[tau] = sum_{t < F - tau} (|U(t)|^2 + |U(t + tau)|^2) = 2 sum(sq) - (the first tau of sq) - (the last tau of sq)
    total = sq.sum(-1, keepdim=True)
    head = torch.cumsum(sq, dim=-1)
    tail = torch.cumsum(sq.flip(-1), dim=-1)
    s1 = 2 * total - torch.cat([torch.zeros_like(total), head[:, :-1]], -1) - torch.cat([torch.zeros_like(total), tail[:, :-1]], -1)
    cnt = torch.arange(F, 0, -1, device="cuda", dtype=torch.float64)
    return ((s1 - 2 * s2) / cnt).mean(0)[:L + 1]


def scaled_down(torch, eng, key):
    """Route (C) and the fused call against the longdouble reference on a small copy of the shape: the largest relative deviations."""
    import msd_ref as mr
    P, per, F, L, dims, drift, os_ = SHAPES[key]
    Ps, Fs = min(P, 16), min(F, 512)
    Ls = min(L, Fs // 2)
    comp = [d for d in range(3) if dims >> d & 1]
    fr = make_frames(torch, Ps, per, Fs, 99)
    box9 = np.diag(BOX).reshape(9)
    groups = np.arange(0, Ps * per + 1, per, dtype=np.uint64) if per > 1 else None
    refset = np.arange(Ps * per, dtype=np.uint64) if drift else None
    ref = mr.msd(fr.cpu().numpy(), boxes=box9, groups=groups, ref_idx=refset, max_lag=Ls, origin_stride=1, dims=dims)
    want = ref["msd"].astype(np.float64)[1:]
    U = unwrap_torch(torch, fr, torch.tensor(BOX, device="cuda", dtype=torch.float64), per, drift)
    c = lags_fft(torch, U, Ls, comp).cpu().numpy()[1:]
    got = eng.msd(fr, boxes=torch.tensor(box9, device="cuda", dtype=torch.float32), groups=None if groups is None else torch.from_numpy(groups.astype(np.int64)).cuda(),
                  ref_idx=None if refset is None else torch.from_numpy(refset.astype(np.int64)).cuda(), max_lag=Ls, dims=dims, m4=False)
    eng.synchronize()
    g = got.msd.double().cpu().numpy()[1:]
    return {"P": Ps, "F": Fs, "max_lag": Ls, "fft_rel_dev": float(np.abs(c / want - 1).max()), "fused_f32_rel_dev": float(np.abs(g / want - 1).max()),
            "largest_excursion2_over_msd1": float((ref["disp"].astype(np.float64) ** 2).sum(-1).max() / want[0])}


def main():
    import torch
    from molar_amd import api, build
    build.build_library()
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 20
    shapes = args[1] if len(args) > 1 else "abcd"
    roof, roof_text = fma_roof()                    # a child process of its own, before this one opens the device
    eng = api.Engine(0)
    lines = [json.dumps({"v_fma_f64_roof_tera_lane_fma_per_s": roof, "microbench": roof_text.strip().splitlines()})]
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
        return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(ts.min()), 3), "max_ms": round(float(ts.max()), 3)}

    gate_ok = True
    for key in shapes:
        P, per, F, L, dims, drift, os_ = SHAPES[key]
        comp = [d for d in range(3) if dims >> d & 1]
        small = scaled_down(torch, eng, key)
        frames = make_frames(torch, P, per, F, 4321 + ord(key))
        n = P * per
        box = torch.tensor(BOX, device="cuda", dtype=torch.float64)
        box9 = torch.tensor(np.diag(BOX).reshape(9), device="cuda", dtype=torch.float32)
        groups = torch.arange(0, n + 1, per, device="cuda", dtype=torch.int64) if per > 1 else None
        refset = torch.arange(n, device="cuda", dtype=torch.int64) if drift else None
        out = api.Msd(torch.zeros(L + 1, device="cuda"), torch.zeros(L + 1, device="cuda"), None, None)
        dout = api.Msd(None, None, None, torch.zeros((F, P, 3), device="cuda"))
        keep = {}

        def fused():
            keep["fused"] = eng.msd(frames, boxes=box9, groups=groups, ref_idx=refset, max_lag=L, origin_stride=os_, dims=dims, out=out)

        def disp_only():
            eng.msd(frames, boxes=box9, groups=groups, ref_idx=refset, max_lag=L, origin_stride=os_, dims=dims, msd=False, m4=False, disp=True, out=dout)

        def route_b():
            keep["b"] = lags_slices(torch, unwrap_torch(torch, frames, box, per, drift), L, os_, comp)

        def route_c():
            keep["c"] = lags_fft(torch, unwrap_torch(torch, frames, box, per, drift), L, comp)

        fused()
        eng.synchronize()
        disp_only()
        eng.synchronize()
        route_b()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        route_c()
        torch.cuda.synchronize()
        c_peak = torch.cuda.max_memory_allocated() - base
        got = keep["fused"]
        bm, b4 = keep["b"]
        diff = {"B_msd_rel": float((got.msd.double()[1:] / bm[1:] - 1).abs().max()), "B_m4_rel": float((got.m4.double()[1:] / b4[1:] - 1).abs().max())}
        if os_ == 1:
            diff["C_msd_rel"] = float((got.msd.double()[1:] / keep["c"][1:] - 1).abs().max())
        keep.clear()
        torch.cuda.empty_cache()
        tf, td, tb, tc = [], [], [], []
        for _ in range(reps):                                              # the routes take turns
            tf.append(bracket(fused))
            td.append(bracket(disp_only))
            tb.append(bracket(route_b))
            keep.clear()
            tc.append(bracket(route_c))
            keep.clear()
        tf, td, tb, tc = stats(tf), stats(td), stats(tb), stats(tc)
        ws, chunk, lb = api.msd_plan(F, n, P, n if drift else 0, L)
        taus = np.arange(L + 1)
        triples = float(P) * float(((F - 1 - taus) // os_ + 1).sum())
        lag_ms = tf["median_ms"] - td["median_ms"]
        ok = tf["median_ms"] < tb["min_ms"]
        gate_ok &= ok
        row = {"shape": key, "P": P, "atoms": n, "F": F, "max_lag": L, "dims": dims, "drift_removal": drift, "origin_stride": os_,
               "workspace_MB": round(ws / 2 ** 20, 1), "particle_chunk": chunk, "lag_block": lb, "fused": tf, "fused_disp_only": td, "route_B_slices": tb,
               "route_C_fft": tc, "route_C_note": "every origin and every lag up to F - 1, no fourth moment" + (" (cannot use origin_stride)" if os_ > 1 else ""),
               "route_C_peak_extra_MB": round(c_peak / 2 ** 20, 1), "B_min_over_fused_median": round(tb["min_ms"] / tf["median_ms"], 2),
               "C_median_over_fused_median": round(tc["median_ms"] / tf["median_ms"], 2), "gate_fused_below_B_min": bool(ok), "routes_differ": diff,
               "scaled_down_vs_longdouble": small, "triples": triples, "lag_stage_ms_by_difference": round(lag_ms, 3),
               "lag_stage_gtriples_per_s": round(triples / (lag_ms * 1e-3) / 1e9, 1) if lag_ms > 0 else None,
               "end_to_end_gtriples_per_s": round(triples / (tf["median_ms"] * 1e-3) / 1e9, 1),
               "lag_stage_fraction_of_fma_roof": round(triples * (len(comp) + 1) / (lag_ms * 1e-3) / 1e12 / roof, 3) if lag_ms > 0 else None}
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        del frames, out, dout
        torch.cuda.empty_cache()
    lines.append(json.dumps({"gate_all_shapes": bool(gate_ok)}))
    print(lines[-1], flush=True)
    write = [a for a in sys.argv[1:] if a.startswith("--write")]
    if write:
        dst = write[0].split("=", 1)[1] if "=" in write[0] else os.path.join(ROOT, "profiles", "msd.txt")
        with open(dst, "w") as f:
            f.write("# python tools/bench_msd.py %d %s --write\n" % (reps, shapes))
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if gate_ok else 1)


if __name__ == "__main__":
    main()
