#!/usr/bin/env python
"""Self van Hove counts (molar_hip_vanhove: the particle-major gather, then per particle the origins of a pass in registers
against a list of lags, counted on chip by integer atomics) against the route a caller had before it, on the same unwrapped
trajectory in torch f64 on the device:

  (B) per lag: the slice difference x[tau::][::stride] - x[: F - tau : stride] of the components of dims in f64,
      `linalg.vector_norm` (or the one component, signed), the bin formula, and one `torch.bincount` over the flattened
      (group, bin) index with one more bin per group for the pairs outside the range.

Shapes (the ones of DESIGN.md 8f, so that msd and van Hove can be read side by side):  (a) P = 4096 lipids, F = 8192, xy, 16
log-spaced lags, 256 bins;  (b) 100 000 particles in two species, F = 1024, 12 lags, 3-D, 200 bins;  (c) P = 256, F = 65 536,
32 lags including 1 and 2, signed x, 512 bins;  (d) as (a) with origin_stride 16.  The trajectories are f32 random walks
resident on the device.

Timing: a warm-up, then `reps` repetitions, the routes taking turns, each bracketed by a pair of events - the first recorded
after a device-wide synchronisation, the second after the engine's stream has been waited for; median, minimum and maximum in
ms.  GATE: the fused median is below route (B)'s minimum; a shape that loses says so.  Per shape also the plan, whether every
bin of the two routes agrees (and how many differ), the pairs per second, and the pairs times the f64 operations of a pair
counted in the source (nd subtractions, nd fused multiply-adds, the square root, v - lo, the division, the product, the floor
and two compares: 2 nd + 7, or 7 signed; the square root and the division are many instructions each, so this undercounts the
work) as a fraction of the v_fma_f64 issue rate measured in the same run, before the engine opens the device, by
profiles/microbench/fma_f64_rate.  With --ab the fused call is also timed with the combining of equal cells of a wave switched
on and with the counts sent straight to memory, on every shape and on shape (c) with its three shortest lags alone (lag 0
included: every pair of a wave in one cell).  Kernel times proper need a trace run (tools/prof_vanhove.py).
One JSON line per shape; the lines go to stdout and, with --write[=PATH], to profiles/vanhove.txt (or PATH).
Usage: python tools/bench_vanhove.py [reps] [shapes, e.g. ac] [--fused-only] [--ab] [--write[=PATH]]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
STEP = 0.05
# P, F, dims, signed, lags, nbins, (lo, hi), groups, origin_stride
SHAPES = {"a": (4096, 8192, 3, False, 16, 256, (0.0, 6.0), 1, 1),
          "b": (100000, 1024, 7, False, 12, 200, (0.0, 3.0), 2, 1),
          "c": (256, 65536, 1, True, 32, 512, (-16.0, 16.0), 1, 1),
          "d": (4096, 8192, 3, False, 16, 256, (0.0, 6.0), 1, 16)}


def lag_list(F, count, with_short):
    """`count` distinct log-spaced lags below F, the first one 1 and the last one F - 1; with_short: 1 and 2 among them."""
    m = count
    while True:
        cand = np.unique(np.round(np.logspace(0, np.log10(F - 1), m)).astype(np.int64))
        if cand.shape[0] >= count:
            break
        m += 1
    head = np.array([1, 2], np.int64) if with_short else np.array([1], np.int64)
    rest = cand[cand > head[-1]]
    take = count - head.shape[0]
    pick = rest[np.round(np.linspace(0, rest.shape[0] - 1, take)).astype(np.int64)]
    lags = np.concatenate([head, pick])
    assert np.unique(lags).shape[0] == count
    return lags


def make_walk(torch, P, F, seed):
    """f32 [F, P, 3]: Gaussian random walks from the origin, summed in f64."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.empty((F, P, 3), device="cuda", dtype=torch.float32)
    pos = torch.zeros((1, P, 3), device="cuda", dtype=torch.float64)
    for f0 in range(0, F, 256):
        n = min(256, F - f0)
        steps = STEP * torch.randn((n, P, 3), device="cuda", dtype=torch.float64, generator=gen)
        walk = pos + torch.cumsum(steps, dim=0)
        x[f0:f0 + n] = walk.float()
        pos = walk[-1:].clone()
    return x


def route_torch(torch, x, lags, lo, hi, nbins, labels, G, stride, dims, signed):
    """(hist [G, L, nbins], outside [G, L]) by route (B)."""
    F = x.shape[0]
    comp = [d for d in range(3) if dims >> d & 1]
    hist = torch.empty((G, len(lags), nbins), device="cuda", dtype=torch.int64)
    outside = torch.empty((G, len(lags)), device="cuda", dtype=torch.int64)
    base = (labels.long() * (nbins + 1)) if labels is not None else None
    for l, tau in enumerate(int(t) for t in lags):
        a, b = x[0:F - tau:stride][:, :, comp].double(), x[tau:F:stride][:, :, comp].double()
        d = b - a
        v = d[:, :, 0] if signed else torch.linalg.vector_norm(d, dim=2)
        bn = torch.floor((v - lo) / (hi - lo) * nbins).clamp_(0, nbins - 1).long()
        bn = torch.where((v >= lo) & (v < hi), bn, nbins)
        if base is not None:
            bn += base[None, :]
        counts = torch.bincount(bn.reshape(-1), minlength=G * (nbins + 1)).reshape(G, nbins + 1)
        hist[:, l] = counts[:, :nbins]
        outside[:, l] = counts[:, nbins]
    return hist, outside


def timed(torch, eng, fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    eng.synchronize()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    return dict(median=round(float(np.median(ts)), 3), min=round(min(ts), 3), max=round(max(ts), 3))


def with_env(name, value, fn):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        return fn()
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opts = dict(a[2:].split("=", 1) if "=" in a else (a[2:], "") for a in sys.argv[1:] if a.startswith("--"))
    reps = int(args[0]) if args else 20
    shapes = args[1] if len(args) > 1 else "abcd"
    fused_only = "fused-only" in opts
    lines = []
    roof = 0.0
    if not fused_only:
        from bench_tcf import microbench
        text = microbench("fma_f64_rate")            # a child process of its own, before this one opens the device
        rows = [dict(zip(ln.split()[0::2], ln.split()[1::2])) for ln in text.splitlines() if ln.startswith("waves_per_simd")]
        roof = max(float(r["tfma"]) for r in rows)
        lines.append(json.dumps({"v_fma_f64_roof_tera_lane_fma_per_s": roof, "microbench": text.strip().splitlines()}))
        print(lines[0], flush=True)
    import torch
    from molar_amd import api
    eng = api.Engine()
    for key in shapes:
        P, F, dims, signed, nl, nbins, (lo, hi), G, stride = SHAPES[key]
        nd = bin(dims).count("1")
        x = make_walk(torch, P, F, 31)
        lags_np = lag_list(F, nl, key == "c")
        assert lags_np.shape[0] == nl and (np.diff(lags_np) > 0).all() and lags_np[-1] < F
        lags = torch.as_tensor(lags_np).cuda()
        labels = (torch.arange(P, device="cuda") % G).to(torch.int32) if G > 1 else None
        kw = dict(labels=labels, ngroups=G if G > 1 else None, origin_stride=stride, dims=dims, signed=signed, want=("hist", "outside"))
        fused = lambda lg=lags: eng.van_hove(x, lg, (lo, hi), nbins, **kw)
        plan = api.vanhove_plan(F, P, G, nl, nbins, nd)
        pairs = int(sum(P * ((F - 1 - int(t)) // stride + 1) for t in lags_np))
        res = dict(shape=key, particles=P, frames=F, dims=dims, signed=signed, lags=[int(t) for t in lags_np], nbins=nbins, range=[lo, hi], groups=G,
                   origin_stride=stride, pairs=pairs, plan=plan._asdict())
        res["plan"]["workspace_MB"] = round(res["plan"].pop("workspace_bytes") / 2 ** 20, 1)
        got = fused()
        eng.synchronize()
        if not fused_only:
            ref_hist, ref_out = route_torch(torch, x, lags_np, lo, hi, nbins, labels, G, stride, dims, signed)
            differ = int((got.hist != ref_hist).sum()) + int((got.outside != ref_out).sum())
            res["bins_agree"] = differ == 0
            res["bins_that_differ"] = f"{differ} of {ref_hist.numel() + ref_out.numel()}"
            res["pairs_outside"] = int(ref_out.sum())
            ts = {"fused": [], "torch": []}
            for _ in range(reps):
                ts["fused"].append(timed(torch, eng, fused))
                ts["torch"].append(timed(torch, eng, lambda: route_torch(torch, x, lags_np, lo, hi, nbins, labels, G, stride, dims, signed)))
            res["ms_fused"], res["ms_torch"] = stats(ts["fused"]), stats(ts["torch"])
            res["gate_fused_median_below_torch_min"] = "won" if res["ms_fused"]["median"] < res["ms_torch"]["min"] else "**LOST**"
            res["torch_min_over_fused_median"] = round(res["ms_torch"]["min"] / res["ms_fused"]["median"], 2)
        else:
            res["ms_fused"] = stats([timed(torch, eng, fused) for _ in range(reps)])
        sec = res["ms_fused"]["median"] * 1e-3
        res["pairs_per_s"] = float("%.4g" % (pairs / sec))
        if not fused_only:
            ops = 7 if signed else 2 * nd + 7
            res["f64_ops_per_pair_counted"] = ops
            res["fraction_of_fma_issue_rate"] = round(pairs * ops / sec / (roof * 1e12), 4)
        if "ab" in opts:
            variants = {"combined": ("MOLAR_HIP_VANHOVE_COMBINE", "1"), "in_memory": ("MOLAR_HIP_VANHOVE_ONCHIP", "0")}
            cases = {"": lags}
            if key == "c":
                cases["_shortest_lags_0_1_2"] = torch.tensor([0, 1, 2], device="cuda")
            for suffix, lg in cases.items():
                rows = {"plain_on_chip": [], "combined": [], "in_memory": []}
                for _ in range(reps):
                    rows["plain_on_chip"].append(timed(torch, eng, lambda: fused(lg)))
                    for name, (var, val) in variants.items():
                        rows[name].append(with_env(var, val, lambda: timed(torch, eng, lambda: fused(lg))))
                res["ab_ms" + suffix] = {name: stats(t) for name, t in rows.items()}
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        del x, got
        torch.cuda.empty_cache()
    if "write" in opts:
        path = opts["write"] or os.path.join(ROOT, "profiles", "vanhove.txt")
        with open(path, "w") as f:
            f.write("# python tools/bench_vanhove.py %d %s %s\n" % (reps, shapes, " ".join("--" + k + ("=" + v if v else "") for k, v in opts.items())))
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
