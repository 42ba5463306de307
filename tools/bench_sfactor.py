#!/usr/bin/env python
"""The static structure factor (molar_hip_sfactor: rho_g(m) over the reciprocal lattice of each frame's box by one complex matrix
product per (frame, group) on the f64 matrix cores, operands formed on chip; S_ab and its shell average) against the two routes
a caller had before it, both written here in torch f64 on the device:

  (B) the direct route: exp(-2 pi i S @ M^T) in chunks of atoms capped at 1 GB of extra memory, the groups' weighted sums over
      the atoms by one [G, chunk] @ [chunk, Q] product per chunk;
  (C) the separable route, the strong one: the phasor-power operands A [n, rows] and B [n, cols] built in complex128 (exp of an
      outer product each, A of two), then one complex A_g^T @ B_g per frame and group - rocBLAS's own complex GEMM.  Its extra
      memory, n (rows + cols) 16 bytes per frame in flight, is reported.
  Both then form S_ab = mean_f Re(rho_a conj rho_b) and the shells (index_add over the bins of |q| of every frame's box).
  Routes (B) and (C) are timed on `--frames-timed` frames and scaled by F / frames timed; the scaling is in the output.

Shapes:  (a) water: 333 334 oxygens of a 1 000 002-atom box x 64 frames, hmax (16, 16, 16), 64 shells, one box;  (b) bilayer: 4000
phosphorus atoms x 4096 frames under per-frame boxes, lateral hmax (32, 32, 0), 64 rings;  (c) mixture: 100 000 atoms in three
species x 256 frames, hmax (8, 8, 8), 32 shells, all six partials.  Frames are random f32 positions resident on the device
(the cost does not depend on the values).

Before anything is timed the routes are compared with the fused call's S_ab and shells on the frames they are timed on.
Timing: a warm-up, then `reps` repetitions, the routes taking turns, each bracketed by a pair of events - the first recorded
after a device-wide synchronisation, the second after the engine's stream has been waited for; median, minimum and maximum in
ms.  Also per shape: the plan, the flop of the lattice points asked for (8 n Q F) and of the tiles the gram kernel issues
(whole 16 x 16 tiles with a row and a column of the grid, atoms padded to 16), and the f64 MFMA roof measured in the same run, before the
engine opens the device, by profiles/microbench/mfma_f64_rate.  Kernel times proper need a trace run (tools/prof_sfactor.py).
One JSON line per shape; the lines go to stdout and, with --write[=PATH], to profiles/sfactor.txt (or PATH).
Usage: python tools/bench_sfactor.py [reps] [shapes, e.g. ac] [--frames-timed=N (default: F / 16, at least 4)] [--fused-only] [--write[=PATH]]"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BOX = (9.0, 9.5, 10.0)
# natoms, selection step, F, hmax, shells, groups, per-frame boxes, signed weights
SHAPES = {"a": (1000002, 3, 64, (16, 16, 16), 64, 1, False, False), "b": (4000, 1, 4096, (32, 32, 0), 64, 1, True, False),
          "c": (100000, 1, 256, (8, 8, 8), 32, 3, False, True)}
QMIN, DQ = 0.0, 0.25


def mfma_roof():
    """TFLOP/s of back-to-back v_mfma_f64_16x16x4_f64 (the best row of the microbenchmark) and its output."""
    src = os.path.join(ROOT, "profiles", "microbench", "mfma_f64_rate.hip")
    exe = src[:-4]
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", src, "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, check=True).stdout
    rows = [dict(zip(ln.split()[0::2], ln.split()[1::2])) for ln in out.splitlines() if ln.startswith("waves_per_simd")]
    return max(float(r["tflops"]) for r in rows), out


def make_case(torch, natoms, step, F, G, per_frame, signed, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    box = torch.tensor(BOX, device="cuda", dtype=torch.float32)
    frames = torch.empty((F, natoms, 3), device="cuda", dtype=torch.float32)
    for f0 in range(0, F, 16):
        n = min(16, F - f0)
        frames[f0:f0 + n] = torch.rand((n, natoms, 3), device="cuda", generator=gen) * box
    idx = torch.arange(0, natoms, step, device="cuda", dtype=torch.int64) if step > 1 else None
    n = natoms if idx is None else int(idx.shape[0])
    labels = torch.randint(0, G, (n,), device="cuda", generator=gen, dtype=torch.int32) if G > 1 else None
    weight = None
    if signed:
        weight = (torch.rand(natoms, device="cuda", generator=gen) + 0.5) * torch.where(torch.rand(natoms, device="cuda", generator=gen) < 0.3, -1.0, 1.0)
        weight = weight.float()
    b9 = torch.zeros(9, device="cuda", dtype=torch.float32)
    b9[[0, 4, 8]] = box
    boxes = b9
    if per_frame:
        boxes = b9[None, :] * (1.0 + 0.02 * (torch.rand((F, 1), device="cuda", generator=gen) - 0.5))
        boxes = boxes.contiguous()
    return frames, idx, n, labels, weight, boxes


def fractional(torch, frames_f, idx, box9):
    """s [n, 3] f64 of one frame under an orthorhombic box (the bench's boxes are)."""
    x = frames_f if idx is None else frames_f[idx]
    return x.double() / box9.double()[[0, 4, 8]]


def finish(torch, rho, boxes, m, canonical, ns, G):
    """S_ab [P, Q] and shells [P, ns] from rho [F, G, Q] complex128, every frame's own box."""
    F = rho.shape[0]
    pairs = [(a, b) for a in range(G) for b in range(a, G)]
    prod = torch.stack([(rho[:, a] * rho[:, b].conj()).real for a, b in pairs], dim=1)            # [F, P, Q]
    sab = prod.mean(dim=0)
    shell = torch.zeros((len(pairs), ns), device="cuda", dtype=torch.float64)
    count = torch.zeros(ns, device="cuda", dtype=torch.float64)
    mc = m[canonical].double()
    for f in range(F):
        b9 = (boxes if boxes.ndim == 1 else boxes[f]).double()
        q = 2 * np.pi * torch.sqrt(((mc / b9[[0, 4, 8]]) ** 2).sum(dim=1))
        b = torch.floor((q - QMIN) / DQ).long()
        ok = (b >= 0) & (b < ns)
        shell.index_add_(1, b[ok], prod[f][:, canonical][:, ok])
        count.index_add_(0, b[ok], torch.ones(int(ok.sum()), device="cuda", dtype=torch.float64))
    return sab, shell / count, count


def route_direct(torch, frames, idx, labels, weight, boxes, m, G, cap=1 << 30):
    F = frames.shape[0]
    n = frames.shape[1] if idx is None else idx.shape[0]
    Q = m.shape[0]
    chunk = max(1, cap // (Q * 16))
    w = torch.ones(n, device="cuda", dtype=torch.float64) if weight is None else (weight if idx is None else weight[idx]).double()
    lab = torch.zeros(n, device="cuda", dtype=torch.long) if labels is None else labels.long()
    onehot = torch.zeros((G, n), device="cuda", dtype=torch.complex128)
    onehot[lab, torch.arange(n, device="cuda")] = w.to(torch.complex128)
    mt = m.double().T.contiguous()
    rho = torch.zeros((F, G, Q), device="cuda", dtype=torch.complex128)
    for f in range(F):
        s = fractional(torch, frames[f], idx, boxes if boxes.ndim == 1 else boxes[f])
        for k0 in range(0, n, chunk):
            ph = s[k0:k0 + chunk] @ mt
            rho[f] += onehot[:, k0:k0 + chunk] @ torch.polar(torch.ones_like(ph), -2 * np.pi * ph)
    return rho, chunk * Q * 16


def route_separable(torch, frames, idx, labels, weight, boxes, hmax, G):
    H, K, L = hmax
    F = frames.shape[0]
    n = frames.shape[1] if idx is None else idx.shape[0]
    w = torch.ones(n, device="cuda", dtype=torch.float64) if weight is None else (weight if idx is None else weight[idx]).double()
    order = torch.arange(n, device="cuda") if labels is None else torch.argsort(labels.long(), stable=True)
    counts = [n] if labels is None else torch.bincount(labels.long(), minlength=G).tolist()
    hk = torch.stack(torch.meshgrid(torch.arange(H + 1, device="cuda"), torch.arange(-K, K + 1, device="cuda"), indexing="ij"), dim=-1).reshape(-1, 2).double()
    ll = torch.arange(-L, L + 1, device="cuda").double()
    Q = hk.shape[0] * ll.shape[0]
    rho = torch.zeros((F, G, Q), device="cuda", dtype=torch.complex128)
    for f in range(F):
        s = fractional(torch, frames[f], idx, boxes if boxes.ndim == 1 else boxes[f])[order]
        pa = s[:, :2] @ hk.T
        A = torch.polar(torch.ones_like(pa), -2 * np.pi * pa)                               # [n, rows]
        pb = s[:, 2:3] * ll[None, :]
        B = torch.polar(w[order][:, None].expand_as(pb).contiguous(), -2 * np.pi * pb)      # [n, cols]
        k0 = 0
        for g, c in enumerate(counts):
            rho[f, g] = (A[k0:k0 + c].T @ B[k0:k0 + c]).reshape(-1)
            k0 += c
    return rho, n * (hk.shape[0] + ll.shape[0]) * 16


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


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opts = dict(a[2:].split("=", 1) if "=" in a else (a[2:], "") for a in sys.argv[1:] if a.startswith("--"))
    reps = int(args[0]) if args else 20
    shapes = args[1] if len(args) > 1 else "abc"
    fused_only = "fused-only" in opts
    roof, roof_out = (0.0, "") if fused_only else mfma_roof()
    import torch
    from molar_amd import api
    eng = api.Engine()
    lines = []
    for key in shapes:
        natoms, step, F, hmax, ns, G, per_frame, signed = SHAPES[key]
        frames, idx, n, labels, weight, boxes = make_case(torch, natoms, step, F, G, per_frame, signed, 17)
        grid = api.sfactor_grid(hmax, QMIN, DQ, ns)
        want = ("frame_ok", "sab", "shell", "shell_count")
        kw = dict(idx=idx, weight=weight, labels=labels, ngroups=G if labels is not None else None, boxes=boxes, want=want)
        fused = lambda fr=frames, bx=boxes: eng.structure_factor(fr, grid, **dict(kw, boxes=bx))
        ws, layout, rb, cb, ac, ks, fb = api.sfactor_plan(F, n, grid, G)
        m_np, can_np = api.sfactor_miller(hmax)
        Q = m_np.shape[0]
        rows, cols = ((2 * hmax[1] + 1), hmax[0] + 1) if layout else ((hmax[0] + 1) * (2 * hmax[1] + 1), 2 * hmax[2] + 1)
        tiles = -(-rows // 16) * -(-cols // 16)                # tile pairs with a row and a column of the grid: the others issue nothing
        res = dict(shape=key, natoms=natoms, n=n, frames=F, hmax=hmax, Q=Q, shells=ns, groups=G, per_frame_boxes=per_frame, workspace_MB=round(ws / 2 ** 20, 1),
                   layout=layout, row_block=rb, col_block=cb, atom_chunk=ac, ksplits=ks, frame_block=fb, flop_asked=8.0 * n * Q * F,
                   flop_issued=8.0 * (-(-n // 16) * 16) * tiles * 256 * F, mfma_roof_tflops=roof)
        if not fused_only:
            Ft = min(F, int(opts["frames-timed"]) if "frames-timed" in opts else max(4, F // 16))
            m = torch.as_tensor(m_np, device="cuda")
            canonical = torch.as_tensor(can_np, device="cuda")
            sub, bsub = frames[:Ft], boxes if boxes.ndim == 1 else boxes[:Ft].contiguous()
            got = fused(sub, bsub)
            eng.synchronize()
            norm = float(got.sab.double().abs().max())
            routes = {"direct": lambda: finish(torch, route_direct(torch, sub, idx, labels, weight, bsub, m, G)[0], bsub, m, canonical, ns, G),
                      "separable": lambda: finish(torch, route_separable(torch, sub, idx, labels, weight, bsub, hmax, G)[0], bsub, m, canonical, ns, G)}
            res["extra_MB"] = dict(direct=round(route_direct(torch, sub[:1], idx, labels, weight, bsub, m, G)[1] / 2 ** 20, 1),
                                   separable=round(route_separable(torch, sub[:1], idx, labels, weight, bsub, hmax, G)[1] / 2 ** 20, 1))
            for name, fn in routes.items():
                sab, shell, count = fn()
                res[f"sab_diff_{name}"] = float((sab - got.sab.double()).abs().max()) / norm            # f32 results: about 1e-7
                fin = (count > 0) & (count == got.shell_count.double())         # a |q| within rounding of an edge may fall either way
                res[f"shells_with_equal_counts_{name}"] = f"{int(fin.sum())} of {int((count > 0).sum())}"
                res[f"shell_diff_{name}"] = float((shell[:, fin] - got.shell.double()[:, fin]).abs().max()) / norm
                assert res[f"sab_diff_{name}"] < 1e-5 and res[f"shell_diff_{name}"] < 1e-5, (name, res)
            ts = {name: [] for name in routes}
            ts["fused_on_frames_timed"] = []
            for _ in range(reps):
                ts["fused_on_frames_timed"].append(timed(torch, eng, lambda: fused(sub, bsub)))
                for name, fn in routes.items():
                    ts[name].append(timed(torch, eng, fn))
            res["frames_timed"] = Ft
            for name, t in ts.items():
                res[f"ms_{name}"] = stats(t)
            for name in routes:
                res[f"ms_{name}_scaled_to_F"] = round(res[f"ms_{name}"]["median"] * F / Ft, 1)
        fused()
        eng.synchronize()
        res["ms_fused"] = stats([timed(torch, eng, fused) for _ in range(reps)])
        res["tflops_asked"] = round(res["flop_asked"] / (res["ms_fused"]["median"] * 1e-3) / 1e12, 2)
        if not fused_only:
            for name in ("direct", "separable"):
                res[f"fused_over_{name}"] = round(res[f"ms_{name}_scaled_to_F"] / res["ms_fused"]["median"], 2)
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        del frames
        torch.cuda.empty_cache()
    if "write" in opts:
        path = opts["write"] or os.path.join(ROOT, "profiles", "sfactor.txt")
        with open(path, "w") as f:
            f.write(roof_out)
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
