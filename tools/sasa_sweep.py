#!/usr/bin/env python
"""Per-atom solvent-accessible surface area: the fused call (molar_hip_sasa) beside the composition of calls that existed
before it, on blobs of 100k and 1M atoms at water-like density (100 atoms / nm^3, no box), 96 and 960 points:
  fused        Engine.sasa on coordinates, radii and results resident in HBM;
  composition  search_resident(SEARCH_DOUBLE_VDW) of the selection against itself with both radii columns vdw + probe (the
               pair list goes to HBM), then the point test over that list in torch (chunks of pairs x points, a scatter-max
               into a buried[n, points] plane), the areas from the exposed counts.
Milliseconds per frame from HIP events on one stream shared by the engine and torch, after an untimed warm-up, median and
best of --reps repetitions.  Also the relative difference of the total area at 96, 192 and 960 points against 3840 points on
the 100k blob (the convergence of Shrake-Rupley towards the exact union-of-spheres area).  Writes a text table.

--vol times the volume call (Engine.sasa_vol, molar_hip_sasa_vol) beside the area call on the same shapes, and with
--base-lib also the area call of another build of the library (the commit before the volumes, say) in the same process on
the same stream, the three taking turns; it checks that the volume call's areas are those of the area call and prints the
total volume and the number of atoms with an empty power cell.

    python tools/sasa_sweep.py [--out profiles/sasa.txt] [--reps 20] [--sizes 100000,1000000] [--fused-only]
    python tools/sasa_sweep.py --vol [--vol-only] [--base-lib other/libmolar_hip.so] [--out profiles/sasa_vol.txt]"""
import argparse
import ctypes as C
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROBE = 0.14
RADII = np.array([0.12, 0.152, 0.155, 0.17, 0.18], np.float32)


def blob(n, seed):
    rng = np.random.default_rng(seed)
    edge = (n / 100.0) ** (1.0 / 3.0)
    return rng.uniform(0, edge, (n, 3)).astype(np.float32), RADII[rng.integers(0, len(RADII), n)]


def timed(fn, reps, stream):
    """(median, best) milliseconds of fn() between two events on `stream`, after one untimed call"""
    import torch
    fn()
    stream.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


_base = {}          # path -> (library, context)


def base_area_call(path, stream, dxyz, dvdw, n, npoints):
    """molar_hip_sasa of the library at `path` on device arrays; returns (call, areas tensor)"""
    import torch
    if path not in _base:
        lib = C.CDLL(path)
        lib.molar_hip_create.restype = C.c_void_p
        lib.molar_hip_create.argtypes = [C.c_int]
        lib.molar_hip_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        lib.molar_hip_sasa.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_float, C.c_uint32, C.c_void_p,
                                       C.c_void_p, C.c_void_p]
        ctx = lib.molar_hip_create(0)
        assert ctx and lib.molar_hip_set_stream(ctx, C.c_void_p(stream.cuda_stream)) == 0
        _base[path] = (lib, ctx)
    lib, ctx = _base[path]
    areas = torch.zeros(n, dtype=torch.float32, device="cuda")
    exposed = torch.zeros(n, dtype=torch.int32, device="cuda")
    total = C.c_double(0.0)

    def call():
        rc = lib.molar_hip_sasa(ctx, dxyz.data_ptr(), n, None, n, dvdw.data_ptr(), PROBE, npoints, areas.data_ptr(), exposed.data_ptr(), C.byref(total))
        assert rc == 0, rc
    return call, areas


def volume_leg(args, eng, stream, say):
    import torch
    say(f"{'atoms':>8} {'points':>6} {'area ms':>18} {'volume ms':>18} {'volume / area':>13} {'base area ms':>18} {'total nm^3':>12} {'empty cells':>11}")
    for n in [int(x) for x in args.sizes.split(",")]:
        xyz, vdw = blob(n, 21)
        dxyz, dvdw = torch.from_numpy(xyz).cuda(), torch.from_numpy(vdw).cuda()
        stream.synchronize()
        for npoints in [int(x) for x in args.points.split(",")]:
            res = {}

            def area():
                res["a"] = eng.sasa(dxyz, dvdw, probe=PROBE, npoints=npoints, want_exposed=True)

            def volume():
                res["v"] = eng.sasa_vol(dxyz, dvdw, probe=PROBE, npoints=npoints, want_exposed=True)
            v_med, v_best = timed(volume, args.reps, stream)
            if args.vol_only:
                say(f"{n:>8} {npoints:>6} {'':>18} {v_med:>10.3f} ({v_best:.3f})")
                continue
            a_med, a_best = timed(area, args.reps, stream)
            base = f"{'-':>18}"
            if args.base_lib:
                call, b_areas = base_area_call(args.base_lib, stream, dxyz, dvdw, n, npoints)
                b_med, b_best = timed(call, args.reps, stream)
                a2_med, a2_best = timed(area, args.reps, stream)              # again, after the other build: the spread of the area call
                base = f"{b_med:>10.3f} ({b_best:.3f})"
                assert torch.equal(b_areas, res["a"].areas), "the area call's results changed"
                say(f"#   area call once more after the base build's: {a2_med:.3f} ({a2_best:.3f})")
            assert torch.equal(res["v"].areas, res["a"].areas) and torch.equal(res["v"].exposed, res["a"].exposed)
            empty = int((res["v"].volumes == 0).sum())
            say(f"{n:>8} {npoints:>6} {a_med:>10.3f} ({a_best:.3f}) {v_med:>10.3f} ({v_best:.3f}) {v_med / a_med:>13.1f} {base} "
                f"{res['v'].total_volume:>12.3f} {empty:>11}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/sasa.txt, profiles/sasa_vol.txt with --vol")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--points", default="96,960")
    ap.add_argument("--fused-only", action="store_true", help="the fused call alone (kernel traces)")
    ap.add_argument("--vol", action="store_true", help="the volume call beside the area call")
    ap.add_argument("--vol-only", action="store_true", help="with --vol: the volume call alone (kernel traces)")
    ap.add_argument("--base-lib", default=None, help="with --vol: another build of libmolar_hip.so whose area call is timed in the same run")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "sasa_vol.txt" if args.vol else "sasa.txt")
    import torch
    from molar_amd import api, build
    build.build_library()
    stream = torch.cuda.Stream()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")

    def say(s):
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()
    say(f"# tools/sasa_sweep.py: {torch.cuda.get_device_name(0)}, blobs at 100 atoms/nm^3, probe {PROBE} nm, "
        f"{args.reps} repetitions after a warm-up, HIP events; ms per frame as median (best)")
    with torch.cuda.stream(stream):
        eng = api.Engine(0, stream=stream.cuda_stream)
        if args.vol:
            volume_leg(args, eng, stream, say)
            out.close()
            return
        say(f"{'atoms':>8} {'points':>6} {'fused ms':>18} {'composition ms':>20} {'search ms':>16} {'pairs':>11} {'speed-up':>8} "
            f"{'exposed differ':>14}")
        for n in [int(x) for x in args.sizes.split(",")]:
            xyz, vdw = blob(n, 21)
            dxyz, dvdw = torch.from_numpy(xyz).cuda(), torch.from_numpy(vdw).cuda()
            dR = dvdw + np.float32(PROBE)
            stream.synchronize()
            for npoints in [int(x) for x in args.points.split(",")]:
                table = torch.from_numpy(api.sasa_points(npoints)).cuda()
                res = {}

                def fused():
                    res["f"] = eng.sasa(dxyz, dvdw, probe=PROBE, npoints=npoints, want_exposed=True)

                def search():
                    cnt, p, _ = eng.search_resident(api.SEARCH_DOUBLE_VDW, None, dxyz, None, dxyz, None, vdw1=dR, vdw2=dR, ids_local=True)
                    res["pairs"] = api.device_view(p, (cnt, 2), torch.int32)

                def composition():
                    search()
                    pairs = res["pairs"]
                    i, j = pairs[:, 0].long(), pairs[:, 1].long()
                    keep = i != j
                    i, j = i[keep], j[keep]
                    d = dxyz[j] - dxyz[i]
                    Ri, Rj2 = dR[i], dR[j] * dR[j]
                    buried = torch.zeros((n, npoints), dtype=torch.uint8, device="cuda")
                    chunk = max(1024, (1 << 27) // npoints)             # 1.5 GB of t per chunk
                    for c0 in range(0, i.shape[0], chunk):
                        sl = slice(c0, c0 + chunk)
                        t = Ri[sl, None, None] * table[None] - d[sl, None, :]
                        hit = ((t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2]) < Rj2[sl, None]
                        buried.scatter_reduce_(0, i[sl, None].expand(-1, npoints), hit.to(torch.uint8), "amax")
                    exposed = npoints - buried.sum(1, dtype=torch.int32)
                    res["c_exposed"] = exposed
                    res["c_areas"] = ((4.0 * math.pi) * (dR.double() * dR.double()) * exposed.double() / npoints).float()
                f_med, f_best = timed(fused, args.reps, stream)
                if args.fused_only:
                    say(f"{n:>8} {npoints:>6} {f_med:>10.3f} ({f_best:.3f})")
                    continue
                s_med, s_best = timed(search, args.reps, stream)
                c_med, c_best = timed(composition, args.reps, stream)
                differ = int((res["c_exposed"] != res["f"].exposed).sum())
                say(f"{n:>8} {npoints:>6} {f_med:>10.3f} ({f_best:.3f}) {c_med:>11.3f} ({c_best:.3f}) {s_med:>8.3f} ({s_best:.3f}) "
                    f"{res['pairs'].shape[0]:>11} {c_med / f_med:>8.1f} {differ:>14}")
                res.clear()
                torch.cuda.empty_cache()
        if not args.fused_only:
            n = 100_000
            xyz, vdw = blob(n, 21)
            dxyz, dvdw = torch.from_numpy(xyz).cuda(), torch.from_numpy(vdw).cuda()
            stream.synchronize()
            ref = eng.sasa(dxyz, dvdw, probe=PROBE, npoints=3840).total_area
            say(f"# convergence on the {n}-atom blob: total area {ref:.4f} nm^2 at 3840 points; relative difference of the total at")
            for npoints in (96, 192, 960):
                tot = eng.sasa(dxyz, dvdw, probe=PROBE, npoints=npoints).total_area
                say(f"#   {npoints:>4} points: {abs(tot - ref) / ref:.2e}")
    out.close()


if __name__ == "__main__":
    main()
