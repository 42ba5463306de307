#!/usr/bin/env python
"""Lifetime correlations (molar_hip_lifetimes: bit matrix, gap filling, intermittent and continuous numerators, run lengths)
against the routes a caller had before it, written here in torch on the device:

  (B) the intermittent curve as ONE SLICE-AND-SUM PER LAG on the dense bool matrix [R, F]: (h[:, :F - tau] & h[:, tau:]).sum();
      the continuous curve as a cumulative AND per lag, alive = alive[:, :-1] & h[:, tau:], and its sum;
  (C) the intermittent curve as the autocorrelation through torch.fft.rfft of the dense f32 rows, zero-padded to 2 F, in chunks
      of rows that fit (no continuous curve: it is no correlation).

Shapes, synthetic presence matrices of independent on/off Markov chains (no trajectory is needed):
  (a) water-water hydrogen bonds: 2e5 rows, 4096 frames, 2049 lags, occupancy ~5 %, mean run ~4 frames;
  (b) contacts: 5e3 rows, 65 536 frames, 8193 lags, occupancy ~50 %, mean run ~200 frames;
  (c) shell survival: 1e6 rows, 1024 frames, 513 lags, occupancy ~2 %, mean run ~4 frames.
Everything is resident on the device: the CSR (frame_offsets, row_of_entry) for the fused call, the dense matrices for the
torch routes (their construction is not timed).

Route (B) is too slow to run in full twenty times: its intermittent part is timed on `--lags-timed` lags spread evenly over
0 .. max_lag (the cost of a lag is proportional to F - tau, so the even spread is unbiased) and multiplied by
(max_lag + 1) / lags_timed; its continuous part, whose lags must be taken in order, on the first `--lags-timed` lags and
multiplied by sum_{tau <= max_lag} (F - tau) / sum_{tau < lags_timed} (F - tau).  Both scalings are in the output.

Before anything is timed the routes are compared with the fused call: route (B) exactly on the lags it computes, route (C) by
the largest absolute deviation of its rounded f32 sums.  Timing: a warm-up, then `reps` repetitions, the routes taking turns,
each between two events (bench_msd.py's bracket); median, minimum and maximum in ms.  Nothing is gated: the numbers are
reported.  Also per shape: the word pairs of the intermittent kernel, R x sum_q (W - q) (a word pair serves 64 lags), their rate
over the time of the fused call asked for `inter` alone, and that rate against the issue bound of the vector ALUs:
VALU_PER_PAIR instructions per word pair in the built inner loop, a wave instruction per 2 cycles per SIMD, 1024 SIMDs at
2.4 GHz (kernel times proper need a trace run: rocprofv3 --kernel-trace --stats on `--fused-only`).
One JSON line per shape; with --write[=PATH] they go to profiles/lifetimes.txt (or PATH) as well.
Usage: python tools/bench_lifetimes.py [reps] [shapes, e.g. ac] [--lags-timed=64] [--fused-only] [--write[=PATH]]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# rows, frames, max_lag, p_on (off -> on), p_off (on -> off): occupancy p_on / (p_on + p_off), mean run 1 / p_off
SHAPES = {"a": (200000, 4096, 2048, 0.25 * 0.05 / 0.95, 0.25), "b": (5000, 65536, 8192, 0.005, 0.005),
          "c": (1000000, 1024, 512, 0.25 * 0.02 / 0.98, 0.25)}
VALU_PER_PAIR = 92 / 16      # lt_inter_kernel's unrolled loop in the built gfx950 assembly: 92 vector instructions for 4 x 4 word pairs
SIMDS, CLOCK_HZ, CYCLES_PER_VALU = 1024, 2.4e9, 2


def make_dense(torch, R, F, p_on, p_off, seed):
    """[F, R] bool on the device: R independent chains from the stationary state"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    h = torch.empty((F, R), dtype=torch.bool, device="cuda")
    state = torch.rand(R, device="cuda", generator=gen) < p_on / (p_on + p_off)
    for t0 in range(0, F, 256):                      # the random numbers in slabs
        u = torch.rand((min(256, F - t0), R), device="cuda", generator=gen)
        for k in range(u.shape[0]):
            h[t0 + k] = state
            state = torch.where(state, u[k] >= p_off, u[k] < p_on)
    return h


def to_csr(torch, h):
    """(frame_offsets int64 [F + 1], row_of_entry int32 [E]) of the dense [F, R] matrix, on the device"""
    per = h.sum(dim=1, dtype=torch.int64)
    off = torch.zeros(h.shape[0] + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(per, 0, out=off[1:])
    rows = torch.empty(int(off[-1]), dtype=torch.int32, device="cuda")
    for t0 in range(0, h.shape[0], 512):             # in slabs: nonzero of the whole matrix makes int64 pairs
        nz = h[t0:t0 + 512].nonzero()
        rows[int(off[t0]):int(off[min(t0 + 512, h.shape[0])])] = nz[:, 1].int()
    return off, rows


def slices_inter(torch, hr, lags):
    F = hr.shape[1]
    return torch.stack([(hr[:, :F - tau] & hr[:, tau:]).sum() for tau in lags])


def slices_cont(torch, hr, nlags):
    alive = hr
    out = [alive.sum()]
    for tau in range(1, nlags):
        alive = alive[:, :-1] & hr[:, tau:]
        out.append(alive.sum())
    return torch.stack(out)


def fft_inter(torch, hr, L, chunk):
    R, F = hr.shape
    acc = torch.zeros(L + 1, dtype=torch.float64, device="cuda")
    for r0 in range(0, R, chunk):
        x = hr[r0:r0 + chunk].float()
        f = torch.fft.rfft(x, n=2 * F, dim=-1)
        acc += torch.fft.irfft(f * f.conj(), n=2 * F, dim=-1)[:, :L + 1].sum(0, dtype=torch.float64)
    return acc


def main():
    import torch
    from molar_amd import api, build
    build.build_library()
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opts = dict(a[2:].split("=", 1) if "=" in a else (a[2:], "") for a in sys.argv[1:] if a.startswith("--"))
    reps = int(args[0]) if args else 20
    shapes = args[1] if len(args) > 1 else "abc"
    K = int(opts.get("lags-timed", 64))
    fused_only = "fused-only" in opts
    eng = api.Engine(0)
    lines = []

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

    def stats(ts, scale=1.0):
        ts = np.array(ts) * scale
        return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(ts.min()), 3), "max_ms": round(float(ts.max()), 3)}

    for key in shapes:
        R, F, L, p_on, p_off = SHAPES[key]
        h = make_dense(torch, R, F, p_on, p_off, 1234 + ord(key))
        off, rows = to_csr(torch, h)
        hr = h.t().contiguous()                      # [R, F]: the rows of the torch routes
        del h
        E = int(off[-1])
        keep = {}

        def fused(want=("inter", "cont")):
            keep["fused"] = eng.lifetimes(off, rows, R, max_lag=L, want=want)

        fused(api.LIFETIME_OUTPUTS)
        res = keep["fused"]
        occupancy = E / (R * F)
        mean_run = float(res.present.sum()) / max(int(res.events.sum()), 1)
        inter, cont = res.inter[0].clone(), res.cont[0].clone()
        W = (F + 63) // 64
        nq = L // 64 + 1
        pairs = float(R) * sum(W - q for q in range(nq))
        ws, _ = api.lifetimes_plan(F, R, 1, True)
        row = {"shape": key, "rows": R, "frames": F, "max_lag": L, "entries": E, "occupancy": round(occupancy, 4), "mean_run_frames": round(mean_run, 2),
               "workspace_MB": round(ws / 2 ** 20, 1), "csr_MB": round((E * 4 + (F + 1) * 8) / 2 ** 20, 1), "word_pairs": pairs}
        if not fused_only:
            lags_b = [int(x) for x in np.unique(np.linspace(0, L, K).round().astype(np.int64))]
            scale_inter = (L + 1) / len(lags_b)
            Kc = min(K, L + 1)
            scale_cont = float(sum(F - tau for tau in range(L + 1))) / float(sum(F - tau for tau in range(Kc)))
            chunk = max(1, min(R, (1 << 30) // (2 * F * 4)))             # 1 GiB of padded f32 rows per chunk
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            b_inter = slices_inter(torch, hr, lags_b)
            b_cont = slices_cont(torch, hr, Kc)
            torch.cuda.synchronize()
            b_peak = torch.cuda.max_memory_allocated() - base
            torch.cuda.reset_peak_memory_stats()
            c_inter = fft_inter(torch, hr, L, chunk)
            torch.cuda.synchronize()
            c_peak = torch.cuda.max_memory_allocated() - base
            row["agreement"] = {"B_inter_equal_on_its_lags": bool(torch.equal(b_inter, inter[lags_b])),
                                "B_cont_equal_on_its_lags": bool(torch.equal(b_cont, cont[:Kc])),
                                "C_inter_largest_abs_deviation": float((c_inter - inter.double()).abs().max()),
                                "C_inter_rounds_to_the_integers": bool(torch.equal(c_inter.round().long(), inter))}
            row["dense_bool_MB"] = round(R * F / 2 ** 20, 1)
            row["route_B_peak_extra_MB"] = round(b_peak / 2 ** 20, 1)
            row["route_C_peak_extra_MB"] = round(c_peak / 2 ** 20, 1)
            row["route_C_rows_per_chunk"] = chunk
            del b_inter, b_cont, c_inter
        keep.clear()
        torch.cuda.empty_cache()
        tf, ti, tc, tbi, tbc, tfft = [], [], [], [], [], []
        for _ in range(reps):                        # the routes take turns
            tf.append(bracket(fused))
            ti.append(bracket(lambda: fused(("inter",))))
            tc.append(bracket(lambda: fused(("cont",))))
            if not fused_only:
                tbi.append(bracket(lambda: slices_inter(torch, hr, lags_b)))
                tbc.append(bracket(lambda: slices_cont(torch, hr, Kc)))
                tfft.append(bracket(lambda: fft_inter(torch, hr, L, chunk)))
        row["fused_inter_and_cont"], row["fused_inter_only"], row["fused_cont_only"] = stats(tf), stats(ti), stats(tc)
        rate = pairs / (row["fused_inter_only"]["median_ms"] * 1e-3)
        bound = SIMDS * CLOCK_HZ / CYCLES_PER_VALU / VALU_PER_PAIR
        row["inter_word_pairs_per_s_end_to_end"] = rate
        row["valu_issue_bound_word_pairs_per_s"] = bound
        row["inter_fraction_of_valu_issue_bound_end_to_end"] = round(rate / bound, 3)
        if not fused_only:
            row["route_B_inter_slices_extrapolated"] = stats(tbi, scale_inter)
            row["route_B_inter_scaling"] = f"{len(lags_b)} lags timed, times {scale_inter:.2f}"
            row["route_B_cont_cumulative_and_extrapolated"] = stats(tbc, scale_cont)
            row["route_B_cont_scaling"] = f"the first {Kc} lags timed, times {scale_cont:.2f}"
            row["route_C_fft_inter"] = stats(tfft)
            row["B_inter_over_fused_inter"] = round(row["route_B_inter_slices_extrapolated"]["median_ms"] / row["fused_inter_only"]["median_ms"], 2)
            row["C_inter_over_fused_inter"] = round(row["route_C_fft_inter"]["median_ms"] / row["fused_inter_only"]["median_ms"], 2)
            row["B_cont_over_fused_cont"] = round(row["route_B_cont_cumulative_and_extrapolated"]["median_ms"] / row["fused_cont_only"]["median_ms"], 2)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        del hr, off, rows
        torch.cuda.empty_cache()
    if "write" in opts:
        dst = opts["write"] or os.path.join(ROOT, "profiles", "lifetimes.txt")
        with open(dst, "w") as f:
            f.write("# python tools/bench_lifetimes.py %d %s --lags-timed=%d --write\n" % (reps, shapes, K))
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
