#!/usr/bin/env python
"""`within` as a set and SearchConnectivity in f64 against the routes an f64 caller had before them, one GPU, one process.
  within shapes, frames and indices resident in HBM, results left there, a device synchronise inside the clock:
    set     Engine.within_set_f64 to a device tensor                      (molar_hip_within_count_f64 + _fill_f64)
    stream  Engine.search_f64(SEARCH_WITHIN, device_out=True) + torch.unique   (count + fill_ids + sort / dedup on the device)
    f32     Engine.within_set on the frame rounded to f32, for scale      (another result: see tests/test_gpu_within_conn_f64.py)
  connectivity shapes, CSR brought to the host:
    csr     Engine.search_connectivity_f64                                (search + CSR on the device + the shared fill call)
    numpy   Engine.search_f64(SEARCH_SINGLE) to the host + the CSR by a stable numpy argsort
The routes alternate ROUNDS times after a warm-up round; per route the best and the spread (max - min) of the per-round
means are reported.  Writes a table to stdout (profiles/within_f64.txt is a copy of it); `--quick` runs fewer rounds."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def alternate(routes, rounds, calls, sync):
    """routes: {name: fn}.  One warm-up round, then `rounds` rounds in which every route runs `calls` times in turn.
    Returns {name: (best ms, spread ms, last result)}."""
    times = {k: [] for k in routes}
    last = {}
    for rnd in range(rounds + 1):
        for name, fn in routes.items():
            sync()
            t0 = time.perf_counter()
            for _ in range(calls):
                last[name] = fn()
            sync()
            if rnd:
                times[name].append((time.perf_counter() - t0) / calls * 1e3)
    return {k: (min(v), max(v) - min(v), last[k]) for k, v in times.items()}


def main():
    import torch
    from molar_amd import api, build, synth
    build.build_library()
    eng = api.Engine(0)
    quick = "--quick" in sys.argv
    rounds = 3 if quick else 6
    dev = torch.device("cuda", 0)

    def sync():
        eng.synchronize()
        torch.cuda.synchronize()

    def ids_out(k):
        return torch.empty(k, dtype=torch.int64, device=dev)

    print(f"# tools/bench_within_f64.py: ms per call, best of {rounds} alternating rounds (spread = max - min of the rounds' means)")
    print(f"# device: {torch.cuda.get_device_name(0)}")

    def within_case(name, n, cutoff, box32, pos64, idx1, idx2, calls):
        box = box32.astype(np.float64)
        dpos = torch.from_numpy(pos64).to(dev)
        dpos32 = torch.from_numpy(pos64.astype(np.float32)).to(dev)
        d1 = None if idx1 is None else torch.from_numpy(idx1.astype(np.int64)).to(dev)
        d2 = torch.from_numpy(idx2.astype(np.int64)).to(dev)
        routes = {
            "set": lambda: eng.within_set_f64(cutoff, dpos, d1, dpos, d2, box=box, pbc=7, device_out=ids_out),
            "stream": lambda: torch.unique(eng.search_f64(api.SEARCH_WITHIN, cutoff, dpos, d1, dpos, d2, box=box, pbc=7, device_out=True)),
            "f32": lambda: eng.within_set(cutoff, dpos32, d1, dpos32, d2, box=box32, pbc=7, device_out=ids_out),
        }
        r = alternate(routes, rounds, calls, sync)
        got, ref = r["set"][2].cpu().numpy(), r["stream"][2].cpu().numpy()
        nstream = len(eng.search_f64(api.SEARCH_WITHIN, cutoff, dpos, d1, dpos, d2, box=box, pbc=7, device_out=True))
        print(f"{name}")
        print(f"    set1 {n if idx1 is None else len(idx1)}  set2 {len(idx2)}  stream {nstream} ids  set {len(got)} ids  f32 set {len(r['f32'][2])} ids"
              f"  sets equal: {'true' if np.array_equal(got, ref) else 'FALSE'}")
        for k, label in (("set", "(a) within_set_f64"), ("stream", "(b) search_f64(WITHIN) + torch.unique"), ("f32", "(c) f32 within_set, rounded frame")):
            print(f"    {label:42s} {r[k][0]:9.3f} ms   spread {r[k][1]:7.3f} ms")
        print(f"    (b) / (a) = {r['stream'][0] / r['set'][0]:.2f}")
        sys.stdout.flush()

    def frame64(n, box32, f):
        pos = synth.frame(n, box32, f).astype(np.float64)
        return pos + np.random.default_rng(f).normal(0, 1e-9, pos.shape)

    # ---- `within 1.0 of <100k atoms>` on the 1M-atom frame (the shape of profiles/r05_within.jsonl)
    n = 1_000_000
    box32 = synth.box_a(n)
    pos = frame64(n, box32, 1)
    centre = box32.astype(np.float64) @ np.array([0.5, 0.5, 0.5])
    order = np.argsort(((pos - centre) ** 2).sum(1))
    blob = np.sort(order[:100_000]).astype(np.uint64)
    within_case("1M atoms (box A), within 1.0 of a compact 100k-atom selection", n, 1.0, box32, pos, None, blob, 2 if quick else 3)
    # ---- 250k atoms, outer = all, inner = a 5 % selection, rc 1.2
    n = 250_000
    box32 = synth.box_a(n)
    pos = frame64(n, box32, 2)
    inner = np.arange(0, n, 20, dtype=np.uint64)
    within_case("250k atoms (C4 box), within 1.2 of every 20th atom (5 %)", n, 1.2, box32, pos, None, inner, 3 if quick else 5)
    # ---- 100k atoms, within 0.8 of 20 atoms
    n = 100_000
    box32 = synth.box_a(n)
    pos = frame64(n, box32, 3)
    order = np.argsort(((pos - box32.astype(np.float64) @ np.array([0.5, 0.5, 0.5])) ** 2).sum(1))
    grp = np.sort(order[:20]).astype(np.uint64)
    within_case("100k atoms, within 0.8 of 20 atoms", n, 0.8, box32, pos, None, grp, 10 if quick else 20)

    # ---- SearchConnectivity to the host
    def numpy_csr(i, j, rows):
        row = np.empty(2 * len(i), np.uint64); nb = np.empty(2 * len(i), np.uint64)
        row[0::2], row[1::2] = i, j
        nb[0::2], nb[1::2] = j, i
        order = np.argsort(row, kind="stable")
        return np.searchsorted(row[order], np.arange(rows + 1, dtype=np.uint64)).astype(np.uint64), nb[order]

    def conn_case(name, n, cutoff, f, calls):
        box32 = synth.box_a(n)
        box = box32.astype(np.float64)
        dpos = torch.from_numpy(frame64(n, box32, f)).to(dev)

        def by_numpy():
            i, j, _ = eng.search_f64(api.SEARCH_SINGLE, cutoff, dpos, box=box, pbc=7)
            return numpy_csr(i, j, n)
        r = alternate({"csr": lambda: eng.search_connectivity_f64(cutoff, dpos, box=box, pbc=7), "numpy": by_numpy}, rounds, calls, sync)
        (off, nb), (woff, wnb) = r["csr"][2], r["numpy"][2]
        print(f"{name}")
        print(f"    rows {n}  entries {len(nb)}  CSRs equal: {'true' if np.array_equal(off, woff) and np.array_equal(nb, wnb) else 'FALSE'}")
        print(f"    {'search_connectivity_f64 + fill to the host':42s} {r['csr'][0]:9.3f} ms   spread {r['csr'][1]:7.3f} ms")
        print(f"    {'search_f64(SINGLE) to the host + numpy CSR':42s} {r['numpy'][0]:9.3f} ms   spread {r['numpy'][1]:7.3f} ms")
        print(f"    numpy route / device route = {r['numpy'][0] / r['csr'][0]:.2f}")
        sys.stdout.flush()

    conn_case("25k atoms, rc 1.0 (lists of ~420 entries)", 25_000, 1.0, 4, 1 if quick else 2)
    conn_case("120k atoms, rc 0.2 (bonded neighbours)", 120_000, 0.2, 5, 3 if quick else 5)


if __name__ == "__main__":
    main()
