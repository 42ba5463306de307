"""Compiles and runs tests/cpp/test_intcoord_gpu.cpp: molar::internal_coords of the C++ host mirror on one small case whose
input and expected numbers (the longdouble reference of tests/intcoord_ref.py with its bounds) are written here (the compile
recipe of test_cpp_msd.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import intcoord_ref as ir  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "cpp", "_build")


def write_case(path):
    F, T, G, nbins, mb = 6, 40, 3, 12, 4
    labels = np.arange(T) % G
    pairs = np.stack([np.arange(T - 1), np.arange(1, T)], 1)
    frames, tuples, box, ref = ir.make_case(51, F, T, 4, box="ortho", nbins=nbins, labels=labels, ngroups=G, pairs=pairs, map_bins=mb)
    ir.margin_ok(ref)

    def tols(want, bound):
        t64 = bound + 2.0 ** -52 * np.abs(want)
        return [want.ravel(), (t64 + ir.half_ulp32(want)).ravel(), t64.ravel()]

    rows = [[F, frames.shape[1], T, G, nbins, len(pairs), mb], tuples.ravel(), labels, pairs.ravel(), box, frames.ravel(), ref.hist.ravel(), ref.map.ravel(),
            ref.valid]
    rows += tols(ref.values, ref.bound) + tols(ref.mean, ref.mean_bound) + tols(ref.spread, ref.spread_bound)
    with open(path, "w") as f:
        for row in rows:
            f.write(" ".join(repr(float(v)) if not float(v).is_integer() or abs(v) > 1e15 else str(int(v)) for v in np.asarray(row, dtype=np.float64)) + "\n")


@pytest.mark.gpu
def test_cpp_intcoord_gpu():
    from molar_amd import build
    build.build_library()
    os.makedirs(OUT, exist_ok=True)
    libdir = os.path.join(ROOT, "molar_amd")
    exe = os.path.join(OUT, "test_intcoord_gpu")
    case = os.path.join(OUT, "intcoord_case.txt")
    write_case(case)
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_intcoord_gpu.cpp"), "-o", exe, "-L", libdir, "-lmolar_hip", "-lpthread",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe, case], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all internal-coordinate host-mirror tests passed" in r.stdout
