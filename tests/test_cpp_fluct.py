"""Compiles and runs tests/cpp/test_fluct_gpu.cpp: molar::fluctuations of the C++ host mirror on one small case whose input
and expected numbers (the numpy reference of tests/fluct_ref.py with its bounds) are written here (the compile recipe of
test_cpp_rmsd_matrix.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fluct_ref as fr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "cpp", "_build")


def write_case(path):
    F, natoms, iterations = 11, 40, 1
    rng = np.random.default_rng(21)
    frames = fr.random_frames(F, natoms, seed=22, sigma=0.08)
    idx = np.flatnonzero(np.arange(natoms) % 7 != 3).astype(np.uint64)
    mass = rng.uniform(1.0, 16.0, natoms).astype(np.float32)
    ref = fr.fluct(frames, idx=idx, mass=mass, fit=True, iterations=iterations)
    k = fr.k_fit()[0]
    rows = [[F, natoms, len(idx), iterations], idx, mass, frames.ravel()]
    b_cov, b_mean, b_rmsf2, _, b_rmsd2 = fr.bounds(ref, fr.EPS32, k)
    rows += [ref.mean.ravel(), b_mean.ravel(), ref.rmsf, b_rmsf2, ref.cov.ravel(), b_cov.ravel(), ref.rmsd, b_rmsd2]
    b_cov, b_mean, b_rmsf2, _, b_rmsd2 = fr.bounds(ref, fr.EPS64, k)
    rows += [b_mean.ravel(), b_rmsf2, b_cov.ravel(), b_rmsd2]
    with open(path, "w") as f:
        for row in rows:
            f.write(" ".join(repr(float(v)) if not float(v).is_integer() or abs(v) > 1e15 else str(int(v)) for v in np.asarray(row, dtype=np.float64)) + "\n")


@pytest.mark.gpu
def test_cpp_fluct_gpu():
    from molar_amd import build
    build.build_library()
    os.makedirs(OUT, exist_ok=True)
    libdir = os.path.join(ROOT, "molar_amd")
    exe = os.path.join(OUT, "test_fluct_gpu")
    case = os.path.join(OUT, "fluct_case.txt")
    write_case(case)
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_fluct_gpu.cpp"), "-o", exe, "-L", libdir, "-lmolar_hip", "-lpthread",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe, case], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all fluctuations host-mirror tests passed" in r.stdout
