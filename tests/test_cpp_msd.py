"""Compiles and runs tests/cpp/test_msd_gpu.cpp: molar::msd of the C++ host mirror on one small case whose input and expected
numbers (the numpy reference of tests/msd_ref.py with its bounds) are written here (the compile recipe of
test_cpp_fluct.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msd_ref as mr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "cpp", "_build")


def write_case(path):
    from molar_amd import api
    F, natoms, L, stride = 17, 40, 9, 2
    rng = np.random.default_rng(31)
    box = mr.ORTHO                                             # exact in f32
    frames, _ = mr.wrapped_walk(F, natoms, 32, box, 0.45)
    idx = np.flatnonzero(np.arange(natoms) % 7 != 3).astype(np.uint64)
    off = mr.groups_unequal(len(idx))
    refset = np.arange(0, natoms, 3).astype(np.uint64)
    mass = rng.uniform(1.0, 16.0, natoms).astype(np.float32)
    ref = mr.msd(frames, idx=idx, mass=mass, boxes=box, groups=off, ref_idx=refset, max_lag=L, origin_stride=stride, dims=3)
    P = len(off) - 1
    chunk = api.msd_plan(F, len(idx), P, len(refset), L)[1]
    rows = [[F, natoms, len(idx), P, len(refset), L, stride, 3], idx, off, refset, mass, box, frames.ravel()]
    for eps in (mr.EPS32, mr.EPS64):
        b_disp, b_msd, b_m4, b_par = mr.bounds(ref, eps, chunk)
        rows += [ref["msd"], b_msd, ref["m4"], b_m4, ref["msd_particle"].ravel(), b_par.ravel(), ref["disp"].ravel(), b_disp.ravel()]
    with open(path, "w") as f:
        for row in rows:
            f.write(" ".join(repr(float(v)) if not float(v).is_integer() or abs(v) > 1e15 else str(int(v)) for v in np.asarray(row, dtype=np.float64)) + "\n")


@pytest.mark.gpu
def test_cpp_msd_gpu():
    from molar_amd import build
    build.build_library()
    os.makedirs(OUT, exist_ok=True)
    libdir = os.path.join(ROOT, "molar_amd")
    exe = os.path.join(OUT, "test_msd_gpu")
    case = os.path.join(OUT, "msd_case.txt")
    write_case(case)
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_msd_gpu.cpp"), "-o", exe, "-L", libdir, "-lmolar_hip", "-lpthread",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe, case], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all msd host-mirror tests passed" in r.stdout
