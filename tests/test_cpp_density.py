"""Compiles and runs tests/cpp/test_density_gpu.cpp: molar::density of the C++ host mirror on one small case whose input and
expected numbers (the numpy reference of tests/density_ref.py with its bounds) are written here (the compile recipe of
test_cpp_msd.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import density_ref as dr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "cpp", "_build")


def write_case(path):
    F, natoms, nz, G = 5, 120, 16, 3
    rng = np.random.default_rng(41)
    box = dr.ORTHO                                             # exact in f32
    frames = dr.scatter_box(42, F, natoms, (1, 1, nz), box)
    idx = np.flatnonzero(np.arange(natoms) % 7 != 3).astype(np.uint64)
    labels = rng.integers(0, G, len(idx))
    mass = rng.uniform(1.0, 16.0, natoms).astype(np.float32)
    ref = dr.density(frames, dr.grid(dr.BOX, (1, 1, nz)), idx=idx, weight=mass, labels=labels, ngroups=G, boxes=box)
    dr.margin_ok(ref)
    d64 = ref["density"].astype(np.float64).ravel()
    tol64 = ref["dens_bound"].ravel() + 2.0 ** -52 * np.abs(d64)
    rows = [[F, natoms, len(idx), nz, G, ref["S"]], idx, labels, mass, box, frames.ravel(), ref["count"].ravel(), ref["outside"], d64,
            tol64 + dr.half_ulp32(d64), tol64]
    with open(path, "w") as f:
        for row in rows:
            f.write(" ".join(repr(float(v)) if not float(v).is_integer() or abs(v) > 1e15 else str(int(v)) for v in np.asarray(row, dtype=np.float64)) + "\n")


@pytest.mark.gpu
def test_cpp_density_gpu():
    from molar_amd import build
    build.build_library()
    os.makedirs(OUT, exist_ok=True)
    libdir = os.path.join(ROOT, "molar_amd")
    exe = os.path.join(OUT, "test_density_gpu")
    case = os.path.join(OUT, "density_case.txt")
    write_case(case)
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_density_gpu.cpp"), "-o", exe, "-L", libdir, "-lmolar_hip", "-lpthread",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe, case], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all density host-mirror tests passed" in r.stdout
