"""Compiles and runs tests/cpp/test_mindist_gpu.cpp: molar::min_distances of the C++ host mirror on one small case whose input and
expected numbers (the longdouble reference of tests/mindist_ref.py with its bounds) are written here (the compile recipe and
the case-file form of test_cpp_sfactor.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mindist_ref as mr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "cpp", "_build")
CASE = mr.C("cpp", 3, 100, 40, 45, box="tric", G1=4, G2=3, idx=True, seed=77)


def write_case(path):
    frames, boxes, idx1, idx2, lab1, lab2 = mr.case_inputs(CASE)
    r32, r64 = mr.case_reference(CASE, mr.EPS32), mr.case_reference(CASE, mr.EPS64)
    rows = [[CASE.F, CASE.natoms, CASE.n1, CASE.n2, CASE.G1, CASE.G2, mr.CUTOFF], idx1, idx2, lab1, lab2, boxes, frames.ravel(),
            r32.pair.ravel(), r32.near1.ravel(), r32.mat_freq.ravel(), r32.frame_ok]
    for name, bound in (("dist", "b_dist"), ("atom1", "b_atom1"), ("atom2", "b_atom2"), ("mat", "b_mat"), ("mat_mean", "b_mean"), ("mat_min", "b_min")):
        want = getattr(r32, name)
        # the expected numbers are written in f64: their own rounding joins the bound
        extra = 2.0 ** -52 * np.abs(np.nan_to_num(want, posinf=0.0))
        rows += [want.ravel(), (getattr(r32, bound) + extra).ravel(), (getattr(r64, bound) + extra).ravel()]
    with open(path, "w") as f:
        for row in rows:
            f.write(" ".join("inf" if np.isposinf(v) else repr(float(v)) if not float(v).is_integer() or abs(v) > 1e15 else str(int(v))
                             for v in np.asarray(row, dtype=np.float64)) + "\n")


def test_case_file_is_written(tmp_path):
    path = tmp_path / "case.txt"
    write_case(str(path))
    lines = open(path).read().split("\n")
    assert lines[0].split() == ["3", "100", "40", "45", "4", "3", "0.4"]
    assert len(lines) == 11 + 18 + 1
    assert "inf" in lines[11 + 9].split(), "the empty group of set 1 is +inf in mat"


@pytest.mark.gpu
def test_cpp_mindist_gpu():
    from molar_amd import build
    build.build_library()
    os.makedirs(OUT, exist_ok=True)
    libdir = os.path.join(ROOT, "molar_amd")
    exe = os.path.join(OUT, "test_mindist_gpu")
    case = os.path.join(OUT, "mindist_case.txt")
    write_case(case)
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_mindist_gpu.cpp"), "-o", exe, "-L", libdir, "-lmolar_hip", "-lpthread",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = {k: v for k, v in os.environ.items() if not k.startswith("MOLAR_HIP_MINDIST_")}
    r = subprocess.run([exe, case], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all minimum-distance host-mirror tests passed" in r.stdout
