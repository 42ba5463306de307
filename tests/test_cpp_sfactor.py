"""Compiles and runs tests/cpp/test_sfactor_gpu.cpp: molar::structure_factor of the C++ host mirror on one small case whose input
and expected numbers (the longdouble reference of tests/sfactor_ref.py with its bounds) are written here (the compile recipe
and the case-file form of test_cpp_tcf.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sfactor_ref as sr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "cpp", "_build")
CASE = sr.C("cpp", 30, 3, (2, 2, 1), box="tric", G=2, idx=True, signed=True, nshells=6)
DEFAULT_ATOM_CHUNK = 2048            # no override here: one K split


def write_case(path):
    frames, boxes, idx, weight, labels = sr.case_inputs(CASE)
    args = (frames, boxes, idx, weight, labels, CASE.G, CASE.hmax, CASE.qmin, CASE.dq, CASE.nshells, DEFAULT_ATOM_CHUNK)
    r32, r64 = sr.reference(*args, sr.EPS32), sr.reference(*args, sr.EPS64)
    rows = [[CASE.F, CASE.natoms, idx.shape[0], CASE.G, *CASE.hmax, CASE.nshells, sr.QMIN, sr.DQ], idx, labels, weight, boxes, frames.ravel(),
            r32.frame_ok, r32.shell_count]
    for name, bound in (("rho", "b_rho"), ("rho_mean", "b_mean"), ("sab", "b_sab"), ("shell", "b_shell")):
        want = getattr(r32, name)
        # the expected numbers are written in f64: their own rounding joins the bound
        extra = 2.0 ** -52 * np.abs(np.nan_to_num(want))
        rows += [want.ravel(), (getattr(r32, bound) + extra).ravel(), (getattr(r64, bound) + extra).ravel()]
    with open(path, "w") as f:
        for row in rows:
            f.write(" ".join("nan" if np.isnan(v) else repr(float(v)) if not float(v).is_integer() or abs(v) > 1e15 else str(int(v))
                             for v in np.asarray(row, dtype=np.float64)) + "\n")


def test_case_file_is_written(tmp_path):
    path = tmp_path / "case.txt"
    write_case(str(path))
    lines = open(path).read().split("\n")
    assert lines[0].split() == ["3", "30", "20", "2", "2", "2", "1", "6", "0.013", "0.37"]
    assert "nan" in lines[-4].split(), "a shell that stays empty is NaN in the reference"


@pytest.mark.gpu
def test_cpp_sfactor_gpu():
    from molar_amd import build
    build.build_library()
    os.makedirs(OUT, exist_ok=True)
    libdir = os.path.join(ROOT, "molar_amd")
    exe = os.path.join(OUT, "test_sfactor_gpu")
    case = os.path.join(OUT, "sfactor_case.txt")
    write_case(case)
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_sfactor_gpu.cpp"), "-o", exe, "-L", libdir, "-lmolar_hip", "-lpthread",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = {k: v for k, v in os.environ.items() if not k.startswith("MOLAR_HIP_SFACTOR_")}
    r = subprocess.run([exe, case], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all structure-factor host-mirror tests passed" in r.stdout
