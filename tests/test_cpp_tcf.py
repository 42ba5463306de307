"""Compiles and runs tests/cpp/test_tcf_gpu.cpp: molar::vector_correlations of the C++ host mirror on one small case whose input
and expected numbers (the longdouble reference of tests/tcf_ref.py with its bounds) are written here (the compile recipe and
the case-file form of test_cpp_intcoord.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tcf_ref as tr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "cpp", "_build")


def write_case(path):
    F, V, G, L = 40, 9, 3, 25
    labels = np.arange(V) % G
    box = np.asarray(tr.ORTHO, np.float64)
    frames, tuples = tr.make_case(F, V, 2, 61, box9=box)
    ref = tr.tcf(frames, tuples, labels=labels, ngroups=G, boxes=box, max_lag=L)
    b32, b64 = tr.bounds(ref, tr.EPS32), tr.bounds(ref, tr.EPS64)
    rows = [[F, frames.shape[1], V, G, L], tuples.ravel(), labels, box, frames.ravel(), ref["nvalid"], ref["bad_frames"]]
    for name in ("c1", "c2", "c1_vec", "c2_vec", "mean", "s2"):
        want = ref[name].astype(np.float64)
        # the expected numbers are written in f64: their own rounding joins the bound
        extra = 2.0 ** -52 * np.abs(want)
        rows += [want.ravel(), (np.broadcast_to(b32[name], want.shape) + extra).ravel(), (np.broadcast_to(b64[name], want.shape) + extra).ravel()]
    with open(path, "w") as f:
        for row in rows:
            f.write(" ".join(repr(float(v)) if not float(v).is_integer() or abs(v) > 1e15 else str(int(v)) for v in np.asarray(row, dtype=np.float64)) + "\n")


def test_case_file_is_written(tmp_path):
    path = tmp_path / "case.txt"
    write_case(str(path))
    head = open(path).readline().split()
    assert head == ["40", "29", "9", "3", "25"]


@pytest.mark.gpu
def test_cpp_tcf_gpu():
    from molar_amd import build
    build.build_library()
    os.makedirs(OUT, exist_ok=True)
    libdir = os.path.join(ROOT, "molar_amd")
    exe = os.path.join(OUT, "test_tcf_gpu")
    case = os.path.join(OUT, "tcf_case.txt")
    write_case(case)
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_tcf_gpu.cpp"), "-o", exe, "-L", libdir, "-lmolar_hip", "-lpthread",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe, case], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all vector-correlation host-mirror tests passed" in r.stdout
