"""Compiles and runs tests/cpp/test_sasa_vol_gpu.cpp: SelBound::sasa_vol of the C++ host mirror against a brute-force
restatement of the definition (the compile recipe of test_cpp_sasa.py; no contraction in the restatement either)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "cpp", "_build")


@pytest.mark.gpu
def test_selbound_sasa_vol_gpu():
    from molar_amd import build
    build.build_library()
    os.makedirs(OUT, exist_ok=True)
    libdir = os.path.join(ROOT, "molar_amd")
    exe = os.path.join(OUT, "test_sasa_vol_gpu")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_sasa_vol_gpu.cpp"), "-o", exe, "-L", libdir, "-lmolar_hip", "-lpthread",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all sasa_vol host-mirror tests passed" in r.stdout
