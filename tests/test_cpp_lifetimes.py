"""Compiles and runs tests/cpp/test_lifetimes_gpu.cpp: molar::lifetimes of the C++ host mirror on one small presence matrix, the
expected integers computed in the test by the definition in plain C++ loops (the compile recipe of test_cpp_hbonds.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "cpp", "_build")


@pytest.mark.gpu
def test_cpp_lifetimes_gpu():
    from molar_amd import build
    build.build_library()
    os.makedirs(OUT, exist_ok=True)
    libdir = os.path.join(ROOT, "molar_amd")
    exe = os.path.join(OUT, "test_lifetimes_gpu")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_lifetimes_gpu.cpp"), "-o", exe, "-L", libdir, "-lmolar_hip", "-lpthread",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all lifetimes host-mirror tests passed" in r.stdout
