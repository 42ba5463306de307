"""Compiles and runs tests/cpp/test_vanhove_gpu.cpp: molar::van_hove of the C++ host mirror on one small shape against counts the
C++ test computes itself (the compile recipe of test_cpp_mindist.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "cpp", "_build")


def command(exe, libdir):
    return ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
            os.path.join(ROOT, "tests", "cpp", "test_vanhove_gpu.cpp"), "-o", exe, "-L", libdir, "-lmolar_hip", "-lpthread",
            f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]


def test_cpp_vanhove_compiles():
    from molar_amd import build
    build.build_library()
    os.makedirs(OUT, exist_ok=True)
    r = subprocess.run(command(os.path.join(OUT, "test_vanhove_gpu"), os.path.join(ROOT, "molar_amd")), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_vanhove_gpu():
    from molar_amd import build
    build.build_library()
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "test_vanhove_gpu")
    r = subprocess.run(command(exe, os.path.join(ROOT, "molar_amd")), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = {k: v for k, v in os.environ.items() if not k.startswith("MOLAR_HIP_VANHOVE_")}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all van Hove host-mirror tests passed" in r.stdout
