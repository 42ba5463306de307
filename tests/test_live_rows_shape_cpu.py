"""Compiles and runs tests/cpp/test_live_rows_shape.cpp: which searches cut their slots from live rows, and the size of the masks
(molar_amd/csrc/search_shape.hpp), on the host - no GPU needed to run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "cpp", "_build")


def test_live_rows_shape_cpu():
    from molar_amd import build
    build.build_library()
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "test_live_rows_shape")
    libdir = os.path.join(ROOT, "molar_amd")
    cmd = ["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-std=c++17",
           os.path.join(ROOT, "tests", "cpp", "test_live_rows_shape.cpp"), "-o", exe, "-L", libdir, "-lmolar_hip", f"-Wl,-rpath,{libdir}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "all live-row shape tests passed" in r.stdout, r.stdout + r.stderr
