"""Compiles and runs tests/cpp/test_clusters_gpu.cpp: molar::clusters / clusters_frames of the C++ host mirror on the blob frame of
tests/clusters_ref.py, whose partition is known by construction (the compile recipe of test_cpp_host.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clusters_ref as cl  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "cpp", "_build")


@pytest.mark.gpu
def test_clusters_gpu():
    from molar_amd import build
    build.build_library()
    os.makedirs(OUT, exist_ok=True)
    pos, box, lab = cl.blob_frame()
    comp_of = cl.canonical(lab)
    # the blobs as groups: every atom goes with the blob nearest to it (a bridge atom with either of the two it joins), 8 groups;
    # the bridged blobs fall together: blob 4 into blob 0's component, blob 3 into blob 2's
    blob = blob_of_atoms(pos, box)
    gcomp_of = cl.canonical([{4: 0, 3: 2}.get(b, b) for b in range(8)])
    case = os.path.join(OUT, "clusters_case.bin")
    with open(case, "wb") as f:
        np.array([len(pos), int(comp_of.max()) + 1], np.uint64).tofile(f)
        np.concatenate([[cl.BLOB_CUTOFF], np.ascontiguousarray(box.T).reshape(9)]).astype(np.float32).tofile(f)      # column-major
        pos.astype(np.float32).tofile(f)
        comp_of.astype(np.uint32).tofile(f)
        blob.astype(np.uint32).tofile(f)
        np.array([8, int(gcomp_of.max()) + 1], np.uint64).tofile(f)
        gcomp_of.astype(np.uint32).tofile(f)
    libdir = os.path.join(ROOT, "molar_amd")
    exe = os.path.join(OUT, "test_clusters_gpu")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_clusters_gpu.cpp"), "-o", exe, "-L", libdir, "-lmolar_hip", "-lpthread",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe, case], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all clusters host-mirror tests passed" in r.stdout


def blob_of_atoms(pos, box):
    """the blob (0 .. 7) nearest to every atom of the blob frame under the minimum image: its 2 x 2 x 2 lattice cell"""
    L = float(box[0, 0])
    centres = np.array([[3.35 * (b >> 2), 0.9 + 3.35 * ((b >> 1) & 1), 0.9 + 3.35 * (b & 1)] for b in range(8)])
    d = pos[:, None, :].astype(np.float64) - centres[None, :, :]
    d -= L * np.round(d / L)
    return np.argmin((d * d).sum(-1), axis=1)
