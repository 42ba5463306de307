"""Compiles and runs tests/cpp/test_contacts_gpu.cpp: ContactMap of the C++ host mirror against the oracle's pair lists, folded
here by tests/contacts_ref.py and handed over in a file (the compile recipe of test_cpp_host.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contacts_ref as cr  # noqa: E402

from molar_amd import synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "cpp", "_build")


@pytest.mark.gpu
def test_contact_map_gpu(orc32):
    from molar_amd import build
    build.build_library()
    os.makedirs(OUT, exist_ok=True)
    natoms, nframes, cutoff = 3000, 3, 0.5
    box = synth.box_a(natoms)
    ob = orc32.box_from_matrix(box)
    frames = np.stack([synth.frame(natoms, box, f) for f in range(nframes)])
    idx1 = np.arange(0, 2000, dtype=np.uint64)
    idx2 = np.arange(1500, natoms, 2, dtype=np.uint64)
    l1 = (np.arange(len(idx1)) // 3).astype(np.uint32)
    G1 = int(l1.max()) + 1
    l2, G2 = cr.ragged_labels(len(idx2))
    i1, i2 = idx1.astype(np.int64), idx2.astype(np.int64)
    _, s_deg, s_map = cr.single(orc32.search_single_pbc(cutoff, frames[0][i1], ob, 7), len(idx1), l1, G1)
    per = [cr.double(orc32.search_double_pbc(cutoff, frames[f][i1], frames[f][i2], ob, 7), len(idx1), len(idx2), l1, G1, l2, G2)
           for f in range(nframes)]
    d_deg1, d_deg2, d_map = sum(p[1] for p in per), sum(p[2] for p in per), sum(p[3] for p in per)
    d_occ = cr.occupancy([p[3] for p in per])
    assert s_map.sum() > 0 and d_map.sum() > 0 and np.any((d_occ > 0) & (d_occ < nframes))
    case = os.path.join(OUT, "contacts_case.bin")
    with open(case, "wb") as f:
        np.array([natoms, nframes, len(idx1), len(idx2), G1, G2], np.uint64).tofile(f)
        np.concatenate([[cutoff], np.ascontiguousarray(box.T).reshape(9)]).astype(np.float32).tofile(f)      # column-major
        for arr in (frames.astype(np.float32), idx1, idx2, l1, l2.astype(np.uint32), s_deg.astype(np.uint64), s_map.astype(np.uint64),
                    d_deg1.astype(np.uint64), d_deg2.astype(np.uint64), d_map.astype(np.uint64), d_occ.astype(np.uint32)):
            np.ascontiguousarray(arr).tofile(f)
    libdir = os.path.join(ROOT, "molar_amd")
    exe = os.path.join(OUT, "test_contacts_gpu")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_contacts_gpu.cpp"), "-o", exe, "-L", libdir, "-lmolar_hip", "-lpthread",
           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe, case], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all contacts host-mirror tests passed" in r.stdout
