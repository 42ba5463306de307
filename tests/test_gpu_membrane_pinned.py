"""The membrane smoothing pass (k_membrane_fit_lanes, k_membrane_fit<float | double>, k_membrane_average, launch_fit) on the
frames of tests/pinned_patches.py: patch lengths on both sides of the sixteen-lane kernel's LDS slice (96 | 97), of the
one-lane kernel's LDS / HBM rule (60 | 61) and of the 16-member rounds; Voronoi cells that end with, or pass through, more
than 16 vertices; reverse counts around the average's rounds of 16; 1 .. 65 lipids; and the 32- and 64-lane workgroups that
launch_fit picks above 32 and 64 lipids per compute unit.  Engine.membrane_smooth against Oracle("f32"), MeasureF64.membrane_smooth
against Oracle("f64"), with the checks of test_gpu_membrane.py (structure exact, floats 2e-5) and test_gpu_membrane_f64.py
(1e-12, lipids invalid on entry untouched).  That the frames are what they claim is asserted in tests/test_pinned_patches_cpu.py."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pinned_patches as pp  # noqa: E402
from test_gpu_membrane import check_smooth  # noqa: E402
from test_gpu_membrane_f64 import PER_LIPID, check_state  # noqa: E402
from test_pinned_patches_cpu import allowance_used  # noqa: E402

pytestmark = pytest.mark.gpu

STATE = PER_LIPID + ("valid", "neib_ids", "voro_vertexes", "fitted_patch_points")
ORACLE_KEYS = dict(coefs="quad_coefs", mean_curv="mean_curv", gauss_curv="gauss_curv", princ_curvs="princ_curvs", princ_dirs="princ_dirs",
                   area="area", normals="normals", head="head_markers", voro="voro_vertexes", fitted="fitted_patch_points")


@pytest.fixture(scope="module")
def eng():
    from molar_amd import build
    from molar_amd.api import Engine
    build.build_library()
    return Engine(0)


@pytest.fixture(scope="module")
def m64(eng):
    from molar_amd.api import MeasureF64
    return MeasureF64(eng)


@functools.lru_cache(maxsize=None)
def frame(name, arg=None):
    if name == "length":
        return pp.length_frame(arg)
    if name == "small":
        return pp.small_frame(arg)
    if name == "large":
        return pp.large_frame(arg)
    return {"ring": pp.ring_frame, "hub": pp.hub_frame}[name]()


def handed_off(f):
    """lipids valid on entry that the sixteen-lane kernel hands to the one-lane kernel by construction: more than 96 members,
    or a cell built to hold more than 16 vertices"""
    rec = f["record"]
    n = int(np.count_nonzero((np.diff(f["patch_off"].astype(np.int64)) > 96) & (f["valid"] == 1)))
    if "built" in rec:
        n += sum(1 for b in rec["built"] if b["m"] > 16 and b["pad"] <= 96)
    return n


def one_pass(prec, gpu, orc, f, st=None, label=""):
    """one smoothing pass of the GPU on the frame (or on the state `st` of an earlier pass) against one pass of the oracle on the
    same inputs; returns the state"""
    from molar_amd import api
    r = np.float32 if prec == "f32" else np.float64
    K = len(f["valid"])
    poff, pids, box = f["patch_off"], f["patch_ids"], f["box"].astype(r)
    if st is None:
        st = api.new_membrane_state(f["head"].astype(r), f["normals"].astype(r), f["valid"], len(pids), dtype=r)
    entry = {k: v.copy() for k, v in st.items() if hasattr(v, "copy")}
    want = orc.membrane_smooth(orc.box_from_matrix(box), entry["head_markers"], entry["normals"], entry["valid"], poff, pids)
    gpu.membrane_smooth(box, st, poff, pids)
    assert np.array_equal(st["valid"], want["valid"]), np.flatnonzero(st["valid"] != want["valid"])[:10]      # over all lipids
    if not want["valid"].any():                          # nothing to compare but the flags and what must stay as it was
        for k in STATE:
            assert st[k].tobytes() == entry[k].tobytes() or k == "valid", k
        print(f"{label} {prec}: no lipid of {K} valid")
    elif prec == "f32":
        if np.array_equal(st["nvert"][want["valid"] == 1], want["nvert"][want["valid"] == 1]):
            used = allowance_used("f32", {k: st[g] for k, g in ORACLE_KEYS.items()}, want, poff)
            top = max(used, key=used.get)
            print(f"{label} f32: {int(want['valid'].sum())} of {K} lipids valid, {handed_off(f)} handed to the one-lane kernel; "
                  f"largest deviation {used[top]:.3f} of the tolerance 2e-5 ({top})")
        check_smooth(dict(st, smoothed_head=st["head_markers"]), want, poff, K)
        off = entry["valid"] == 0                        # lipids invalid on entry keep their values, byte for byte
        for k in PER_LIPID:
            assert st[k][off].tobytes() == entry[k][off].tobytes(), k
    else:
        check_state(st, want, poff, K, entry=entry, label=f"{label} f64: {int(want['valid'].sum())} of {K} lipids valid;")
    return st, want


@pytest.fixture(params=["f32", "f64"])
def side(request, eng, m64, orc32, orc64):
    return (request.param, eng, orc32) if request.param == "f32" else (request.param, m64, orc64)


@pytest.mark.parametrize("order", pp.ORDERS)
def test_patch_lengths(side, order):
    f = frame("length", order)
    st, want = one_pass(*side, f, label=f"length_frame {order}")
    n = f["record"]["np"]
    ok = st["valid"].astype(bool)
    for t in pp.LENGTH_TABLE[1:]:
        assert np.count_nonzero(ok & (n == t)) >= 2, t
    assert not ok[n == 0].any()


def test_cell_sizes(side):
    f = frame("ring")
    st, want = one_pass(*side, f, label="ring_frame")
    rec = f["record"]
    po = f["patch_off"].astype(np.int64)
    for c, b in zip(rec["centres"], rec["built"]):
        m = b["m"]
        assert st["valid"][c] and st["nvert"][c] == (6 if b["kind"] == "transient" else m), b
        s0 = int(po[c]) + 4 * int(c)
        first = {"final": 0, "transient": m, "last": 8}[b["kind"]]
        ring = f["patch_ids"][po[c] + first:po[c] + first + (6 if b["kind"] == "transient" else m)]
        nb = st["neib_ids"][s0:s0 + len(ring)]
        assert sorted(nb.tolist()) == sorted(ring.tolist()), b        # the direct neighbours are the ring that was built
        if side[0] == "f32" and m <= 16 and not b["pad"] and b["kind"] != "transient":
            # wholly in the sixteen-lane kernel: the ring of lanes, read out from the cell's init vertex, in the oracle's order
            assert np.array_equal(nb, want["neib_ids"][s0:s0 + m]), b


def test_reverse_counts(side):
    f = frame("hub")
    rec = f["record"]
    st, want = one_pass(*side, f, label="hub_frame pass 1")
    assert np.array_equal(pp.reverse_counts(f)[rec["hubs"]], rec["counts"])
    hubs = rec["hubs"]
    assert st["valid"][hubs].all() and not st["valid"][rec["role"] != 0].any()
    tol = 2e-5 if side[0] == "f32" else 1e-12            # (the checks above hold every valid lipid's marker; the hubs once more, by name)
    assert np.allclose(st["head_markers"][hubs], want["head"][hubs], rtol=tol, atol=tol)
    # second iteration: the flags of the first carry over, the owners it dropped stay out of the hubs' averages
    st, want = one_pass(*side, f, st=st, label="hub_frame pass 2")
    assert st["valid"][hubs].all()
    assert np.allclose(st["head_markers"][hubs], want["head"][hubs], rtol=tol, atol=tol)


@pytest.mark.parametrize("K", pp.SMALL_K)
def test_small_k(side, K):
    f = frame("small", K)
    st, _ = one_pass(*side, f, label=f"small_frame {K}")
    assert bool(st["valid"][0]) == (K >= 8) and not st["valid"][1:].any()
    if K >= 8:
        assert st["nvert"][0] == 7


@pytest.mark.parametrize("prec,per_cu", [("f32", 32), ("f32", 64), ("f64", 32)])
def test_workgroup_shapes(eng, m64, orc32, orc64, prec, per_cu):
    """one lipid more than 32 (64) per compute unit: launch_fit goes from 16 to 32 lanes a workgroup (to 64 in f32, 32 in f64)"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    K = per_cu * cus + 1
    f = frame("large", K)
    assert len(f["valid"]) == K
    gpu, orc = (eng, orc32) if prec == "f32" else (m64, orc64)
    st, _ = one_pass(prec, gpu, orc, f, label=f"large_frame {K} ({cus} compute units)")
    rec = f["record"]
    assert [int(st["nvert"][c]) for c in rec["centres"]] == list(pp.LARGE_BUILT)
    sheet = rec["kind"] == 1
    assert st["valid"][sheet & (f["valid"] == 1)].all()
    for t in pp.LARGE_CYCLE:
        assert np.count_nonzero(sheet & (rec["np"] == t) & (st["valid"] == 1)) >= 8, t


@pytest.mark.parametrize("name,arg", [("length", "shuffled"), ("ring", None)])
def test_two_calls_give_the_same_bytes(side, name, arg):
    from molar_amd import api
    prec, gpu, _ = side
    r = np.float32 if prec == "f32" else np.float64
    f = frame(name, arg)
    runs = []
    for _ in range(2):
        st = api.new_membrane_state(f["head"].astype(r), f["normals"].astype(r), f["valid"], len(f["patch_ids"]), dtype=r)
        gpu.membrane_smooth(f["box"].astype(r), st, f["patch_off"], f["patch_ids"])
        runs.append(st)
    for k in STATE:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k
    again = pp.length_frame(arg) if name == "length" else pp.ring_frame()
    for k in ("head", "normals", "box", "valid", "patch_off", "patch_ids"):
        assert again[k].tobytes() == f[k].tobytes(), k
