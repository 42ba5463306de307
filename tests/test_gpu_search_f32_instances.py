"""Every compiled instance of the f32 pair search against the f32 oracle, at pinned cell occupancies: the cases of
tests/search_f32_cases.py (proved without a GPU by tests/test_search_f32_cases_cpu.py), each compared for exact equality - ids,
order and distance bits of the lists, ids of `within`, histogram bins as integers.  Nothing is compared with a tolerance.

What the cases pin, and where the edge comes from:

  pair_small.hip     small_pair_kernel<FILL, G = 16 | 32>: rows and candidates of 15 / 16 / 17, 31 / 32 / 33, 63 / 64 / 65 (blocks of G
                     rows, blocks of G candidates, slots of 64 rows), crowded cells of up to 129 atoms in a sparse grid
  pair_kernels.hpp   run_task_nch: the register instances of 1 .. 8 chunks (KREG) and the streaming loop above 512 atoms; the
                     matrix-core count up to 320 atoms (32 * MFMA_TILES) and the vector count of 1 .. 5 chunks behind it, reached
                     by cases scaled until mfma_bound_usable declines; KMAX_WIDE: the instances of 9 .. 16 chunks and the
                     hand-over at 1024 / 1025; KMAX_HUGE: the rounded sizes 16 / 20 / 24 / 28 / 32 with their padding, entered
                     from 513, 1024, 1025, 1280, 1281, 1536, 1537, 1792, 1793, 2048, and the hand-over at 2048 / 2049; slots of 2
                     and 8 rows for the corner entries of a sheared box; run_task with the chunk count at run time for vdW and
                     `within`; live-row and consecutive-slot variants (pair_kernel<.., LIVE>)
  search_shape.hpp   pair_family at 13, 19, 448 and 1000 atoms per judged cell - all cells on the first search of a shape, the
                     occupied ones after it -, live_row_slots, wrapped_pair_policy (band-classified with 4 cells or more per
                     periodic dimension, exact below)
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import search_f32_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = sc.all_cases()
NBINS = 300


@pytest.fixture(scope="module")
def eng():
    from molar_amd import build
    from molar_amd.api import Engine
    build.build_library()
    return Engine(0)


def api():
    import molar_amd.api as a
    return a


def same(got, ref, what):
    """(i, j, d) equal to the oracle's entry by entry, distances bit for bit; on a mismatch the first differing index is reported"""
    gi, gj, gd = got
    assert gd.dtype == np.float32 and ref["d"].dtype == np.float32
    got = (np.asarray(gi).astype(np.uint64), np.asarray(gj).astype(np.uint64), np.asarray(gd).view(np.uint32))
    want = (ref["i"], ref["j"], ref["d"].view(np.uint32))
    n = min(len(got[0]), len(want[0]))
    bad = np.zeros(n, bool)
    for g, w in zip(got, want):
        bad |= g[:n] != w[:n]
    if bad.any() or len(got[0]) != len(want[0]):
        k = int(np.argmax(bad)) if bad.any() else n
        lo, hi = max(k - 1, 0), k + 2
        pytest.fail(f"{what}: {len(got[0])} pairs, oracle {len(want[0])}; first difference at {k}: engine "
                    f"{[g[lo:hi].tolist() for g in got]}, oracle {[w[lo:hi].tolist() for w in want]}")


def same_ids(got, want, what):
    got = np.asarray(got).astype(np.uint64)
    if not np.array_equal(got, want):
        n = min(len(got), len(want))
        bad = np.flatnonzero(got[:n] != want[:n])
        pytest.fail(f"{what}: {len(got)} ids, oracle {len(want)}; first difference at {int(bad[0]) if len(bad) else n}")


def request(c, device=False):
    """(kind, cutoff, positional and keyword arguments) of the engine's search calls for a case"""
    a = api()
    kind = {"single": a.SEARCH_SINGLE, "double": a.SEARCH_DOUBLE, "vdw": a.SEARCH_DOUBLE_VDW, "within": a.SEARCH_WITHIN}[c["kind"]]
    kw = dict(box=c["box"], pbc=c["pbc"]) if c["box"] is not None else {}
    if c["lower"] is not None:
        kw = dict(lower=c["lower"], upper=c["upper"])
    p1, p2 = c["p1"], c["p2"]
    if device:
        import torch
        p1 = torch.from_numpy(p1).cuda()
        p2 = None if p2 is None else torch.from_numpy(p2).cuda()
    if c["kind"] == "vdw":
        kw.update(vdw1=c["v1"], vdw2=c["v2"])
    return kind, (None if c["kind"] == "vdw" else c["cutoff"]), (p1, None, p2, None), kw


def forget_the_last_shape(eng):
    """The context judges a shape it has just searched by its occupied cells.  A search of another shape in between makes the
    next one the first of its shape again, whatever ran before this test."""
    a = api()
    assert eng.search_count(a.SEARCH_SINGLE, 0.5, np.array([[0.1, 0.1, 0.1], [0.3, 0.1, 0.1], [2.0, 2.0, 2.0]], np.float32)) == 1


def check_shape(eng, c, ref, call, what):
    """grid, reported family and slot counts after search call number `call` of the case's shape"""
    assert eng.grid_dims() == tuple(ref["dims"]) == c["dims"], what
    assert eng.search_cell_kernels()[0] == c["family"][min(call, 1)], (what, eng.search_cell_kernels(), c["family"])
    slots, rows = eng.search_slot_counts()
    if c["live"][min(call, 1)]:
        assert 0 < slots <= rows, (what, slots, rows)
    else:
        assert 0 < slots == rows, (what, slots, rows)


@pytest.mark.parametrize("name", list(CASES))
def test_instance_at_pinned_occupancies(eng, orc32, name):
    """One case: count + fill, resident + fill (vdW included), the fused histogram of the fixed-cutoff kinds, the `within` stream
    and set - each the oracle's, with the grid, the kernel family and the slot counts checked after every search call."""
    c = CASES[name]
    ref = sc.cached_reference(orc32, c)
    kind, rc, pos, kw = request(c)
    a = api()
    forget_the_last_shape(eng)
    cnt = eng.search_count(kind, rc, *pos, **kw)
    check_shape(eng, c, ref, 0, name + " (count)")
    assert cnt == len(ref["i"]) > 0, (name, cnt, len(ref["i"]))
    if c["kind"] == "within":
        same_ids(eng.search_fill_ids(cnt), ref["i"], name + " (count + fill)")
        cnt2 = eng.search_count(kind, rc, *pos, **kw)
        check_shape(eng, c, ref, 1, name + " (second count)")
        same_ids(eng.search_fill_ids(cnt2), ref["i"], name + " (second count + fill)")
        ids = eng.within_set(rc, *pos, **kw)
        same_ids(ids, np.unique(ref["i"]), name + " (within set)")
        return
    pairs, d = eng.search_fill(cnt)
    same((pairs[:, 0], pairs[:, 1], d), ref, name + " (count + fill)")
    cnt2, _, _ = eng.search_resident(kind, rc, *pos, **kw)
    check_shape(eng, c, ref, 1, name + " (resident)")
    assert cnt2 == cnt
    pairs2, d2 = eng.search_fill(cnt2)
    same((pairs2[:, 0], pairs2[:, 1], d2), ref, name + " (resident + fill)")
    assert np.array_equal(pairs, pairs2) and np.array_equal(d.view(np.uint32), d2.view(np.uint32))
    if c["kind"] in sc.FIXED:
        hmax = c["cutoff"]
        want = orc32.histogram_add(0.0, hmax, NBINS, ref["d"]).astype(np.uint64)
        bins, hcnt = eng.search_histogram(kind, rc, 0.0, hmax, NBINS, *pos, **kw)          # (leaves no cached search: no grid to ask for)
        assert eng.search_cell_kernels()[0] == c["family"][1], (name, "after the histogram")
        assert hcnt == len(ref["d"]) and np.array_equal(np.asarray(bins, np.uint64), want), name + " (histogram)"


RESIDENT = ("small16-double-tric-0", "small32-single-ortho7-0", "regular-single-ortho7-0", "regular-double-notlive", "regular-single-ortho7-0-declined",
            "wide-single-band-0", "wide-double-tric-0", "huge-single-band-0", "huge-double-tric-0", "huge-single-nobox", "regular-vdw-tric-0")


@pytest.mark.parametrize("name", RESIDENT)
def test_coordinates_resident_and_result_left_on_the_device(eng, orc32, name):
    """Coordinates in device memory (no staging copy), the result filled into tensors of the caller's on the device."""
    import torch
    c = CASES[name]
    ref = sc.cached_reference(orc32, c)
    kind, rc, pos, kw = request(c, device=True)
    forget_the_last_shape(eng)
    cnt = eng.search_count(kind, rc, *pos, **kw)
    check_shape(eng, c, ref, 0, name + " (count, resident coordinates)")
    assert cnt == len(ref["i"])
    pairs = torch.empty((cnt, 2), dtype=torch.int32, device="cuda")
    dist = torch.empty(cnt, dtype=torch.float32, device="cuda")
    eng.search_fill_into(pairs, dist)
    torch.cuda.synchronize()
    hp = pairs.cpu().numpy().view(np.uint32)
    same((hp[:, 0], hp[:, 1], dist.cpu().numpy()), ref, name + " (device fill)")
    cnt2, pp, dp = eng.search_resident(kind, rc, *pos, **kw)
    check_shape(eng, c, ref, 1, name + " (resident, resident coordinates)")
    assert cnt2 == cnt and pp and dp
    hp = api().device_view(pp, (cnt2, 2), torch.int32).cpu().numpy().view(np.uint32)          # the engine's own buffers, read in place
    hd = api().device_view(dp, (cnt2,), torch.float32).cpu().numpy()
    same((hp[:, 0], hp[:, 1], hd), ref, name + " (resident, the engine's buffers)")


@pytest.mark.parametrize("mean", [t[0] for t in sc.THRESHOLDS])
@pytest.mark.parametrize("kind", sc.FIXED)
def test_one_atom_changes_the_family(eng, orc32, mean, kind):
    """N = mean * cells and one atom more on the same grid, one after the other on one context: the reported family changes, and
    changes back, and every list is the oracle's."""
    a = api()
    at, above = CASES[f"threshold-{mean}-{kind}"], CASES[f"threshold-{mean}+1-{kind}"]
    assert at["family"] != above["family"]
    forget_the_last_shape(eng)
    for c in (at, above, at):
        ref = sc.cached_reference(orc32, c)
        k, rc, pos, kw = request(c)
        cnt = eng.search_count(k, rc, *pos, **kw)
        assert eng.search_cell_kernels()[0] == c["family"][0], (c["name"], eng.search_cell_kernels())
        pairs, d = eng.search_fill(cnt)
        same((pairs[:, 0], pairs[:, 1], d), ref, c["name"])
