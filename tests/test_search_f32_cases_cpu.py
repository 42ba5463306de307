"""The inputs of tests/test_gpu_search_f32_instances.py proved on the f32 oracle and numpy alone (no GPU): every case of
tests/search_f32_cases.py has the grid, the cell populations, the kernel family and the live-row plan it was built for, and the
cases together reach every instance of the f32 pair search - the table REQUIRED of the cases module, no entry excused:

  pair_kernels.hpp   run_task_nch: chunk counts 1 .. 8 (KREG), 9 .. 16 (KMAX_WIDE), the rounded sizes 16 / 20 / 24 / 28 / 32
                     (KMAX_HUGE) from their lowest and their highest chunk count, the streaming loop of each family, the vector
                     count where the matrix-core count (MFMA_TILES: second cells up to 320 atoms) declines, first cells of 1, 63,
                     64, 65, 512 and 513 rows, slots of 2 and of 8 rows (decode_task)
  pair_small.hip     rows and candidates on either side of 16, 32 and 64
  search_shape.hpp   small_cell_lanes, pair_family with judged_cells (13, 19, 448 and 1000 atoms per cell, by all cells and by
                     occupied cells), live_row_slots, wrapped_pair_policy (band or exact)

A frame that cannot reach what it was built for fails here, not on the GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pinned_cells as pc  # noqa: E402
import search_f32_cases as sc  # noqa: E402
import search_f64_cases as s64  # noqa: E402

CASES = sc.all_cases()


def _valid_entries(c):
    """(first cell, second cell) populations of the plan entries with both cells non-empty"""
    two = c["kind"] != "single"
    pops1 = np.asarray(c["pops1"])
    pops2 = np.asarray(c["pops2"]) if two else pops1
    ca, cb, _ = s64.plan_cell_pairs(c["dims"], c["pbc"], two)
    keep = (pops1[ca] > 0) & (pops2[cb] > 0)
    return pops1[ca][keep], pops2[cb][keep]


def _oracle_plan_len(c):
    """the reference keeps an entry of two grids when either order of its two cells has atoms on both sides"""
    two = c["kind"] != "single"
    pops1 = np.asarray(c["pops1"])
    pops2 = np.asarray(c["pops2"]) if two else pops1
    ca, cb, _ = s64.plan_cell_pairs(c["dims"], c["pbc"], two)
    ok = (pops1[ca] > 0) & (pops2[cb] > 0)
    return int((ok[0::2] | ok[1::2]).sum()) if two else int(ok.sum())


@pytest.mark.parametrize("name", list(CASES))
def test_case_is_what_it_was_built_to_be(orc32, name):
    c = CASES[name]
    two = c["p2"] is not None
    assert c["p1"].dtype == np.float32 and (not two or c["p2"].dtype == np.float32)
    ref = sc.cached_reference(orc32, c)
    # the grid
    assert tuple(ref["dims"]) == c["dims"], (ref["dims"], c["dims"])
    # the populations, recomputed from the float32 positions
    if c["box"] is not None:
        assert np.array_equal(pc.binned(c["p1"], c["box"], c["dims"]), c["pops1"])
        assert not two or np.array_equal(pc.binned(c["p2"], c["box"], c["dims"]), c["pops2"])
    else:          # Grid::populate in float32 (cases module); no atom falls outside the padded bounding box
        assert int(c["pops1"].sum()) == len(c["p1"]) and (not two or int(c["pops2"].sum()) == len(c["p2"]))
        fullest = int((c["pops2"] if two else c["pops1"]).max())
        print(name, "fullest second cell", fullest, "chunks", (fullest + 63) // 64, "above 320" if fullest > 320 else "at most 320")
    # the plan: the shared 14-mask walk gives the oracle's plan and plan_slots' slot count
    n1, n2 = _valid_entries(c)
    assert _oracle_plan_len(c) == ref["plan_len"], (_oracle_plan_len(c), ref["plan_len"])
    assert int(((n1 + 63) // 64).sum()) == s64.plan_slots(c["pops1"], c["pops2"], c["dims"], c["pbc"])
    # the family, by all cells (the first search of a shape on a context) and by occupied cells (every later one)
    nc = pc.ncells(c["dims"])
    na, nb = len(c["p1"]), len(c["p2"]) if two else 0
    oa, ob = int(np.count_nonzero(c["pops1"])), int(np.count_nonzero(c["pops2"])) if two else 0
    fam = (sc.pair_family(c["kind"], na, nb, nc, nc), sc.pair_family(c["kind"], na, nb, sc.judged_cells(nc, oa), sc.judged_cells(nc, ob)))
    assert fam == c["family"] == c["intended"], (fam, c["family"], c["intended"])
    if c["covers"]:
        assert fam[0] == fam[1], "a table frame must be judged alike by all cells and by occupied cells"
    # the live-row plan: the regular family of the fixed-cutoff kinds, but for the frame built to fall outside it
    want_live = tuple(c["kind"] in sc.FIXED and f == 0 and "notlive" not in name for f in fam)
    assert c["live"] == want_live, (c["live"], want_live)
    if "notlive" in name:
        assert sc.plan_entry_count(nc, c["kind"]) > 8192 and na < 96 * nc and fam == (0, 0)
    # the result
    assert 0 < len(ref["i"]) <= sc.MAX_PAIRS, len(ref["i"])
    if c["declined"]:          # mfma_bound_usable: E >= 2^-22 is never below 0.02 cutoff^2
        assert np.float32(c["cutoff"]) ** 2 < 2.0 ** -22 / 0.02


def test_without_a_box_the_fullest_second_cell_is_on_the_intended_side_of_320():
    """The grid comes from the padded bounding box; what is pinned is the fullest second cell's chunk count and its side of 320
    (octant cases: every population)."""
    want = {"small16-single": (2, 2), "small16-double": (3, 3), "small32": (2, 2), "regular-within": (6, 6), "regular": (10, 10),
            "wide-single-nobox": (10, 10), "wide-double-nobox": (10, 10), "huge-single-nobox": (19, 19), "huge-double-nobox": (19, 19),
            "wide-vdw": (12, 12), "wide-within": (14, 14), "huge-vdw": (22, 22), "huge-within": (21, 21)}
    seen = 0
    for name, c in CASES.items():
        if c["box"] is not None:
            continue
        seen += 1
        fullest = int((c["pops1"] if c["p2"] is None else c["pops2"]).max())
        lo, hi = next(v for k, v in want.items() if name.startswith(k))
        assert lo <= (fullest + 63) // 64 <= hi, (name, fullest)
        assert (fullest > 320) == (lo > 5), (name, fullest)
    assert seen == 16


def test_thresholds_change_the_family_by_one_atom():
    for mean, dims, _, _, fams in sc.THRESHOLDS:
        for kind in sc.FIXED:
            at, above = CASES[f"threshold-{mean}-{kind}"], CASES[f"threshold-{mean}+1-{kind}"]
            nc = pc.ncells(dims)
            assert len(at["p1"]) == mean * nc and len(above["p1"]) == mean * nc + 1
            assert np.count_nonzero(at["pops1"]) == nc
            assert at["family"] == (fams[0], fams[0]) and above["family"] == (fams[1], fams[1]) and fams[0] != fams[1]


def test_every_instance_is_reached():
    """(family, kind, entry class, instance) over all table frames == REQUIRED"""
    got = set()
    for c in CASES.values():
        if c["covers"]:
            got |= sc.reached(c)
    missing, extra = sorted(sc.REQUIRED - got, key=str), sorted(got - sc.REQUIRED, key=str)
    assert not missing and not extra, f"not reached: {missing}; reached but not in the table: {extra}"
    # what the table must hold at the least, spelled out once more
    for kind in sc.FIXED:
        for n in range(1, 9):
            assert (0, kind, "plain", f"2nd:k{n}") in sc.REQUIRED
        for n in range(9, 17):
            assert (-1, kind, "plain", f"2nd:k{n}") in sc.REQUIRED
        for size in (16, 20, 24, 28, 32):
            assert (-2, kind, "plain", f"2nd:r{size}:lo") in sc.REQUIRED and (-2, kind, "plain", f"2nd:r{size}:hi") in sc.REQUIRED
        for fam in (0, -1, -2):
            assert (fam, kind, "plain", "2nd:stream") in sc.REQUIRED
        for n in (1, 63, 64, 65, 512, 513):
            assert (0, kind, "plain", f"1st:r{n}") in sc.REQUIRED
        for lanes in (16, 32):
            for n in (15, 16, 17, 31, 32, 33, 63, 64, 65):
                assert (lanes, kind, "plain", f"1st:r{n}") in sc.REQUIRED and (lanes, kind, "plain", f"2nd:c{n}") in sc.REQUIRED
        for n in range(1, 6):
            assert (0, kind, "plain", f"2nd:k{n}/declined") in sc.REQUIRED


@pytest.mark.parametrize("fam", [16, 32, 0, -1, -2])
def test_every_value_of_the_table_is_a_first_and_a_second_cell(fam):
    """... of every entry class of VALUE_CLASSES, in the frames of one and of two sets taken together; and cells next to each
    other hold different values"""
    seen = set()
    differing = 0
    for c in CASES.values():
        if not (c["covers"] and c["kind"] in sc.FIXED and c["family"] == (fam, fam)) or c["declined"]:
            continue
        for cls, n1, n2 in sc.plan_entries(c):
            seen.add((cls, "first", n1))
            seen.add((cls, "second", n2))
            differing += cls != "tri" and n1 != n2
    missing = [(cls, side, v) for cls in sc.VALUE_CLASSES[fam] for v in sc.TABLES[fam] for side in ("first", "second")
               if v >= (2 if cls == "tri" else 1) and (cls, side, v) not in seen]
    assert not missing, missing
    assert differing > 100
    if 0 in sc.TABLES[fam]:          # an empty cell among the crowded ones
        assert any(c["covers"] and c["family"] == (fam, fam) and (np.asarray(c["pops1"]) == 0).any() for c in CASES.values())
