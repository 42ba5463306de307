"""The inputs of tests/test_gpu_search_f64_instances.py against the f64 oracle alone (no GPU): the lattice builder gives the
occupancies it promises, plan_slots counts the plan the reference builds, the planted pairs reach every wrap mask, and the
randomised generator of tools/fuzz_search_f64.py covers what its slice in the suite requires of it."""
import importlib.util
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import search_f64_cases as sc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("K", [63, 64, 65, 128, 129, 192, 193, 256, 257, 320])
def test_lattice_occupancy_is_exact_in_a_sheared_box(orc64, K):
    """A box with negative off-diagonal terms: get_lab_extents (the row sums) gives 3 x 3 x 4 cells, not 4 x 4 x 4."""
    pos = sc.lattice(sc.BOX_334, (3, 3, 4), K, seed=K)
    ref = orc64.search_single_pbc(1.0, pos, orc64.box_from_matrix(sc.BOX_334), 7, nthreads=16)
    assert ref["dims"] == (3, 3, 4)
    occ = sc.occupancy_box(pos, sc.BOX_334, ref["dims"])
    assert (occ == K).all()
    assert len(ref["i"]) > 100_000
    # every one of the 36 * 14 entries is non-empty: ceil(K / 64) slots each
    assert ref["plan_len"] == 36 * 14
    assert sc.plan_slots(occ, None, ref["dims"], 7) == 36 * 14 * ((K + 63) // 64)


def _plan_slots_by_loops(occ1, occ2, dims, pbc):
    """plan_slots, cell by cell."""
    dx, dy, dz = dims
    total = 0
    for x in range(dx):
        for y in range(dy):
            for z in range(dz):
                for m in sc.MASKS:
                    cells = []
                    for off in (m[:3], m[3:]):
                        c = [x + off[0], y + off[1], z + off[2]]
                        for d in range(3):
                            if c[d] == dims[d]:
                                c[d] = 0 if (pbc >> d) & 1 else None
                        cells.append(None if None in c else c[0] + dx * (c[1] + dy * c[2]))
                    if None in cells:
                        continue
                    orders = [(cells[0], cells[1])] if occ2 is None else [(cells[0], cells[1]), (cells[1], cells[0])]
                    for ca, cb in orders:
                        n1, n2 = occ1[ca], (occ1 if occ2 is None else occ2)[cb]
                        if n1 and n2:
                            total += (n1 + 63) // 64
    return total


@pytest.mark.parametrize("dims", [(4, 5, 6), (3, 2, 3), (1, 2, 7)])
@pytest.mark.parametrize("pbc", [0, 1, 3, 5, 6, 7])
def test_plan_slots_equals_the_plan_walked_cell_by_cell(dims, pbc):
    rng = np.random.default_rng(sum(dims) + pbc)
    n = int(np.prod(dims))
    occ1 = rng.choice([0, 0, 1, 63, 64, 65, 128, 129, 300], n)
    occ2 = rng.choice([0, 0, 1, 64, 257], n)
    assert sc.plan_slots(occ1, None, dims, pbc) == _plan_slots_by_loops(occ1, None, dims, pbc)
    assert sc.plan_slots(occ1, occ2, dims, pbc) == _plan_slots_by_loops(occ1, occ2, dims, pbc)


def test_plan_slots_of_the_large_launch(orc64):
    """400 000 atoms give a plan of more than 2^20 slots (a 2-D launch), 200 000 do not.  With at most 64 atoms in every cell a
    slot is an entry with two non-empty cells, which is what the oracle reports as the length of its plan."""
    for n, above in ((400_000, True), (200_000, False)):
        box, rc, pos = sc.many_slots_case(n)
        ref = orc64.search_single_pbc(rc, pos, orc64.box_from_matrix(box), 7, nthreads=16)
        occ = sc.occupancy_box(pos, box, ref["dims"])
        assert occ.sum() == n and occ.max() <= 64
        slots = sc.plan_slots(occ, None, ref["dims"], 7)
        assert slots == ref["plan_len"]
        assert (slots > 2 ** 20) == above, (n, slots)
        assert len(ref["i"]) > 1_000_000


@pytest.mark.parametrize("pbc", [7, 3, 5, 0])
def test_plan_slots_equals_the_oracles_plan_under_partial_periodicity(orc64, pbc):
    pos = sc.lattice(sc.BOX_4, (4, 4, 4), 40, seed=3)
    ref = orc64.search_single_pbc(1.0, pos, orc64.box_from_matrix(sc.BOX_4), pbc, nthreads=16) if pbc \
        else orc64.search_single(1.0, pos, nthreads=16)
    if pbc:
        occ = sc.occupancy_box(pos, sc.BOX_4, ref["dims"])
    else:
        lower, upper = sc.bounding_box(1.0, pos)
        assert sc.dims_of(lower, upper, 1.0) == ref["dims"]
        occ = sc.occupancy_no_box(pos, lower, upper, ref["dims"])
    assert occ.sum() == len(pos) and occ.max() <= 64
    assert sc.plan_slots(occ, None, ref["dims"], pbc) == ref["plan_len"]


def test_planted_pairs_reach_every_wrap_mask(orc64):
    box, rc, pos = sc.wrap_masks_case()
    ref = orc64.search_single_pbc(rc, pos, orc64.box_from_matrix(box), 7, nthreads=16)
    assert ref["dims"] == (10, 10, 10)
    per_mask = sc.near_cutoff_hits_per_mask(pos, box, rc, ref)
    # 1500 pairs planted per mask, about half of them inside the cutoff
    assert (per_mask[1:] >= 500).all() and (per_mask[1:] <= 1000).all(), per_mask
    assert len(ref["i"]) < 2e7


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("situation", sc.SITUATIONS)
@pytest.mark.parametrize("K2", [1, 65, 257])
def test_sweep_cases_reach_the_instance_they_are_named_after(orc64, K2, kind, situation):
    c = sc.sweep_case(K2, kind, situation)
    ref = sc.sweep_reference(orc64, c)
    slots = sc.sweep_check_inputs(c, ref)
    assert slots > 0
    if c["pbc"] == 7:
        ncells = int(np.prod(c["dims"]))
        assert slots == ncells * 14 * (2 if c["p2"] is not None else 1) * ((c["K1"] + 63) // 64)


class _OracleEngine:
    """Stands in for the engine: answers a request of the fuzzer with the oracle's own result, so that what is tested is the
    generator (which cases it makes, that the oracle accepts them, that request and reference describe the same search)."""
    host_only = True

    def __init__(self, orc):
        self.o = orc

    def search_f64(self, kind, cutoff, xyz1, idx1=None, xyz2=None, idx2=None, box=None, pbc=0, vdw1=None, vdw2=None,
                   ids_local=False, lower=None, upper=None):
        o = self.o
        ob = o.box_from_matrix(box) if box is not None else None
        p1 = xyz1 if idx1 is None else xyz1[idx1.astype(int)]
        p2 = None if xyz2 is None else (xyz2 if idx2 is None else xyz2[idx2.astype(int)])
        i1, i2 = (None, None) if ids_local else (idx1, idx2)
        if kind == 0:
            r = o.search_single_pbc(cutoff, p1, ob, pbc, ids=i1, nthreads=4) if pbc else o.search_single(cutoff, p1, ids=i1, nthreads=4)
        elif kind == 1:
            r = o.search_double_pbc(cutoff, p1, p2, ob, pbc, i1, i2, nthreads=4) if pbc else o.search_double(cutoff, p1, p2, i1, i2, nthreads=4)
        elif kind == 3:
            r = o.search_double_vdw_pbc(p1, p2, vdw1, vdw2, ob, pbc, nthreads=4) if pbc else o.search_double_vdw(p1, p2, vdw1, vdw2, nthreads=4)
        else:
            r = o.search_within_pbc(cutoff, p1, p2, ob, pbc, i1, i2, nthreads=4) if pbc \
                else o.search_within(cutoff, p1, p2, lower, upper, i1, i2, nthreads=4)
            return r["i"]
        return r["i"], r["j"], r["d"]


def fuzzer():
    spec = importlib.util.spec_from_file_location("fuzz_search_f64", os.path.join(ROOT, "tools", "fuzz_search_f64.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("seed", [11, 12])
def test_fuzzer_slice_skips_little_and_covers_the_classified_entries(orc64, seed):
    """What test_randomised_differential_f64 requires of a 250-case slice, with the oracle on both sides."""
    stats = fuzzer().run(250, seed, eng=_OracleEngine(orc64), verbose=False)
    assert stats["fails"] == 0
    assert stats["skipped"] <= 250 * 5 // 100
    assert stats["full_pbc_4cells"] >= 15
    assert stats["cells_above_256"] >= 5 and stats["empty"] >= 5
