"""Inputs that pin every compiled instance of the f32 pair search at its cell-occupancy edges.  Numpy only; nothing here touches
the code under test.  tests/test_search_f32_cases_cpu.py proves the cases on the oracle alone, tests/test_gpu_search_f32_instances.py
runs them on the GPU.

The search picks a kernel from the frame's shape and an instance from every plan entry's two cells:

  search_shape.hpp   small_cell_lanes / pair_family: 16 lanes per slot up to 13 atoms per judged cell, 32 up to 19 (pair_small.hip),
                     the regular kernels above, the wide instances above 448 per judged cell of the second set, the huge ones
                     above 1000; judged_cells: all cells on the first search of a shape, the occupied ones after it;
                     live_row_slots: slots cut from live rows for the regular family on plans of at most 8192 entries or frames of
                     at least 96 atoms per cell.
  pair_kernels.hpp   run_task_nch: one register instance per chunk count (64 atoms) of the second cell, 1 .. KREG = 8, the
                     streaming loop above; KMAX_WIDE = 16: instances 9 .. 16 of the wide family; KMAX_HUGE = 32: the chunk count
                     rounded up to 16 / 20 / 24 / 28 / 32, the padding filled with "never a hit" coordinates; MFMA_TILES = 10: the
                     matrix-core count for second cells of up to 320 atoms, declined (mfma_bound_usable) where the bound
                     2^-22 * (.. + 1) is not below 0.02 cutoff^2; decode_task: entries that wrap in all three dimensions of a
                     sheared box are cut into slots of 2 rows (first cells up to 1024 atoms) or 8 (up to 4096); vdW and `within`
                     check the chunk count at run time (run_task).
  pair_small.hip     G = 16 or 32 lanes per slot: rows in blocks of G, candidates in blocks of G, slots of up to 64 rows.
  search.hip         wrapped_pair_policy (search_shape.hpp): wrapped entries are classified by the distance to the adjacent image
                     inside a band where every periodic dimension has 4 cells or more, evaluated exactly below.

A case is a dict: name, kind, cutoff, p1 / p2 (float32; p2 None: one set), v1 / v2 (vdW radii), box (float32 3x3, columns = box
vectors; None: no box), pbc, pops1 / pops2 (atoms per cell, flat index x + y * dx + z * dx * dy), dims, family = (what
search_cell_kernels()[0] reports after the first search of the shape on a context, after every later one), live = the live-row
predicate for the same two, intended (the family the frame was built for), lower / upper (`within` without a box), declined (the
matrix-core count must decline every slot), covers (a table frame, counted for the instance table REQUIRED; frames without a box
- their grid is the padded bounding box's - and the threshold pairs are not).

The frames, family by family (all_cases):
  small16 / small32   (6, 6, 6) cells with pbc 7 (band) and pbc 3, the same atoms without a box, (3, 3, 8) cells (exact), a sheared box of
                      (4, 4, 5) cells with the table's edges planted in the eight cells of the corner entries
  regular             (4, 4, 4) with pbc 7 (live rows; also scaled by 2^-10: the matrix-core count declined) and pbc 5, the same atoms
                      without a box, (9, 9, 8) (more than 8192 entries, 30 atoms per cell: consecutive slots), (3, 3, 3) and (3, 2, 4)
                      (exact, duplicate cell pairs), the sheared (4, 4, 5) box; vdW and `within` on the same frames
  wide / huge         (4, 4, 1) with pbc 3 / (4, 2, 1) with pbc 1 (band), (3, 2, 1) with pbc 3 (exact), a sheared box of (2, 2, 2) cells whose
                      eight cells are those of the corner entries (2 rows per slot up to 1024 atoms, 8 above), eight octants without a
                      box (huge: four of them occupied - wide on the first search of the shape, huge after it); vdW and `within` on
                      the same occupancies
  threshold           N = 13, 19, 448, 1000 atoms per cell exactly and one atom more
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pinned_cells as pc  # noqa: E402
import search_f64_cases as s64  # noqa: E402

F32_EPS = np.float32(1.1920929e-07)
CUTOFF = 0.5
MAX_PAIRS = 15_000_000          # the oracle's list of any one case

KREG, KMAX_WIDE, KMAX_HUGE, MFMA_TILES = 8, 16, 32, 10          # pair_kernels.hpp
LIVE_MAX_ENTRIES, FPLAN_MAX_TASKS, LIVE_MEAN = 8192, 1 << 22, 96          # search_shape.hpp
FIXED = ("single", "double")
KINDS = ("single", "double", "vdw", "within")

# ---------------------------------------------------------------- search_shape.hpp, restated


def judged_cells(ncells, occupied):
    return min(occupied, ncells) if occupied else ncells


def small_cell_lanes(kind, n1, n2, cells1, cells2):
    if kind not in FIXED:
        return 0
    lanes = 16
    for n, cells in ((n1, cells1), (n2, cells2))[: 1 if kind == "single" else 2]:
        one = 16 if n <= 13 * cells else (32 if n <= 19 * cells else 0)
        lanes = 0 if (one == 0 or lanes == 0) else max(lanes, one)
    return lanes


def pair_family(kind, n1, n2, cells1, cells2):
    lanes = small_cell_lanes(kind, n1, n2, cells1, cells2)
    if lanes:
        return lanes
    if kind not in FIXED:
        return 0
    n, cells = (n1, cells1) if kind == "single" else (n2, cells2)
    return -2 if n > 1000 * cells else (-1 if n > 448 * cells else 0)


def plan_entry_count(ncells, kind):
    return ncells * 14 * (1 if kind == "single" else 2)


def live_row_slots(kind, family, n1, ncells):
    entries = plan_entry_count(ncells, kind)
    return kind in FIXED and family == 0 and entries + 1 <= FPLAN_MAX_TASKS and (entries <= LIVE_MAX_ENTRIES or n1 >= LIVE_MEAN * ncells)


def families_of(kind, pops1, pops2):
    """(family, live) judged by all cells (the first search of a shape on a context) and by the occupied ones (every later one)"""
    nc = len(pops1)
    n1 = int(np.sum(pops1))
    n2 = int(np.sum(pops2)) if pops2 is not None else 0
    o1 = int(np.count_nonzero(pops1))
    o2 = int(np.count_nonzero(pops2)) if pops2 is not None else 0
    fam = (pair_family(kind, n1, n2, nc, nc), pair_family(kind, n1, n2, judged_cells(nc, o1), judged_cells(nc, o2)))
    return fam, tuple(live_row_slots(kind, f, n1, nc) for f in fam)


def approx_wrapped(box, pbc, dims, cutoff, n1, n2):
    """wrapped_pair_policy: are wrapped entries classified by the band (True) or evaluated exactly (False)?"""
    if box is None:
        return False
    m = np.asarray(box, np.float64)              # m[d, k]: component d of box vector k
    ok = n1 + n2 < (1 << 26)
    for d in range(3):
        if (pbc >> d) & 1 and dims[d] < 4:
            ok = False
    lmax = max(np.abs(m.sum(1)).max(), np.abs(m).max(), np.abs(m).sum(1).max())
    kappa = (np.abs(m) @ np.abs(np.linalg.inv(m))).sum(1).max()
    u = 5.9604645e-8
    e = (4.0 * kappa + 9.0) * u * lmax
    rel = 2.0e-4 + 4.0 * 2.0 * 1.7320508 * e / cutoff
    margin = 1.0e-3 + 4.0 * 1.7320508 * e
    if not margin < 0.05 * cutoff or not np.isfinite(kappa):
        ok = False
    return bool(ok and rel < 0.05)


def sheared(box):
    """PeriodicBox::from_matrix keeps lattice shifts for every box that is not diagonal"""
    return box is not None and bool(np.any(np.asarray(box)[~np.eye(3, dtype=bool)] != 0.0))


# ---------------------------------------------------------------- plan entries and the instances they run

CLASSES = ("tri", "plain", "band", "exact", "corner2", "corner8")


def plan_entries(c):
    """Every plan entry of a case with both cells non-empty (a same-cell entry: at least two atoms), as (class, rows of the first
    cell, atoms of the second cell).  Classes: tri (the same cell of one set), plain, band / exact (wrapped, classified by the
    band or evaluated exactly), corner2 / corner8 (wrapped in all three dimensions of a sheared box: 2 or 8 rows per slot)."""
    two = c["kind"] != "single"
    pops1 = np.asarray(c["pops1"], np.int64)
    pops2 = np.asarray(c["pops2"], np.int64) if two else pops1
    ca, cb, wrap = s64.plan_cell_pairs(c["dims"], c["pbc"] if c["box"] is not None else 0, two)
    n1, n2 = pops1[ca], pops2[cb]
    tri = (ca == cb) & (not two)
    keep = (n1 > 0) & (n2 > 0) & ~(tri & (n1 < 2))
    approx = approx_wrapped(c["box"], c["pbc"], c["dims"], c["cutoff"], int(pops1.sum()), int(pops2.sum()) if two else 0)
    shear = sheared(c["box"])
    out = []
    for a, b, w, t in zip(n1[keep], n2[keep], wrap[keep], tri[keep]):
        if w == 0:
            cls = "tri" if t else "plain"
        else:
            assert not t, "a cell next to itself round the boundary: one periodic cell in a dimension"
            if w == 7 and shear and a <= 4096:
                cls = "corner2" if a <= 1024 else "corner8"
                assert cls in CLASSES
            else:
                cls = "band" if approx else "exact"
        out.append((cls, int(a), int(b)))
    return out


SMALL_EDGES = (15, 16, 17, 31, 32, 33, 63, 64, 65)
ROW_EDGES = (1, 63, 64, 65, 512, 513)


def second_instance(family, kind, n2, declined=False):
    """the instance run_task_nch (or small_pair_kernel) picks for a second cell of n2 atoms"""
    nch = (n2 + 63) // 64
    if kind not in FIXED:
        return f"loop{nch}" if nch <= KREG else "stream"          # run_task<.., KREG, true>: the chunk count at run time
    if family in (16, 32):
        return f"c{n2}" if n2 in SMALL_EDGES else "other"
    if nch <= KREG:
        mfma = n2 <= 32 * MFMA_TILES
        assert mfma == (nch <= 5)
        return f"k{nch}" + ("/declined" if declined and mfma else "")
    if family == 0:
        return "stream"
    if family == -1:
        return f"k{nch}" if nch <= KMAX_WIDE else "stream"
    if nch > KMAX_HUGE:
        return "stream"
    size = next(s for s in (16, 20, 24, 28, 32) if nch <= s)
    lowest = KREG + 1 if size == 16 else size - 3
    return f"r{size}:" + ("lo" if nch == lowest else ("hi" if nch == size else "mid"))


def first_instance(family, kind, n1):
    if family in (16, 32) and kind in FIXED:
        return f"r{n1}" if n1 in SMALL_EDGES else "other"
    return f"r{n1}" if n1 in ROW_EDGES else "other"


def reached(c):
    """the (family, kind, entry class, instance) tuples of a case: `2nd:` instances by the second cell, `1st:` by the first"""
    out = set()
    for fam in set(c["family"]):
        for cls, n1, n2 in plan_entries(c):
            off = c["declined"] and cls in ("tri", "plain")          # (wrapped entries of the scaled cases are all exact)
            out.add((fam, c["kind"], cls, "2nd:" + second_instance(fam, c["kind"], n2, off)))
            out.add((fam, c["kind"], cls, "1st:" + first_instance(fam, c["kind"], n1)))
    return out


# ---------------------------------------------------------------- the occupancy tables

SMALL_TABLE = (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 66, 129)
REGULAR_TABLE = (0, 1, 63, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 448, 449, 512, 513, 600)
WIDE_TABLE = (64, 320, 321, 512, 513, 576, 577, 640, 641, 704, 705, 768, 769, 832, 833, 896, 897, 960, 961, 1023, 1024, 1025, 1100)
HUGE_TABLE = (64, 512, 513, 1024, 1025, 1280, 1281, 1536, 1537, 1792, 1793, 2047, 2048, 2049, 2200)
TABLES = {16: SMALL_TABLE, 32: SMALL_TABLE, 0: REGULAR_TABLE, -1: WIDE_TABLE, -2: HUGE_TABLE}

# classes in which EVERY value of a family's table must occur as a first and as a second cell (in a frame of one set or of two);
# the wrapped classes of the large families - a handful of entries per frame - and the corner entries - four per frame - are
# held to every INSTANCE instead (REQUIRED)
VALUE_CLASSES = {16: ("tri", "plain", "band"), 32: ("tri", "plain", "band"), 0: ("tri", "plain", "band", "exact"),
                 -1: ("tri", "plain"), -2: ("tri", "plain")}


def _required():
    """The instance table: every (family, kind, entry class, instance) the table frames must reach - and they reach nothing else."""
    req = set()

    def add(fam, kinds, classes, seconds, firsts):
        for kind in kinds:
            for cls in classes:
                if cls == "tri" and kind != "single":
                    continue
                req.update((fam, kind, cls, "2nd:" + s) for s in seconds)
                req.update((fam, kind, cls, "1st:" + f) for f in firsts if not (cls == "tri" and f == "r1"))
    # small cells: rows and candidates on either side of 16, 32 and 64
    edge_c = [f"c{n}" for n in SMALL_EDGES] + ["other"]
    edge_r = [f"r{n}" for n in SMALL_EDGES] + ["other"]
    for lanes in (16, 32):
        add(lanes, FIXED, ("tri", "plain", "band", "exact", "corner2"), edge_c, edge_r)
    # regular: chunk counts 1 .. 8 and the streaming loop; first cells of 1, 63, 64, 65, 512, 513 rows
    rows = [f"r{n}" for n in ROW_EDGES] + ["other"]
    reg = [f"k{n}" for n in range(1, KREG + 1)] + ["stream"]
    add(0, FIXED, ("tri", "plain", "band", "exact", "corner2"), reg, rows)
    # ... with the matrix-core count declined: the vector count instances of 1 .. 5 chunks (plain and same-cell entries)
    add(0, FIXED, ("tri", "plain"), [f"k{n}/declined" for n in range(1, 6)], [])
    # vdW and `within`: the run-time chunk loop and the streaming loop, on regular, wide and huge occupancies
    loops = [f"loop{n}" for n in range(1, KREG + 1)] + ["stream"]
    add(0, ("vdw", "within"), ("plain", "band", "exact", "corner2"), loops, rows)
    add(0, ("vdw", "within"), ("corner8",), ["loop8", "stream"], ["other"])
    # wide: what the table reaches of 1 .. 8 (64, 320, 321, 512 atoms), every instance 9 .. 16, the streaming loop
    wide = ["k1", "k5", "k6", "k8"] + [f"k{n}" for n in range(KREG + 1, KMAX_WIDE + 1)] + ["stream"]
    large_rows = ["r64", "r512", "r513", "other"]
    add(-1, FIXED, ("tri", "plain", "band", "exact", "corner2"), wide, large_rows)
    # huge: every rounded size from its lowest and its highest chunk count, the streaming loop
    huge = ["k1", "k8"] + [f"r{s}:{e}" for s in (16, 20, 24, 28, 32) for e in ("lo", "hi")] + ["stream"]
    add(-2, FIXED, ("tri", "plain", "band", "exact", "corner2"), huge, large_rows)
    add(-2, FIXED, ("corner8",), huge, ["other"])
    return req


REQUIRED = _required()

# ---------------------------------------------------------------- frames


def _case(name, kind, box, pbc, dims, pops1, pops2, rng, intended, cutoff=CUTOFF, covers=True):
    two = kind != "single"
    pops1 = np.asarray(pops1, np.int64)
    pops2 = np.asarray(pops2, np.int64) if two else None
    p1 = pc.frame(box, dims, pops1, rng)[0]
    p2 = pc.frame(box, dims, pops2, rng)[0] if two else None
    c = {"name": name, "kind": kind, "cutoff": float(cutoff), "p1": p1, "p2": p2, "v1": None, "v2": None, "box": box, "pbc": pbc,
         "pops1": pops1, "pops2": pops2, "dims": tuple(int(d) for d in dims), "lower": None, "upper": None, "declined": False,
         "covers": covers, "intended": intended}
    if kind == "vdw":
        _radii(c, rng)
    c["family"], c["live"] = families_of(kind, pops1, pops2)
    return c


def _radii(c, rng):
    """pair cutoffs 0.6 .. 1.0 of the grid's; the largest radius of each set is half of it: the grid of the other kinds"""
    half = np.float32(0.5 * c["cutoff"])
    for k, p in (("v1", c["p1"]), ("v2", c["p2"])):
        v = rng.uniform(0.3 * c["cutoff"], 0.5 * c["cutoff"], len(p)).astype(np.float32)
        v[len(p) // 2] = half
        c[k] = np.minimum(v, half)
    c["cutoff"] = float((half + half) + F32_EPS)


def without_box(c, intended=None):
    """The same atoms searched without a box: the grid comes from the zero-seeded bounding box padded by the cutoff (`within`: from
    the caller's bounds, the first set's extremes padded, selection/ast.rs:597-602), the cells and their populations from
    Grid::populate - every operation in float32, as the engine and the oracle perform it.  Not counted for the instance table."""
    c = dict(c)
    rc = np.float32(c["cutoff"])
    sets = [c["p1"]] + ([c["p2"]] if c["p2"] is not None else [])
    if c["kind"] == "within":
        lo = c["p1"].min(0) + (np.float32(-rc) - F32_EPS)
        up = c["p1"].max(0) + (rc + F32_EPS)
    else:
        lo = np.minimum(np.float32(0.0), np.min([p.min(0) for p in sets], 0)) + (np.float32(-rc) - F32_EPS)
        up = np.maximum(np.float32(0.0), np.max([p.max(0) for p in sets], 0)) + (rc + F32_EPS)
    lo, up = lo.astype(np.float32), up.astype(np.float32)
    ext = (up - lo).astype(np.float32)
    dims = tuple(int(max(np.floor(np.float32(e) / rc), 1)) for e in ext)
    fd = np.asarray(dims, np.float32)

    def pops(p):
        f = np.floor((fd * (p - lo).astype(np.float32)).astype(np.float32) / ext).astype(np.int64)
        ok = ((f >= 0) & (f < np.asarray(dims))).all(1)
        f = f[ok]
        return np.bincount(f[:, 0] + dims[0] * (f[:, 1] + dims[1] * f[:, 2]), minlength=pc.ncells(dims))
    c.update(name=c["name"] + "-nobox", box=None, pbc=0, dims=dims, pops1=pops(c["p1"]), pops2=pops(c["p2"]) if c["p2"] is not None else None,
             covers=False)
    if c["kind"] == "within":
        c["lower"], c["upper"] = lo, up
    c["family"], c["live"] = families_of(c["kind"], c["pops1"], c["pops2"])
    c["intended"] = c["family"] if intended is None else intended
    return c


def octant_case(name, kind, pops1, pops2, rng, intended, cutoff=CUTOFF):
    """No box, few cells: every coordinate in [0, 0.9] cutoffs, one atom at 0.9 in all three, so that the zero-seeded bounding
    box padded by the cutoff is 2.9 cutoffs wide: (2, 2, 2) cells that meet at 0.45.  Octant o = x + 2 y + 4 z holds pops[o]
    atoms, in 0.03 .. 0.40 or 0.50 .. 0.88 along each axis: the populations are exact, the fullest second cell's chunk count
    and its side of 320 with them.  All cells are judged on the first search of the shape, the occupied ones from then on."""
    def atoms(pops, corner):
        cell = np.repeat(np.arange(8), pops)
        bits = np.stack([cell & 1, (cell >> 1) & 1, (cell >> 2) & 1], -1)
        u = rng.random((len(cell), 3))
        pos = np.where(bits == 1, 0.50 + 0.38 * u, 0.03 + 0.37 * u)
        if corner:
            pos[-1] = 0.9
        return (pos[rng.permutation(len(pos))] * cutoff).astype(np.float32)
    assert pops1[7] > 0
    two = kind != "single"
    c = {"name": name, "kind": kind, "cutoff": float(cutoff), "p1": atoms(pops1, True), "p2": atoms(pops2, False) if two else None, "v1": None,
         "v2": None, "box": None, "pbc": 0, "lower": None, "upper": None, "declined": False}
    c = without_box(c, intended)
    assert c["dims"] == (2, 2, 2) and np.array_equal(c["pops1"], pops1) and (not two or np.array_equal(c["pops2"], pops2)), name
    return c


def declined(c):
    """The whole case scaled by 2^-10 (exact in float32: every distance and every comparison scales with it).  cutoff^2 is then
    below 2^-22 / 0.02, so mfma_bound_usable - E >= 2^-22 against 0.02 cutoff^2 - is false for every slot.  (The wrap policy's
    margin of 0.001 is absolute: at this scale every wrapped entry is evaluated exactly.)"""
    s = np.float32(2.0 ** -10)
    c = dict(c)
    c.update(name=c["name"] + "-declined", p1=c["p1"] * s, p2=None if c["p2"] is None else c["p2"] * s, box=c["box"] * s,
             cutoff=float(np.float32(c["cutoff"]) * s), declined=True)
    return c


def _rng(*key):
    return np.random.default_rng([7] + [int(k) + 1000 for k in key])


def _corner_plants(kind, dims, first_a, second_a, first_b=None, second_b=None):
    """{cell: population} for the two sets.  One set: the four corner entries' first cells hold first_a, their second cells
    second_a.  Two sets: every entry runs as (c1, c2) and as (c2, c1), rows from set 1 and candidates from set 2 - the first
    order pairs first_a with second_a, the second one first_b with second_b."""
    fc, sc = pc.corner_cells(dims)
    if kind == "single":
        one = {**dict(zip(sc, second_a)), **dict(zip(fc, first_a))}
        return one, one
    first_b = first_a if first_b is None else first_b
    second_b = second_a if second_b is None else second_b
    return {**dict(zip(fc, first_a)), **dict(zip(sc, first_b))}, {**dict(zip(sc, second_a)), **dict(zip(fc, second_b))}


def _take(table, part, parts):
    return tuple(table)[part::parts]


# sheared boxes: (lab extents in cutoffs, cells)
TRIC_445 = ((4.1, 4.1, 5.1), (4, 4, 5))
TRIC_222 = ((2.9, 2.9, 2.9), (2, 2, 2))

# corner plants: (first cells, second cells) of the four entries that wrap in all three dimensions, frame by frame
SMALL_CORNERS = (((15, 16, 17, 31), (32, 33, 63, 64)), ((32, 33, 63, 64), (65, 15, 16, 17)), ((65, 66, 129, 2), (31, 47, 1, 129)))
REGULAR_CORNERS = (((1, 63, 64, 65), (64, 128, 192, 256)), ((512, 513, 600, 129), (320, 384, 448, 512)), ((65, 1, 64, 63), (513, 600, 1, 65)))


def small_cases(lanes):
    """16 lanes: at most 13 atoms per judged cell, 32 lanes: at most 19 - crowded cells of the table in a sparse background."""
    out = []
    bg = {16: (3, 9), 32: (12, 17)}[lanes]
    bg_few = {16: (2, 6), 32: (10, 13)}[lanes]
    both = (lanes, lanes)
    for kind in FIXED:
        ki = FIXED.index(kind)
        for seed in range(3):                                   # (6, 6, 6) cells, every wrapped entry classified by the band
            rng = _rng(lanes, ki, 1, seed)
            dims = (6, 6, 6)
            pops = [pc.plant(dims, SMALL_TABLE, bg, rng) for _ in range(2)]
            out.append(_case(f"small{lanes}-{kind}-ortho7-{seed}", kind, pc.ortho_box(dims), 7, dims, pops[0], pops[1], rng, both))
        rng = _rng(lanes, ki, 2)
        pops = [pc.plant((6, 6, 6), SMALL_TABLE, bg, rng) for _ in range(2)]
        part = _case(f"small{lanes}-{kind}-pbc3", kind, pc.ortho_box((6, 6, 6)), 3, (6, 6, 6), pops[0], pops[1], rng, both)
        out += [part, without_box(part)]
        for seed in range(5):                                   # periodic dimensions of 3 cells: every wrapped entry exact
            rng = _rng(lanes, ki, 3, seed)
            dims = (3, 3, 8)
            # (cell (0, 0, 0) is the second cell and (2, 0, 0) the first cell of an entry that wraps in x)
            pops = [pc.plant(dims, _take(SMALL_TABLE, (seed + k) % 3, 3), bg_few, rng,
                             {0: SMALL_EDGES[(2 * seed + k) % 9], 2: SMALL_EDGES[(2 * seed + k + 4) % 9]}) for k in range(2)]
            out.append(_case(f"small{lanes}-{kind}-exact-{seed}", kind, pc.ortho_box(dims), 7, dims, pops[0], pops[1], rng, both))
        for seed, (firsts, seconds) in enumerate(SMALL_CORNERS):          # a sheared box of (4, 4, 5) cells: corner entries
            rng = _rng(lanes, ki, 4, seed)
            rows, dims = TRIC_445
            values = [v for v in _take(SMALL_TABLE, seed, 3) if v < 129]
            plants = _corner_plants(kind, dims, firsts, seconds, SMALL_CORNERS[(seed + 1) % 3][0], SMALL_CORNERS[(seed + 1) % 3][1])
            pops = [pc.plant(dims, values, bg_few, rng, fx) for fx in plants]
            out.append(_case(f"small{lanes}-{kind}-tric-{seed}", kind, pc.sheared_box(rows), 7, dims, pops[0], pops[1], rng, both))
    return out


def regular_cases():
    out = []
    reg = (0, 0)
    for kind in KINDS:
        ki = KINDS.index(kind)
        fixed_kind = kind in FIXED
        for seed in range(3 if fixed_kind else 1):              # (4, 4, 4): a plan of at most 8192 entries - live rows
            rng = _rng(0, ki, 1, seed)
            dims = (4, 4, 4)
            pops = [pc.plant(dims, REGULAR_TABLE, (25, 40), rng) for _ in range(2)]
            c = _case(f"regular-{kind}-ortho7-{seed}", kind, pc.ortho_box(dims), 7, dims, pops[0], pops[1], rng, reg)
            out.append(c)
            if fixed_kind and seed < 2:
                out.append(declined(c))
        if fixed_kind:                                           # more than 8192 entries, below 96 atoms per cell: consecutive slots
            rng = _rng(0, ki, 2)
            dims = (9, 9, 8)
            pops = [pc.plant(dims, REGULAR_TABLE, (25, 35), rng) for _ in range(2)]
            out.append(_case(f"regular-{kind}-notlive", kind, pc.ortho_box(dims), 7, dims, pops[0], pops[1], rng, reg))
        for seed in range(2 if fixed_kind else 1):              # 3 and 2 cells per periodic dimension: exact, duplicate cell pairs
            rng = _rng(0, ki, 3, seed)
            dims = (3, 3, 3) if seed == 0 else (3, 2, 4)
            pops = [pc.plant(dims, REGULAR_TABLE, (25, 40), rng) for _ in range(2)]
            out.append(_case(f"regular-{kind}-exact-{seed}", kind, pc.ortho_box(dims), 7, dims, pops[0], pops[1], rng, reg))
        for seed, (firsts, seconds) in enumerate(REGULAR_CORNERS):          # a sheared box of (4, 4, 5) cells: corner entries
            rng = _rng(0, ki, 4, seed)
            rows, dims = TRIC_445
            values = _take(REGULAR_TABLE, seed, 3)
            plants = _corner_plants(kind, dims, firsts, seconds, REGULAR_CORNERS[(seed + 1) % 3][0], REGULAR_CORNERS[(seed + 1) % 3][1])
            pops = [pc.plant(dims, values, (25, 40), rng, fx) for fx in plants]
            out.append(_case(f"regular-{kind}-tric-{seed}", kind, pc.sheared_box(rows), 7, dims, pops[0], pops[1], rng, reg))
        rng = _rng(0, ki, 5)                                      # partial periodicity, and the same atoms without a box
        dims = (4, 4, 4)
        pops = [pc.plant(dims, REGULAR_TABLE, (25, 40), rng) for _ in range(2)]
        part = _case(f"regular-{kind}-pbc5", kind, pc.ortho_box(dims), 5, dims, pops[0], pops[1], rng, reg)
        out += [part, without_box(part, reg)]
    return out


# The wide and huge frames: few cells with long edges - one cell in a non-periodic dimension is up to 2 cutoffs long, two cells
# 1.5, four periodic cells (the band classification) 1.25.
WIDE_BAND = ((4, 4, 1), (1.02, 1.02, 1.9), 3)
HUGE_BAND = ((4, 2, 1), (1.24, 1.45, 1.9), 1)
LARGE_EXACT = ((3, 2, 1), (1.3, 1.45, 1.9), 3)

WIDE_SECONDS = ((64, 1025, 577, 833), (320, 1100, 641, 705), (321, 513, 769, 897), (512, 1024, 961, 576))
WIDE_FIRSTS = (64, 512, 513, 1000)
HUGE_SECONDS = ((64, 2048, 2200, 513), (512, 2049, 1793, 1024), (1025, 1280, 1281, 1536), (1537, 1792, 2047, 64))
HUGE_FIRSTS_2 = ((513, 1024, 1024, 1024), (512, 1024, 1024, 1024), (64, 1024, 1024, 1024), (1024, 1024, 1024, 1024))          # 2 rows per slot
HUGE_FIRSTS_8 = ((1025, 1537, 2049, 1281), (2200, 1280, 1025, 1793), (1536, 2048, 1281, 1792), (1537, 1025, 2047, 1793))     # 8 rows per slot
# Two sets: the list holds n1 * n2 * (share within the cutoff) pairs, twice what one set of the same size gives.  The family is
# judged by the SECOND set, which takes the table; the first set holds the row counts of the instance table in cells of a few
# hundred atoms, and for the slots of 8 rows as little above 1024 as will do.
LARGE_ROWS = (64, 512, 513, 100, 200, 300, 400, 150)


def _lift(values, fam, rng):
    """a frame's populations with its mean kept inside the family: the smallest values but one are replaced by values from the
    table's upper half until the mean is above the family's threshold; for the wide family the largest ones but one by 576
    until it is not above 1000"""
    values = [int(v) for v in values]
    low, high = (448, 1000) if fam == -1 else (1000, 1 << 30)
    upper = [v for v in TABLES[fam] if low < v]
    order = np.argsort(values)
    k = 1
    while not low * len(values) < sum(values) and k < len(values):
        values[order[k]] = int(rng.choice(upper[len(upper) // 2:]))
        k += 1
    order = np.argsort(values)[::-1]
    k = 1
    while sum(values) > high * len(values) and k < len(values):
        values[order[k]] = 576
        k += 1
    return np.asarray(values, np.int64)


def _huge_band_pops(frame, k, last, rng):
    """(4, 2, 1) cells, x periodic: the wrapped entries' second cells are (0, 0), (0, 1), (3, 1) - two sets: and (3, 0) - , their first
    cells (3, 0), (3, 1), (0, 0).  These four take the table three values at a time; the inner cells hold the largest values."""
    t = HUGE_TABLE
    pops = np.zeros(8, np.int64)
    vals = [t[(3 * frame + j + 7 * k) % len(t)] for j in range(3)] + [t[(3 * frame + last + 7 * k) % len(t)]]
    for (x, y), v in zip(((0, 0), (0, 1), (3, 1), (3, 0)), vals):
        pops[x + 4 * y] = v
    for (x, y), v in zip(((1, 0), (2, 0), (1, 1), (2, 1)), rng.permutation([2200, 2049, 1281, 1025])):
        pops[x + 4 * y] = v
    return pops


def _huge_band_rows(frame, rng):
    """the first set beside _huge_band_pops: 64, 512, 513 and 100 in turn in the four cells of the wrapped entries"""
    pops = np.zeros(8, np.int64)
    for (x, y), v in zip(((0, 0), (0, 1), (3, 1), (3, 0)), np.roll(LARGE_ROWS[:4], frame)):
        pops[x + 4 * y] = v
    for (x, y), v in zip(((1, 0), (2, 0), (1, 1), (2, 1)), rng.permutation(LARGE_ROWS[4:])):
        pops[x + 4 * y] = v
    return pops


def large_cases(fam):
    """the wide (-1) and huge (-2) families; vdW and `within` on the same occupancies"""
    out = []
    table = TABLES[fam]
    name = {-1: "wide", -2: "huge"}[fam]
    for kind in KINDS:
        ki = KINDS.index(kind)
        fixed_kind = kind in FIXED
        want = (fam, fam) if fixed_kind else (0, 0)
        # four periodic cells: wrapped entries classified by the band
        dims, edges, pbc = WIDE_BAND if fam == -1 else HUGE_BAND
        nc = pc.ncells(dims)
        for seed in range((4 if fam == -1 else 6) if fixed_kind else 1):
            rng = _rng(fam, ki, 1, seed)
            if fam == -1:
                pops = [rng.permutation(_lift(np.roll(table, -(seed * nc + 3 * k))[:nc], fam, rng)) for k in range(2)]
            else:
                pops = [_huge_band_pops(seed, k, 1 if kind == "single" else 8, rng) for k in range(2)]
            if kind != "single":
                pops[0] = rng.permutation(np.resize(LARGE_ROWS, nc)) if fam == -1 else _huge_band_rows(seed, rng)
            c = _case(f"{name}-{kind}-band-{seed}", kind, pc.ortho_box_edges(dims, edges), pbc, dims, pops[0], pops[1], rng, want)
            out.append(c)
            if not fixed_kind:
                out.append(without_box(c, (0, 0)))
        # three and two periodic cells: wrapped entries evaluated exactly, duplicate cell pairs
        dims, edges, pbc = LARGE_EXACT
        nc = pc.ncells(dims)
        for seed in range((len(table) + nc - 1) // nc + 2 if fixed_kind else 1):
            rng = _rng(fam, ki, 2, seed)
            pops = [rng.permutation(_lift(np.roll(table, -(seed * (nc - 1) + 2 * k))[:nc], fam, rng)) for k in range(2)]
            if kind != "single":
                pops[0] = rng.permutation(np.roll(LARGE_ROWS, seed)[:nc])
            out.append(_case(f"{name}-{kind}-exact-{seed}", kind, pc.ortho_box_edges(dims, edges), pbc, dims, pops[0], pops[1], rng, want))
        # a sheared box of (2, 2, 2) cells: all eight cells are cells of the corner entries
        rows, dims = TRIC_222
        if fam == -1:
            plants = [_corner_plants(kind, dims, np.roll(WIDE_FIRSTS, s), WIDE_SECONDS[s], np.roll(LARGE_ROWS[:4], s), WIDE_SECONDS[(s + 1) % 4])
                      for s in range(4)]
        elif kind == "single":
            plants = [_corner_plants(kind, dims, f[s], HUGE_SECONDS[s]) for f in (HUGE_FIRSTS_2, HUGE_FIRSTS_8) for s in range(4)]
        else:
            plants = [_corner_plants(kind, dims, np.roll(LARGE_ROWS[:4], s), HUGE_SECONDS[s], (1025,) * 4, HUGE_SECONDS[(s + 1) % 4]) for s in range(4)]
        for seed, (fix1, fix2) in enumerate(plants if fixed_kind else plants[:2]):
            rng = _rng(fam, ki, 3, seed)
            pops = [pc.plant(dims, (), (0, 0), rng, fx) for fx in (fix1, fix2)]
            out.append(_case(f"{name}-{kind}-tric-{seed}", kind, pc.sheared_box(rows), 7, dims, pops[0], pops[1], rng, want))
        # no box
        if fixed_kind:
            rng = _rng(fam, ki, 4)
            if fam == -1:
                p2 = np.array([460, 500, 520, 600, 450, 470, 580, 640])
                out.append(octant_case(f"wide-{kind}", kind, p2 if kind == "single" else np.full(8, 100), p2, rng, (-1, -1)))
            else:           # four of eight cells occupied: wide on the first search of the shape, huge on every later one
                p2 = np.array([0, 1100, 0, 1030, 0, 1150, 0, 1200])
                out.append(octant_case(f"huge-{kind}", kind, p2 if kind == "single" else p2 // 5, p2, rng, (-1, -2)))
    return out


THRESHOLDS = ((13, (6, 6, 6), (1.02, 1.02, 1.02), 7, (16, 32)), (19, (6, 6, 6), (1.02, 1.02, 1.02), 7, (32, 0)),
              (448, (4, 2, 1), (1.24, 1.45, 1.9), 1, (0, -1)), (1000, (4, 2, 1), (1.24, 1.45, 1.9), 1, (-1, -2)))


def threshold_cases():
    """N exactly mean * cells and one atom more, every cell occupied: the reported family must change between the two frames"""
    out = []
    for mean, dims, edges, pbc, fams in THRESHOLDS:
        for kind in FIXED:
            for extra in (0, 1):
                rng = _rng(99, mean, FIXED.index(kind), extra)
                pops = np.full(pc.ncells(dims), mean, np.int64)
                pops[int(rng.integers(len(pops)))] += extra
                out.append(_case(f"threshold-{mean}{'+1' if extra else ''}-{kind}", kind, pc.ortho_box_edges(dims, edges), pbc, dims, pops, pops,
                                 rng, (fams[extra], fams[extra]), covers=False))
    return out


_CACHE = {}


def all_cases():
    """every case by name, built once per process (a fifth of a second)"""
    if not _CACHE:
        cases = small_cases(16) + small_cases(32) + regular_cases() + large_cases(-1) + large_cases(-2) + threshold_cases()
        assert len(set(c["name"] for c in cases)) == len(cases)
        _CACHE.update((c["name"], c) for c in cases)
    return _CACHE


def reference(orc, c, nthreads=16):
    """the f32 oracle's result for a case"""
    ob = orc.box_from_matrix(c["box"]) if c["box"] is not None else None
    k, rc, p1, p2, pbc = c["kind"], c["cutoff"], c["p1"], c["p2"], c["pbc"]
    if k == "single":
        return orc.search_single_pbc(rc, p1, ob, pbc, nthreads=nthreads) if ob is not None else orc.search_single(rc, p1, nthreads=nthreads)
    if k == "double":
        return orc.search_double_pbc(rc, p1, p2, ob, pbc, nthreads=nthreads) if ob is not None else orc.search_double(rc, p1, p2, nthreads=nthreads)
    if k == "vdw":
        return orc.search_double_vdw_pbc(p1, p2, c["v1"], c["v2"], ob, pbc, nthreads=nthreads) if ob is not None \
            else orc.search_double_vdw(p1, p2, c["v1"], c["v2"], nthreads=nthreads)
    return orc.search_within_pbc(rc, p1, p2, ob, pbc, nthreads=nthreads) if ob is not None \
        else orc.search_within(rc, p1, p2, c["lower"], c["upper"], nthreads=nthreads)


_REFS = {}


def cached_reference(orc, c):
    """computed once, shared by the tests of a process, never written to"""
    if c["name"] not in _REFS:
        ref = reference(orc, c)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFS[c["name"]] = ref
    return _REFS[c["name"]]
