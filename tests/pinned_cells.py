"""Frames with CHOSEN cell populations for the consumers of the search's slot records (contact_kernel, cluster_kernel).
Nothing here touches the code under test: numpy alone, every coordinate from one seeded generator.

The reference bins a periodic frame by fractional coordinates, cell = floor(inv(box) * p * dims), with dims = floor(extent /
cutoff) per axis; an atom placed at the fractional position (cell + 0.05 + 0.9 * u) / dims, u in [0, 1), cannot be moved to
another cell by the rounding of the binning.  Rows of a cell are in input order, so in CELL-MAJOR input order (cells in the
reference's flat order x + y * dx + z * dx * dy, the atoms of one cell next to each other) labels given by selection position
dictate the label runs inside every cell; PERMUTED order interleaves the cells.

    frame(box, dims, pops, rng, order)  -> pos float32 [n, 3], box, pops[ncells], cell of every atom
    binned(pos, box, dims)              -> population of every cell by fractional binning (for the oracle's dims)

Boxes: ortho_box(dims, cutoff), tric_box(cutoff) (a synth.box_a-style shear: lattice shifts exist); for the f32 search's
instance cases (tests/search_f32_cases.py) ortho_box_edges (a cell edge per axis: few long cells), sheared_box (a shear with chosen
lab extents), plant (a table of populations inside a background) and corner_cells.  tests/test_pinned_cells_cpu.py
asserts on the reference alone that every frame the GPU tests use is what it was built to be.
"""
import numpy as np

# occupancies of first and second cells at which the kernels change their path: the 64-atom chunk and its multiples, both sides
EDGE_TABLE = (0, 1, 2, 3, 62, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 200)
CUTOFF = 0.5
ORDERS = ("cell_major", "permuted")


def ortho_box(dims, cutoff=CUTOFF, edge=1.02):
    """cells of `edge` cutoffs: floor(dims * edge) == dims for every edge in [1, 1 + 1 / dims)"""
    return np.diag([d * edge * cutoff for d in dims]).astype(np.float32)


def ortho_box_edges(dims, edges, cutoff=CUTOFF):
    """cells of edges[d] cutoffs along d: floor(dims[d] * edges[d]) == dims[d] needs 1 <= edges[d] < 1 + 1 / dims[d] - one cell
    may be up to 2 cutoffs long, two cells 1.5, four cells 1.25 (asserted)"""
    assert all(int(np.floor(d * e)) == d for d, e in zip(dims, edges)), (dims, edges)
    return np.diag([d * e * cutoff for d, e in zip(dims, edges)]).astype(np.float32)


def sheared_box(rows, shear=(-0.4, -0.3), cutoff=CUTOFF):
    """An upper-triangular box (c leans by shear[0] / shear[1] cutoffs in x / y) whose ROW sums - the reference's lab extents,
    which size its grid - are rows[d] cutoffs: lattice shifts exist, and floor(rows[d]) cells along d"""
    sx, sy = shear
    return (np.array([[rows[0] - sx, 0.0, sx], [0.0, rows[1] - sy, sy], [0.0, 0.0, rows[2]]]) * cutoff).astype(np.float32)


def plant(dims, values, background, rng, fixed=None):
    """Populations with every entry of `values` in a cell of its own (cells drawn without replacement) inside a background drawn
    uniformly from background = (lo, hi), both included; fixed = {cell: population} is applied last (its cells are kept free of
    `values`)."""
    nc = ncells(dims)
    fixed = dict(fixed or {})
    free = np.array([c for c in rng.permutation(nc) if int(c) not in fixed], np.int64)
    assert len(values) <= len(free), (len(values), len(free))
    pops = rng.integers(background[0], background[1] + 1, size=nc).astype(np.int64)
    pops[free[: len(values)]] = np.asarray(values, np.int64)
    for c, v in fixed.items():
        pops[c] = v
    return pops


def corner_cells(dims):
    """(first cells, second cells) of the four plan entries that wrap in all three dimensions (masks 7, 11, 12, 13 of the cell
    (dx - 1, dy - 1, dz - 1)), as flat indices, entry by entry"""
    dx, dy, dz = (int(d) for d in dims)
    first = [(dx - 1, dy - 1, dz - 1), (0, 0, dz - 1), (0, dy - 1, 0), (dx - 1, 0, 0)]
    second = [(0, 0, 0), (dx - 1, dy - 1, 0), (dx - 1, 0, dz - 1), (0, dy - 1, dz - 1)]
    return [cell_index(dims, *c) for c in first], [cell_index(dims, *c) for c in second]


TRIC_DIMS = (3, 3, 4)          # what the reference makes of tric_box (asserted in the CPU test, from one oracle call)


def tric_box(cutoff=CUTOFF):
    """synth.box_a's shape (c = (-0.139 L, -0.139 L, L)) with a diagonal of 4 * 1.02 cutoffs"""
    L = 4 * 1.02 * cutoff
    sh = -3.0 / 21.544 * L
    return np.array([[L, 0.0, sh], [0.0, L, sh], [0.0, 0.0, L]], dtype=np.float32)


def ncells(dims):
    return int(dims[0]) * int(dims[1]) * int(dims[2])


def cell_xyz(dims, c):
    c = np.asarray(c, np.int64)
    return np.stack([c % dims[0], (c // dims[0]) % dims[1], c // (dims[0] * dims[1])], -1)


def cell_index(dims, x, y, z):
    return int(x) + int(y) * int(dims[0]) + int(z) * int(dims[0]) * int(dims[1])


def table_pops(dims, rng, table=EDGE_TABLE, permute=True):
    """every entry of `table` as often as the grid has room for (the rest: the table's first entries), assigned to the cells
    in table order or permuted"""
    nc = ncells(dims)
    pops = np.resize(np.asarray(table, np.int64), nc)
    return rng.permutation(pops) if permute else pops


def frame(box, dims, pops, rng, order="permuted", corners=None):
    """pops[c] atoms in cell c (flat index x + y * dx + z * dx * dy).  corners = None: uniform in the inner 90 % of the cell.
    corners = (lo, hi, jitter): atom k of a cell sits at one of the 8 corners (lo / hi per axis) of the cell, +- jitter (all
    in cell edges); the first 8 atoms of a cell take the 8 corners in turn, the others a random one, the same for atoms
    8 and 9, 10 and 11 ... of the cell (pair_labels)."""
    assert order in ORDERS
    pops = np.asarray(pops, np.int64)
    assert len(pops) == ncells(dims)
    cell = np.repeat(np.arange(len(pops)), pops)
    n = len(cell)
    if corners is None:
        u = 0.05 + 0.9 * rng.random((n, 3))
    else:
        lo, hi, jit = corners
        first = np.concatenate([[0], np.cumsum(pops)[:-1]])
        k = np.arange(n) - first[cell]                             # rank of the atom in its cell
        draw = rng.integers(0, 8, size=n)
        blob = np.where(k < 8, k, draw[np.arange(n) - np.where(k >= 8, (k - 8) % 2, 0)])
        bits = np.stack([blob & 1, (blob >> 1) & 1, (blob >> 2) & 1], -1)
        u = np.where(bits == 1, hi, lo) + rng.uniform(-jit, jit, size=(n, 3))
    if order == "permuted":
        perm = rng.permutation(n)
        cell, u = cell[perm], u[perm]
    frac = (cell_xyz(dims, cell) + u) / np.asarray(dims, np.float64)
    pos = frac @ np.asarray(box, np.float64).T
    return pos.astype(np.float32), box, pops, cell


def pair_labels(cell):
    """Particles of a CELL-MAJOR corner frame, ascending with the position: the first 8 atoms of a cell are particles of their
    own, then two atoms next to each other (which share a blob) form one - pos // 2 fitted to the cells.  Returns (labels, G)."""
    cell = np.asarray(cell, np.int64)
    assert np.all(np.diff(cell) >= 0), "cell-major order only"
    pops = np.bincount(cell)
    first = np.concatenate([[0], np.cumsum(pops)[:-1]])
    k = np.arange(len(cell)) - first[cell]
    local = np.where(k < 8, k, 8 + (k - 8) // 2)
    per_cell = np.where(pops <= 8, pops, 8 + (pops - 8 + 1) // 2)
    base = np.concatenate([[0], np.cumsum(per_cell)[:-1]])
    return (base[cell] + local).astype(np.uint32), int(per_cell.sum())


def cell_of(pos, box, dims):
    """the reference's binning of atoms inside the box, in double precision"""
    rel = np.asarray(pos, np.float64) @ np.linalg.inv(np.asarray(box, np.float64)).T
    loc = np.floor(rel * np.asarray(dims, np.float64)).astype(np.int64)
    assert np.all(loc >= 0) and np.all(loc < np.asarray(dims)), "an atom outside the box"
    return loc[:, 0] + loc[:, 1] * dims[0] + loc[:, 2] * dims[0] * dims[1]


def binned(pos, box, dims):
    return np.bincount(cell_of(pos, box, dims), minlength=ncells(dims))


def neighbours(dims, pbc, faces_only=False):
    """ordered pairs (a, b) of DIFFERENT cells next to each other (offsets -1 / 0 / 1, through the periodic faces of `pbc`);
    faces_only: cells that share a face"""
    nc = ncells(dims)
    xyz = cell_xyz(dims, np.arange(nc))
    out = set()
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                if faces_only and abs(dx) + abs(dy) + abs(dz) != 1:
                    continue
                t = xyz + (dx, dy, dz)
                ok = np.ones(nc, bool)
                for d in range(3):
                    if (pbc >> d) & 1:
                        t[:, d] %= dims[d]
                    else:
                        ok &= (t[:, d] >= 0) & (t[:, d] < dims[d])
                b = t[:, 0] + t[:, 1] * dims[0] + t[:, 2] * dims[0] * dims[1]
                out |= set((int(a), int(bb)) for a, bb in zip(np.arange(nc)[ok], b[ok]) if a != bb)
    return out


# ---------------------------------------------------------------- the shapes of the GPU tests

VARIANTS = {"ortho7": ((4, 4, 4), 7), "ortho3": ((4, 4, 4), 3), "tric7": (TRIC_DIMS, 7)}


def variant_box(variant, cutoff=CUTOFF):
    dims, pbc = VARIANTS[variant]
    return (tric_box(cutoff) if variant == "tric7" else ortho_box(dims, cutoff)), dims, pbc


def edge_frame(variant, seed=1, order="permuted"):
    """the edge table over the grid of `variant`, permuted over the cells: (4, 4, 4) holds every entry four times"""
    box, dims, pbc = variant_box(variant)
    rng = np.random.default_rng(seed)
    pos, box, pops, cell = frame(box, dims, table_pops(dims, rng), rng, order)
    return pos, box, pops, cell, dims, pbc


# (n1, n2) of neighbouring cells the DOUBLE tests must meet; (0, k) and (k, 0) with some k > 64 besides
DOUBLE_PAIRS = ((1, 193), (193, 1), (64, 64), (65, 63), (63, 65), (129, 65))


def has_double_pairs(dims, pbc, pops1, pops2):
    got = set((int(pops1[a]), int(pops2[b])) for a, b in neighbours(dims, pbc, faces_only=True))
    return (all(p in got for p in DOUBLE_PAIRS) and any(a == 0 and b > 64 for a, b in got) and any(a > 64 and b == 0 for a, b in got))


def double_frames(variant, seed=2, order="permuted"):
    """Two sets with the edge table each, permuted independently until cells that share a face hold DOUBLE_PAIRS.  Returns
    (all, idx1, idx2, pos1, pos2, box, pops1, pops2, dims, pbc): pos1 / pos2 are the sets as arrays of their own, and
    all[idx1] == pos1, all[idx2] == pos2 are OVERLAPPING selections of one array (half of min(pops1, pops2) atoms of every
    cell belong to both sets)."""
    box, dims, pbc = variant_box(variant)
    rng = np.random.default_rng(seed)
    for _ in range(1000):
        pops1, pops2 = table_pops(dims, rng), table_pops(dims, rng)
        if has_double_pairs(dims, pbc, pops1, pops2):
            break
    else:
        raise AssertionError("no assignment with the pairs asked for")
    shared = np.minimum(pops1, pops2) // 2
    only1 = frame(box, dims, pops1 - shared, rng, order)[0]
    both = frame(box, dims, shared, rng, order)[0]
    only2 = frame(box, dims, pops2 - shared, rng, order)[0]
    every = np.concatenate([only1, both, only2])
    idx1 = np.arange(0, len(only1) + len(both), dtype=np.uint64)
    idx2 = np.arange(len(only1), len(every), dtype=np.uint64)
    return every, idx1, idx2, np.ascontiguousarray(every[: len(idx1)]), np.ascontiguousarray(every[len(only1):]), box, pops1, pops2, dims, pbc


# ---------------------------------------------------------------- label runs (cell-major order)

RUN_POPS = (129, 193, 64, 65, 1, 66, 128, 192)          # over (4, 4, 4): each eight times, cell c holds RUN_POPS[c % 8]
RUN_STRIDE = 80                                        # labels of one cell: base + 0 .. 79

# label runs of a cell in row order as (local label, length); the list is cycled (with labels moved on) until the cell is full
RUN_PATTERNS = {
    "ends_at_lane_63": [(0, 40), (1, 24), (2, 10), (3, 54), (4, 1)],
    "aligned_64": [(0, 64), (1, 64), (2, 7)],
    "crossing_64": [(0, 1), (1, 64), (2, 30), (3, 33), (4, 1)],          # lanes 1..63 of chunk 0 and lane 0 of chunk 1
    "run_of_65": [(0, 65), (1, 20), (2, 43), (3, 1)],
    "a_b_a": [(0, 20), (1, 10), (0, 20), (2, 14), (1, 30), (3, 3), (1, 31)],
    "distinct_beside_runs": [(k, 1) for k in range(64)] + [(64, 30), (65, 34)],
    "rows_1_32_63": [(0, 1), (1, 31), (2, 31), (3, 1), (4, 1), (5, 31), (6, 31), (7, 1)],
}


def run_frame(seed=3):
    """(4, 4, 4), cell c holds RUN_POPS[c % 8] atoms, cell-major order"""
    box, dims, pbc = variant_box("ortho7")
    rng = np.random.default_rng(seed)
    pos, box, pops, cell = frame(box, dims, table_pops(dims, rng, RUN_POPS, permute=False), rng, "cell_major")
    return pos, box, pops, cell, dims, pbc


def cell_labels(pattern, n):
    """the first n local labels of RUN_PATTERNS[pattern], cycled; labels stay below RUN_STRIDE"""
    runs = RUN_PATTERNS[pattern]
    span = max(l for l, _ in runs) + 1
    out, shift = [], 0
    while len(out) < n:
        for lab, length in runs:
            out += [(lab + shift) % RUN_STRIDE] * length
        shift += span
    return np.array(out[:n], np.int64)


def run_labels(pattern, cell, bases="ascending"):
    """labels by position for a CELL-MAJOR frame (cell = cell of every atom): every cell carries the pattern in row order, on
    top of a base of its own - (c % 8) * RUN_STRIDE ascending, descending, or 0 for all ("shared": the same labels in every
    cell).  Neighbours in x and y differ in c % 8, neighbours in z share it.  Returns (labels uint32, number of groups)."""
    cell = np.asarray(cell, np.int64)
    assert np.all(np.diff(cell) >= 0), "cell-major order only"
    g = np.empty(len(cell), np.int64)
    for c in np.unique(cell):
        at = np.nonzero(cell == c)[0]
        base = {"ascending": c % 8, "descending": 7 - c % 8, "shared": 0}[bases] * RUN_STRIDE
        g[at] = base + cell_labels(pattern, len(at))
    return g.astype(np.uint32), (1 if bases == "shared" else 8) * RUN_STRIDE


def runs_of(labels):
    """[(label, length)] of consecutive equal labels"""
    labels = np.asarray(labels, np.int64)
    if len(labels) == 0:
        return []
    cut = np.concatenate([[0], np.nonzero(np.diff(labels))[0] + 1, [len(labels)]])
    return [(int(labels[a]), int(b - a)) for a, b in zip(cut[:-1], cut[1:])]


# ---------------------------------------------------------------- rows per slot = 2 (triclinic, entries that wrap in x, y and z)

RPS_HOME = (1, 2, 3, 65)


def rps_frame(home, seed=4, order="permuted"):
    """A small triclinic frame whose home cell (dx - 1, dy - 1, dz - 1) holds `home` atoms.  The other first cells of the entries
    that wrap in all three dimensions - (0, 0, dz - 1), (0, dy - 1, 0), (dx - 1, 0, 0) - hold the next values of RPS_HOME in
    turn; every other cell holds one of 1, 2, 3, 5, 8, 65, 70."""
    box, dims, pbc = variant_box("tric7")
    rng = np.random.default_rng(seed + home)
    pops = rng.choice(np.array([1, 2, 3, 5, 8, 65, 70]), size=ncells(dims))
    k = RPS_HOME.index(home)
    dx, dy, dz = dims
    for n, c in enumerate([(dx - 1, dy - 1, dz - 1), (0, 0, dz - 1), (0, dy - 1, 0), (dx - 1, 0, 0)]):
        pops[cell_index(dims, *c)] = RPS_HOME[(k + n) % 4]
    pos, box, pops, cell = frame(box, dims, pops, rng, order)
    return pos, box, pops, cell, dims, pbc


# ---------------------------------------------------------------- corner blobs (cluster kernel)

BLOB_TABLE = (8, 63, 64, 65, 70, 100, 127, 128, 129, 193)
BLOB_CORNERS = (0.08, 0.92, 0.01)
BLOB_DIMS = (3, 3, 3)


def blob_frame(pbc=7, seed=5, order="permuted", dims=BLOB_DIMS, table=BLOB_TABLE, edge=1.3):
    """Cells of `edge` cutoffs with 8 tight blobs each, at the corners 0.08 / 0.92 of the cell, +- 0.01: two blobs of one cell
    are at least 0.82 * 1.3 = 1.07 cutoffs apart, the 8 blobs around a grid vertex at most 0.18 * 1.3 * sqrt(3) = 0.41 cutoffs.
    So the components are the grid's vertices: 27 with pbc = 7, 36 with z open (the 9 vertices on the open face fall in two).
    Every cell holds at least one atom per blob (table entries >= 8).  With blobs at 0.1 / 0.9 and +- 0.02 the frame collapses
    to one component at edge 1.3: the margin matters."""
    box = ortho_box(dims, CUTOFF, edge)
    rng = np.random.default_rng(seed)
    pos, box, pops, cell = frame(box, dims, table_pops(dims, rng, table), rng, order, corners=BLOB_CORNERS)
    return pos, box, pops, cell, dims, pbc


def edge_blob_frame(seed=6, order="permuted"):
    """The edge table (4, 4, 4) for the cluster kernel.  dims = floor(L / cutoff) ties the cell edge to 1 .. 1.25 cutoffs, and a
    cell of that size filled uniformly with 60 .. 200 atoms is far above percolation whatever the cutoff: one giant component.
    So the atoms sit in the corner blobs, and the cutoff is the smallest one that keeps the grid: cells of 1.24 cutoffs (two
    blobs of a cell are 0.82 * 1.24 = 1.017 cutoffs apart or more).  Cells of 0 .. 3 atoms leave corners empty."""
    return blob_frame(7, seed, order, dims=(4, 4, 4), table=EDGE_TABLE, edge=1.24)


# ---------------------------------------------------------------- blocks of frames (the frames forms)

def edge_block(seeds=(11, 12, 13)):
    """3 edge-table frames of one shape (ortho7, cell-major) whose tables are permuted differently: the same atom count, other
    cells crowded in every frame.  Returns (frames [3, n, 3], box, [pops], dims, pbc)."""
    fr = [edge_frame("ortho7", s, "cell_major") for s in seeds]
    return np.stack([f[0] for f in fr]), fr[0][1], [f[2] for f in fr], fr[0][4], fr[0][5]


def double_block(seeds=(21, 22, 23)):
    """3 pairs of separate sets (frames1 [3, n1, 3], frames2 [3, n2, 3], box, [pops1], [pops2], dims, pbc)"""
    fr = [double_frames("ortho7", s, "cell_major") for s in seeds]
    return np.stack([f[3] for f in fr]), np.stack([f[4] for f in fr]), fr[0][5], [f[6] for f in fr], [f[7] for f in fr], fr[0][8], fr[0][9]


def blob_block(seeds=(31, 32, 33)):
    fr = [blob_frame(7, s) for s in seeds]
    return np.stack([f[0] for f in fr]), fr[0][1], [f[2] for f in fr], fr[0][4], fr[0][5]
