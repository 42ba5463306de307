"""Input builders for the tests of the f64 pair search: frames whose cell occupancies are known exactly, the number of 64-row
slots their plan has, pairs planted at the cutoff across every face, edge and corner of a periodic cell.  Pure numpy.

Boxes are 3x3 matrices with the box vectors as COLUMNS (pos = frac @ box.T), cells are numbered x + y * dx + z * dx * dy as the
grid of distance_search.rs numbers them."""
import numpy as np

EPS = 2.220446049250313e-16

# the 14 (first cell, second cell) offsets of the half-shell stencil (distance_search.rs:39-60)
MASKS = np.array([
    [0, 0, 0, 0, 0, 0],
    [0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 1],
    [0, 0, 0, 1, 1, 0], [0, 0, 0, 1, 0, 1], [0, 0, 0, 0, 1, 1],
    [0, 0, 0, 1, 1, 1],
    [1, 0, 0, 0, 1, 0], [1, 0, 0, 0, 0, 1], [0, 1, 0, 0, 0, 1],
    [1, 1, 0, 0, 0, 1], [1, 0, 1, 0, 1, 0], [0, 1, 1, 1, 0, 0],
])

# sheared boxes of the instance sweep at rc = 1.0; get_lab_extents is the ROW sums, so the negative shear shrinks the grid
BOX_4 = np.array([[5.3, 0.0, -0.9], [0.0, 5.2, -0.8], [0.0, 0.0, 4.4]])        # dims (4, 4, 4)
BOX_334 = np.array([[4.3, 0.0, -0.9], [0.0, 4.2, -0.8], [0.0, 0.0, 4.4]])      # dims (3, 3, 4)
BOX_323 = np.array([[4.3, 0.0, -0.9], [0.0, 3.4, -0.8], [0.0, 0.0, 3.4]])      # dims (3, 2, 3)


def _lattice_one(box, dims, K, rng, delta):
    dims = np.asarray(dims, np.int64)
    cells = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1).reshape(-1, 3)
    c = np.repeat(cells, K, axis=0).astype(np.float64)
    frac = (c + delta + (1.0 - 2.0 * delta) * rng.random(c.shape)) / dims
    frac = frac[rng.permutation(len(frac))]                    # selection order unrelated to cell order
    return frac @ np.asarray(box, np.float64).T


def lattice(box, dims, K, seed, delta=0.02, K2=None):
    """Exactly K atoms in every cell of a `dims` grid over `box`: fractional coordinates uniform in [c + delta, c + 1 - delta] /
    dims per cell c, shuffled, mapped through the box.  The reference assigns cells from fractional coordinates, so every cell
    holds K atoms whatever the shear, and the margin keeps that free of rounding.  With K2: two sets, (K per cell, K2 per cell)."""
    rng = np.random.default_rng(seed)
    first = _lattice_one(box, dims, K, rng, delta)
    return first if K2 is None else (first, _lattice_one(box, dims, K2, rng, delta))


def cells_box(pos, box, dims):
    """Cell index triplets of positions inside a periodic box (Grid::populate_pbc for atoms that need no wrapping)."""
    dims = np.asarray(dims, np.int64)
    frac = np.linalg.solve(np.asarray(box, np.float64), np.asarray(pos, np.float64).T).T
    return np.minimum(np.floor(frac * dims).astype(np.int64), dims - 1)


def occupancy_box(pos, box, dims):
    """Atoms per cell, [dx * dy * dz], recomputed from the positions."""
    c = cells_box(pos, box, dims)
    assert (c >= 0).all()
    return np.bincount(c[:, 0] + dims[0] * (c[:, 1] + dims[1] * c[:, 2]), minlength=int(np.prod(dims)))


def bounding_box(rc, *sets):
    """compute_bounding_box_single / _double (distance_search.rs:602-646): min / max seeded with ZERO, padded by rc + eps."""
    lo = np.zeros(3)
    hi = np.zeros(3)
    for p in sets:
        lo = np.minimum(lo, p.min(0))
        hi = np.maximum(hi, p.max(0))
    return lo + (-rc - EPS), hi + (rc + EPS)


def dims_of(lower, upper, rc):
    return tuple(int(max(np.floor((u - l) / rc), 1)) for l, u in zip(lower, upper))


def occupancy_no_box(pos, lower, upper, dims):
    """Atoms per cell of the non-periodic grid (Grid::populate, distance_search.rs:120-142)."""
    d = np.asarray(dims, np.int64)
    c = np.floor(d * (pos - lower) / (upper - lower)).astype(np.int64)
    keep = ((c >= 0) & (c < d)).all(1)
    c = c[keep]
    return np.bincount(c[:, 0] + d[0] * (c[:, 1] + d[1] * c[:, 2]), minlength=int(np.prod(d)))


def plan_slots(occ1, occ2, dims, pbc):
    """64-row slots of the 14-mask plan (distance_search.rs:39-60, 217-269) for per-cell occupancies `occ1` (and `occ2` of a
    second set, else None): an entry with both cells non-empty counts ceil(rows / 64); cells wrap only in the periodic
    dimensions of `pbc`, entries leaving the grid elsewhere are dropped; two sets count (first, second) and (second, first)."""
    dims = tuple(int(x) for x in dims)
    a = np.asarray(occ1, np.int64).reshape(dims[2], dims[1], dims[0]).transpose(2, 1, 0)      # a[x, y, z]
    b = a if occ2 is None else np.asarray(occ2, np.int64).reshape(dims[2], dims[1], dims[0]).transpose(2, 1, 0)

    def at(arr, off):                     # arr[cell + off], and where cell + off is a cell of the grid
        ok = np.ones(dims, bool)
        for d in range(3):
            if off[d]:
                arr = np.roll(arr, -1, axis=d)
                if not (pbc >> d) & 1:
                    edge = [slice(None)] * 3
                    edge[d] = dims[d] - 1
                    ok[tuple(edge)] = False
        return arr, ok
    total = 0
    for m in MASKS:
        a1, ok1 = at(a, m[:3])
        b2, ok2 = at(b, m[3:])
        ok = ok1 & ok2
        total += int((((a1 + 63) // 64) * (b2 > 0) * ok).sum())
        if occ2 is not None:
            a2, _ = at(a, m[3:])
            b1, _ = at(b, m[:3])
            total += int((((a2 + 63) // 64) * (b1 > 0) * ok).sum())
    return total


def plan_cell_pairs(dims, pbc, two=False):
    """The 14-mask plan entry by entry, in plan order (x outer, z inner, the masks; two sets: (c1, c2) then (c2, c1)): arrays
    (first cell, second cell, wrap) - flat cell indices into the first and the second set's grid, and the dimensions in which
    one of the two cells went round the periodic boundary (bit d).  Entries that leave the grid in a non-periodic dimension
    are dropped; empty cells are not looked at."""
    dx, dy, dz = (int(x) for x in dims)
    out = []
    for x in range(dx):
        for y in range(dy):
            for z in range(dz):
                for m in MASKS:
                    cells, wrap = [], 0
                    for off in (m[:3], m[3:]):
                        c = [x + int(off[0]), y + int(off[1]), z + int(off[2])]
                        for d in range(3):
                            if c[d] == (dx, dy, dz)[d]:
                                if (pbc >> d) & 1:
                                    c[d] = 0
                                    wrap |= 1 << d
                                else:
                                    c = None
                                    break
                        cells.append(None if c is None else c[0] + dx * (c[1] + dy * c[2]))
                        if c is None:
                            break
                    if None in cells:
                        continue
                    out.append((cells[0], cells[1], wrap))
                    if two:
                        out.append((cells[1], cells[0], wrap))
    a = np.array(out, np.int64).reshape(-1, 3)
    return a[:, 0], a[:, 1], a[:, 2]


def planted_wrap_pairs(box, rc, dims, per_mask, seed, emin=-15.5, emax=-8.0):
    """Pairs at rc * (1 +- 10^e), e uniform in [emin, emax], across every face, edge and corner of the periodic cell: for each of
    the seven wrap masks `per_mask` pairs whose second atom leaves the cell in exactly that mask's dimensions (on the low or
    the high side, so the first atom sits on either side of the boundary), the second atom stored at its wrapped position."""
    rng = np.random.default_rng(seed)
    M = np.asarray(box, np.float64)
    dims = np.asarray(dims, np.float64)
    out = []
    for mask in range(1, 8):
        want = np.array([(mask >> d) & 1 for d in range(3)], bool)
        got = 0
        while got < per_mask:
            n = 4 * per_mask
            fa = rng.random((n, 3))
            side = rng.integers(0, 2, (n, 3))
            near = 0.6 * rng.random((n, 3)) / dims                         # within 0.6 of a cell of the face
            fa = np.where(want, np.where(side == 1, 1.0 - near, near), 0.2 + 0.6 * fa)
            a = fa @ M.T
            u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
            e = 10.0 ** rng.uniform(emin, emax, n) * rng.choice([-1.0, 1.0], n)
            b = a + rc * (1.0 + e)[:, None] * u
            fb = np.linalg.solve(M, b.T).T
            left = (fb < 0.0) | (fb >= 1.0)
            ok = (left == want).all(1)
            take = np.flatnonzero(ok)[: per_mask - got]
            out.append(np.stack([a[take], (fb[take] % 1.0) @ M.T], 1).reshape(-1, 3))
            got += len(take)
    return np.concatenate(out)


def wrap_mask_of_pairs(pos, box, dims, i, j):
    """Wrap mask of the cell pair of each (i, j): the dimensions in which the two cells are neighbours only round the boundary.
    Needs >= 4 cells per dimension (then cells one apart and cells dims - 1 apart cannot be confused)."""
    c = cells_box(pos, box, dims)
    diff = np.abs(c[np.asarray(i, np.int64)] - c[np.asarray(j, np.int64)])
    d = np.asarray(dims, np.int64)
    return ((diff == d - 1) * np.array([1, 2, 4])).sum(1)


def boundary_pairs(box, rc, npairs, seed, emin=-15.5, emax=-8.0):
    """Pairs that cross a periodic face with distance rc * (1 +- 10^e), e uniform in [emin, emax], first atoms anywhere on the
    face (the construction of the f32 suite's large sheared boxes, in f64)."""
    rng = np.random.default_rng(seed)
    M = np.asarray(box, np.float64)
    L = float(np.abs(M).sum(1).max())
    pts = []
    have = 0
    while have < npairs:
        n = 2 * npairs
        fa = rng.random((n, 3))
        fa[np.arange(n), rng.integers(0, 3, n)] = 1.0 - (0.5 * rc / L) * rng.random(n)
        a = fa @ M.T
        u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
        e = 10.0 ** rng.uniform(emin, emax, n) * rng.choice([-1.0, 1.0], n)
        b = a + rc * (1.0 + e)[:, None] * u
        fb = np.linalg.solve(M, b.T).T
        take = np.flatnonzero(((fb < 0) | (fb >= 1)).any(1))[: npairs - have]
        pts.append(np.stack([a[take], (fb[take] % 1.0) @ M.T], 1).reshape(-1, 3))
        have += len(take)
    return np.concatenate(pts)


BUCKETS = ((0, 64), (65, 128), (129, 192), (193, 256), (257, 1 << 30))


def bucket_of(K):
    """The occupancy bucket (lo, hi) a case of K atoms per second cell is named after: the register instances of 1-4 chunks
    and the chunk loop."""
    return next(b for b in BUCKETS if K <= b[1])


# ---- the cases of the instance sweep: exact occupancies per second cell, so that every register instance (1-4 chunks of 64
# columns), the hand-over to the chunk loop and the chunk loop itself are reached by every kind

K2S = (1, 63, 64, 65, 128, 129, 192, 193, 256, 257, 320, 600)
KINDS = ("single", "double", "vdw", "within")
SITUATIONS = ("tric_4_cells", "tric_2_3_cells", "pbc_xy", "pbc_xz", "no_box")
SWEEP_RC = 1.0
K1_TWO_SETS = 130           # three slots per entry, the last one of two rows


def _radii(n, rng):
    v = rng.uniform(0.3, 0.5, n)                 # pair cutoffs 0.6 .. 1.0: never above the cell size of the case
    v[0] = 0.5                                   # the largest pair cutoff is (0.5 + 0.5) + eps: the grid of the other kinds
    return v


def sweep_case(K2, kind, situation, seed=0):
    """One case of the sweep as a dict: kind, rc (the cutoff that sizes the grid), p1, p2 (None: single), v1, v2, box, pbc,
    lower, upper (no box only), dims (the grid the case is built for), K1, K2 (atoms per cell and set; without a box the
    second set's count after scaling into the bucket of the K2 the case is named after), bucket."""
    rng = np.random.default_rng([seed, K2, KINDS.index(kind), SITUATIONS.index(situation)])
    box, dims = (BOX_323, (3, 2, 3)) if situation == "tric_2_3_cells" else (BOX_4, (4, 4, 4))
    pbc = {"tric_4_cells": 7, "tric_2_3_cells": 7, "pbc_xy": 3, "pbc_xz": 5, "no_box": 0}[situation]
    two = kind != "single"
    c = {"kind": kind, "rc": SWEEP_RC, "box": box if pbc else None, "pbc": pbc, "bucket": bucket_of(K2), "v1": None, "v2": None,
         "lower": None, "upper": None, "p2": None}
    lseed = int(rng.integers(1 << 30))

    def make(K):
        if two:
            return lattice(box, dims, K1_TWO_SETS, lseed, K2=K)
        return lattice(box, dims, K, lseed), None
    K = K2
    p1, p2 = make(K)
    if not pbc:
        # the grid comes from the padded bounding box: scale the count until the fullest second cell is in the bucket
        lo, hi = c["bucket"]
        aim = min(K2, 48) if hi == 64 else (lo + hi) // 2 if hi < (1 << 30) else 330
        for _ in range(12):
            lower, upper = bounding_box(SWEEP_RC + (EPS if kind == "vdw" else 0.0), *([p1, p2] if two else [p1]))
            nd = dims_of(lower, upper, SWEEP_RC + (EPS if kind == "vdw" else 0.0))
            top = int(occupancy_no_box(p2 if two else p1, lower, upper, nd).max())
            if lo <= top <= hi or K2 == 1:
                break
            K = max(1, int(round(K * aim / top)))
            p1, p2 = make(K)
        c["lower"], c["upper"], dims = lower, upper, nd
    if kind == "vdw":
        c["v1"], c["v2"] = _radii(len(p1), rng), _radii(len(p2), rng)
        c["rc"] = (0.5 + 0.5) + EPS
    c.update(p1=p1, p2=p2, dims=tuple(dims), K1=K1_TWO_SETS if two else K, K2=K)
    return c


def sweep_reference(orc, c, nthreads=16):
    """The f64 oracle's result for a case of sweep_case."""
    ob = orc.box_from_matrix(c["box"]) if c["pbc"] else None
    k, rc, p1, p2, pbc = c["kind"], c["rc"], c["p1"], c["p2"], c["pbc"]
    if k == "single":
        return orc.search_single_pbc(rc, p1, ob, pbc, nthreads=nthreads) if pbc else orc.search_single(rc, p1, nthreads=nthreads)
    if k == "double":
        return orc.search_double_pbc(rc, p1, p2, ob, pbc, nthreads=nthreads) if pbc else orc.search_double(rc, p1, p2, nthreads=nthreads)
    if k == "vdw":
        return orc.search_double_vdw_pbc(p1, p2, c["v1"], c["v2"], ob, pbc, nthreads=nthreads) if pbc \
            else orc.search_double_vdw(p1, p2, c["v1"], c["v2"], nthreads=nthreads)
    return orc.search_within_pbc(rc, p1, p2, ob, pbc, nthreads=nthreads) if pbc \
        else orc.search_within(rc, p1, p2, c["lower"], c["upper"], nthreads=nthreads)


def sweep_check_inputs(c, ref):
    """What a case of the sweep promises about its own input, asserted against the oracle's grid: returns the slots of its plan."""
    dims = tuple(int(x) for x in ref["dims"])
    assert dims == c["dims"], (dims, c["dims"])
    two = c["p2"] is not None
    if c["pbc"]:
        occ1 = occupancy_box(c["p1"], c["box"], dims)
        occ2 = occupancy_box(c["p2"], c["box"], dims) if two else None
        assert (occ1 == c["K1"]).all() and (occ2 is None or (occ2 == c["K2"]).all())
    else:
        occ1 = occupancy_no_box(c["p1"], c["lower"], c["upper"], dims)
        occ2 = occupancy_no_box(c["p2"], c["lower"], c["upper"], dims) if two else None
        top = int((occ2 if two else occ1).max())
        assert c["bucket"][0] <= top <= c["bucket"][1] or (c["bucket"][0] == 0 and top <= 64), (top, c["bucket"])
    assert len(ref["i"]) > (1000 if c["K2"] >= 63 else 0)
    return plan_slots(occ1, occ2, dims, c["pbc"])


WRAP_BOX = 1.65 * BOX_4             # 10 x 10 x 10 cells at rc 0.7
WRAP_RC = 0.7


def wrap_masks_case(per_mask=1500, background=6000, seed=41):
    """(box, rc, positions): pairs at the cutoff planted across every face, edge and corner of a sheared periodic cell, the
    two atoms of a planted pair next to each other in the frame (2 k, 2 k + 1), then random atoms."""
    rng = np.random.default_rng(seed)
    dims = dims_of(np.zeros(3), WRAP_BOX.sum(1), WRAP_RC)
    pairs = planted_wrap_pairs(WRAP_BOX, WRAP_RC, dims, per_mask, seed)
    return WRAP_BOX, WRAP_RC, np.concatenate([pairs, rng.random((background + background % 2, 3)) @ WRAP_BOX.T])


def near_cutoff_hits_per_mask(pos, box, rc, ref, tol=1e-9):
    """Oracle hits within `tol` (relative) of the cutoff, counted by the wrap mask of their cell pair: [8]."""
    near = np.abs(ref["d"] / rc - 1.0) < tol
    m = wrap_mask_of_pairs(pos, box, ref["dims"], ref["i"][near], ref["j"][near])
    return np.bincount(m, minlength=8)


MANY_SLOTS_BOX = 1.107 * np.array([[13.5, 0.0, -0.8], [0.0, 13.9, -0.6], [0.0, 0.0, 15.7]])     # 4000 nm^3
MANY_SLOTS_RC = 0.3


def many_slots_case(n=400_000, seed=7):
    """(box, rc, positions): n atoms at 100 nm^-3 in a mildly sheared box - at 400 000 atoms more than 2^20 slots."""
    rng = np.random.default_rng(seed)
    box = MANY_SLOTS_BOX * (n / 400_000.0) ** (1.0 / 3.0)
    return box, MANY_SLOTS_RC, rng.random((n, 3)) @ box.T
