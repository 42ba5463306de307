"""A longdouble numpy restatement of the internal coordinates of molar_hip.h (molar_hip_intcoord), by another route where
there is one, with a bound on the device's f64 evaluation for every value, and the seeded generators of the tests.

Routes: the minimum image is the shortest of the 125 lattice images over the masked dimensions (the device reduces in
fractional coordinates and tries the stored shifts); the angle is arccos of the normalised dot product (the device: atan2
of the cross product's length and the dot product); the dihedral is the angle between the parts of A - B and D - C normal to
b2, atan2((b2^ x v) . w, v . w) (the device: atan2(|b2| (b1 . n2), n1 . n2)).

Bounds, eps = 2^-53 (the device works in f64 without fused operations, OpenCL's atan2 is within 6 ulp):
  a bond vector d = B - A without a box carries one rounding per component, |err| <= eps |d|.  With a box the device
  forms f = inv v, f - round(f), m f: the inverse carries a few eps kappa (kappa = |m| |inv|, row-sum norms), each product of
  a 3-vector a few eps of its terms, so |err| <= e_d = 32 eps kappa (|v| + |d| + L), v the raw difference and L the largest
  box-vector length - ample, not tight.
  DISTANCE: |err| <= e_d + 2 eps |d| (the squares, their sum and the square root).
  ANGLE: the angle between two vectors moves by at most the angle each vector turns, e_u / |u| + e_v / |v|; the cross and dot
  products carry at most 8 eps |u| |v| between them, which atan2 turns into at most 16 eps of angle; atan2 itself 6 ulp of a
  value below pi: 12 eps pi.
  DIHEDRAL: (n1 x n2) . b2^ = |b2| (b1 . n2) exactly, so phi is the signed angle between n1 and n2 whatever the errors of the
  bonds, and moves by the angles n1 and n2 turn: (e1 / |b1| + e2 / |b2|) / sin a1 and (e2 / |b2| + e3 / |b3|) / sin a2 to first
  order (a1, a2 the bond angles), doubled for the higher orders; the products' roundings at most 32 eps / (sin a1 sin a2);
  atan2 12 eps pi.
  The reference's own error (eps_ld = 2^-64 times the same conditioning) is covered by 1e-17 added to every bound.
margin_ok asserts that every value is further than its bound from every bin edge that matters, that both bond angles of
every valid angle and dihedral have a sine of at least 0.1, and that every bound is below 1e-9: then integers can be compared
for equality and values within the bounds.
"""
import collections

import numpy as np

LD = np.longdouble
EPS = LD(2.0) ** -53
PI = 4 * np.arctan(LD(1))
DISTANCE, ANGLE, DIHEDRAL = 2, 3, 4

Ref = collections.namedtuple("Ref", ["kind", "values", "bound", "hist", "map", "mean", "spread", "valid", "mean_bound", "spread_bound",
                                     "sin_min", "edge_margin", "nbins", "map_bins", "range"])


def _dot(a, b):
    return (a * b).sum(-1)


def _norm(a):
    return np.sqrt(_dot(a, a))


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _inverse3(m):
    """closed-form inverse of [..., 3, 3] in longdouble"""
    c = np.empty_like(m)
    for i in range(3):
        for j in range(3):
            r = [k for k in range(3) if k != i]
            s = [k for k in range(3) if k != j]
            minor = m[..., r[0], s[0]] * m[..., r[1], s[1]] - m[..., r[0], s[1]] * m[..., r[1], s[0]]
            c[..., j, i] = (-1) ** (i + j) * minor
    det = (m[..., 0, :] * c[..., :, 0]).sum(-1)
    return c / det[..., None, None]


def _box_rows(boxes, F):
    """[F, 3, 3] longdouble with the box vectors as ROWS from [9] column-major (columns = box vectors) or [F, 9]"""
    b = np.asarray(boxes, np.float64).astype(LD)
    if b.ndim == 1:
        b = np.broadcast_to(b, (F, 9))
    return b.reshape(F, 3, 3)            # column-major 3x3: the k-th triple is column k = box vector k


def _min_image(v, rows, pbc):
    """the shortest lattice image of v [F, T, 3] over the masked dimensions, rows [F, 3, 3]"""
    rng = [(-2, -1, 0, 1, 2) if pbc >> d & 1 else (0,) for d in range(3)]
    best = v.copy()
    best2 = _dot(v, v)
    for i in rng[0]:
        for j in rng[1]:
            for k in rng[2]:
                sh = (i * rows[:, 0] + j * rows[:, 1] + k * rows[:, 2])[:, None, :]
                c = v + sh
                c2 = _dot(c, c)
                better = c2 < best2
                best = np.where(better[..., None], c, best)
                best2 = np.where(better, c2, best2)
    return best


def _bonds(x, tuples, kind, rows, pbc):
    """bond vectors [kind - 1][F, T, 3] (ANGLE: u = A - B, v = C - B), their error bounds [kind - 1][F, T], finite [F, T]"""
    p = [x[:, tuples[:, j].astype(np.int64), :] for j in range(kind)]
    fin = np.ones(p[0].shape[:2], bool)
    for q in p:
        fin &= np.isfinite(q.astype(np.float64)).all(-1)
    if kind == ANGLE:
        raw = [p[0] - p[1], p[2] - p[1]]
    else:
        raw = [p[j + 1] - p[j] for j in range(kind - 1)]
    with np.errstate(invalid="ignore"):
        if rows is None or pbc == 0:
            return raw, [EPS * _norm(r) for r in raw], fin
        inv = _inverse3(rows)
        kappa = (np.abs(rows).sum(-1).max(-1) * np.abs(inv).sum(-1).max(-1))[:, None]
        L = _norm(rows).max(-1)[:, None]
        out, err = [], []
        for r in raw:
            d = _min_image(np.where(fin[..., None], r, 0), rows, pbc)
            out.append(d)
            err.append(32 * EPS * kappa * (_norm(np.where(fin[..., None], r, 0)) + _norm(d) + L))
        return out, err, fin


def _bin(v, kind, nbins, rng):
    """(bin or -1, distance of v to the nearest edge that decides its bin)"""
    v = v.astype(LD)
    if kind == DISTANCE:
        lo, hi = LD(rng[0]), LD(rng[1])
        u = (v - lo) / (hi - lo) * nbins
        width = (hi - lo) / nbins
        inside = (v >= lo) & (v < hi)
    elif kind == ANGLE:
        u = v / PI * nbins
        width = PI / nbins
        inside = np.ones(v.shape, bool)
    else:
        u = (v + PI) / (2 * PI) * nbins
        width = 2 * PI / nbins
        inside = np.ones(v.shape, bool)
    with np.errstate(invalid="ignore"):
        b = np.floor(u)
        margin = np.minimum(u - b, b + 1 - u) * width
        if kind == ANGLE:
            # 0 and pi are no edges: nothing lies below 0 and pi itself goes to the last bin
            margin = np.where(b <= 0, (1 - u) * width, margin)
            margin = np.where(b >= nbins - 1, (u - (nbins - 1)) * width, margin)
            if nbins == 1:
                margin = np.full(v.shape, LD(np.inf))
        if kind == DIHEDRAL and nbins == 1:
            margin = np.full(v.shape, LD(np.inf))
        bi = np.where(np.isfinite(u.astype(np.float64)), b, 0).astype(np.int64)
        if kind == DIHEDRAL:
            bi = bi % nbins
        bi = np.minimum(bi, nbins - 1)
    return np.where(inside, bi, -1), margin


def reference(frames, tuples, kind=None, labels=None, ngroups=None, boxes=None, pbc=7, nbins=0, range=None, pairs=None, pair_labels=None,
              npair_groups=None, map_bins=0):
    x = np.asarray(frames, np.float64).astype(LD)
    F = x.shape[0]
    tuples = np.asarray(tuples, np.uint64)
    T = tuples.shape[0]
    kind = tuples.shape[1] if kind is None else kind
    rows = None if boxes is None else _box_rows(boxes, F)
    if boxes is None:
        pbc = 0
    b, e, fin = _bonds(x, tuples, kind, rows, pbc)
    tiny = LD(1e-17)
    sin_min = np.full((F, T), np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        if kind == DISTANCE:
            val = _norm(b[0])
            ok = fin.copy()
            bound = e[0] + 2 * EPS * val + tiny
        elif kind == ANGLE:
            nu, nv = _norm(b[0]), _norm(b[1])
            ok = fin & (nu > 0) & (nv > 0)
            c = np.clip(_dot(b[0] / nu[..., None], b[1] / nv[..., None]), -1, 1)
            val = np.arccos(c)
            bound = e[0] / nu + e[1] / nv + 16 * EPS + 12 * EPS * PI + tiny
            sin_min = np.where(ok, np.sqrt(np.maximum(0, 1 - c * c)), np.inf).astype(np.float64)
        else:
            n1, n2 = _cross(b[0], b[1]), _cross(b[1], b[2])
            ok = fin & (n1 != 0).any(-1) & (n2 != 0).any(-1)
            l1, l2, l3 = _norm(b[0]), _norm(b[1]), _norm(b[2])
            h = b[1] / l2[..., None]
            v = -b[0] + _dot(b[0], h)[..., None] * h          # the part of A - B normal to b2
            w = b[2] - _dot(b[2], h)[..., None] * h           # the part of D - C normal to b2
            val = np.arctan2(_dot(_cross(h, v), w), _dot(v, w))
            s1, s2 = _norm(n1) / (l1 * l2), _norm(n2) / (l2 * l3)
            bound = 2 * (e[0] / l1 + e[1] / l2) / s1 + 2 * (e[1] / l2 + e[2] / l3) / s2 + 32 * EPS / (s1 * s2) + 12 * EPS * PI + tiny
            sin_min = np.where(ok, np.minimum(s1, s2), np.inf).astype(np.float64)
    ok &= np.isfinite(val.astype(np.float64))
    val = np.where(ok, val, LD(np.nan))
    bound = np.where(ok, bound, 0)
    valid = ok.sum(0).astype(np.uint64)

    edge_margin = np.full((F, T), LD(np.inf))
    if kind == DIHEDRAL:
        edge_margin = np.where(ok, PI - np.abs(val), LD(np.inf))      # the seam: +pi and -pi are one angle, two values
    hist = hmap = None
    G = 1 if labels is None else int(ngroups if ngroups is not None else np.max(labels) + 1)
    if nbins:
        bi, m = _bin(val, kind, nbins, range)
        if kind == DISTANCE:
            m = np.minimum(m, np.minimum(np.abs(val - LD(range[0])), np.abs(val - LD(range[1]))))
        edge_margin = np.minimum(edge_margin, np.where(ok, m, LD(np.inf)))
        lab = np.zeros(T, np.int64) if labels is None else np.asarray(labels).astype(np.int64)
        hist = np.zeros((G, nbins), np.uint64)
        sel = ok & (bi >= 0)
        np.add.at(hist, (np.broadcast_to(lab, (F, T))[sel], bi[sel]), 1)
    if map_bins and pairs is not None:
        pairs = np.asarray(pairs).astype(np.int64).reshape(-1, 2)
        P = pairs.shape[0]
        G2 = 1 if pair_labels is None else int(npair_groups if npair_groups is not None else np.max(pair_labels) + 1)
        bi, m = _bin(val, kind, map_bins, range)
        if kind == DISTANCE:
            m = np.minimum(m, np.minimum(np.abs(val - LD(range[0])), np.abs(val - LD(range[1]))))
        used = np.zeros(T, bool)
        used[pairs.reshape(-1)] = True
        edge_margin = np.minimum(edge_margin, np.where(ok & used[None, :], m, LD(np.inf)))
        plab = np.zeros(P, np.int64) if pair_labels is None else np.asarray(pair_labels).astype(np.int64)
        hmap = np.zeros((G2, map_bins, map_bins), np.uint64)
        b0, b1 = bi[:, pairs[:, 0]], bi[:, pairs[:, 1]]
        sel = ok[:, pairs[:, 0]] & ok[:, pairs[:, 1]] & (b0 >= 0) & (b1 >= 0)
        np.add.at(hmap, (np.broadcast_to(plab, (F, P))[sel], b0[sel], b1[sel]), 1)

    # statistics over the valid frames, and what the device's sums in f64 may differ by
    n = ok.sum(0).astype(LD)
    v0 = np.where(ok, val, 0)
    e0 = np.where(ok, bound, 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        if kind == DIHEDRAL:
            Cs, Sn = np.where(ok, np.cos(v0), 0).sum(0), np.where(ok, np.sin(v0), 0).sum(0)
            R = np.hypot(Cs, Sn)
            mean = np.arctan2(Sn, Cs)
            spread = 1 - R / n
            # every term: the value's bound (|d cos|, |d sin| <= |d phi|) and 4 eps of sincos; the sums n eps each
            d = np.sqrt(LD(2)) * (e0.sum(0) + (4 + n) * n * EPS)
            mean_bound = 2 * d / R + 12 * EPS * PI + tiny
            spread_bound = d / n + 8 * EPS + tiny
        else:
            S1, S2 = v0.sum(0), (v0 * v0).sum(0)
            mean = S1 / n
            var = S2 / n - mean * mean
            spread = np.sqrt(np.maximum(var, 0))
            vmax = np.abs(v0).max(0)
            mean_bound = e0.max(0) + (n + 2) * EPS * vmax + tiny
            # the device's S2 / n - mean^2 cancels: its error in the variance is e_var whatever the variance
            e_var = 4 * vmax * e0.max(0) + (2 * n + 8) * EPS * (S2 / n + mean * mean) + tiny
            spread_bound = np.sqrt(np.maximum(var, 0) + e_var) - np.sqrt(np.maximum(var - e_var, 0)) + 4 * EPS * spread + tiny
    nan = LD(np.nan)
    mean, spread = np.where(n > 0, mean, nan), np.where(n > 0, spread, nan)
    mean_bound, spread_bound = np.where(n > 0, mean_bound, 0), np.where(n > 0, spread_bound, 0)
    return Ref(kind, val.astype(np.float64), bound.astype(np.float64), hist, hmap, mean.astype(np.float64), spread.astype(np.float64), valid,
               mean_bound.astype(np.float64), spread_bound.astype(np.float64), sin_min, edge_margin.astype(np.float64), nbins, map_bins, range)


def margin_violations(ref):
    """[F, T] bool: the values margin_ok would refuse"""
    ok = np.isfinite(ref.values)
    bad = ok & ~(ref.edge_margin > ref.bound)
    bad |= ok & ~(ref.bound < 1e-9)
    if ref.kind != DISTANCE:
        bad |= ok & ~(ref.sin_min >= 0.1)
    return bad


def margin_ok(ref):
    ok = np.isfinite(ref.values)
    assert (ref.edge_margin[ok] > ref.bound[ok]).all(), "a value within its bound of a bin edge, of the range or of the seam at pi"
    if ref.kind != DISTANCE:
        assert (ref.sin_min[ok] >= 0.1).all(), "a bond angle with a sine below 0.1"
    assert (ref.bound[ok] < 1e-9).all(), "a bound of 1e-9 rad or more"
    return True


# ---------------------------------------------------------------- generators

def ortho_box(lengths):
    """[9] column-major"""
    return np.diag(np.asarray(lengths, np.float32)).reshape(9)


def tric_box(lengths, skew=(0.2, -0.15, 0.25)):
    """[9] column-major, box vectors a = (lx, 0, 0), b = (s0 lx, ly, 0), c = (s1 lx, s2 ly, lz): GROMACS' lower triangle"""
    lx, ly, lz = (float(v) for v in lengths)
    rows = np.array([[lx, 0, 0], [skew[0] * lx, ly, 0], [skew[1] * lx, skew[2] * ly, lz]], np.float32)
    return rows.reshape(9)


def make_chain(rng, natoms):
    """A chain of natoms atoms with bonds of 1 .. 1.5 and bond angles of 40 .. 140 degrees, float64 [natoms, 3]."""
    x = np.zeros((natoms, 3))
    d = np.array([1.0, 0.0, 0.0])
    for i in range(1, natoms):
        while True:
            nd = rng.normal(size=3)
            nd /= np.linalg.norm(nd)
            c = -float(nd @ d)                      # cosine of the bond angle at atom i - 1
            if abs(c) < np.cos(np.radians(40.0)):
                break
        d = nd
        x[i] = x[i - 1] + d * rng.uniform(1.0, 1.5)
    return x


def wrap_into(x, box9, pbc=7):
    """every atom on its own into the cell of the column-major box along the masked dimensions (float64 in and out)"""
    m = np.asarray(box9, np.float64).reshape(3, 3).T          # columns = box vectors
    s = np.linalg.solve(m, x.T).T
    mask = np.array([pbc >> d & 1 for d in range(3)], bool)
    s = np.where(mask[None, :], s - np.floor(s), s)
    return (m @ s.T).T


def make_case(seed, F, T, kind, box="none", pbc=7, natoms=None, noise=0.03, windows="random", base=None, tuples=None, **ref_args):
    """Seeded frames (float32 [F, natoms, 3]), tuples (uint64 [T, kind]), boxes (None, [9] or [F, 9] float32) and their
    reference: a chain (or `base`) with thermal noise per frame, tuples over windows of consecutive atoms (or `tuples`), every
    atom wrapped into the cell on its own under a box.  A frame that holds a value margin_ok would refuse is drawn again until none is left."""
    rng = np.random.default_rng(seed)
    if base is None:
        natoms = natoms or max(kind + 3, min(T + kind, 96))
        base = make_chain(rng, natoms)
    natoms = base.shape[0]
    if tuples is None:
        if windows == "random":
            start = rng.integers(0, natoms - kind + 1, size=T)
        else:
            start = np.arange(T) % (natoms - kind + 1)
        tuples = (start[:, None] + np.arange(kind)[None, :]).astype(np.uint64)
        flip = rng.random(T) < 0.3
        tuples[flip] = tuples[flip, ::-1]
    tuples = np.asarray(tuples, np.uint64)
    boxes = None
    if box == "ortho":
        boxes = ortho_box((9.0, 10.0, 11.0))
    elif box == "tric":
        boxes = np.stack([tric_box(np.array([9.0, 10.0, 11.0]) * (1.0 + 0.05 * np.sin(0.7 * f + np.arange(3)))) for f in range(F)])
    frames = np.zeros((F, natoms, 3), np.float32)

    def draw(f):
        x = base + noise * rng.normal(size=base.shape)
        if boxes is not None:
            x = wrap_into(x, boxes if boxes.ndim == 1 else boxes[f], pbc)
        frames[f] = x.astype(np.float32)

    for f in range(F):
        draw(f)
    for _ in range(100):
        ref = reference(frames, tuples, kind, boxes=boxes, pbc=pbc, **ref_args)
        bad = margin_violations(ref).any(1)
        if not bad.any():
            return frames, tuples, boxes, ref
        for f in np.nonzero(bad)[0]:
            draw(f)
    raise AssertionError("the generator did not find frames that keep the margins")


def half_ulp32(x):
    x = np.abs(np.asarray(x, np.float64))
    return 2.0 ** -24 * x + 2.0 ** -150
