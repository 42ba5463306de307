"""The reference of the minimum-distance calls (molar_hip_mindist*, the definition: include/molar_hip.h) in numpy longdouble, with
a bound for every distance derived from the f64 rounding of the operations, the gap of every reported minimum to its runner-up,
and the assertions that make a comparison of integers fair: on its own inputs no decided pair sits within its bound of a
rounding flip under a triclinic box, and every argmin and every decision against the cutoff is separated by more than the sum of
the two bounds.  Shared by test_mindist_cpu.py (which runs the assertions for every case committed), test_gpu_mindist.py and
test_cpp_mindist.py.

The metric is PeriodicBox::shortest_vector on the box record the library forms in f64 (box_from_matrix: the matrix, its inverse
by cofactors, the correction shifts).  That record is DATA of the definition, so it is formed here in f64 by the same operations
(python floats are IEEE doubles and nothing is contracted) and then taken as exact; shortest_vector itself is restated on
longdouble.  On orthorhombic boxes it is checked against another route: the enumeration of the 27 (9, 3) images."""
import collections

import numpy as np

LD = np.longdouble
U = 2.0 ** -53                 # unit roundoff of f64
EPS32, EPS64 = 2.0 ** -24, 0.0  # what rounding a result to Real adds, relative
SAFETY = 2.0                   # second-order terms of the first-order bounds below
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
ERR_SIZES, ERR_INVALID, ERR_TOO_LARGE = 1, 50, 51          # MOLAR_HIP_ERR_*


# ---------------------------------------------------------------- the box record, in f64 as the library forms it

def _n2(v):
    return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]


def inverse3(m):
    """linalg3.hpp inverse3 on a column-major matrix, operation by operation; None: det == 0."""
    m11, m21, m31, m12, m22, m32, m13, m23, m33 = (float(x) for x in m)
    mi1 = m22 * m33 - m32 * m23
    mi2 = m21 * m33 - m31 * m23
    mi3 = m21 * m32 - m31 * m22
    det = (m11 * mi1 - m12 * mi2) + m13 * mi3
    if det == 0.0:
        return None
    o = np.zeros(9)
    o[0] = mi1 / det
    o[3] = (m13 * m32 - m33 * m12) / det
    o[6] = (m12 * m23 - m22 * m13) / det
    o[1] = -mi2 / det
    o[4] = (m11 * m33 - m31 * m13) / det
    o[7] = (m13 * m21 - m23 * m11) / det
    o[2] = mi3 / det
    o[5] = (m12 * m31 - m32 * m11) / det
    o[8] = (m11 * m22 - m21 * m12) / det
    return o


Box = collections.namedtuple("Box", ["m", "inv", "shifts"])


def box_from_matrix(m9):
    """boxmath.hpp box_from_matrix in f64; None: refused (a vector of zero length, no inverse)."""
    m = np.asarray(m9, np.float64).reshape(9)
    if not np.all(np.isfinite(m)):
        # a matrix that is not finite has no finite inverse; the library's record is NaN and so is every distance
        return None
    col = [m[0:3].copy(), m[3:6].copy(), m[6:9].copy()]
    for cv in col:
        if np.sqrt(_n2(cv)) == 0.0:
            return None
    inv = inverse3(m)
    if inv is None:
        return None
    shifts = []
    if not all(m[q] == 0.0 for q in (1, 2, 3, 5, 6, 7)):
        a, b, c = col
        ln = lambda v: np.sqrt(_n2(v))
        longest = max(max(max(ln((a + b) + c), ln((a + b) - c)), ln((a - b) + c)), ln((-a + b) + c))
        half = 0.5 * longest
        two = 2.0 * half
        bound2 = two * two
        for i in (-1, 0, 1):
            for j in (-1, 0, 1):
                for k in (-1, 0, 1):
                    if i == 0 and j == 0 and k == 0:
                        continue
                    s = (float(i) * a + float(j) * b) + float(k) * c
                    if _n2(s) < bound2:
                        shifts.append(s)
    return Box(m, inv, np.array(shifts, np.float64).reshape(-1, 3))


# ---------------------------------------------------------------- shortest_vector on longdouble, and the bound of a distance

def round_away(x):
    return np.trunc(x + np.copysign(LD(0.5), x))


def shortest_vector(box, v, pbc):
    """(best [..., 3], margin [...]): shortest_vector of boxmath.hpp on longdouble v [..., 3]; margin: how far the nearest
    rounded fractional component is from a flip (0.5 - |f - round f|, the smallest over the periodic dimensions)."""
    m, inv = box.m.astype(LD), box.inv.astype(LD)
    f = [(inv[r] * v[..., 0] + inv[3 + r] * v[..., 1]) + inv[6 + r] * v[..., 2] for r in range(3)]
    margin = np.full(v.shape[:-1], np.inf)
    for d in range(3):
        if pbc & (1 << d):
            f[d] = f[d] - round_away(f[d])
            margin = np.minimum(margin, (LD(0.5) - np.abs(f[d])).astype(np.float64))
    start = np.stack([(m[r] * f[0] + m[3 + r] * f[1]) + m[6 + r] * f[2] for r in range(3)], axis=-1)
    if box.shifts.shape[0] == 0 or pbc != 7:
        return start, margin, np.stack(f, axis=-1)
    cands = start[..., None, :] + np.concatenate([np.zeros((1, 3)), box.shifts]).astype(LD)       # candidate 0: start
    n2 = (cands[..., 0] * cands[..., 0] + cands[..., 1] * cands[..., 1]) + cands[..., 2] * cands[..., 2]
    k = np.argmin(n2, axis=-1)                                                                    # the first of equal norms
    best = np.take_along_axis(cands, k[..., None, None], axis=-2)[..., 0, :]
    return best, margin, np.stack(f, axis=-1)


def distance_bound(box, v, g, best, d, shifted):
    """A bound of |f64 distance - d| for the difference v, the rounded fractional vector g, the vector kept and its length d,
    from the f64 rounding of the operations, first order (times SAFETY):
      v = x_j - x_i: one rounding per component, u |v_c|;
      f_r = sum_c inv_rc v_c: three products, two sums and v's own error: 4u sum_c |inv_rc v_c|; f - round(f) is exact;
      s_r = sum_c m_rc g_c: sum_c |m_rc| df_c + 3u sum_c |m_rc g_c|;   a candidate s + shift: one more u |cand_r|;
      n2 = sum c_r^2: 2 sum |c_r| dc_r + 3u n2;   d = sqrt(n2): dn2 / (2 d) (never more than sqrt(dn2)) + u d."""
    av = np.abs(v).astype(np.float64)
    ab = np.abs(best).astype(np.float64)
    dd = np.asarray(d, np.float64)
    if box is None:
        dc = U * av
    else:
        am, ai = np.abs(box.m), np.abs(box.inv)
        ag = np.abs(g).astype(np.float64)
        df = np.stack([4.0 * U * ((ai[r] * av[..., 0] + ai[3 + r] * av[..., 1]) + ai[6 + r] * av[..., 2]) for r in range(3)], axis=-1)
        dc = np.stack([(am[r] * df[..., 0] + am[3 + r] * df[..., 1] + am[6 + r] * df[..., 2])
                       + 3.0 * U * (am[r] * ag[..., 0] + am[3 + r] * ag[..., 1] + am[6 + r] * ag[..., 2]) for r in range(3)], axis=-1)
        if shifted:
            dc = dc + U * ab
    dn2 = 2.0 * (ab * dc).sum(axis=-1) + 3.0 * U * dd * dd
    with np.errstate(divide="ignore", invalid="ignore"):
        first = np.where(dd > 0.0, dn2 / (2.0 * dd), np.inf)
    return SAFETY * (np.minimum(first, np.sqrt(dn2)) + U * dd)


def frac_bound(box, v):
    """The bound of a fractional component: 4u max_r sum_c |inv_rc v_c| (distance_bound's df)."""
    av, ai = np.abs(v).astype(np.float64), np.abs(box.inv)
    return SAFETY * 4.0 * U * np.max(np.stack([(ai[r] * av[..., 0] + ai[3 + r] * av[..., 1]) + ai[6 + r] * av[..., 2] for r in range(3)], axis=-1), axis=-1)


def image_enumeration(box_lengths, v, pbc):
    """Another route on an orthorhombic box: the smallest |v + k L| over the images k of the periodic dimensions."""
    ks = [(-2, -1, 0, 1, 2) if pbc & (1 << d) else (0,) for d in range(3)]
    best = np.full(v.shape[:-1], np.inf, LD)
    L = np.asarray(box_lengths, np.float64).astype(LD)
    # the differences here reach +-2.5 L at the most
    for kx in ks[0]:
        for ky in ks[1]:
            for kz in ks[2]:
                w = v + np.array([kx, ky, kz], LD) * L
                best = np.minimum(best, (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2])
    return np.sqrt(best)


# ---------------------------------------------------------------- the call

Ref = collections.namedtuple("Ref", ["dist", "pair", "atom1", "near1", "atom2", "mat", "mat_mean", "mat_min", "mat_freq", "frame_ok", "nvalid",
                                     "b_dist", "b_atom1", "b_atom2", "b_mat", "b_mean", "b_min", "D", "B"])


def all_distances(frames, boxes, idx1, idx2, pbc, check=True):
    """D [F, n1, n2] longdouble, its bounds B float64, and frame_ok; with check, the assertion on the rounding flips is made by
    the caller on the decided pairs through `margins` (returned as the fourth value: margin - bound of the fraction)."""
    F = frames.shape[0]
    x1 = frames[:, idx1, :].astype(LD)
    x2 = frames[:, idx2, :].astype(LD)
    n1, n2 = x1.shape[1], x2.shape[1]
    D = np.zeros((F, n1, n2), LD)
    B = np.zeros((F, n1, n2))
    slack = np.full((F, n1, n2), np.inf)
    ok = np.ones(F, np.uint32)
    use_box = boxes is not None and pbc != 0
    for f in range(F):
        if not (np.all(np.isfinite(frames[f, idx1])) and np.all(np.isfinite(frames[f, idx2]))):
            ok[f] = 0
        box = None
        if use_box:
            box = box_from_matrix(boxes[f] if boxes.ndim == 2 else boxes)
            if box is None:
                ok[f] = 0
        if not ok[f]:
            D[f] = np.nan
            B[f] = np.nan
            continue
        v = x2[f][None, :, :] - x1[f][:, None, :]
        if box is None:
            best, g = v, None
        else:
            best, margin, g = shortest_vector(box, v, pbc)
            if box.shifts.shape[0]:
                slack[f] = margin - frac_bound(box, v)
        d = np.sqrt((best[..., 0] * best[..., 0] + best[..., 1] * best[..., 1]) + best[..., 2] * best[..., 2])
        D[f] = d
        B[f] = distance_bound(box, v, g, best, d, box is not None and box.shifts.shape[0] > 0 and pbc == 7)
    return D, B, ok, slack


def _min_with_gap(D, B, axis_size):
    """Over the last axis of D [..., K] (inf: not a pair): (value, argmin, bound, gap - bounds of the two); argmin -1 and value
    inf without a pair; the separation is inf without a runner-up."""
    Df = D.astype(np.float64)                       # ordering only; the values are taken from D
    order = np.argsort(Df, axis=-1, kind="stable")
    k0 = order[..., 0]
    v0 = np.take_along_axis(D, k0[..., None], axis=-1)[..., 0]
    b0 = np.take_along_axis(B, k0[..., None], axis=-1)[..., 0]
    if D.shape[-1] > 1:
        k1 = order[..., 1]
        v1 = np.take_along_axis(D, k1[..., None], axis=-1)[..., 0]
        b1 = np.take_along_axis(B, k1[..., None], axis=-1)[..., 0]
        with np.errstate(invalid="ignore"):
            sep = np.where(np.isfinite(v1.astype(np.float64)), (v1 - v0).astype(np.float64) - (b0 + b1), np.inf)
    else:
        sep = np.full(v0.shape, np.inf)
    none = ~np.isfinite(v0.astype(np.float64))
    k0 = np.where(none, -1, k0)
    sep = np.where(none, np.inf, sep)
    return v0, k0, np.where(none, 0.0, b0), sep


def reference(frames, boxes=None, idx1=None, idx2=None, labels1=None, labels2=None, G1=None, G2=None, pbc=7, same=False, exclude_same_group=False,
              cutoff=0.0, eps_out=EPS64, check=True):
    """Every output of the call on float64 `frames` [F, natoms, 3] (values a float32 entry can hold exactly when it is the
    reference of one), with the bounds b_* (what rounding the result to Real adds included: eps_out).  check: the assertions
    of the module's docstring, on these inputs."""
    frames = np.asarray(frames, np.float64)
    F, natoms = frames.shape[0], frames.shape[1]
    idx1 = np.arange(natoms) if idx1 is None else np.asarray(idx1).astype(np.int64)
    idx2 = idx1 if same else (np.arange(natoms) if idx2 is None else np.asarray(idx2).astype(np.int64))
    n1, n2 = idx1.shape[0], idx2.shape[0]
    lab1 = np.zeros(n1, np.int64) if labels1 is None else np.asarray(labels1).astype(np.int64)
    lab2 = lab1 if same else (np.zeros(n2, np.int64) if labels2 is None else np.asarray(labels2).astype(np.int64))
    G1 = 1 if labels1 is None else int(G1)
    G2 = G1 if same else (1 if labels2 is None else int(G2))
    boxes = None if boxes is None else np.asarray(boxes, np.float64)
    D, B, ok, slack = all_distances(frames, boxes, idx1, idx2, pbc)
    excluded = np.zeros((n1, n2), bool)
    if same:
        excluded |= np.eye(n1, dtype=bool)
        if exclude_same_group:
            excluded |= lab1[:, None] == lab2[None, :]
    Dx = np.where(excluded[None], LD(np.inf), D)
    good = ok.astype(bool)
    nan = np.nan
    decided = []                                    # (frame, i, j) of every pair a reported integer or distance rests on

    # per atom
    a1, near1, b_a1, sep1 = _min_with_gap(np.where(good[:, None, None], Dx, LD(np.inf)), np.nan_to_num(B), n2)
    a2, near2, b_a2, sep2 = _min_with_gap(np.where(good[:, None, None], Dx, LD(np.inf)).transpose(0, 2, 1), np.nan_to_num(B).transpose(0, 2, 1), n1)
    # per frame: the smallest under (d, i, j); the flattened order is (i, j)
    flatD = np.where(good[:, None, None], Dx, LD(np.inf)).reshape(F, -1)
    dist, kf, b_dist, sepf = _min_with_gap(flatD, np.nan_to_num(B).reshape(F, -1), n1 * n2)
    if same:
        # (i, j) and (j, i) are one pair with one distance, to the bit; the lower position pair is reported.  The runner-up is
        # looked for among the pairs i < j.
        upper = np.where(np.triu(np.ones((n1, n2), bool), 1)[None], np.where(good[:, None, None], Dx, LD(np.inf)), LD(np.inf)).reshape(F, -1)
        _, ku, _, sepf = _min_with_gap(upper, np.nan_to_num(B).reshape(F, -1), n1 * n2)
        assert np.array_equal(ku, kf), "the lowest pair of a symmetric matrix has i < j"
    pair = np.stack([np.where(kf < 0, -1, kf // n2), np.where(kf < 0, -1, kf % n2)], axis=1)
    # per cell
    mat = np.full((F, G1, G2), np.inf, LD)
    b_mat = np.zeros((F, G1, G2))
    members1 = [np.nonzero(lab1 == a)[0] for a in range(G1)]
    members2 = [np.nonzero(lab2 == b)[0] for b in range(G2)]
    cell_pair = {}
    for a in range(G1):
        for b in range(G2):
            if members1[a].size == 0 or members2[b].size == 0:
                continue
            sub = np.where(good[:, None, None], Dx, LD(np.inf))[:, members1[a]][:, :, members2[b]].reshape(F, -1)
            k = np.argmin(sub.astype(np.float64), axis=1)
            mat[:, a, b] = sub[np.arange(F), k]
            b_mat[:, a, b] = np.nan_to_num(B)[:, members1[a]][:, :, members2[b]].reshape(F, -1)[np.arange(F), k]
            cell_pair[(a, b)] = (members1[a][k // members2[b].size], members2[b][k % members2[b].size])
    b_mat = np.where(np.isfinite(mat.astype(np.float64)), b_mat, 0.0)

    nvalid = int(good.sum())
    matv = mat[good]
    if nvalid:
        s = np.zeros((G1, G2), LD)
        for f in np.nonzero(good)[0]:
            s = s + mat[f]
        mat_mean = s / LD(nvalid)
        mat_min = matv.min(axis=0)
        kmin = np.argmin(matv.astype(np.float64), axis=0)
        b_min = np.take_along_axis(b_mat[good], kmin[None], axis=0)[0]
        finite_mean = np.isfinite(mat_mean.astype(np.float64))
        # every term's own bound and its rounding to f64, the nvalid - 1 additions and the division
        with np.errstate(invalid="ignore"):
            b_mean = np.where(finite_mean, (b_mat[good] + U * np.nan_to_num(matv.astype(np.float64), posinf=0.0)).sum(axis=0) / nvalid
                              + SAFETY * (nvalid + 1) * U * np.nan_to_num(mat_mean.astype(np.float64), posinf=0.0), 0.0)
        mat_freq = (matv < LD(cutoff)).sum(axis=0).astype(np.uint32)
    else:
        mat_mean = np.full((G1, G2), nan, LD)
        mat_min = np.full((G1, G2), np.inf, LD)
        b_min = np.zeros((G1, G2))
        b_mean = np.zeros((G1, G2))
        mat_freq = np.zeros((G1, G2), np.uint32)

    if check:
        assert np.all(sep1[good] > 0.0), "an atom1 argmin is not separated by more than the two bounds"
        assert np.all(sepf[good] > 0.0), "a frame's argmin is not separated by more than the two bounds"
        with np.errstate(invalid="ignore"):
            dec = np.abs(matv.astype(np.float64) - float(cutoff)) > b_mat[good]
        assert np.all(dec | ~np.isfinite(matv.astype(np.float64))), "a mat_freq decision is within its bound of the cutoff"
        # the decided pairs under a triclinic box: no fractional component within its bound of a flip
        for f in np.nonzero(good)[0]:
            i = np.arange(n1)
            j = near1[f]
            keep = j >= 0
            assert np.all(slack[f][i[keep], j[keep]] > 0.0), "a decided pair (atom1) is within its bound of a rounding flip"
            j2 = np.arange(n2)
            i2 = near2[f]
            keep = i2 >= 0
            assert np.all(slack[f][i2[keep], j2[keep]] > 0.0), "a decided pair (atom2) is within its bound of a rounding flip"
            for (a, b), (ii, jj) in cell_pair.items():
                if np.isfinite(float(mat[f, a, b])):
                    assert slack[f][ii[f], jj[f]] > 0.0, "a decided pair (mat) is within its bound of a rounding flip"

    def per_frame(x, fill=nan):
        x = x.astype(np.float64)
        x[~good] = fill
        return x
    eo = float(eps_out)
    out_b = lambda v, b: b + eo * np.nan_to_num(np.abs(v.astype(np.float64)), posinf=0.0, nan=0.0)
    u64 = lambda k: np.where(k < 0, NONE, k.astype(np.uint64)).astype(np.uint64)
    near1_out = u64(near1)
    near1_out[~good] = NONE
    pair_out = u64(pair)
    pair_out[~good] = NONE
    return Ref(per_frame(dist), pair_out, per_frame(a1), near1_out, per_frame(a2), per_frame(mat), mat_mean.astype(np.float64), mat_min.astype(np.float64),
               mat_freq, ok, nvalid, out_b(dist, b_dist), out_b(a1, b_a1), out_b(a2, b_a2), out_b(mat, b_mat), b_mean, out_b(mat_min, b_min), D, B)


# ---------------------------------------------------------------- the cases

TRIC = np.array([3.1, 0.0, 0.0, 1.2, 2.9, 0.0, -1.0, 1.3, 2.7])            # column-major: a, b, c; sheared, with correction shifts
ORTHO = np.array([3.0, 0.0, 0.0, 0.0, 2.5, 0.0, 0.0, 0.0, 3.5])

Case = collections.namedtuple("Case", ["name", "F", "natoms", "n1", "n2", "box", "pbc", "G1", "G2", "same", "excl", "idx", "seed", "bad"])


def C(name, F, natoms, n1, n2, box="ortho", pbc=7, G1=0, G2=0, same=False, excl=False, idx=False, seed=0, bad=()):
    """box: "none", "ortho", "tric" (one box), "frames" (per-frame orthorhombic), "tricframes" (per-frame triclinic);
    G = 0: no labels; idx: index arrays (a permuted subset) instead of the first n atoms; bad: frames given a coordinate that is
    not finite."""
    return Case(name, F, natoms, n1, n2, box, pbc, G1, G2, same, excl, idx, seed, tuple(bad))


def f32_exact(x):
    return np.asarray(x, np.float32).astype(np.float64)


def labels_for(rng, n, G):
    """Unsorted labels below G with an empty group (when G > 2) and a group of one atom (when n allows)."""
    if G == 0:
        return None
    if G == 1:
        return np.zeros(n, np.uint32)
    live = [g for g in range(G) if not (G > 2 and g == 1)]           # group 1 stays empty
    lab = rng.choice(live, size=n).astype(np.uint32)
    if n > len(live) + 1 and len(live) > 1:
        lab[lab == live[-1]] = live[0]
        lab[rng.integers(0, n)] = live[-1]                           # a group of one atom
    return lab


def case_inputs(c):
    """frames, boxes, idx1, idx2, labels1, labels2 of a case; all coordinates and boxes are exact in float32."""
    rng = np.random.default_rng(1000 + c.seed)
    assert c.same or c.n1 + c.n2 <= c.natoms, "the two sets of a case are disjoint"
    span = np.array([3.0, 2.5, 3.5])
    frames = f32_exact(rng.uniform(-0.6, 1.6, (c.F, c.natoms, 3)) * span)
    boxes = None
    if c.box == "ortho":
        boxes = f32_exact(ORTHO)
    elif c.box == "tric":
        boxes = f32_exact(TRIC)
    elif c.box == "frames":
        boxes = f32_exact(ORTHO[None, :] * (1.0 + 0.05 * rng.uniform(-1, 1, (c.F, 1))))
    elif c.box == "tricframes":
        boxes = f32_exact(TRIC[None, :] * (1.0 + 0.05 * rng.uniform(-1, 1, (c.F, 1))))
    if c.idx:
        perm = rng.permutation(c.natoms)
        idx1 = perm[:c.n1].astype(np.uint64)
        idx2 = None if c.same else perm[c.n1:c.n1 + c.n2].astype(np.uint64)          # disjoint: a shared atom is a distance of 0 twice
    else:
        idx1 = None
        idx2 = None if c.same else np.arange(c.natoms - c.n2, c.natoms).astype(np.uint64)      # the last n2 atoms
    lab1 = labels_for(rng, c.n1, c.G1)
    lab2 = None if c.same else labels_for(rng, c.n2, c.G2)
    for f in c.bad:
        a = int(idx1[0]) if idx1 is not None else 0
        frames[f, a, 1] = np.nan
    return frames, boxes, idx1, idx2, lab1, lab2


def case_reference(c, eps_out=EPS64, cutoff=None, check=True):
    frames, boxes, idx1, idx2, lab1, lab2 = case_inputs(c)
    i1 = np.arange(c.n1) if idx1 is None else idx1
    return reference(frames, boxes, i1, idx2, lab1, lab2, c.G1, c.G2, c.pbc, c.same, c.excl, CUTOFF if cutoff is None else cutoff, eps_out, check)


CUTOFF = 0.4

# The committed cases.  The sizes around the plan's edges (rows per wave 128, rows per block 512, columns per tile 64) are in
# test_gpu_mindist.py, which builds them with C(...) from the plan function; these are the fixed ones both files share.
CASES = [
    C("none", 3, 90, 40, 50, box="none"),
    C("ortho", 3, 90, 40, 50),
    C("ortho_idx", 2, 150, 70, 65, idx=True, seed=1),
    C("frames", 3, 90, 40, 50, box="frames", seed=2),
    C("tric", 3, 90, 40, 50, box="tric", seed=3),
    C("tricframes", 2, 90, 40, 50, box="tricframes", seed=4),
    C("groups", 3, 140, 70, 70, G1=7, G2=5, seed=5),
    C("groups_tric", 2, 150, 70, 70, box="tric", G1=7, G2=1, idx=True, seed=6),
    C("same", 3, 80, 80, 80, same=True, G1=9, seed=7),
    C("same_excl", 3, 80, 80, 80, same=True, excl=True, G1=9, seed=8),
    C("same_nolabels", 2, 60, 60, 60, same=True, box="tric", seed=9),
    C("bad", 4, 90, 40, 50, box="frames", G1=4, G2=3, seed=10, bad=(1,)),
] + [C("mask%d_%s" % (p, b), 2, 70, 30, 40, box=b, pbc=p, seed=20 + p) for p in (0, 1, 3, 5, 7) for b in ("ortho", "tric")]

# What the GPU tests override the plan to, and the sizes molar_hip_mindist_plan reports (checked against it there).
COL_SPLITS, FRAME_BLOCK = 3, 2
ROWS_WAVE, ROWS_BLOCK, COL_TILE = 128, 512, 64
# (n1, n2): one below, at and one above rows per wave, rows per workgroup, the column tile (one split: n2 <= 64; two: 65 ..
# 128; three: 129 .. 192), both sets labelled so that groups straddle waves and tiles
SIZES = [(1, 1), (1, 5), (5, 1), (63, 65), (64, 64), (65, 63), (127, 129), (128, 128), (129, 127), (511, 70), (512, 64), (513, 193)]
SIZE_CASES = [C("n%dx%d" % (a, b), 1, a + b, a, b, box="frames" if (a + b) % 2 else "tric", G1=min(a, 3), G2=min(b, 4), seed=40 + k)
              for k, (a, b) in enumerate(SIZES)]
FRAME_CASES = [C("F%d" % F, F, 60, 30, 30, box="frames", G1=3, G2=2, seed=60 + F) for F in (1, FRAME_BLOCK, FRAME_BLOCK + 1, 2 * FRAME_BLOCK + 1)]
ALL_CASES = CASES + SIZE_CASES + FRAME_CASES
