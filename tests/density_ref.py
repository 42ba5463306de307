"""The numpy reference of the density calls (molar_hip_density / _f64; the definition: include/molar_hip.h), the generators of
the test cases, the C entry spelt out, and the bounds the GPU tests accept.

Positions, fractional coordinates and centres are formed in numpy longdouble (x87: 64 bits of mantissa) from the exact
inputs; the weights' scale S and the quantised weights q_k = rint(w_k 2^S) are formed as the definition says (w 2^S is exact
in float64, rint rounds to even, as llrint does) and summed in int64, which they fit by construction.

WHY THE INTEGERS ARE COMPARED FOR EQUALITY.  An atom's bin is floor(u_d nbins_d), and the kernels form u_d in float64.  The
reference reports, per case,
  margin_bin : the smallest distance of x = u_d nbins_d from an integer, over the kept atoms and the dimensions with more
               than one bin (on a wrapped dimension 0 and nbins_d are integers like the others: the wrap-around edge),
  margin_edge: the smallest distance, in bin widths, of any u_d from 0 and from 1 on the dimensions that are not wrapped
               (there an atom is dropped or kept), over all atoms with finite coordinates,
  u_bound    : a bound, in bin widths, on |x(kernel) - x(reference)|, derived below.
A test asserts min(margin_bin, margin_edge) >= 1e-3 and u_bound < that margin: then no atom can sit in another bin than the
reference's, and count, I_f, outside and everything formed from integers alone must be EQUAL.  The generators place atoms at
a bin centre plus a jitter of at most 0.4 bin widths, so the margin is about 0.1 by construction.

THE BOUND on x, with eps = 2^-53 (the reference's own 2^-64 roundings are covered by the slack of the constants).
BOX mode.  inv = inverse3(box) in float64: nine cofactors of two products and a difference, a determinant of six products,
  a division: |d inv_ij| <= 8 eps K max|inv|, K = 1 + 9 max|M| max|inv| (the condition of the box; cancellation inside a
  cofactor or the determinant costs at most that factor).  s_d = sum_j inv_dj p_j in three products and two sums:
      ds <= (8 K + 4) eps sum_j max|inv| |p_j|.
  u = (s - c) + 1/2 and the wrap u - floor(u): four roundings of numbers no larger than |s| + |c| + 1, plus dc:
      du <= ds + dc + 4 eps (|s| + |c| + 1);       dx <= nbins (du + eps |u|).
  The circular mean of ncentre atoms: theta = 2 pi s has dtheta <= 2 pi ds + 3 eps |theta|; sin and cos to 2 ulp, the
  products with w and the sums of ncentre terms (thread-strided partial sums, then a tree: any order is covered by ncentre):
      dS, dC <= W (dtheta + (ncentre + 4) eps),   W = sum w;
  atan2 of a vector of length R = |(S, C)| turns by at most (dS + dC) / R, and is itself good to 4 ulp of pi:
      dc <= ((dS + dC) / R + 4 pi eps) / (2 pi) + 3 eps.
  This is why the tests assert the resultant length R / W > 0.1: the bound scales with W / R.  A plain mean (a masked
  dimension that is not periodic): dc <= ds + (ncentre + 4) eps sum w |s| / W.
LAB mode.  u = ((p - c) - lo) * (1 / (hi - lo)):  du <= (dc + 3 eps (|p| + |c| + |lo|)) / (hi - lo) + 3 eps |u|, with
  dc <= (ncentre + 4) eps sum w |p| / W for the weighted mean.  Where lo = 0, there is no centring and hi - lo and nbins are
  powers of two, every operation is exact and the bound is 0 (the half-open edge cases rely on it: they put atoms ON the edges).

THE BOUND on density.  One lane adds term_f = (double)I_f * (2^-S / binvol_f) over the frames in order and divides by F: a
conversion, a division, a product and an addition per frame and a final division, (F + 4) eps sum_f |term_f| / F with
binvol_f taken as exact; binvol_f itself carries the determinant's 12 eps sum |products| / |det|, relative, which is added.
The float32 entry rounds that once more: half an ulp of the float32 result."""
import ctypes as C
import math

import numpy as np

import msd_ref as mr

LD = np.longdouble
EPS = 2.0 ** -53
BOX, LAB = 0, 1
ORTHO, TRICLINIC = mr.ORTHO, mr.TRICLINIC
ERR_SIZES, ERR_ZERO_MASS, ERR_NO_PBC, ERR_ZERO_LENGTH, ERR_INVERSE, ERR_INVALID, ERR_TOO_LARGE = 1, 2, 4, 5, 6, 50, 51
TWO_PI = 8 * np.arctan(LD(1))


def grid(mode, nbins, lo=(0.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0), centre_dims=0):
    from molar_amd import api
    return api.DensityGrid(mode, tuple(int(v) for v in nbins), tuple(float(v) for v in lo), tuple(float(v) for v in hi), int(centre_dims))


def ceil_log2(n):
    return 0 if n <= 1 else int(n - 1).bit_length()


def weight_scale(w_sel, n):
    """S of the definition for the selected weights (float64 array), n = len of the selection."""
    wmax = float(np.abs(w_sel).max()) if len(w_sel) else 0.0
    if wmax == 0.0:
        return 52
    e = math.frexp(wmax)[1]                                  # wmax = m 2^e, 1/2 <= m < 1: the smallest e with wmax < 2^e
    return min(52, 62 - ceil_log2(n) - e)


def _inverse_ld(M):
    m11, m21, m31, m12, m22, m32, m13, m23, m33 = (M[0, 0], M[1, 0], M[2, 0], M[0, 1], M[1, 1], M[2, 1], M[0, 2], M[1, 2], M[2, 2])
    mi1, mi2, mi3 = m22 * m33 - m32 * m23, m21 * m33 - m31 * m23, m21 * m32 - m31 * m22
    det = (m11 * mi1 - m12 * mi2) + m13 * mi3
    inv = np.array([[mi1, m13 * m32 - m33 * m12, m12 * m23 - m22 * m13],
                    [-mi2, m11 * m33 - m31 * m13, m13 * m21 - m23 * m11],
                    [mi3, m12 * m31 - m32 * m11, m11 * m22 - m21 * m12]], dtype=LD) / det
    prods = (abs(m11 * m22 * m33) + abs(m11 * m32 * m23) + abs(m12 * m21 * m33) + abs(m12 * m31 * m23) + abs(m13 * m21 * m32) + abs(m13 * m31 * m22))
    return inv, det, prods


def _pow2(x):
    return x > 0 and math.frexp(float(x))[0] == 0.5


def density(frames, grd, idx=None, weight=None, labels=None, ngroups=None, boxes=None, pbc=7, centre_idx=None, centre_weight=None):
    """The reference.  frames [F, natoms, 3] float32 or float64.  Returns a dict: count [G, nb] uint64, I [F, G, nb] int64,
    density [G, nb] longdouble and its bound dens_bound (float64), outside [F], centre [F, 3] longdouble and centre_bound,
    binvol [F] longdouble and binvol_rel (the relative bound), S, margin_bin, margin_edge, u_bound, resultant (the smallest
    resultant length of a circular mean, inf without one)."""
    frames = np.asarray(frames)
    F, natoms = frames.shape[:2]
    sel = np.arange(natoms) if idx is None else np.asarray(idx, np.int64)
    n = len(sel)
    nbins = np.array(grd.nbins, np.int64)
    nb = int(nbins.prod())
    lab = np.zeros(n, np.int64) if labels is None else np.asarray(labels, np.int64)
    G = 1 if labels is None else int(ngroups)
    w_sel = None if weight is None else np.asarray(weight, np.float64)[sel]
    S = 0 if weight is None else weight_scale(w_sel, n)
    q = np.ones(n, np.int64) if weight is None else np.array([int(np.rint(v * 2.0 ** S)) for v in w_sel], dtype=np.int64)
    box_mode = grd.mode == BOX
    cdims = grd.centre_dims if (centre_idx is not None and len(centre_idx)) else 0
    csel = None if not cdims else np.asarray(centre_idx, np.int64)
    cw = None if not cdims else (np.ones(natoms) if centre_weight is None else np.asarray(centre_weight, np.float64))[csel].astype(LD)
    lo, hi = np.array(grd.lo, LD), np.array(grd.hi, LD)
    wrapped = [box_mode and bool(pbc >> d & 1) for d in range(3)]
    exact = (not box_mode) and not cdims and all(float(v) == 0.0 for v in lo) and all(_pow2(float(h)) for h in hi) and all(_pow2(int(b)) for b in nbins)

    count = np.zeros(G * nb, np.uint64)
    I = np.zeros((F, G * nb), np.int64)
    outside = np.zeros(F, np.uint64)
    centre = np.zeros((F, 3), LD)
    binvol = np.zeros(F, LD)
    binvol_rel = 0.0
    margin_bin = margin_edge = resultant = np.inf
    u_bound = centre_bound = 0.0
    bx = None if boxes is None else np.asarray(boxes, np.float64)
    for f in range(F):
        p = frames[f].astype(LD)
        dc = np.zeros(3)
        c = np.zeros(3, LD)
        if box_mode:
            M = mr.box_matrix(bx if bx.ndim == 1 else bx[f]).astype(LD)
            inv, det, prods = _inverse_ld(M)
            binvol[f] = abs(det) / nb
            binvol_rel = max(binvol_rel, float(12 * EPS * prods / abs(det)))
            ainv, amat = float(np.abs(inv).max()), float(np.abs(M).max())
            K = 1.0 + 9.0 * amat * ainv
            coord = p @ inv.T                                             # s of every atom
            dcoord = (8 * K + 4) * EPS * ainv * np.abs(p).astype(np.float64).sum(1)          # ds of every atom
        else:
            w3 = (hi - lo) / nbins.astype(LD)
            binvol[f] = (w3[0] * w3[1]) * w3[2]
            coord = p
            dcoord = np.zeros(natoms)
        if cdims:
            W = cw.sum()
            for d in range(3):
                if not cdims >> d & 1:
                    continue
                x = coord[csel, d]
                if wrapped[d]:
                    th = TWO_PI * x
                    Ss, Cc = (cw * np.sin(th)).sum(), (cw * np.cos(th)).sum()
                    c[d] = np.arctan2(-Ss, -Cc) / TWO_PI + LD(0.5)
                    R = float(np.hypot(Ss, Cc))
                    resultant = min(resultant, R / float(W))
                    dth = float((2 * np.pi * dcoord[csel] + 3 * EPS * np.abs(th).astype(np.float64)).max())
                    dSC = float(W) * (dth + (len(csel) + 4) * EPS)
                    dc[d] = (2 * dSC / R + 4 * np.pi * EPS) / (2 * np.pi) + 3 * EPS if R > 0 else np.inf
                else:
                    c[d] = (cw * x).sum() / W
                    dc[d] = float(dcoord[csel].max()) + (len(csel) + 4) * EPS * float((cw * np.abs(x)).sum() / W)
            centre[f] = c
            if np.isfinite(c).all():                                      # (a centre that is not finite drops its frame: nothing to bound)
                centre_bound = max(centre_bound, float(dc.max()))
        ps = coord[sel]
        u = np.zeros((n, 3), LD)
        du = np.zeros((n, 3))
        for d in range(3):
            if box_mode:
                v = ps[:, d]
                if cdims >> d & 1:
                    v = (v - c[d]) + LD(0.5)
                av = np.abs(ps[:, d]).astype(np.float64)
                du[:, d] = dcoord[sel] + dc[d] + 4 * EPS * (av + abs(float(c[d])) + 1.0)
                if wrapped[d]:
                    v = v - np.floor(v)
                u[:, d] = v
            else:
                inw = 1 / (hi[d] - lo[d])
                u[:, d] = ((ps[:, d] - c[d]) - lo[d]) * inw
                du[:, d] = (dc[d] + 3 * EPS * (np.abs(ps[:, d]).astype(np.float64) + abs(float(c[d])) + abs(float(lo[d])))) * float(inw)
                du[:, d] += 3 * EPS * np.abs(u[:, d]).astype(np.float64)
        finite = np.isfinite(u).all(1) & bool(np.isfinite(c).all())
        keep = finite.copy()
        for d in range(3):
            if not wrapped[d]:
                keep &= (u[:, d] >= 0) & (u[:, d] < 1)
        x = u * nbins.astype(LD)[None]
        dx = nbins[None].astype(np.float64) * (du + EPS * np.abs(u).astype(np.float64))
        if not exact and finite.any():
            u_bound = max(u_bound, float(dx[finite].max()))
        for d in range(3):
            if not wrapped[d] and finite.any():
                e = np.minimum(np.abs(u[finite, d]), np.abs(u[finite, d] - 1)) * nbins[d]
                margin_edge = min(margin_edge, float(e.min()))
            if nbins[d] > 1 and keep.any():
                xd = x[keep, d]
                margin_bin = min(margin_bin, float(np.abs(xd - np.rint(xd)).min()))
        b = np.minimum(np.floor(np.where(keep[:, None], x, 0)).astype(np.int64), nbins[None] - 1)
        cell = lab * nb + (b[:, 0] * nbins[1] + b[:, 1]) * nbins[2] + b[:, 2]
        np.add.at(count, cell[keep], np.uint64(1))
        np.add.at(I[f], cell[keep], q[keep])
        outside[f] = n - int(keep.sum())
    unit = LD(2) ** -S
    terms = I.astype(LD) * (unit / binvol)[:, None] / F
    dens = terms.sum(0)
    tabs = np.abs(terms).astype(np.float64).sum(0)
    dens_bound = (F + 4) * EPS * tabs + binvol_rel * tabs
    return dict(count=count.reshape(G, nb), I=I.reshape(F, G, nb), density=dens.reshape(G, nb), dens_bound=dens_bound.reshape(G, nb), outside=outside,
                centre=centre, centre_bound=centre_bound, binvol=binvol, binvol_rel=binvol_rel, S=S, margin_bin=margin_bin, margin_edge=margin_edge,
                u_bound=u_bound, resultant=resultant, exact=exact, F=F, G=G, nb=nb)


def margin_ok(ref):
    """The two assertions that license the comparison of the integers for equality (module docstring)."""
    m = min(ref["margin_bin"], ref["margin_edge"])
    assert m >= 1e-3, ("an atom within 1e-3 bin widths of an edge", ref["margin_bin"], ref["margin_edge"])
    assert ref["u_bound"] < m, ("the rounding bound reaches the margin", ref["u_bound"], m)
    return m


def half_ulp32(x):
    x = np.abs(np.asarray(x, np.float64))
    return 2.0 ** -24 * x + 2.0 ** -150


# ---------------------------------------------------------------- generators

def box_of(boxes, f):
    b = np.asarray(boxes, np.float64)
    return mr.box_matrix(b if b.ndim == 1 else b[f])


def scatter_box(seed, F, n, nbins, boxes=ORTHO, pbc=7, images=3, out_frac=0.15, dtype=np.float32, natoms=None):
    """Frames [F, natoms, 3] for a BOX grid: every atom at a bin centre plus a jitter of at most 0.4 bin widths in fractional
    space, moved by up to +-`images` box lengths on the periodic dimensions and, a fraction out_frac of them, by one box length
    on the others (outside), then through the frame's box and rounded to dtype."""
    rng = np.random.default_rng(seed)
    natoms = n if natoms is None else natoms
    nbins = np.asarray(nbins)
    ub = rng.integers(0, nbins, size=(F, natoms, 3))
    u = (ub + 0.5 + rng.uniform(-0.4, 0.4, size=(F, natoms, 3))) / nbins
    for d in range(3):
        if pbc >> d & 1:
            u[:, :, d] += rng.integers(-images, images + 1, size=(F, natoms))
        else:
            out = rng.uniform(size=(F, natoms)) < out_frac
            u[:, :, d] += out * rng.choice([-1.0, 1.0], size=(F, natoms))
    fr = np.stack([u[f] @ box_of(boxes, f).T for f in range(F)])
    return fr.astype(dtype)


def scatter_lab(seed, F, n, nbins, lo, hi, out_frac=0.15, dtype=np.float32, origin=None):
    """The same for a LAB grid lo .. hi (relative to `origin` [F, 3] when given): a fraction out_frac one range length outside."""
    rng = np.random.default_rng(seed)
    nbins, lo, hi = np.asarray(nbins), np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ub = rng.integers(0, nbins, size=(F, n, 3))
    u = (ub + 0.5 + rng.uniform(-0.4, 0.4, size=(F, n, 3))) / nbins
    out = rng.uniform(size=(F, n, 3)) < out_frac / 3
    u = u + out * rng.choice([-1.0, 1.0], size=(F, n, 3))
    x = lo + u * (hi - lo)
    if origin is not None:
        x = x + np.asarray(origin)[:, None, :]
    return x.astype(dtype)


def slab(seed, F, npairs, nz, z0, boxes=ORTHO, half_width=0.2, shift=None, dtype=np.float32):
    """A slab for a z profile of nz (even) bins centred on itself: npairs pairs of atoms at fractional z = z0[f] +- delta, each
    delta a bin centre plus jitter counted from the slab's middle, so the circular mean is z0[f] by symmetry (to the rounding
    of the coordinates) and every atom sits 0.1 bin widths or more from an edge of the CENTRED grid.  x and y are uniform.
    The pairs are the same in every frame.  shift [F, 3]: fractional translations added per frame.  Returns frames
    [F, 2 npairs, 3] (atom 2 i and 2 i + 1 form pair i) and the per-pair weights helper is up to the caller."""
    rng = np.random.default_rng(seed)
    assert nz % 2 == 0
    kmax = max(1, int(half_width * nz))
    k = rng.integers(0, kmax, size=npairs)
    delta = (k + 0.5 + rng.uniform(-0.4, 0.4, size=npairs)) / nz
    xy = rng.uniform(0.05, 0.95, size=(2 * npairs, 2))
    u = np.zeros((F, 2 * npairs, 3))
    for f in range(F):
        u[f, :, :2] = xy
        u[f, 0::2, 2] = z0[f] + delta
        u[f, 1::2, 2] = z0[f] - delta
        if shift is not None:
            u[f] += np.asarray(shift)[f][None]
    fr = np.stack([u[f] @ box_of(boxes, f).T for f in range(F)])
    return fr.astype(dtype)


# ---------------------------------------------------------------- the C entry spelt out

def addr_of(x, keep, dtype=None):
    """The address of a numpy array (made contiguous, of dtype) or a torch tensor; None -> None."""
    if x is None:
        return None
    if type(x).__module__.startswith("torch"):
        keep.append(x)
        return x.data_ptr()
    a = np.ascontiguousarray(x, dtype=dtype)
    keep.append(a)
    return a.ctypes.data


def raw_density(fn, ctx, frames, grd, real=np.float32, **kw):
    """The C entry with every argument spelt out: numpy arrays go as host memory, torch CUDA tensors as device memory.
    Outputs are passed by name (density, count, outside, centre, binvol) and written in place.  Returns (status, S)."""
    from molar_amd import api
    keep = []
    g = kw.get
    shape = tuple(frames.shape)
    F, natoms = shape[:2]
    gs = api._grid_struct(grd) if grd is not None else None
    S = C.c_int32(-999)
    st = fn(ctx, addr_of(frames, keep, real), g("F", F), g("stride", 3 * natoms), g("natoms", natoms), addr_of(g("idx"), keep, np.uint64), g("n", natoms),
            addr_of(g("weight"), keep, real), addr_of(g("labels"), keep, np.uint32), g("ngroups", 1), addr_of(g("boxes"), keep, real), g("box_stride", 0),
            g("pbc", 7), None if gs is None else C.addressof(gs), addr_of(g("centre_idx"), keep, np.uint64), g("ncentre", 0),
            addr_of(g("centre_weight"), keep, real), *(addr_of(g(k), keep) for k in ("density", "count", "outside", "centre", "binvol")), C.addressof(S))
    return st, S.value


def argument_errors(fn, ctx, real=np.float32):
    """Every error the arguments alone decide: (what, expected status, got status)."""
    fr = np.zeros((4, 5, 3), real)
    box = ORTHO
    ok = grid(BOX, (1, 1, 8))
    rows = [("n == 0", ERR_SIZES, ok, dict(n=0, boxes=box)),
            ("labels with ngroups == 0", ERR_SIZES, ok, dict(labels=[0] * 5, ngroups=0, boxes=box)),
            ("a null grid", ERR_INVALID, None, dict(boxes=box)),
            ("a mode other than the two", ERR_INVALID, grid(2, (1, 1, 8)), dict(boxes=box)),
            ("nbins[d] == 0", ERR_INVALID, grid(BOX, (1, 0, 8)), dict(boxes=box)),
            ("hi <= lo in LAB mode", ERR_INVALID, grid(LAB, (2, 2, 2), (0, 0, 0), (1, 0, 1)), dict()),
            ("centre_dims > 7", ERR_INVALID, grid(BOX, (1, 1, 8), centre_dims=8), dict(boxes=box)),
            ("2^31 bins", ERR_TOO_LARGE, grid(BOX, (2048, 1024, 1024)), dict(boxes=box)),
            ("pbc > 7", ERR_INVALID, ok, dict(pbc=8, boxes=box)),
            ("a box_stride other than 0 and 9", ERR_INVALID, ok, dict(box_stride=3, boxes=box)),
            ("natoms == 0", ERR_INVALID, ok, dict(natoms=0, idx=[0], n=1, boxes=box)),
            ("n > natoms without an index", ERR_INVALID, ok, dict(n=6, boxes=box)),
            ("ncentre > natoms without an index", ERR_INVALID, ok, dict(ncentre=6, boxes=box)),
            ("a stride below 3 natoms", ERR_INVALID, ok, dict(stride=14, boxes=box)),
            ("an index not below natoms", ERR_INVALID, ok, dict(idx=[0, 5], n=2, boxes=box)),
            ("a centre index not below natoms", ERR_INVALID, ok, dict(centre_idx=[7], ncentre=1, boxes=box)),
            ("a label not below ngroups", ERR_INVALID, ok, dict(labels=[0, 1, 2, 1, 0], ngroups=2, boxes=box)),
            ("BOX mode without boxes", ERR_NO_PBC, ok, dict())]
    return [(what, want, raw_density(fn, ctx, fr, g, real, **kw)[0]) for what, want, g, kw in rows]
