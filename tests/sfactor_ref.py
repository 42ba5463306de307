"""numpy reference of the static structure factor (molar_hip_sfactor: the collective density rho_g(m; f) over the reciprocal
lattice of each frame's box, its mean, the partial products S_ab and their shell averages), the acceptance bounds of the GPU
tests, and the inputs those tests share.

The reference follows the definition in include/molar_hip.h by another route than the kernels, in np.longdouble (2^-64 on
x86) throughout:
  * s = inv(box_f) p with a longdouble inverse of the box (msd_ref.ld_inverse: numpy's f64 inverse polished by two Newton
    steps in longdouble);
  * the phase m.s reduced mod 1 in longdouble, one cos and one sin per (atom, m): no powers, no recurrence;
  * every sum by np.sum over the atoms, the frames or the members of a shell.
It ASSERTS on its inputs that the shells are unambiguous: every |q_f(m)| of the canonical half-space lies further from
every shell edge qmin + j dq than EDGE_REL |q| (1e-9; the kernel's |q| carries (9 kappa + 10) u |q|, about 1e-14 here: the
cofactor inverse, three products and two sums per component, the norm, the square root and the factor 2 pi), so that the
membership and shell_count are compared for equality and a kernel that disagrees is wrong, not unlucky.

Bounds (u = 2^-53; eps_out = 2^-24 for the f32 entry, 2^-53 for the f64 entry; f32 inputs are exact in f64, so both entries
are held to one reference).  Quantities of the input, taken from the reference itself, per frame f and group g:
  kappa_f  the largest row sum of |M| |M^-1| of the frame's box;
  smax_f   the largest sum_c |inv_dc| |p_c| over the selected atoms and d: what |s_d| can reach before the floor;
  W_g      sum |w| over the group;  npad_g its atoms rounded up to a multiple of 4;  nsplit_g = ceil(npad_g / atom_chunk);
  |m|_1    |h| + |k| + |l|.
The fractional coordinate: the inverse by cofactors (two products and a difference per cofactor, five roundings in the
determinant, one division: 9, acting through |M^-1| |M| |M^-1|, hence 9 kappa) and s = inv p (three products, two sums: 3):
  ds_f = (9 kappa_f + 3) u smax_f;            s - floor(s) is exact.
A power E^p (the header: runs of SEG = 8 powers, a sincospi at the head of a run, then at most SEG - 1 products with E^1):
  the head's argument t = p0 s rounds once, u p0, a phase error of 2 pi u p0 <= 2 pi u p; sincospi is good to an ulp, 2u per
  component of a number below 1, 3u on the complex value, for the head and for E^1; a complex product of two numbers of
  modulus 1 adds 3u and passes on the 3u of E^1: 6u per step.
  e_pow(p) = u (2 pi p + 3 + 6 (SEG - 1)) = u (2 pi p + 45).
An operand pair: A = X Y is one more complex product (3u), B = w Z two real products (u), their product and the place in the
MFMA chain 2u more; the chain itself adds 2 npad_g terms (Ar Br and Ai Bi, or Ar Bi and Ai Br) and the splits nsplit_g more,
each rounding at most u times the sum of the moduli, W_g:
  E_rho(f, g, m) = W_g u [ 2 pi |m|_1 (ds_f / u + 1) + 3 * 45 + 6 + 2 npad_g + nsplit_g ]
  |rho - ref| <= E_rho + eps_out |ref|        per component (the bound is on the modulus).
Products, from the double rho:  e_ab = |rho_a| E_b + |rho_b| E_a + E_a E_b + 3u |rho_a| |rho_b|  per (frame, m).
  sab:       mean_f e_ab + (Fv + 1) u mean_f |rho_a| |rho_b| + eps_out |ref|      (the chain over the Fv ok frames, the division)
  rho_mean:  mean_f E_rho + (Fv + 1) u mean_f |rho| + eps_out |ref|
  shell:     [ sum over the members of e_ab + (Fv + nmax + 2) u sum over the members of |rho_a| |rho_b| ] / count
             + eps_out |ref|,  nmax the most members of the shell in one frame: a term passes through the chain over the
             members of a frame and the chain over the frames (box_stride 9), or the other way round (box_stride 0).
The reference's own error, a few 2^-64 times the same sums, is a thousandth of these and is left out."""
import collections
import functools

import numpy as np

import msd_ref
from msd_ref import LD, ORTHO, TRICLINIC, box_matrix, ld_inverse

U = 2.0 ** -53
EPS64 = 2.0 ** -53
EPS32 = 2.0 ** -24
SEG = 8                     # powers per run (SF_SEG of sfactor.hip)
ROW_BLOCK, COL_BLOCK = 128, 64
EDGE_REL = 1e-9
ATOM_CHUNK = 64             # the tests' MOLAR_HIP_SFACTOR_ATOM_CHUNK
FRAME_BLOCK = 2             # the tests' MOLAR_HIP_SFACTOR_FRAME_BLOCK
QMIN, DQ = 0.013, 0.37      # shell edges no |q| of the boxes used here comes near (asserted by shell_bins)

TRICLINIC32 = TRICLINIC.astype(np.float32).astype(np.float64)


def miller(hmax):
    H, K, L = (int(v) for v in hmax)
    h, k, l = np.meshgrid(np.arange(H + 1), np.arange(-K, K + 1), np.arange(-L, L + 1), indexing="ij")
    m = np.stack([h.ravel(), k.ravel(), l.ravel()], axis=1).astype(np.int64)
    canonical = (m[:, 0] > 0) | ((m[:, 0] == 0) & (m[:, 1] > 0)) | ((m[:, 0] == 0) & (m[:, 1] == 0) & (m[:, 2] > 0))
    return m, canonical


def pairs_of(G):
    return [(a, b) for a in range(G) for b in range(a, G)]


def qnorm(box9, m):
    """|q(m)| = 2 pi |inv(box)^T m| in longdouble."""
    inv = ld_inverse(box_matrix(box9))
    v = m.astype(LD) @ inv                                 # row vector m times inv: component r = sum_c m_c inv[c][r]
    return 2 * LD(np.pi) * np.sqrt((v * v).sum(axis=1))


def shell_bins(box9, m, canonical, qmin, dq, nshells):
    """The shell of every m under this box (-1: none), asserting that no |q| of the half-space is near an edge."""
    q = qnorm(box9, m)
    edges = LD(qmin) + LD(dq) * np.arange(nshells + 1).astype(LD)
    dist = np.abs(q[canonical, None] - edges[None, :])
    assert np.all(dist > EDGE_REL * np.maximum(q[canonical, None], LD(1e-300))), "a |q| lies on a shell edge: choose another qmin or dq"
    b = np.floor((q - LD(qmin)) / LD(dq)).astype(np.int64)
    b[~canonical] = -1
    b[(b < 0) | (b >= nshells)] = -1
    return b


Result = collections.namedtuple("Result", ["rho", "frame_ok", "rho_mean", "sab", "shell", "shell_count",
                                           "b_rho", "b_mean", "b_sab", "b_shell"])


def reference(frames, boxes, idx, weight, labels, G, hmax, qmin=0.0, dq=0.0, nshells=0, atom_chunk=ATOM_CHUNK, eps_out=EPS32):
    """frames [F, natoms, 3] and boxes [9] or [F, 9] float64 (the exact values of the inputs); idx, weight (per atom), labels
    (per selected atom) or None.  Returns Result: the outputs in float64 (rounded from longdouble) and their bounds."""
    frames = np.asarray(frames, np.float64)
    F, natoms = frames.shape[:2]
    boxes = np.asarray(boxes, np.float64)
    sel = np.arange(natoms) if idx is None else np.asarray(idx).astype(np.int64)
    n = sel.shape[0]
    w = np.ones(n) if weight is None else np.asarray(weight, np.float64)[sel]
    lab = np.zeros(n, np.int64) if labels is None else np.asarray(labels).astype(np.int64)
    m, canonical = miller(hmax)
    Q = m.shape[0]
    m1 = np.abs(m).sum(axis=1).astype(np.float64)
    P = pairs_of(G)
    rho = np.zeros((F, G, Q), dtype=np.clongdouble)
    e_rho = np.zeros((F, G, Q))
    ok = np.ones(F, np.uint32)
    Wg = np.array([np.abs(w[lab == g]).sum() for g in range(G)])
    npad = np.array([(int((lab == g).sum()) + 3) // 4 * 4 for g in range(G)])
    nsplit = -(-npad // atom_chunk)
    for f in range(F):
        box9 = boxes if boxes.ndim == 1 else boxes[f]
        M = box_matrix(box9)
        p = frames[f, sel]
        if not np.all(np.isfinite(p)):
            ok[f] = 0
            rho[f] = complex(np.nan, np.nan)
            continue
        inv = ld_inverse(M)
        s = p.astype(LD) @ inv.T
        kappa = float((np.abs(M) @ np.abs(np.asarray(inv, np.float64))).sum(axis=1).max())
        smax = float((np.abs(p) @ np.abs(np.asarray(inv, np.float64)).T).max())
        ds_over_u = (9.0 * kappa + 3.0) * smax
        ph = s @ m.astype(LD).T                                   # [n, Q]
        ph -= np.floor(ph)
        ang = 2 * LD(np.pi) * ph
        term = (np.cos(ang) - 1j * np.sin(ang)) * w.astype(LD)[:, None]
        for g in range(G):
            rho[f, g] = term[lab == g].sum(axis=0)
            e_rho[f, g] = Wg[g] * U * (2 * np.pi * m1 * (ds_over_u + 1.0) + 3 * 45 + 6 + 2 * npad[g] + nsplit[g])
    good = ok.astype(bool)
    Fv = int(good.sum())
    arho = np.abs(rho).astype(np.float64)
    out_rho = np.stack([rho.real, rho.imag], axis=-1).astype(np.float64)
    b_rho = np.repeat((e_rho + eps_out * arho)[..., None], 2, axis=-1)
    nan = np.full((), np.nan)
    if Fv:
        mean = rho[good].sum(axis=0) / Fv
        rho_mean = np.stack([mean.real, mean.imag], axis=-1).astype(np.float64)
        b_mean = e_rho[good].mean(axis=0) + (Fv + 1) * U * arho[good].mean(axis=0) + eps_out * np.abs(mean).astype(np.float64)
        b_mean = np.repeat(b_mean[..., None], 2, axis=-1)
    else:
        rho_mean = np.full((G, Q, 2), nan)
        b_mean = np.zeros((G, Q, 2))
    prod = np.zeros((F, len(P), Q), dtype=LD)
    e_ab = np.zeros((F, len(P), Q))
    mag = np.zeros((F, len(P), Q))
    for pi, (a, b) in enumerate(P):
        prod[:, pi] = (rho[:, a] * np.conj(rho[:, b])).real
        mag[:, pi] = arho[:, a] * arho[:, b]
        e_ab[:, pi] = arho[:, a] * e_rho[:, b] + arho[:, b] * e_rho[:, a] + e_rho[:, a] * e_rho[:, b] + 3 * U * mag[:, pi]
    if Fv:
        sab_ld = prod[good].sum(axis=0) / Fv
        sab = sab_ld.astype(np.float64)
        b_sab = e_ab[good].mean(axis=0) + (Fv + 1) * U * mag[good].mean(axis=0) + eps_out * np.abs(sab)
    else:
        sab = np.full((len(P), Q), nan)
        b_sab = np.zeros((len(P), Q))
    shell = np.full((len(P), nshells), nan)
    b_shell = np.zeros((len(P), nshells))
    count = np.zeros(nshells, np.uint64)
    if nshells:
        ssum = np.zeros((len(P), nshells), dtype=LD)
        esum = np.zeros((len(P), nshells))
        msum = np.zeros((len(P), nshells))
        nmax = np.zeros(nshells)
        for f in range(F):
            if not good[f]:
                continue
            bins = shell_bins(boxes if boxes.ndim == 1 else boxes[f], m, canonical, qmin, dq, nshells)
            for sb in range(nshells):
                mem = bins == sb
                c = int(mem.sum())
                count[sb] += np.uint64(c)
                nmax[sb] = max(nmax[sb], c)
                ssum[:, sb] += prod[f][:, mem].sum(axis=1)
                esum[:, sb] += e_ab[f][:, mem].sum(axis=1)
                msum[:, sb] += mag[f][:, mem].sum(axis=1)
        has = count > 0
        cnt = count[has].astype(np.float64)
        shell[:, has] = (ssum[:, has] / cnt.astype(LD)).astype(np.float64)
        b_shell[:, has] = (esum[:, has] + (Fv + nmax[has] + 2) * U * msum[:, has]) / cnt + eps_out * np.abs(shell[:, has])
    return Result(out_rho, ok, rho_mean, sab, shell, count, b_rho, b_mean, b_sab, b_shell)


# ---------------------------------------------------------------- the kernel's route restated in float64

def inverse3(M):
    """linalg3.hpp's inverse of a 3 x 3 matrix, operation by operation in float64; M[r][c]."""
    m11, m21, m31, m12, m22, m32, m13, m23, m33 = (M[0, 0], M[1, 0], M[2, 0], M[0, 1], M[1, 1], M[2, 1], M[0, 2], M[1, 2], M[2, 2])
    mi1 = m22 * m33 - m32 * m23
    mi2 = m21 * m33 - m31 * m23
    mi3 = m21 * m32 - m31 * m22
    det = (m11 * mi1 - m12 * mi2) + m13 * mi3
    o = np.empty((3, 3))
    o[0, 0] = mi1 / det
    o[0, 1] = (m13 * m32 - m33 * m12) / det
    o[0, 2] = (m12 * m23 - m22 * m13) / det
    o[1, 0] = -mi2 / det
    o[1, 1] = (m11 * m33 - m31 * m13) / det
    o[1, 2] = (m13 * m21 - m23 * m11) / det
    o[2, 0] = mi3 / det
    o[2, 1] = (m12 * m31 - m32 * m11) / det
    o[2, 2] = (m11 * m22 - m21 * m12) / det
    return o


def layout_of(hmax):
    H, K, L = (int(v) for v in hmax)
    lay = 1 if (L == 0 and K > 0) else 0
    W = 2 * K + 1
    R = W if lay else (H + 1) * W
    Cn = H + 1 if lay else 2 * L + 1
    return lay, W, R, Cn


def _powers(s, lo, hi):
    """E^p, p = lo .. hi, of the phasors of s [n] as the kernel forms them: runs of SEG, a head by cos and sin of
    2 pi (p0 s - floor(p0 s)), then products with E^1.  [n, hi - lo + 1] complex128, the products written out."""
    n = s.shape[0]
    out = np.empty((n, hi - lo + 1), np.complex128)
    e1r, e1i = np.cos(2 * np.pi * s), -np.sin(2 * np.pi * s)
    for q0 in range(0, hi - lo + 1, SEG):
        t = float(lo + q0) * s
        t = t - np.floor(t)
        cr, ci = np.cos(2 * np.pi * t), -np.sin(2 * np.pi * t)
        out[:, q0] = cr + 1j * ci
        for q in range(q0 + 1, min(q0 + SEG, hi - lo + 1)):
            cr, ci = cr * e1r - ci * e1i, cr * e1i + ci * e1r
            out[:, q] = cr + 1j * ci
    return out


def kernel_route(frames, boxes, idx, weight, labels, G, hmax, atom_chunk=ATOM_CHUNK):
    """rho [F, G, Q, 2] float64 by the kernel's route in float64: the cofactor inverse, s - floor(s), the power tables of every
    block of ROW_BLOCK x COL_BLOCK, operands by one complex product, the atoms of a group in selection order in splits of
    atom_chunk, the splits added in order.  (Within a split np.sum stands for the MFMA chain.)"""
    frames = np.asarray(frames, np.float64)
    F, natoms = frames.shape[:2]
    boxes = np.asarray(boxes, np.float64)
    sel = np.arange(natoms) if idx is None else np.asarray(idx).astype(np.int64)
    n = sel.shape[0]
    w = np.ones(n) if weight is None else np.asarray(weight, np.float64)[sel]
    lab = np.zeros(n, np.int64) if labels is None else np.asarray(labels).astype(np.int64)
    H, K, L = (int(v) for v in hmax)
    lay, W, R, Cn = layout_of(hmax)
    Q = (H + 1) * W * (2 * L + 1)
    rows = np.arange(R)
    cols = np.arange(Cn)
    if lay:
        rh, rk = np.zeros(R, np.int64), rows - K
        cp = cols
    else:
        rh, rk = rows // W, rows % W - K
        cp = cols - L
    rho = np.zeros((F, G, Q, 2))
    for f in range(F):
        M = box_matrix(boxes if boxes.ndim == 1 else boxes[f])
        inv = inverse3(M)
        p = frames[f, sel]
        s = np.stack([(inv[d, 0] * p[:, 0] + inv[d, 1] * p[:, 1]) + inv[d, 2] * p[:, 2] for d in range(3)], axis=1)
        s = s - np.floor(s)
        C = np.zeros((G, R, Cn), np.complex128)
        for r0 in range(0, R, ROW_BLOCK):
            rr = slice(r0, min(r0 + ROW_BLOCK, R))
            ak = np.abs(rk[rr])
            Y = _powers(s[:, 1], int(ak.min()), int(ak.max()))[:, ak - ak.min()]
            Y = np.where(rk[rr][None, :] < 0, np.conj(Y), Y)
            if lay:
                A = Y
            else:
                hh = rh[rr]
                X = _powers(s[:, 0], int(hh.min()), int(hh.max()))[:, hh - hh.min()]
                A = (X.real * Y.real - X.imag * Y.imag) + 1j * (X.real * Y.imag + X.imag * Y.real)
            for c0 in range(0, Cn, COL_BLOCK):
                cc = slice(c0, min(c0 + COL_BLOCK, Cn))
                ap = np.abs(cp[cc])
                Z = _powers(s[:, 0 if lay else 2], int(ap.min()), int(ap.max()))[:, ap - ap.min()]
                Z = np.where(cp[cc][None, :] < 0, np.conj(Z), Z)
                B = w[:, None] * Z.real + 1j * (w[:, None] * Z.imag)
                for g in range(G):
                    members = np.nonzero(lab == g)[0]
                    acc = np.zeros((rr.stop - rr.start, cc.stop - cc.start), np.complex128)
                    for k0 in range(0, len(members), atom_chunk):
                        mm = members[k0:k0 + atom_chunk]
                        Ar, Ai, Br, Bi = A[mm].real, A[mm].imag, B[mm].real, B[mm].imag
                        acc = acc + ((Ar.T @ Br - Ai.T @ Bi) + 1j * (Ar.T @ Bi + Ai.T @ Br))
                    C[g, rr, cc] = acc
        if not np.all(np.isfinite(p)):
            rho[f] = np.nan
            continue
        flat = C.transpose(0, 2, 1).reshape(G, Q) if lay else C.reshape(G, Q)
        rho[f, :, :, 0] = flat.real
        rho[f, :, :, 1] = flat.imag
    return rho


# ---------------------------------------------------------------- shared inputs

Case = collections.namedtuple("Case", ["name", "natoms", "F", "hmax", "box", "G", "idx", "signed", "nshells", "qmin", "dq"])


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """(frames [F, natoms, 3] float32, boxes float32 [9] or [F, 9], idx or None, weight float32 [natoms] or None, labels or
    None) of a case: positions from half a box below to half a box above the cell, weights of both signs when `signed`,
    labels unsorted with group 1 empty, group 0 of one atom and the rest in group 2 when G == 3."""
    rng = np.random.default_rng(sum(case.name.encode()) * 7919 + case.natoms)
    base = {"ortho": ORTHO, "tric": TRICLINIC32, "scaled": ORTHO, "scaled_tric": TRICLINIC32}[case.box]
    if case.box.startswith("scaled"):
        boxes = msd_ref.scaled_boxes(case.F, 5, base).astype(np.float32)
    else:
        boxes = base.astype(np.float32)
    M = box_matrix(base)
    frac = rng.uniform(-0.5, 1.5, size=(case.F, case.natoms, 3))
    frames = np.ascontiguousarray((frac @ M.T).astype(np.float32))
    idx = None
    n = case.natoms
    if case.idx:
        idx = rng.permutation(case.natoms)[:max(1, (2 * case.natoms) // 3)].astype(np.uint64)
        n = idx.shape[0]
    weight = None
    if case.signed:
        weight = rng.uniform(0.5, 2.0, size=case.natoms) * np.where(rng.random(case.natoms) < 0.35, -1.0, 1.0)
        weight = weight.astype(np.float32)
    labels = None
    if case.G == 3:
        labels = np.full(n, 2, np.uint32)
        labels[n // 2] = 0                                      # a group of one atom, not at the front; group 1 stays empty
    elif case.G > 1:
        labels = rng.integers(0, case.G, size=n).astype(np.uint32)
    return frames, boxes, idx, weight, labels


@functools.lru_cache(maxsize=None)
def case_reference(case, eps_out):
    frames, boxes, idx, weight, labels = case_inputs(case)
    return reference(frames, boxes, idx, weight, labels, case.G, case.hmax, case.qmin, case.dq, case.nshells, ATOM_CHUNK, eps_out)


def C(name, natoms, F, hmax, box="ortho", G=1, idx=False, signed=False, nshells=0, qmin=QMIN, dq=DQ):
    return Case(name, natoms, F, tuple(hmax), box, G, idx, signed, nshells, qmin, dq)


# the sizes at which the kernels take another path: atoms around a multiple of 4 and of atom_chunk (64), rows and columns
# around the tiles (16) and the blocks (128 x 64), both layouts and K = L = 0, frames around frame_block (2)
ATOM_CASES = [C(f"atoms{n}", n, 1, (2, 2, 2), signed=True) for n in (1, 3, 4, 5, 63, 64, 65, 131)]
SHAPE_CASES = [
    C("rows1_cols15", 9, 1, (0, 0, 7)),
    C("rows15_cols17", 9, 1, (4, 1, 8), box="tric"),
    C("rows16_cols3", 9, 1, (15, 0, 1)),
    C("rows17_cols65", 7, 1, (0, 8, 32)),
    C("rows127_cols3", 7, 1, (0, 63, 1)),
    C("rows129_cols3", 7, 1, (2, 21, 1), box="tric"),
    C("lat_rows15_cols16", 9, 1, (15, 7, 0)),
    C("lat_rows17_cols1", 9, 1, (0, 8, 0), box="tric"),
    C("lat_rows127_cols65", 5, 1, (64, 63, 0)),
    C("lat_rows129_cols15", 5, 1, (14, 64, 0)),
    C("profile_rows21", 9, 1, (20, 0, 0)),
]
FRAME_CASES = [C(f"frames{F}", 21, F, (2, 2, 1), box="scaled", G=3, signed=True, nshells=6) for F in (1, 2, 3)]
GROUP_CASES = [
    C("groups3_tric", 70, 3, (3, 2, 2), box="tric", G=3, idx=True, signed=True, nshells=8),
    C("groups3_scaled_tric", 23, 3, (2, 3, 2), box="scaled_tric", G=3, signed=True, nshells=8),
    C("groups2_lateral", 150, 3, (5, 5, 0), box="scaled", G=2, idx=True, signed=True, nshells=12),
    C("one_shell", 11, 2, (2, 2, 2), box="ortho", nshells=1, dq=10 * DQ),      # one shell that holds the first lattice points
]
ALL_CASES = ATOM_CASES + SHAPE_CASES + FRAME_CASES + GROUP_CASES


def fraction(got, ref, bound):
    """The largest |got - ref| / bound where both are finite; NaN positions must coincide."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN positions differ"
    fin = ~np.isnan(ref)
    exact = fin & (bound == 0.0)                      # an empty group: nothing was added, nothing may differ
    assert np.array_equal(got[exact], ref[exact]), "an entry with a bound of 0 differs"
    fin &= bound > 0.0
    if not fin.any():
        return 0.0
    return float((np.abs(got[fin] - ref[fin]) / bound[fin]).max())


# ---------------------------------------------------------------- the C entries called directly (argument errors)

ERR_SIZES, ERR_NO_PBC, ERR_ZERO_LENGTH, ERR_INVERSE, ERR_INVALID, ERR_TOO_LARGE = 1, 4, 5, 6, 50, 51


def raw_sfactor(fn, ctx, real, F=2, natoms=5, stride=None, idx=None, n=None, weight=None, labels=None, ngroups=1, boxes="ortho", box_stride=0,
                hmax=(1, 1, 1), qmin=0.0, dq=0.1, nshells=0, reserved=0, grid=True, rho_stride=None, want_rho=False, frames=True):
    """One call with host arrays made here; returns the status.  No output is given unless want_rho."""
    import ctypes as C
    from molar_amd import _lib
    fr = np.ones((max(F, 1), natoms, 3), real)
    g = _lib.SfactorGrid()
    for d in range(3):
        g.hmax[d] = hmax[d]
    g.qmin, g.dq, g.nshells, g.reserved = qmin, dq, nshells, reserved
    keep = [fr, g]

    def ptr(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dt)
        keep.append(a)
        return a.ctypes.data

    bx = None if boxes is None else ptr(ORTHO if isinstance(boxes, str) else boxes, real)
    Q = (hmax[0] + 1) * (2 * hmax[1] + 1) * (2 * hmax[2] + 1)
    nsel = (natoms if idx is None else len(idx)) if n is None else n
    rho = np.zeros((max(F, 1), max(ngroups, 1), Q, 2), real) if want_rho else None
    keep.append(rho)
    return fn(ctx, fr.ctypes.data if frames else None, F, 3 * natoms if stride is None else stride, natoms, ptr(idx, np.uint64), nsel, ptr(weight, real),
              ptr(labels, np.uint32), ngroups, bx, box_stride, C.addressof(g) if grid else None, None if rho is None else rho.ctypes.data,
              2 * Q if rho_stride is None else rho_stride, None, None, None, None, None)


def argument_errors(fn, ctx, real):
    """(what, expected status, status) of every error of the arguments alone."""
    r = lambda **kw: raw_sfactor(fn, ctx, real, **kw)
    return [
        ("empty selection", ERR_SIZES, r(n=0)),
        ("labels with ngroups = 0", ERR_SIZES, r(labels=[0] * 5, ngroups=0)),
        ("null grid", ERR_INVALID, r(grid=False)),
        ("reserved", ERR_INVALID, r(reserved=1)),
        ("hmax 2^10", ERR_TOO_LARGE, r(hmax=(1024, 0, 0))),
        ("dq = 0 with shells", ERR_INVALID, r(nshells=3, dq=0.0)),
        ("dq < 0 with shells", ERR_INVALID, r(nshells=3, dq=-1.0)),
        ("dq not finite with shells", ERR_INVALID, r(nshells=3, dq=float("inf"))),
        ("qmin not finite with shells", ERR_INVALID, r(nshells=3, qmin=float("nan"))),
        ("box_stride 3", ERR_INVALID, r(box_stride=3)),
        ("natoms = 0", ERR_INVALID, r(natoms=0, n=1)),
        ("n > natoms without an index", ERR_INVALID, r(n=6)),
        ("stride below 3 natoms", ERR_INVALID, r(stride=14)),
        ("rho_stride below 2 Q", ERR_INVALID, r(want_rho=True, rho_stride=35)),
        ("no box", ERR_NO_PBC, r(boxes=None)),
        ("G Q >= 2^31", ERR_TOO_LARGE, r(hmax=(1023, 1023, 1023))),
        ("G Q >= 2^31 by the groups", ERR_TOO_LARGE, r(labels=[0] * 5, ngroups=2 ** 26, hmax=(3, 3, 3))),
        ("host index not below natoms", ERR_INVALID, r(idx=[0, 5])),
        ("host label not below ngroups", ERR_INVALID, r(labels=[0, 1, 2, 0, 0], ngroups=2)),
        ("null frames", ERR_INVALID, r(frames=False)),
    ]


def cubic_lattice(c, box9=ORTHO, offset=0.0):
    """c^3 atoms on a simple cubic lattice of the box, fractional (i + offset) / c: positions [c^3, 3] float64."""
    g = (np.arange(c) + offset) / c
    frac = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return frac @ box_matrix(box9).T
