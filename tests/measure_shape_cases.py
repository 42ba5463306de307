"""Inputs, references and bounds that aim the Measure entry points (measure.hip, measure_f64.hip) at their launch shapes.
Importable without a GPU: tests/test_measure_shape_cases_cpu.py checks the cases themselves, tests/test_gpu_measure_shapes.py
runs the engine against them.

1. The launch arithmetic, mirrored (C = compute units)
------------------------------------------------------
single-frame reductions (blocks_for(.., 1), blocks64): nb = min(ceil(n / 1024), 4 C) workgroups of 256 threads, every thread
walks k = block * 256 + thread, += nb * 256 - up to four trips below the cap (1023 or 65 536 atoms make four already), five
at 4096 C + 1 and nine at 2 * 4096 C + 257, where the last one ends inside its second workgroup; the finalisers (k_fin_sum,
k_fit_final, k64_total) add the nb partial records 64 at a time.  fit_rmsd_batch (f32): 2048 atoms per workgroup from 8 frames on, at most 16 workgroups from 64 frames on, the
packed kernels from 4 frames on, four atoms `stride` apart per trip with one guard each.  fit_rmsd_batch_f64: nb =
min(ceil(n / 2048), 64).  CSR kernels: one wave per selection in steps of 64 atoms, four waves per workgroup.  lipid order:
16 tails per workgroup in f32, 64 in f64.  `single_shape`, `fit32_shape`, `fit64_shape`, `csr_shape`, `lipid_shape` return
these numbers; the CPU test asserts what every case claims about them for C = 64 and C = 256.

2. Exact sums
-------------
Coordinates are integers / 8 with |x| <= 64, masses integers 1..32 (`UNIT`, `XMAX`, `SENT_MASS`).  Then every term the
kernels accumulate without a rounded centre in it - m, m p, p, m p p^T, |p2 - p1|^2, m |p2 - p1|^2, m q p^T - is an integer
multiple of 2^-6 far below 2^24 (f32) resp. 2^53 (f64) times that, so the f32 products are exact (the CPU test multiplies
them out in float32 and compares) and every f64 partial sum is exact whatever its grouping: n <= 2^22 terms of at most
2^5 * 2^20 / 2^6.  (For |p2 - p1|^2 * m the bulk displacement is kept small and the sentinels' mass is a power of two.)
The references are these sums in integer arithmetic (numpy int64, then Python integers / Fractions), each output derived
from them as an exact rational and rounded once (`float(Fraction)` is correctly rounded).

Periodic entries: an orthorhombic box with edge 512 = 2^9, coordinates wrapped into [0, 512).  1 / 512 and every
v / 512, round, v - 512 k are exact for multiples of 1/8 below 2^10, so closest_image(p, p0) is the exact image and the
periodic centres are sums of exact terms as well; the cluster is 128 wide, so no difference sits on the tie L / 2.  In
`E` coordinates (the images relative to the first selected atom; raw wrapped values in a dimension that is not periodic)
the periodic outputs are the plain formulas with the reference's centre quirk (the first position enters unweighted,
measure.rs:197-220): c = (S m E - (m0 - 1) E0) / M.  One triclinic case per periodic entry stays at the project's
tolerances against the f64 oracle (`triclinic_case`).

3. Bounds (what remains after exact sums), U32 = 2^-23, U64 = 2^-53
-------------------------------------------------------------------
f32 engine, value computed in f64 from exact sums and cast: the cast is half an ulp, the f64 division / root 2^-53.
  centres (plain and periodic)      U32 |ref|                       (one f32 ulp; S / M and the cast)
  rmsd, rmsd_mw                     U32 ref                         (sqrt(S / n) in f64, cast)
  gyration, inertia tensor          U32 |ref| + e                   the engine centres S m p p^T on the f32-ROUNDED centre c:
                                                                    S m |p - c|^2 = exact + M |c - c_true|^2 <= M (2^-24 |c|)^2,
                                                                    and ((raw - c S) - S c) + M c c loses <= 8 * 2^-53 of raw:
                                                                    e(Rg^2) = 2^-46 |c|^2 + 2^-49 (S m |p|^2 / M + |c|^2),
                                                                    e(T) = M e(Rg^2); a root turns e into `root_err`.
  periodic gyration / inertia       the terms m |d|^2 ARE rounded in f32.  First d = fl(p - c): the kernel subtracts the
                                    centre from the WRAPPED coordinate, so the half ulp is that of |p_wrapped - c|, up to
                                    2^-16 for an atom wrapped to ~500, however small the image d is after the (exact)
                                    shift by a box edge.  Its cost is taken from the data, not from a relative figure:
                                    e_d = sum_k m_k (2 |d_k|_1 delta_k + 3 delta_k^2) (`difference_error`), which bounds
                                    the movement of S m |d|^2 and of every tensor sum.  Then, on the rounded d: square,
                                    two additions, product with m, 4 * 2^-24 per non-negative term, hence of their exactly
                                    accumulated sum; Rg: half of that plus the cast, 3 * 2^-24; stated as 2^-21 ref
                                    (8 * 2^-24), tensor entries 2^-21 S m |d|^2.  Together: 2^-21 ref + root_err(e_d / M).
                                    The reference uses c = the correctly rounded f32 of the exact quirk centre; the
                                    engine's f64-then-f32 rounding may differ by one ulp(c): e(Rg^2) = 2 |c - com| ulp32(c)
                                    (first order, the centre is off the centre of mass by the quirk) is added.
f64 engine: sums of exact terms are exact: centres 2 U64 |ref| (division, and the reference's own rounding), rmsd
  4 U64 ref.  Gyration / inertia are centred per term on the f64 centre: each term carries <= 6 U64, every addition on
  the path of a term U64 more: D = trips per thread + 6 (wave) + 4 (workgroup) + finaliser trips + 6 (wave) additions, so
  (D + 16) U64 relative on sums of non-negative terms (the 16: the term itself, division, root, the reference); tensor entries
  (D + 16) U64 S m |d|^2 + 2^-50 M |c|^2 (centre rounding, first order zero).  "6 U64 per term" holds where d = p - c
  is formed from the coordinate itself (no box); with a box the difference is rounded at the scale of the wrapped
  coordinate, and e_d (above, with f64 half ulps) is added to the periodic f64 bounds as well.
fit_rmsd_batch: gyration of the fitted selection is rotation invariant and gets the gyration bound (f32: from uncentred
  exact sums; f64: S m |p - c1|^2 centred per term, (D + 16) U64).
Rotation-dependent outputs keep the project's tolerances (R_ATOL32 .. below): R, t, the centre of mass and the RMSD after
a fit (the RMSD is unweighted but the fit mass-weighted, so it is not stationary in R), inertia moments / axes through
A diag(m) A^T.  translate, apply_transform, unwrap_simple, min_max are compared bit for bit with the oracle.

4. Sentinels and the one-atom condition
---------------------------------------
`stride_probes(n, start)`: first and last element of every 256-atom block - every workgroup's range in every grid-stride
segment, which contains the first and last element of every trip of the four-atom loop and of every segment - and n - 1;
for start = 0 and for start = 1, where the periodic kernels' loops begin (element 0 is their anchor).
`csr_probes`: first and last element of every 64-lane step of a selection.  The atoms there carry mass 32 and sit on the
corners (+-64, +-64, +-64), all eight in turn, so their centre stays at the origin; the bulk has |x| <= 8 and masses 1..8;
atoms outside the selection sit at +-62.5 with mass 31.  The CPU test removes each probed element from the sums and counts
it twice and requires, per kernel family, an output that moves by >= 16 bounds.  With ONE atom both are void (nothing left /
every output is a ratio that does not change), so n = 1 is exempt; min_max, whose extremes are shared by many sentinels,
and the data-movement entries are exact comparisons of every element instead.  Of a fit, only the gyration radius (the
frame's gather) is that sharp; the reference selection's gather is seen through R, t and the RMSD at their tolerances."""
import functools
import math
from fractions import Fraction

import numpy as np

RB = 256
UNIT = 8                     # coordinates are integers / UNIT
XMAX = 64 * UNIT             # |x| <= 64
BULK = 8 * UNIT              # the bulk: |x| <= 8
SENT_MASS = 32
BOX_EDGE = 512               # power of two; 4096 units
U32 = 2.0 ** -23
U64 = 2.0 ** -53
SENS = 16                    # a probed atom must move an output by this many bounds

# the project's tolerances for rotation-dependent outputs (tests/test_gpu_measure.py, tests/test_gpu_measure_f64.py)
R_ATOL32, T_RTOL32, T_ATOL32 = 1e-5, 1e-5, 2e-4
RMSD_FIT_RTOL32 = 1e-5
AXES_RTOL32 = 1e-4
RTOL_ROT64 = 1e-10
RMSD_FIT_RTOL64 = 1e-9
COM_FIT_ATOL64 = 1e-11 * 20
AXES_ATOL64 = 1e-10
CSR_R_ATOL32, CSR_T_ATOL32, CSR_RMSD_RTOL32 = 2e-5, 2e-4, 2e-5
PBC_GYR_BATCH_RTOL32 = 2e-5

FIXED_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 65536, 65537)
SIZE_KEYS = ("2*4096C+257", "4096C+1", "4096C") + tuple(str(n) for n in FIXED_SIZES)     # largest first, then 1, the rest


def size_of(key, C):
    return {"4096C": 4096 * C, "4096C+1": 4096 * C + 1, "2*4096C+257": 2 * 4096 * C + 257}.get(key) or int(key)


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ launch mirror

def single_shape(C, n, start=0):
    """blocks_for(c, n, 1) / blocks64(c, n) and the loops behind them; start = 1 for the periodic kernels (k = 1 + ...)."""
    want = max(1, cdiv(n, 4 * RB))
    nb = min(want, 4 * C)
    stride = nb * RB
    return dict(nb=nb, capped=want > 4 * C, stride=stride, trips=cdiv(max(n - start, 0), stride), fin_trips=cdiv(nb, 64))


def fit32_shape(C, n, F):
    """molar_hip_fit_rmsd_batch: blocks_for(c, n, F), k_fit_sums(_packed)'s four-atom trips, k_fit_final's loop."""
    per = 8 if F >= 8 else 4
    want = max(1, cdiv(n, RB * per))
    cap = 16 if F >= 64 else 4 * C
    nb = min(want, cap)
    stride = nb * RB
    whole, rest = divmod(n, 4 * stride)
    return dict(nb=nb, capped=want > cap, cap16=F >= 64, per=per, packed=F >= 4, stride=stride, trips=cdiv(n, 4 * stride),
                whole_trips=whole, partial_trip=rest > 0,
                mixed_guards=rest > 0 and rest % stride != 0,           # within one `u` some threads are on, some off
                fin_trips=cdiv(nb, 64))


def fit64_shape(n):
    want = max(1, cdiv(n, RB * 8))
    nb = min(want, 64)
    return dict(nb=nb, capped=want > 64, stride=nb * RB, trips=cdiv(n, nb * RB), fin_trips=cdiv(nb, 64))


def csr_shape(sizes):
    return dict(nb=cdiv(len(sizes), 4), idle_waves=(-len(sizes)) % 4, steps=[cdiv(int(s), 64) for s in sizes])


def lipid_shape(ntails, per_block):
    return dict(nb=cdiv(ntails, per_block), idle=(-ntails) % per_block)


def depth64(sh):
    """additions on the path of one term through an f64 reduction (see 3.)"""
    return sh["trips"] + 6 + 4 + sh["fin_trips"] + 6


def stride_probes(n, start=0):
    b0 = np.arange(start, n, RB, dtype=np.int64)
    last = np.minimum(b0 + RB, n) - 1
    return np.unique(np.concatenate([b0, last, [n - 1]])) if n > start else np.array([n - 1], np.int64)


def csr_probes(size):
    b0 = np.arange(0, size, 64, dtype=np.int64)
    return np.unique(np.concatenate([b0, np.minimum(b0 + 64, size) - 1]))


def corners(j):
    j = np.asarray(j, np.int64)
    return XMAX * np.stack([1 - 2 * (j & 1), 1 - 2 * ((j >> 1) & 1), 1 - 2 * ((j >> 2) & 1)], -1)


# ------------------------------------------------------------------------------------------------ inputs

ROT90 = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.int64)          # exact on the grid
SHIFT2 = np.array([8, -16, 24], np.int64)                               # (1, -2, 3) nm


def _selection(rng, natoms, n):
    keep = np.ones(natoms, bool)
    keep[rng.choice(natoms, natoms - n, replace=False)] = False           # (the few that leave: cheaper than drawing the many)
    return np.flatnonzero(keep).astype(np.int64)


def _fill(rng, natoms, sel, probes):
    """frame and mass column: bulk, sentinels on the probed positions of the selection, far heavy atoms outside it"""
    X = rng.integers(-BULK, BULK + 1, (natoms, 3)).astype(np.int64)
    mass = rng.integers(1, 9, natoms).astype(np.int64)
    outside = np.ones(natoms, bool)
    outside[sel] = False
    X[outside] = rng.choice([-500, 500], (int(outside.sum()), 3))
    mass[outside] = 31
    X[sel[probes]] = corners(np.arange(len(probes)))
    mass[sel[probes]] = SENT_MASS
    return X, mass


@functools.lru_cache(maxsize=2)
def system(n, with_idx):
    """Two frames and a mass column for the single-call entries.  with_idx: natoms > n, two different sorted index sets with
    gaps (frame 2 is gathered through its own); else the identity selection (idx = None)."""
    rng = np.random.default_rng(7919 * n + (1 if with_idx else 0))
    natoms = n + n // 4 + 5 if with_idx else n
    sel = _selection(rng, natoms, n) if with_idx else np.arange(n, dtype=np.int64)
    sel2 = _selection(rng, natoms, n) if with_idx else sel
    probes, pbc_probes = stride_probes(n), stride_probes(n, 1)           # the periodic kernels' loops start at k = 1
    X1, mass = _fill(rng, natoms, sel, np.union1d(probes, pbc_probes))
    X2 = rng.choice([-500, 500], (natoms, 3)).astype(np.int64)
    X2[sel2] = X1[sel] @ ROT90.T + SHIFT2 + rng.integers(-2, 3, (n, 3))
    Xw = X1 % (BOX_EDGE * UNIT)                                           # wrapped into [0, 512)
    s = dict(n=n, natoms=natoms, with_idx=with_idx, sel=sel, sel2=sel2, probes=probes, pbc_probes=pbc_probes[pbc_probes > 0],
             X1=X1, X2=X2, Xw=Xw, mass=mass)
    # the integer sums and the probed atoms' own terms, once per system (element 0 is the periodic anchor, no term of the loop)
    A, B, m, pp = X1[sel], X2[sel2], mass[sel], s["pbc_probes"]
    s["sums"] = dict(plain=(term_sums(A, m, B), terms(A[probes], m[probes], B[probes])))
    for dims in (7, 3):
        E = pbc_coords(s, dims)
        s["sums"][dims] = (term_sums(E, m), terms(E[pp], m[pp]), E[0].copy())
        if dims == 7:
            s["E7"] = E.astype(np.int32)
    return s


def as_real(X, dtype):
    return np.ascontiguousarray(np.asarray(X, np.float64) / UNIT, dtype=dtype)


def idx_arg(s, which="sel"):
    return s[which].astype(np.uint64) if s["with_idx"] else None


BOX = np.diag([float(BOX_EDGE)] * 3)


def pbc_coords(s, dims):
    """E: the images relative to the first selected atom (exact integers), raw wrapped values where not periodic"""
    sel = s["sel"]
    A, W = s["X1"][sel], s["Xw"][sel]
    off = W[0] - A[0]                                                    # 0 or one box edge per component
    E = A + off
    for d in range(3):
        if not (dims >> d) & 1:
            E[:, d] = W[:, d]
    assert (np.abs(A - A[0]) < BOX_EDGE * UNIT // 2).all()               # no image on the tie
    return E


# ------------------------------------------------------------------------------------------------ exact sums

PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def _columns(A, m, B=None):
    A = np.asarray(A, np.int64)
    m = np.asarray(m, np.int64)
    cols = [m, np.ones_like(m)] + [m * A[:, d] for d in range(3)] + [A[:, d] for d in range(3)]
    cols += [m * A[:, a] * A[:, b] for a, b in PAIRS]
    if B is not None:
        d2 = ((np.asarray(B, np.int64) - A) ** 2).sum(1)
        cols += [d2, d2 * m]
    else:
        cols += [np.zeros_like(m), np.zeros_like(m)]
    return cols


def terms(A, m, B=None):
    """per-atom integer terms, columns: m, N, S1(3), P(3), S2(6), D2, D2m"""
    return np.stack(_columns(A, m, B), 1)


def term_sums(A, m, B=None):
    """the column sums of `terms` without the table"""
    return np.array([int(c.sum()) for c in _columns(A, m, B)], np.int64)


def pack(row, frac):
    """a row of `terms` columns (summed) as the dict `derive` takes; frac: exact rationals, else float arrays"""
    f = (lambda v: Fraction(int(v))) if frac else (lambda v: np.asarray(v, np.float64))
    r = [f(row[..., i]) for i in range(row.shape[-1])]
    return dict(M=r[0], N=r[1], S1=r[2:5], P=r[5:8], S2=r[8:14], D2=r[14], D2m=r[15])


def variants(tot, rows):
    """sums with each probed element (its terms: rows) removed, then with each counted twice: float dict of arrays [2 K]"""
    return pack(np.concatenate([tot - rows, tot + rows]), False)


def derive(S):
    """outputs in nm from sums in grid units; squares where the engine takes a root.  Field operations only: exact on
    Fractions, elementwise on float arrays."""
    M, N = S["M"], S["N"]
    com = [S["S1"][d] / M for d in range(3)]
    tr = S["S2"][0] + S["S2"][1] + S["S2"][2]
    cc = com[0] * com[0] + com[1] * com[1] + com[2] * com[2]
    c2 = [S["S2"][i] - M * com[a] * com[b] for i, (a, b) in enumerate(PAIRS)]
    u2 = UNIT * UNIT
    return dict(cog=[S["P"][d] / N / UNIT for d in range(3)], com=[c / UNIT for c in com],
                rg2=(tr / M - cc) / u2, raw2=tr / M / u2, cc=cc / u2, M=M,
                tensor=[(c2[1] + c2[2]) / u2, (c2[0] + c2[2]) / u2, (c2[0] + c2[1]) / u2, -c2[3] / u2, -c2[4] / u2, -c2[5] / u2],
                msd=S["D2"] / N / u2, msd_mw=S["D2m"] / M / u2)


def derive_pbc(S, m0, E0, centre=None):
    """periodic centres with the reference's quirk; gyration / tensor about `centre` (grid units; default: the quirk centre)"""
    M, N = S["M"], S["N"]
    cq = [(S["S1"][d] - (m0 - 1) * int(E0[d])) / M for d in range(3)]
    c = cq if centre is None else centre
    com = [S["S1"][d] / M for d in range(3)]
    c2 = [S["S2"][i] - c[a] * S["S1"][b] - S["S1"][a] * c[b] + M * c[a] * c[b] for i, (a, b) in enumerate(PAIRS)]
    u2 = UNIT * UNIT
    return dict(cog=[S["P"][d] / N / UNIT for d in range(3)], com=[x / UNIT for x in cq],
                rg2=(c2[0] + c2[1] + c2[2]) / M / u2, smd2=(c2[0] + c2[1] + c2[2]) / u2, M=M,
                off=[(c[d] - com[d]) / UNIT for d in range(3)], centre=[x / UNIT for x in c],
                tensor=[(c2[1] + c2[2]) / u2, (c2[0] + c2[2]) / u2, (c2[0] + c2[1]) / u2, -c2[3] / u2, -c2[4] / u2, -c2[5] / u2])


def rounded_centre(cq_nm, dtype):
    """the engine's centre: the exact quirk centre rounded to the working precision, back in grid units as rationals"""
    return [Fraction(float(dtype(float(x)))) * UNIT for x in cq_nm]


def root_err(a, e):
    """|sqrt(a') - sqrt(a)| for |a' - a| <= e"""
    a, e = float(a), float(e)
    return math.sqrt(a + e) if a <= e else e / (math.sqrt(a) + math.sqrt(a - e))


def fl(x):
    return float(x)


def vec(v):
    return np.array([float(x) for x in v])


def ulp32(x):
    return float(np.spacing(np.float32(abs(float(x)))))


# ------------------------------------------------------------------------------------------------ references with bounds

def plain_reference(o, prec, sh):
    """{name: (value, bound)} of the non-periodic outputs from derive() on exact Fractions; sh: single_shape (f64 depth)"""
    rg = math.sqrt(fl(o["rg2"]))
    tens = vec(o["tensor"])
    M = fl(o["M"])
    if prec == 32:
        e = 2.0 ** -46 * fl(o["cc"]) + 2.0 ** -49 * (fl(o["raw2"]) + fl(o["cc"]))
        return dict(cog=(vec(o["cog"]), U32 * np.abs(vec(o["cog"]))), com=(vec(o["com"]), U32 * np.abs(vec(o["com"]))),
                    gyration=(rg, U32 * rg + root_err(o["rg2"], e)), tensor=(tens, U32 * np.abs(tens) + M * e),
                    rmsd=(math.sqrt(fl(o["msd"])), U32 * math.sqrt(fl(o["msd"]))),
                    rmsd_mw=(math.sqrt(fl(o["msd_mw"])), U32 * math.sqrt(fl(o["msd_mw"]))))
    k = (depth64(sh) + 16) * U64
    return dict(cog=(vec(o["cog"]), 2 * U64 * np.abs(vec(o["cog"]))), com=(vec(o["com"]), 2 * U64 * np.abs(vec(o["com"]))),
                gyration=(rg, k * rg), tensor=(tens, np.full(6, k * M * fl(o["rg2"]) + 2.0 ** -50 * M * fl(o["cc"]))),
                rmsd=(math.sqrt(fl(o["msd"])), 4 * U64 * math.sqrt(fl(o["msd"]))),
                rmsd_mw=(math.sqrt(fl(o["msd_mw"])), 4 * U64 * math.sqrt(fl(o["msd_mw"]))))


def pbc_centre_reference(o, prec):
    u = U32 if prec == 32 else 2 * U64
    return dict(cog_pbc=(vec(o["cog"]), u * np.abs(vec(o["cog"]))), com_pbc=(vec(o["com"]), u * np.abs(vec(o["com"]))))


def difference_error(s, centre_nm, dtype):
    """e_d: what the rounding of d = fl(p - c) costs the periodic sums, from the data.  The kernel subtracts the centre from
    the WRAPPED coordinate, so the half ulp is that of |p_wrapped - c| (up to 512) however small the image d is afterwards
    (the shift by a box edge is exact).  With delta_k the largest of an atom's three half ulps, every term m d_a d_b moves by
    at most m (|d_a| + |d_b|) delta + m delta^2, hence each of S m |d|^2 and the six tensor sums by at most
    sum_k m_k (2 |d_k|_1 delta_k + 3 delta_k^2)."""
    sel = s["sel"]
    c = np.array([float(x) for x in centre_nm])
    pre = np.abs(s["Xw"][sel] / UNIT - c)
    delta = (0.5 * np.spacing(pre.astype(dtype)).astype(np.float64)).max(1)
    d1 = np.abs(s["E7"] / UNIT - c).sum(1)
    return float((s["mass"][sel] * (2.0 * d1 * delta + 3.0 * delta * delta)).sum())


def pbc_central_reference(o, prec, sh, e_d):
    """gyration / inertia with a box: o = derive_pbc(.., centre=rounded_centre(..)), e_d = difference_error(..)"""
    rg = math.sqrt(fl(o["rg2"]))
    tens = vec(o["tensor"])
    M, smd2 = fl(o["M"]), fl(o["smd2"])
    if prec == 32:
        e = 2.0 * sum(abs(fl(x)) * ulp32(c) for x, c in zip(o["off"], o["centre"]))
        return dict(gyration_pbc=(rg, 2.0 ** -21 * rg + root_err(o["rg2"], e + e_d / M)),
                    tensor_pbc=(tens, U32 * np.abs(tens) + 2.0 ** -21 * smd2 + 2 * M * e + e_d))
    k = (depth64(sh) + 16) * U64
    cc = sum(fl(c) ** 2 for c in o["centre"])
    return dict(gyration_pbc=(rg, k * rg + root_err(o["rg2"], e_d / M)),
                tensor_pbc=(tens, np.full(6, k * smd2 + 2.0 ** -50 * M * cc + e_d)))


def moved(base, var, bound):
    """largest movement of an output over its bound, per variant (arrays [2 K]); roots taken here"""
    base, var, bound = np.asarray(base, np.float64), np.asarray(var, np.float64), np.asarray(bound, np.float64)
    return np.abs(var - base) / np.maximum(bound, 1e-300)


FAMILIES = {"sums": ("cog", "com"), "moments": ("gyration", "tensor"), "rmsd": ("rmsd", "rmsd_mw")}


def plain_sensitivity(o_var, ref):
    """{family: smallest over the variants of the largest movement/bound over the family's outputs}"""
    val = dict(cog=np.stack(o_var["cog"], -1), com=np.stack(o_var["com"], -1), gyration=np.sqrt(np.maximum(o_var["rg2"], 0)),
               tensor=np.stack(o_var["tensor"], -1), rmsd=np.sqrt(o_var["msd"]), rmsd_mw=np.sqrt(o_var["msd_mw"]))
    out = {}
    for fam, names in FAMILIES.items():
        r = [moved(ref[k][0], val[k], ref[k][1]) for k in names]
        r = [x if x.ndim == 1 else x.max(-1) for x in r]
        out[fam] = float(np.max(r, 0).min())
    return out


def pbc_sensitivity(o_var, ref, names):
    val = dict(cog_pbc=np.stack(o_var["cog"], -1), com_pbc=np.stack(o_var["com"], -1),
               gyration_pbc=np.sqrt(np.maximum(o_var["rg2"], 0)), tensor_pbc=np.stack(o_var["tensor"], -1))
    r = [moved(ref[k][0], val[k.rstrip("37")], ref[k][1]) for k in names]
    r = [x if x.ndim == 1 else x.max(-1) for x in r]
    return float(np.max(r, 0).min())


def single_reference(s, prec, C):
    """every exact-sum reference of the single-call entries for system s: {name: (value, bound)}"""
    ref = plain_reference(derive(pack(s["sums"]["plain"][0], True)), prec, single_shape(C, s["n"]))
    dt = np.float32 if prec == 32 else np.float64
    m0 = int(s["mass"][s["sel"][0]])
    for dims in (7, 3):
        tot, _, E0 = s["sums"][dims]
        S = pack(tot, True)
        o = derive_pbc(S, m0, E0)
        for k, v in pbc_centre_reference(o, prec).items():
            ref[f"{k}{dims}"] = v
        if dims == 7:
            oc = derive_pbc(S, m0, E0, centre=rounded_centre(o["com"], dt))
            ref.update(pbc_central_reference(oc, prec, single_shape(C, s["n"], 0), difference_error(s, oc["centre"], dt)))
    return ref


def single_sensitivities(s, prec, C):
    """the one-atom condition of every kernel family of the single-call entries: {family: worst movement / bound}"""
    ref = single_reference(s, prec, C)
    out = plain_sensitivity(derive(variants(*s["sums"]["plain"])), ref)
    if len(s["pbc_probes"]):
        m0 = int(s["mass"][s["sel"][0]])
        for dims in (7, 3):
            tot, rows, E0 = s["sums"][dims]
            ov = derive_pbc(variants(tot, rows), m0, E0)
            out[f"sums_pbc{dims}"] = pbc_sensitivity(ov, ref, (f"cog_pbc{dims}", f"com_pbc{dims}"))
            if dims == 7:
                out["central_pbc"] = pbc_sensitivity(ov, ref, ("gyration_pbc", "tensor_pbc"))
    return out


def exact_in_f32(s):
    """the f32 products the kernels form without a rounded centre are exact: multiply them out in float32"""
    sel = s["sel"]
    p = as_real(s["X1"][sel], np.float32)
    q = as_real(s["X2"][s["sel2"]], np.float32)
    m = s["mass"][sel].astype(np.float32)
    ok = np.array_equal((p * m[:, None]).astype(np.float64), p.astype(np.float64) * m[:, None].astype(np.float64))
    v = q - p
    d2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    v64 = q.astype(np.float64) - p.astype(np.float64)
    d264 = (v64 ** 2).sum(1)
    ok &= np.array_equal(d2.astype(np.float64), d264)
    ok &= np.array_equal((d2 * m).astype(np.float64), d264 * m.astype(np.float64))
    return bool(ok)


def triclinic_case(prec, n=65537):
    """one triclinic case per periodic entry, at the project's tolerances against the f64 oracle: a blob split over the
    images of a sheared cell, a gathered selection, two finaliser trips"""
    rng = np.random.default_rng(77)
    box = np.array([[9.0, 0.0, 0.0], [2.5, 8.0, 0.0], [-1.5, 3.0, 7.0]]).T           # columns = box vectors
    natoms = n + n // 4
    blob = rng.normal(0, 0.6, (natoms, 3)) + rng.uniform(0, 5, 3)
    wrapped = ((blob @ np.linalg.inv(box).T) % 1.0) @ box.T
    dt = np.float32 if prec == 32 else np.float64
    return dict(box=box.astype(dt), xyz=np.ascontiguousarray(wrapped, dtype=dt), mass=rng.uniform(1, 16, natoms).astype(dt),
                idx=np.sort(rng.choice(natoms, n, replace=False)).astype(np.uint64), n=n)


# ------------------------------------------------------------------------------------------------ fit_rmsd_batch

FIT32_CASES = ([(F, n) for F in (1, 3, 4, 7, 8, 63, 64, 65) for n in (1023, 1025, 2047, 2049)]
               + [(F, n) for F in (64, 65) for n in (16384, 16385, 32768, 32769, 36865)]
               + [(F, n) for F in (1, 4) for n in ("65537", "4096C+1")])
FIT64_CASES = [(F, n) for F in (1, 2, 5) for n in (1, 2047, 2048, 2049, 131072, 131073, 262444)]


def _rotations():
    out = []
    for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        for sg in range(8):
            R = np.zeros((3, 3), np.int64)
            for r in range(3):
                R[r, perm[r]] = 1 - 2 * ((sg >> r) & 1)
            if round(np.linalg.det(R)) == 1:
                out.append(R)
    return out


ROTATIONS = _rotations()           # the 24 proper rotations of the grid


@functools.lru_cache(maxsize=2)
def fit_system(n, F):
    """reference frame, F frames and one mass column; frames[f][sel] = R_f ref[ref_sel] + t_f + noise, sentinels on the probed
    positions of the selection (R_f maps corners to corners; |t_f| <= 3 nm, so a frame reaches 64 + 3.25 nm: still exact);
    `ref_same` holds the same reference atoms at sel, for calls with ref_idx == idx"""
    rng = np.random.default_rng(104729 * n + F)
    natoms = n + n // 8 + 3
    sel = _selection(rng, natoms, n)
    ref_sel = _selection(rng, natoms, n)
    probes = stride_probes(n)
    Q = rng.integers(-BULK, BULK + 1, (n, 3)).astype(np.int64)
    Q[probes] = corners(np.arange(len(probes)))
    mass = rng.integers(1, 9, natoms).astype(np.int64)
    mass[sel[probes]] = SENT_MASS
    ref = rng.integers(-BULK, BULK + 1, (natoms, 3)).astype(np.int64)
    ref_same = ref.copy()
    ref[ref_sel] = Q
    ref_same[sel] = Q
    frames = rng.integers(-BULK, BULK + 1, (F, natoms, 3)).astype(np.int64)
    for f in range(F):
        frames[f][sel] = Q @ ROTATIONS[(5 * f + 1) % 24].T + rng.integers(-24, 25, 3) + rng.integers(-2, 3, (n, 3))
    return dict(n=n, F=F, natoms=natoms, sel=sel, ref_sel=ref_sel, probes=probes, mass=mass, ref=ref, ref_same=ref_same,
                frames=frames.astype(np.int32))


def fit_gyration_reference(fs, f, prec, sh):
    """(value, bound) of the gyration radius of frame f's (fitted) selection; sh: fit64_shape for the f64 bound"""
    o = derive(pack(terms(fs["frames"][f][fs["sel"]], fs["mass"][fs["sel"]]).sum(0), True))
    rg = math.sqrt(fl(o["rg2"]))
    if prec == 32:
        e = 2.0 ** -49 * (fl(o["raw2"]) + fl(o["cc"]))                 # S16 / S0 - |cm|^2 in f64, cm not rounded
        return rg, U32 * rg + root_err(o["rg2"], e)
    return rg, (depth64(sh) + 16) * U64 * rg


def fit_gyration_sensitivity(fs, f, prec, sh):
    T = terms(fs["frames"][f][fs["sel"]], fs["mass"][fs["sel"]])
    ref, bound = fit_gyration_reference(fs, f, prec, sh)
    ov = derive(variants(T.sum(0), T[fs["probes"]]))
    return float(moved(ref, np.sqrt(np.maximum(ov["rg2"], 0)), bound).min())


# ------------------------------------------------------------------------------------------------ CSR batches

CSR_SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 1000)
CSR_ORDER2 = (1000, 129, 65, 3, 128, 1, 64, 127, 2, 63)
CSR_NSEL = (1, 3, 4, 5, 8, 9, 20)


@functools.lru_cache(maxsize=1)
def csr_system():
    """20 consecutive, disjoint selections (CSR_SIZES, then CSR_ORDER2) with sentinels on the first and last element of every
    64-lane step: a wave that reads one element into its neighbour meets one.  Two frames, a second index set, wrapped
    coordinates for the periodic entries."""
    rng = np.random.default_rng(4242)
    sizes = np.array(CSR_SIZES + CSR_ORDER2, np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    natoms = int(off[-1]) + 900
    perm = rng.permutation(natoms)
    perm2 = rng.permutation(natoms)
    idx = np.concatenate([np.sort(perm[off[k]:off[k + 1]]) for k in range(len(sizes))]).astype(np.int64)
    idx2 = np.concatenate([np.sort(perm2[off[k]:off[k + 1]]) for k in range(len(sizes))]).astype(np.int64)
    probes = np.concatenate([off[k] + csr_probes(int(sizes[k])) for k in range(len(sizes))])
    X1, mass = _fill(rng, natoms, idx, probes)
    X2 = rng.choice([-500, 500], (natoms, 3)).astype(np.int64)
    X2[idx2] = X1[idx] @ ROT90.T + SHIFT2 + rng.integers(-2, 3, (len(idx), 3))
    X3 = rng.choice([-500, 500], (natoms, 3)).astype(np.int64)           # the second frame read through the SAME index
    X3[idx] = X1[idx] @ ROT90.T + SHIFT2 + rng.integers(-2, 3, (len(idx), 3))
    return dict(sizes=sizes, off=off, natoms=natoms, idx=idx, idx2=idx2, probes=probes, X1=X1, X2=X2, X3=X3,
                Xw=X1 % (BOX_EDGE * UNIT), mass=mass)


def csr_reference(cs, k, prec, second="X2"):
    """exact-sum outputs of selection k: centre of geometry / of mass, gyration, rmsd, rmsd_mw as {name: (value, bound)};
    second: the frame of the rmsd, "X2" read through idx2 or "X3" read through idx"""
    a, b = int(cs["off"][k]), int(cs["off"][k + 1])
    sel, sel2 = cs["idx"][a:b], (cs["idx2"] if second == "X2" else cs["idx"])[a:b]
    T = terms(cs["X1"][sel], cs["mass"][sel], cs[second][sel2])
    o = derive(pack(T.sum(0), True))
    return plain_reference(o, prec, dict(trips=cdiv(b - a, 64), fin_trips=0))


def csr_pbc_gyration(cs, k):
    """periodic gyration radius of selection k (wrapped coordinates, BOX) from exact sums, and how far one probed atom moves
    it, relative.  k_gyration_batch centres the terms on an f32 centre, so the entry keeps the project's tolerance
    (PBC_GYR_BATCH_RTOL32 against the f64 oracle); this figure shows that tolerance still sees one atom."""
    a, b = int(cs["off"][k]), int(cs["off"][k + 1])
    sel = cs["idx"][a:b]
    E = cs["X1"][sel] + (cs["Xw"][sel[0]] - cs["X1"][sel[0]])
    T = terms(E, cs["mass"][sel])
    m0 = int(cs["mass"][sel[0]])
    ref = math.sqrt(fl(derive_pbc(pack(T.sum(0), True), m0, E[0])["rg2"]))
    pp = csr_probes(b - a)
    pp = pp[pp > 0]
    if not len(pp):
        return ref, math.inf
    ov = derive_pbc(variants(T.sum(0), T[pp]), m0, E[0])
    return ref, float((np.abs(np.sqrt(np.maximum(ov["rg2"], 0)) - ref) / ref).min())


def csr_sensitivity(cs, k, prec):
    a, b = int(cs["off"][k]), int(cs["off"][k + 1])
    out = {}
    for second in ("X2", "X3"):
        sel, sel2 = cs["idx"][a:b], (cs["idx2"] if second == "X2" else cs["idx"])[a:b]
        T = terms(cs["X1"][sel], cs["mass"][sel], cs[second][sel2])
        r = plain_sensitivity(derive(variants(T.sum(0), T[csr_probes(b - a)])), csr_reference(cs, k, prec, second))
        out = {f: min(v, out.get(f, math.inf)) for f, v in r.items()}
    return out


# ------------------------------------------------------------------------------------------------ lipid tails

LIPID_NTAILS = {32: (1, 15, 16, 17, 33), 64: (1, 63, 64, 65)}
LIPID_LENGTHS = (3, 4, 18)


def lipid_tails(ntails, dtype, seed=0):
    """ntails random-walk tails of 3, 4, 18, 3, .. carbons (C-C 0.153 nm); a double bond inside every other 18-carbon tail;
    normals one per tail or one per bond in turn"""
    rng = np.random.default_rng(900 + ntails + seed)
    lens = [LIPID_LENGTHS[t % 3] for t in range(ntails)]
    natoms = sum(lens) + 50
    xyz = rng.uniform(0, 10, (natoms, 3))
    order = rng.permutation(natoms)
    tails, bonds, normals, used = [], [], [], 0
    for t, n in enumerate(lens):
        ids = order[used:used + n]
        used += n
        p = np.zeros((n, 3))
        p[0] = rng.uniform(1, 9, 3)
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        for k in range(1, n):
            d = d + 0.9 * rng.normal(size=3)
            d /= np.linalg.norm(d)
            p[k] = p[k - 1] + 0.153 * d
        xyz[ids] = p
        bo = np.ones(n - 1, np.uint8)
        if n == 18 and (t // 3) % 2 == 0:
            bo[int(rng.integers(2, n - 4))] = 2
        nn = 1 if t % 2 == 0 else n - 2
        nv = rng.normal(size=(nn, 3))
        nv /= np.linalg.norm(nv, axis=1)[:, None]
        tails.append(ids.astype(np.uint64))
        bonds.append(bo)
        normals.append(nv.astype(dtype))
    return np.ascontiguousarray(xyz, dtype=dtype), tails, bonds, normals
