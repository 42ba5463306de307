"""numpy reference of the time correlation functions of vectors (molar_hip_tcf: a vector per tuple and frame, the first and
second Legendre polynomial of u(t) . u(t + tau) over all time origins per vector and per group, the mean vector and the order
parameter S^2), the acceptance bounds of the GPU tests, and the inputs those tests share.

The reference follows the definition in include/molar_hip.h by another route than the kernels, in np.longdouble (2^-64 on
x86) throughout:
  * the minimum image by msd_ref.min_image: route "round" (the fractional bond minus its rounding, a longdouble inverse of the
    box) or route "brute" (the shortest of 125 images; the full mask), each with its own assertion that the image is
    unambiguous - every fractional bond component within 0.47 of an integer, the second-best image longer by 1e-6;
  * the lag sums by vectorised slices U[tau::os] . U[:F - tau:os], never a chain over the origins;
  * the group curves from the per-vector sums, the order parameter from the 3 x 3 moment matrix (np.einsum).
It ASSERTS on its inputs, so that validity is unambiguous: every (vector, frame) has either |w| > 1e-3 or w exactly zero or
not finite, and the vectors that come out bad are exactly those the caller declared (`bad=`); a kernel that disagrees is
wrong, not unlucky.  The test inputs sit on the grid of multiples of 2^-10 where exactness matters (differences, and the
products of a collinear triple, are exact in f64 and in longdouble alike).

Bounds (u = 2^-53; eps_out = 2^-24 for the f32 entry, 2^-53 for the f64 entry; F frames; nd components in dims).  Quantities
of the input, all taken from the reference itself:
  B      the largest norm of a box vector or of a raw bond p[b] - p[a];   kappa: the largest row sum of |M| |M^-1| (msd_ref);
  Nb     the largest norm of a bond after the minimum image;   wmin, wmax: the smallest and largest |w| of a valid vector;
  M      the largest |u|: 1 + 2^-40 in UNIT mode (the computed unit vector is 1 to a few u), wmax in RAW mode.
Forming w, per component:
  kind 1: exact (f32 and f64 inputs are exact in f64).                                                  E_w = 0
  kind 2: the difference rounds once for f64 inputs (u B); the minimum image costs c_b u B with msd_ref's
          c_b = 15 kappa + 8 (its docstring counts the roundings of shortest_vector).                    E_b = (c_b + 1) u B
  kind 3: a component of b x c is two products and a difference: 2 E_b (|b| + |c|) + 2 E_b^2 from the operands and
          3 u |b| |c| from the three roundings.                                          E_w = 4 E_b Nb + 2 E_b^2 + 3 u Nb^2
UNIT: u = w / sqrt(|w|^2).  |w|^2 is 3 products and 2 sums (3 u relative), the root halves that and adds u, the division
adds u: 4 u |u_a| <= 4 u per component.  An error dw of w moves u by (dw - u (u . dw)) / |w|: per component at most
(1 + sqrt 3) E_w / wmin, and 2 (E_w / wmin)^2 for the second order.
  E_u = (1 + sqrt 3) E_w / wmin + 2 (E_w / wmin)^2 + 4 u      (UNIT);        E_u = E_w      (RAW)
A pair:  d = u . u' with both operands off by E_u per component and three roundings of terms that add up to at most M^2:
  E_d = 2 sqrt(nd) E_u M + nd E_u^2 + 3 u M^2
Sums.  A sum of T terms x_i in ANY order of additions carries at most (T - 1) u sum |x_i| <= T u (T max|x|).  Every chain the
header documents (origins in order; the valid vectors of a label run, the runs of a chunk, the chunks in order) adds T =
n(tau) terms for a vector and T = N_g n(tau) terms for a group, so after the division by T:
  |c1_vec - ref| <= E_d + (n + 1) u M^2 + (u + eps_out) |ref|
  |c1 - ref|     <= E_d + (N_g n + 2) u M^2 + (u + eps_out) |ref|           (the product N_g n rounds once more)
d^2 by fma(d, d, .): 2 M^2 E_d + E_d^2 from d, then the same sum bound with terms of at most M^4; c2 = 1.5 (S2 / T) - 0.5
multiplies the error by 1.5 and rounds twice more (values of at most 1.5 M^4 and |c2|):
  |c2_vec - ref| <= 1.5 (2 M^2 E_d + E_d^2 + (n + 2) u M^4) + (2 u + eps_out) |ref| + 2 u
  |c2 - ref|     <= 1.5 (2 M^2 E_d + E_d^2 + (N_g n + 3) u M^4) + (2 u + eps_out) |ref| + 2 u
mean = sum_f u / F:          |mean - ref| <= E_u + (F + 1) u M + eps_out |ref|
s2: a second moment m_ab = sum_f u_a u_b / F carries E_m = 2 M E_u + E_u^2 + (F + 2) u M^2; q = sum_ab m_ab^2 (nine terms,
sum |m_ab| <= 3 M^2) carries 6 M^2 E_m + 9 E_m^2 and the eight roundings of its formula (8 u M^4):
  |s2 - ref| <= 1.5 (6 M^2 E_m + 9 E_m^2 + 8 u M^4) + 2 u + eps_out |ref|
Integers (nvalid, bad_frames) and the positions of NaN are compared for equality."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msd_ref as mr  # noqa: E402

U = 2.0 ** -53
EPS64 = 2.0 ** -53
EPS32 = 2.0 ** -24
LD = np.longdouble
ORTHO, TRICLINIC = mr.ORTHO, mr.TRICLINIC
UNIT, RAW = 0, 1


def n_of_tau(F, L, os_):
    return (F - 1 - np.arange(L + 1, dtype=np.int64)) // min(os_, F) + 1


def form_vectors(frames, tuples, boxes=None, pbc=7, dims=7, route=None):
    """w [F, V, 3] in longdouble from the exact inputs, and the quantities of the bounds (B, kappa, Nb)."""
    x = np.asarray(frames).astype(LD)
    F = x.shape[0]
    tuples = np.asarray(tuples, np.int64).reshape(len(tuples), -1)
    kind = tuples.shape[1]
    big, kappa, nb = 0.0, 1.0, 0.0
    use_box = boxes is not None and pbc != 0 and kind >= 2

    def image(s, f):
        nonlocal big
        fin = np.all(np.isfinite(s.astype(np.float64)), axis=1)
        out = s.copy()
        if fin.any():
            big = max(big, float(np.sqrt((s[fin] * s[fin]).sum(-1)).max()))
        if use_box and fin.any():
            b = np.asarray(boxes, np.float64)
            b = b if b.ndim == 1 else b[f]
            r = route or ("brute" if pbc == 7 and not mr.is_ortho(b) else "round")
            out[fin] = mr.min_image(s[fin], b, pbc, r)
        return out

    if kind == 1:
        w = x[:, tuples[:, 0]].copy()
    else:
        w = np.empty((F, len(tuples), 3), LD)
        for f in range(F):
            b = image(x[f, tuples[:, 1]] - x[f, tuples[:, 0]], f)
            if kind == 3:
                c = image(x[f, tuples[:, 2]] - x[f, tuples[:, 0]], f)
                for v in (b, c):
                    fin = np.all(np.isfinite(v.astype(np.float64)), axis=1)
                    if fin.any():
                        nb = max(nb, float(np.sqrt((v[fin] * v[fin]).sum(-1)).max()))
                w[f] = np.cross(b, c)
            else:
                w[f] = b
    for d in range(3):
        if not dims >> d & 1:
            w[..., d] = 0
    if use_box:
        for b in np.asarray(boxes, np.float64).reshape(-1, 9):
            M = mr.box_matrix(b)
            kappa = max(kappa, float((np.abs(M) @ np.abs(np.linalg.inv(M))).sum(1).max()))
            big = max(big, float(np.sqrt((M * M).sum(0)).max()))
    return w, dict(B=big, kappa=kappa, Nb=nb, kind=kind, use_box=use_box)


def tcf(frames, tuples, labels=None, ngroups=None, boxes=None, pbc=7, mode=UNIT, dims=7, max_lag=None, origin_stride=1, route=None, bad=()):
    """The reference: a dict with c1, c2 [G, L + 1], c1_vec, c2_vec [V, L + 1], mean [V, 3], s2 [V] in longdouble (c2, c2_vec, s2:
    None in RAW mode), nvalid [G], bad_frames [V], n [L + 1], and the quantities the bounds need.  `bad`: the vectors the caller
    made bad on purpose; asserted to be exactly the vectors that come out bad."""
    frames = np.asarray(frames)
    F = frames.shape[0]
    w, q = form_vectors(frames, tuples, boxes, pbc, dims, route)
    V = w.shape[1]
    L = F - 1 if max_lag is None else max_lag
    fin = np.all(np.isfinite(w.astype(np.float64)), axis=2)
    n2 = np.where(fin, (w * w).sum(-1), LD(1))
    norm = np.sqrt(n2)
    zero = fin & (n2 == 0)
    assert np.all((~fin) | zero | (norm > 1e-3)), "a vector that is neither exactly zero nor longer than 1e-3: validity is ambiguous"
    badf = ~fin | zero if mode == UNIT else ~fin
    bad_frames = badf.sum(0).astype(np.uint32)
    valid = bad_frames == 0
    assert set(np.nonzero(~valid)[0].tolist()) == set(int(b) for b in bad), "the bad vectors are not the ones declared"
    u = np.zeros_like(w)
    ok = valid[None, :] & np.ones((F, 1), bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        u[ok] = (w / norm[..., None])[ok] if mode == UNIT else w[ok]
    lab = np.zeros(V, np.int64) if labels is None else np.asarray(labels, np.int64)
    G = 1 if labels is None else int(ngroups if ngroups is not None else lab.max() + 1)
    n = n_of_tau(F, L, origin_stride)
    os_ = min(origin_stride, F)
    s1, s2 = np.zeros((V, L + 1), LD), np.zeros((V, L + 1), LD)
    for tau in range(L + 1):
        a = u[: F - tau: os_]
        d = (u[tau::os_][: len(a)] * a).sum(-1)                       # [origins, V]
        assert d.shape[0] == n[tau]
        s1[:, tau], s2[:, tau] = d.sum(0), (d * d).sum(0)
    nan = LD(np.nan)
    c1v = np.where(valid[:, None], s1 / n[None], nan)
    c2v = np.where(valid[:, None], LD(1.5) * s2 / n[None] - LD(0.5), nan)
    nvalid = np.array([int((valid & (lab == g)).sum()) for g in range(G)], np.uint64)
    c1, c2 = np.full((G, L + 1), nan), np.full((G, L + 1), nan)
    for g in range(G):
        m = valid & (lab == g)
        if m.any():
            c1[g] = s1[m].sum(0) / (int(m.sum()) * n)
            c2[g] = LD(1.5) * s2[m].sum(0) / (int(m.sum()) * n) - LD(0.5)
    mean = np.where(valid[:, None], u.sum(0) / F, nan)
    mom = np.einsum("fva,fvb->vab", u, u) / F
    s2o = np.where(valid, LD(1.5) * (mom * mom).sum((1, 2)) - LD(0.5), nan)
    vn = norm[:, valid]
    unit = mode == UNIT
    return dict(c1=c1, c2=c2 if unit else None, c1_vec=c1v, c2_vec=c2v if unit else None, nvalid=nvalid, mean=mean, s2=s2o if unit else None,
                bad_frames=bad_frames, n=n, F=F, V=V, G=G, L=L, nd=bin(dims).count("1"), unit=unit, valid=valid, labels=lab,
                wmin=float(vn.min()) if vn.size else 1.0, wmax=float(vn.max()) if vn.size else 1.0, **q)


def errors(ref):
    """(E_u, E_d, M) of the docstring."""
    c_b = 15.0 * ref["kappa"] + 8.0
    e_b = (c_b + 1.0) * U * ref["B"] if ref["kind"] >= 2 else 0.0
    e_w = e_b if ref["kind"] <= 2 else 4 * e_b * ref["Nb"] + 2 * e_b * e_b + 3 * U * ref["Nb"] ** 2
    if ref["unit"]:
        r = e_w / ref["wmin"]
        e_u, M = (1 + np.sqrt(3.0)) * r + 2 * r * r + 4 * U, 1.0 + 2.0 ** -40
    else:
        e_u, M = e_w, max(ref["wmax"], 1e-300)
    nd = ref["nd"]
    e_d = 2 * np.sqrt(nd) * e_u * M + nd * e_u * e_u + 3 * U * M * M
    return e_u, e_d, M


def bounds(ref, eps_out):
    """name -> bound, each of the shape of its output."""
    e_u, e_d, M = errors(ref)
    n = ref["n"].astype(np.float64)
    F = ref["F"]
    ng = ref["nvalid"].astype(np.float64)[:, None]
    a = lambda x: np.abs(np.nan_to_num(np.asarray(x, LD).astype(np.float64)))
    out = {"c1_vec": e_d + (n + 1)[None] * U * M * M + (U + eps_out) * a(ref["c1_vec"]),
           "c1": e_d + (ng * n[None] + 2) * U * M * M + (U + eps_out) * a(ref["c1"]),
           "mean": e_u + (F + 1) * U * M + eps_out * a(ref["mean"])}
    if ref["unit"]:
        p2 = 2 * M * M * e_d + e_d * e_d
        out["c2_vec"] = 1.5 * (p2 + (n + 2)[None] * U * M ** 4) + (2 * U + eps_out) * a(ref["c2_vec"]) + 2 * U
        out["c2"] = 1.5 * (p2 + (ng * n[None] + 3) * U * M ** 4) + (2 * U + eps_out) * a(ref["c2"]) + 2 * U
        e_m = 2 * M * e_u + e_u * e_u + (F + 2) * U * M * M
        out["s2"] = 1.5 * (6 * M * M * e_m + 9 * e_m * e_m + 8 * U * M ** 4) + 2 * U + eps_out * a(ref["s2"])
    return out


REPORT = {}          # output and entry -> the largest used fraction seen by check()
FLOATS = ("c1", "c2", "c1_vec", "c2_vec", "mean", "s2")


def check(got, ref, eps_out, what=""):
    """got: a mapping (or VectorCorrelations) of outputs, entries may be None.  NaN where and only where the reference has
    NaN; integers equal; prints the used fraction of every bound before it asserts, and returns them."""
    get = (lambda k: got.get(k)) if isinstance(got, dict) else (lambda k: getattr(got, k, None))
    lim = bounds(ref, eps_out)
    used = {}
    for name in FLOATS:
        g, r = get(name), ref[name]
        if g is None:
            continue
        assert r is not None, f"{what}: {name} is not defined in RAW mode"
        g = np.asarray(g)
        assert g.shape == r.shape, f"{what}: {name} has shape {g.shape}, expected {r.shape}"
        rn = np.isnan(r.astype(np.float64))
        assert np.array_equal(np.isnan(g), rn), f"{what}: {name} is NaN elsewhere than the reference"
        err = np.abs(g.astype(LD) - r).astype(np.float64)
        used[name] = mr.worst(err[~rn], np.broadcast_to(lim[name], err.shape)[~rn])
        key = name + (" f32" if eps_out == EPS32 else " f64")
        REPORT[key] = max(REPORT.get(key, 0.0), used[name])
    print(f"tcf bounds used {what}: " + " ".join(f"{k}={v:.3g}" for k, v in used.items()))
    for name in ("nvalid", "bad_frames"):
        g = get(name)
        if g is not None:
            assert np.array_equal(np.asarray(g).astype(np.int64), ref[name].astype(np.int64)), f"{what}: {name} differs"
    for name, v in used.items():
        assert v <= 1.0, f"{what}: {name} uses {v:.3g} of its bound"
    return used


# ---------------------------------------------------------------- the kernels' route restated in f64 (CPU test of the bounds)

def kernel_route(frames, tuples, labels=None, ngroups=None, boxes=None, pbc=7, mode=UNIT, dims=7, max_lag=None, origin_stride=1, vec_chunk=1,
                 frame_chunk=64):
    """The outputs in plain f64 with the sums in the order tcf.hip documents (origins in order; runs of one label within a chunk
    of vec_chunk vectors, the runs and the chunks in order; frames in order within chunks of frame_chunk, the chunks in order).
    numpy has no fused multiply-add: products and sums round separately here, which the bounds cover as well."""
    x = np.asarray(frames).astype(np.float64)
    F = x.shape[0]
    tuples = np.asarray(tuples, np.int64).reshape(len(tuples), -1)
    V, kind = tuples.shape
    L = F - 1 if max_lag is None else max_lag
    os_ = min(origin_stride, F)

    def sv(d, f):
        if boxes is None or pbc == 0:
            return d
        b = np.asarray(boxes, np.float64)
        M = mr.box_matrix(b if b.ndim == 1 else b[f])
        fr = mr._matvec(mr._inverse3(M), d)
        for k in range(3):
            if pbc >> k & 1:
                fr[:, k] -= np.sign(fr[:, k]) * np.floor(np.abs(fr[:, k]) + 0.5)
        d = mr._matvec(M, fr)
        if pbc == 7 and not mr.is_ortho(M.T.reshape(9)):
            best, best2 = d.copy(), (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            for s in mr._shifts(M):
                c = d + s[None]
                n2 = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
                m = n2 < best2
                best[m], best2[m] = c[m], n2[m]
            d = best
        return d

    u = np.zeros((F, V, 3))
    badf = np.zeros((F, V), bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for f in range(F):
            w = x[f, tuples[:, 0]].copy()
            if kind >= 2:
                b = sv(x[f, tuples[:, 1]] - w, f)
                if kind == 3:
                    c = sv(x[f, tuples[:, 2]] - w, f)
                    w = np.stack([b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1], b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2], b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]], -1)
                else:
                    w = b
            for d in range(3):
                if not dims >> d & 1:
                    w[:, d] = 0.0
            ok = np.all(np.isfinite(w), axis=1)
            if mode == UNIT:
                n2 = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]
                ok &= n2 != 0
                w = w / np.sqrt(n2)[:, None]
            badf[f] = ~ok
            u[f] = np.where(ok[:, None], w, 0.0)
    bad_frames = badf.sum(0).astype(np.uint32)
    valid = bad_frames == 0
    nan = np.nan
    # moments: frames in order within a chunk, the chunks in order
    mom = np.zeros((V, 9))
    for c0 in range(0, F, frame_chunk):
        part = np.zeros((V, 9))
        for f in range(c0, min(F, c0 + frame_chunk)):
            a = u[f]
            terms = [a[:, 0], a[:, 1], a[:, 2], a[:, 0] * a[:, 0], a[:, 1] * a[:, 1], a[:, 2] * a[:, 2], a[:, 0] * a[:, 1], a[:, 0] * a[:, 2], a[:, 1] * a[:, 2]]
            part = part + np.where(badf[f][:, None], 0.0, np.stack(terms, -1))
        mom = mom + part
    mom = mom / float(F)
    mean = np.where(valid[:, None], mom[:, :3], nan)
    q = ((mom[:, 3] ** 2 + mom[:, 4] ** 2) + mom[:, 5] ** 2) + 2.0 * ((mom[:, 6] ** 2 + mom[:, 7] ** 2) + mom[:, 8] ** 2)
    s2o = np.where(valid, 1.5 * q - 0.5, nan)
    n = n_of_tau(F, L, origin_stride).astype(np.float64)
    s1, s2 = np.zeros((V, L + 1)), np.zeros((V, L + 1))
    for tau in range(L + 1):
        for t in range(0, F - tau, os_):
            d = (u[t, :, 0] * u[t + tau, :, 0] + u[t, :, 1] * u[t + tau, :, 1]) + u[t, :, 2] * u[t + tau, :, 2]
            s1[:, tau] += d
            s2[:, tau] += d * d
    c1v = np.where(valid[:, None], s1 / n[None], nan)
    c2v = np.where(valid[:, None], 1.5 * (s2 / n[None]) - 0.5, nan)
    lab = np.zeros(V, np.int64) if labels is None else np.asarray(labels, np.int64)
    G = 1 if labels is None else int(ngroups if ngroups is not None else lab.max() + 1)
    nchunks = -(-V // vec_chunk)
    part = np.zeros((nchunks, G, L + 1, 2))
    for ch in range(nchunks):
        g0, g1 = ch * vec_chunk, min(V, (ch + 1) * vec_chunk)
        cur, tot = lab[g0], np.zeros((L + 1, 2))
        for g in range(g0, g1):
            if lab[g] != cur:
                part[ch, cur] += tot
                cur, tot = lab[g], np.zeros((L + 1, 2))
            if valid[g]:
                tot = tot + np.stack([s1[g], s2[g]], -1)
        part[ch, cur] += tot
    tot = np.zeros((G, L + 1, 2))
    for ch in range(nchunks):
        tot = tot + part[ch]
    nvalid = np.array([int((valid & (lab == g)).sum()) for g in range(G)], np.uint64)
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = nvalid.astype(np.float64)[:, None] * n[None]
        c1 = np.where(nvalid[:, None] > 0, tot[..., 0] / scale, nan)
        c2 = np.where(nvalid[:, None] > 0, 1.5 * (tot[..., 1] / scale) - 0.5, nan)
    unit = mode == UNIT
    return dict(c1=c1, c2=c2 if unit else None, c1_vec=c1v, c2_vec=c2v if unit else None, nvalid=nvalid, mean=mean, s2=s2o if unit else None,
                bad_frames=bad_frames)


# ---------------------------------------------------------------- shared inputs

def make_case(F, V, kind, seed, box9=None, boxes=None, dtype=np.float32):
    """(frames [F, 3 V + 2, 3], tuples [V, kind]) on the grid of multiples of 2^-10: vector v is made of the atoms 3 v, 3 v + 1,
    3 v + 2, drawn afresh in every frame.  Atom A anywhere in the cell (every component at least 8 grid units from 0, so that
    a kind-1 vector is long enough under any mask used); B - A = (+-[64, lim], [-16, 16], +-[8, lim]) and
    C - A = ([-16, 16], +-[64, lim], +-[8, lim]) grid units, lim = 0.4 of the cell along that component (0.25 of the shortest
    edge for a skewed cell): |w| > 1e-3 for kinds 1, 2, 3 under the masks 7, 3 and 4, and every bond component within 0.41 of
    the cell of zero.  With a box every atom is wrapped into the cell of its frame on its own, so that bonds are cut by the
    boundary; exactly for an orthorhombic cell on the grid, else rounded to f32 afterwards."""
    rng = np.random.default_rng(seed)
    ref_box = np.asarray(ORTHO if box9 is None else box9, np.float64)
    cells = (ref_box[[0, 4, 8]] * 1024).astype(np.int64)
    lim = (cells * 0.4).astype(np.int64) if mr.is_ortho(ref_box) else np.full(3, int(cells.min() * 0.25))
    sign = lambda shape: rng.integers(0, 2, size=shape) * 2 - 1
    a = np.stack([rng.integers(8, cells[d], size=(F, V)) for d in range(3)], -1)
    big = lambda d: sign((F, V)) * rng.integers(64, lim[d] + 1, size=(F, V))
    any_ = lambda d: sign((F, V)) * rng.integers(8, lim[d] + 1, size=(F, V))
    small = lambda: rng.integers(-16, 17, size=(F, V))
    db = np.stack([big(0), small(), any_(2)], -1)
    dc = np.stack([small(), big(1), any_(2)], -1)
    x = np.zeros((F, 3 * V + 2, 3))
    x[:, 0:3 * V:3], x[:, 1:3 * V:3], x[:, 2:3 * V:3] = a / 1024.0, (a + db) / 1024.0, (a + dc) / 1024.0
    x[:, 3 * V:] = 1.0
    if box9 is not None or boxes is not None:
        bx = ref_box if boxes is None else np.asarray(boxes, np.float64)
        if bx.ndim == 1 and mr.is_ortho(bx):
            x = mr.wrap_ortho(x, bx)
        else:
            x = mr.wrap(x, bx)
    fr = x.astype(np.float32)
    if boxes is None and (box9 is None or mr.is_ortho(ref_box)):
        assert np.array_equal(fr.astype(np.float64), x)
    tuples = (3 * np.arange(V)[:, None] + np.arange(kind)[None]).astype(np.uint64)
    return np.ascontiguousarray(fr.astype(dtype)), tuples


def make_bad(frames, tuples, v, f, how="zero"):
    """Vector v made bad in frame f, in place: "zero": kind 1 the atom at the origin, kind 2 B on A, kind 3 C on B (two equal
    bonds: a cross product of exactly zero under any box); "nan": a coordinate of its last atom is NaN."""
    t = [int(k) for k in tuples[v]]
    if how == "nan":
        frames[f, t[-1], 1] = np.nan
    elif len(t) == 1:
        frames[f, t[0]] = 0.0
    else:
        frames[f, t[-1]] = frames[f, t[-2]]


# ---------------------------------------------------------------- the C entry spelt out, and the errors its arguments alone decide

ERR_SIZES, ERR_NO_PBC, ERR_ZERO_LENGTH, ERR_INVERSE, ERR_INVALID, ERR_TOO_LARGE = 1, 4, 5, 6, 50, 51


def raw_tcf(fn, ctx, frames, real=np.float32, **kw):
    """The C entry with every argument spelt out; returns the status.  Outputs (numpy arrays) by their names."""
    import ctypes as C
    from molar_amd import _lib
    frames = np.ascontiguousarray(frames, dtype=real)
    F, natoms = frames.shape[:2]
    keep = [frames]

    def addr(x, dtype):
        if x is None:
            return None
        a = np.ascontiguousarray(x, dtype=dtype)
        keep.append(a)
        return a.ctypes.data

    g = kw.get
    tuples = np.asarray(g("tuples", [[0, 1]]), np.uint64)
    tuples = tuples.reshape(len(tuples), -1)
    sp = _lib.TcfSpec(g("kind", tuples.shape[1]), g("mode", UNIT), g("dims", 7), g("reserved", 0))
    out = [g(k) for k in ("c1", "c2", "c1_vec", "c2_vec", "nvalid", "mean", "s2", "bad_frames")]
    o = [None if x is None else x.ctypes.data for x in out]
    return fn(ctx, frames.ctypes.data, g("F", F), g("stride", 3 * natoms), g("natoms", natoms), None if g("no_tuples") else addr(tuples, np.uint64),
              g("V", len(tuples)), addr(g("labels"), np.uint32), g("G", 0), addr(g("boxes"), real), g("box_stride", 0), g("pbc", 0),
              None if g("no_spec") else C.addressof(sp), g("L", 0), g("os", 1), o[0], o[1], o[2], o[3], g("ld", 0), o[4], o[5], o[6], o[7])


def argument_errors(fn, ctx, real=np.float32):
    """Every error of the definition's table that the arguments alone decide: (what, expected status, got status)."""
    fr = np.ones((4, 5, 3), real)
    row = np.zeros((1, 2), real)
    one = np.zeros(1, real)
    rows = [("nvectors == 0", ERR_SIZES, dict(V=0)),
            ("labels with ngroups == 0", ERR_SIZES, dict(labels=[0], G=0)),
            ("ld too small for c1_vec", ERR_SIZES, dict(L=2, c1_vec=row, ld=2)),
            ("ld too small for c2_vec", ERR_SIZES, dict(L=2, c2_vec=row, ld=2)),
            ("spec == NULL", ERR_INVALID, dict(no_spec=True)),
            ("kind == 0", ERR_INVALID, dict(kind=0)),
            ("kind == 4", ERR_INVALID, dict(kind=4)),
            ("a mode other than the two", ERR_INVALID, dict(mode=2)),
            ("dims == 0", ERR_INVALID, dict(dims=0)),
            ("dims > 7", ERR_INVALID, dict(dims=8)),
            ("reserved != 0", ERR_INVALID, dict(reserved=1)),
            ("pbc > 7", ERR_INVALID, dict(pbc=8, boxes=ORTHO)),
            ("box_stride other than 0 and 9", ERR_INVALID, dict(box_stride=3, boxes=ORTHO, pbc=7)),
            ("max_lag >= nframes", ERR_INVALID, dict(L=4)),
            ("origin_stride == 0", ERR_INVALID, dict(os=0)),
            ("an index not below natoms", ERR_INVALID, dict(tuples=[[0, 5]])),
            ("a label not below ngroups", ERR_INVALID, dict(labels=[2], G=2)),
            ("natoms == 0", ERR_INVALID, dict(natoms=0)),
            ("tuples == NULL", ERR_INVALID, dict(no_tuples=True)),
            ("a stride below 3 natoms", ERR_INVALID, dict(stride=14)),
            ("c2 in RAW mode", ERR_INVALID, dict(mode=RAW, c2=row)),
            ("c2_vec in RAW mode", ERR_INVALID, dict(mode=RAW, c2_vec=row, ld=1)),
            ("s2 in RAW mode", ERR_INVALID, dict(mode=RAW, s2=one)),
            ("pbc without boxes, kind 2", ERR_NO_PBC, dict(pbc=7)),
            ("pbc without boxes, kind 3", ERR_NO_PBC, dict(pbc=1, tuples=[[0, 1, 2]]))]
    return [(what, want, raw_tcf(fn, ctx, fr, real, **kw)) for what, want, kw in rows]
