"""numpy reference of the mean-squared displacement (molar_hip_msd: no-jump unwrap along time, particle displacements, drift
removal, MSD / fourth moment / per-particle curves over all time origins), the acceptance bounds of the GPU tests, and the
inputs those tests share.

The reference follows the definition in include/molar_hip.h by another route than the kernels, in np.longdouble (2^-64 on
x86) throughout:
  * unwrap, route "round" (any box, any mask; what the definition prescribes unless the box is triclinic AND the mask full):
    the fractional step inv s with a longdouble inverse of the box (numpy's f64 inverse polished by two Newton steps
    X <- X (2 I - M X) in longdouble), minus its rounding half away from zero on the periodic dimensions, times the box;
  * unwrap, route "brute" (full mask): the shortest of the 125 images s - (i a + j b + k c), i, j, k in -2 .. 2;
  * the lag sums by vectorised slices U[tau::os] - U[:F - tau:os], never a chain over the origins.
It ASSERTS on its inputs that the image is unambiguous - every fractional step component within 0.47 of an integer (route
"round"), the second-best image longer than the best by more than 1e-6 nm (route "brute") - so that a kernel that disagrees
is wrong, not unlucky.

Bounds (u = 2^-53; eps_out = 2^-24 for the f32 entry, 2^-53 for the f64 entry; F frames; nd = number of components in
msd_dims).  Quantities of the input, all taken from the reference itself:
  B      the largest norm of a box vector or of a raw step x(f) - x(f-1) (a step across the box edge is a box vector long);
  kappa  the largest row sum of |M| |M^-1| over the boxes (1 for an orthorhombic box, below 2 for the skewed boxes here);
  Ua     the largest |u_k(f)| component-wise norm of an ATOM (selection and reference set), Umax >= every |U_g| likewise;
  n_g    the largest group, n_r the reference set.
c_b counts the roundings of shortest_vector (boxmath.hpp) in units of u B on one component of d:
  the inverse by cofactors (two products and a difference per cofactor, five roundings in the determinant, one division: 9),
  f = inv s (three products, two sums: 3) - both act on |s| <= B through |M| |M^-1|, hence (9 + 3) kappa;  f - round(f) is
  exact;  start = M f' (3, again through kappa: |M| |f'| <= kappa |d|-ish, taken at B);  the triclinic search adds a shift
  that itself carries two roundings per component of a vector of at most 3 B (6) and one for the sum (1);  one more for the
  exact-input difference s of the f64 entry (f32 inputs are exact in f64, f64 inputs round once: 1).
  c_b = 15 kappa + 8.
A particle displacement:  u_k(f) is a chain of f additions, each rounding at most u Ua, over steps that each carry
c_b u B;  the group's mean is n_g products, n_g - 1 additions (a tree or pieces pass a term through fewer) and a division:
  E_P = F (c_b u B + u Ua) + (n_g + 2) u Ua            [+ the same with n_r for the drift D(f), + u Ua for its subtraction]
  |disp - ref| <= E_P + eps_out |ref|                  per component.
Ua, not the largest |U_g|, stands in both places: the chain's roundings scale with the ATOM's own |u|, which exceeds |U_g|
when a group's atoms move apart or when the drift is removed.
Lag sums:  Delta = U(t + tau) - U(t) carries 2 E_P + u |Delta| per component, so r^2 = sum_d Delta_d^2 carries
4 sqrt(nd) E_P r + 4 nd E_P^2 + (nd + 2) u r^2 (Cauchy-Schwarz over the components; the factor sqrt(nd) is there because
E_P bounds ONE component and the error vector of nd of them is sqrt(nd) longer).  Averaged over origins and
particles, mean(r) <= sqrt(mean r^2) = sqrt(ref).  A term then passes through the kernel's own summation order: the chain over the
count[tau] origins of one particle, the chain over the particle_chunk particles of a workgroup, the chain over the chunks,
the product P count and the division:
  N_S = count[tau] + particle_chunk + nchunks + nd + 6
  |msd[tau] - ref|        <= N_S u ref + 4 sqrt(nd) E_P sqrt(ref) + 4 nd E_P^2 + eps_out ref
  |msd_particle - ref_g|  <= (count[tau] + nd + 6) u ref_g + 4 sqrt(nd) E_P sqrt(ref_g) + 4 nd E_P^2 + eps_out ref_g
r^4 = (r^2)^2 doubles the relative error of r^2 and adds its square; with e = 4 sqrt(nd) E_P r + 4 nd E_P^2 the error is
2 r^2 e + e^2, and mean(r^3) <= ref4^(3/4), mean(r^2) <= ref4^(1/2), mean(r) <= ref4^(1/4) (power means):
  |m4[tau] - ref4| <= (N_S + nd + 4) u ref4 + 8 sqrt(nd) E_P ref4^(3/4) + 24 nd E_P^2 ref4^(1/2)
                      + 32 nd^(3/2) E_P^3 ref4^(1/4) + 16 nd^2 E_P^4 + eps_out ref4."""
import functools

import numpy as np

U = 2.0 ** -53
EPS64 = 2.0 ** -53
EPS32 = 2.0 ** -24
LD = np.longdouble

ORTHO = np.array([3.0, 0, 0, 0, 3.5, 0, 0, 0, 4.0])                      # column-major box9: columns a, b, c
TRICLINIC = np.array([3.0, 0, 0, 0.9, 3.2, 0, -0.7, 1.1, 3.6])           # a GROMACS-like skewed cell


def box_matrix(box9):
    return np.asarray(box9, dtype=np.float64).reshape(3, 3).T               # M[:, c] = column c


def wrap(x, boxes):
    """positions [F, n, 3] wrapped into the box of their frame (boxes: [9] or [F, 9])."""
    boxes = np.asarray(boxes, np.float64)
    out = np.empty_like(x)
    for f in range(x.shape[0]):
        M = box_matrix(boxes if boxes.ndim == 1 else boxes[f])
        fr = np.linalg.solve(M, x[f].T).T
        out[f] = (M @ (fr - np.floor(fr)).T).T
    return out


def wrap_ortho(x, box9):
    """positions wrapped into one orthorhombic box as x - L floor(x / L): exact when x and L are binary fractions of one grid."""
    L = np.asarray(box9, np.float64)[[0, 4, 8]]
    return x - L * np.floor(x / L)


def grid_walk(F, n, seed, box9=ORTHO, step=0.45):
    """An unwrapped walk on the grid of multiples of 2^-10 (steps within +-step of the box), exactly representable in f32 both
    as it is and wrapped into the box (whose edges are on the grid too)."""
    rng = np.random.default_rng(seed)
    cells = (np.asarray(box9, np.float64)[[0, 4, 8]] * 1024).astype(np.int64)
    lim = (cells * step).astype(np.int64)
    x0 = rng.integers(0, cells, size=(n, 3))
    steps = rng.integers(-lim, lim + 1, size=(F - 1, n, 3))
    x = np.concatenate([x0[None], x0[None] + np.cumsum(steps, axis=0)], axis=0) / 1024.0
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
    return x


def random_walk(F, n, seed, box9=ORTHO, step=0.45, start_in_box=True):
    """An unwrapped f64 walk [F, n, 3]: steps uniform in +-step of the box in every fractional coordinate."""
    rng = np.random.default_rng(seed)
    M = box_matrix(box9)
    x0 = (M @ rng.random((n, 3)).T).T if start_in_box else np.zeros((n, 3))
    steps = (M @ rng.uniform(-step, step, size=(F - 1, n, 3)).reshape(-1, 3).T).T.reshape(F - 1, n, 3) if F > 1 else np.zeros((0, n, 3))
    return np.concatenate([x0[None], x0[None] + np.cumsum(steps, axis=0)], axis=0)


def wrapped_walk(F, n, seed, box9=ORTHO, step=0.45, dtype=np.float32, boxes=None):
    """(frames wrapped and rounded to f32 (then cast to dtype), the unwrapped walk they came from)."""
    x = random_walk(F, n, seed, box9, step)
    return np.ascontiguousarray(wrap(x, box9 if boxes is None else boxes).astype(np.float32).astype(dtype)), x


def scaled_boxes(F, seed, box9=ORTHO, amount=0.02):
    rng = np.random.default_rng(seed)
    return np.asarray(box9)[None, :] * (1.0 + rng.uniform(-amount, amount, size=(F, 1)))


def ld_inverse(M):
    X = np.linalg.inv(M).astype(LD)
    A = M.astype(LD)
    eye = np.eye(3, dtype=LD)
    for _ in range(2):
        X = X @ (2 * eye - A @ X)
    return X


def round_away(x):
    return np.sign(x) * np.floor(np.abs(x) + LD(0.5))


def min_image(s, box9, pbc, route):
    """shortest_vector_dims of the steps s [m, 3] (longdouble) by the named route; asserts that the image is unambiguous."""
    M = box_matrix(box9).astype(LD)
    if route == "round":
        f = s @ ld_inverse(box_matrix(box9)).T
        for d in range(3):
            if pbc >> d & 1:
                r = round_away(f[:, d])
                assert np.all(np.abs(f[:, d] - r) <= 0.47), "a fractional step within 0.03 of a half: the image is ambiguous"
                f[:, d] -= r
        return f @ M.T
    assert route == "brute" and pbc == 7
    g = np.arange(-2, 3)
    ijk = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(LD)
    cand = s[:, None, :] - (ijk @ M.T)[None, :, :]
    n2 = np.sqrt((cand * cand).sum(-1))
    order = np.argsort(n2, axis=1)
    best, second = np.take_along_axis(n2, order[:, :1], 1)[:, 0], np.take_along_axis(n2, order[:, 1:2], 1)[:, 0]
    assert np.all(second - best > 1e-6), "two images within 1e-6 nm: the image is ambiguous"
    inner = np.all(np.abs(np.take_along_axis(ijk[None].repeat(len(s), 0), order[:, :1, None].repeat(3, 2), 1)[:, 0]) < 2, axis=1)
    assert np.all(inner), "the shortest image lies on the rim of the searched images"
    return np.take_along_axis(cand, order[:, :1, None].repeat(3, 2), 1)[:, 0]


def is_ortho(box9):
    b = np.asarray(box9)
    return all(b[i] == 0 for i in (1, 2, 3, 5, 6, 7))


def unwrap(frames, boxes, pbc, route=None):
    """u [F, natoms, 3] in longdouble: the no-jump displacements of every atom, and the raw steps' largest norm."""
    x = np.asarray(frames).astype(LD)
    F = x.shape[0]
    u = np.zeros_like(x)
    big = 0.0
    for f in range(1, F):
        s = x[f] - x[f - 1]
        big = max(big, float(np.sqrt((s * s).sum(-1)).max()))
        if boxes is None or pbc == 0:
            d = s
        else:
            b = np.asarray(boxes, np.float64)
            b = b if b.ndim == 1 else b[f]
            r = route or ("brute" if pbc == 7 and not is_ortho(b) else "round")
            d = min_image(s, b, pbc, r)
        u[f] = u[f - 1] + d
    return u, big


def dims_list(dims):
    return [d for d in range(3) if dims >> d & 1]


def particles(u, natoms, idx, mass, groups):
    idx = np.arange(natoms) if idx is None else np.asarray(idx, dtype=np.int64)
    w = (np.ones(natoms) if mass is None else np.asarray(mass, np.float64)).astype(LD)[idx]
    us = u[:, idx, :]
    if groups is None:
        return us * w[None, :, None] / w[None, :, None], 1, us
    off = np.asarray(groups, dtype=np.int64)
    Ug = np.stack([(us[:, a:b] * w[None, a:b, None]).sum(1) / w[a:b].sum() for a, b in zip(off[:-1], off[1:])], axis=1)
    return Ug, int(np.diff(off).max()), us


def msd(frames, idx=None, mass=None, boxes=None, pbc=7, groups=None, ref_idx=None, max_lag=None, origin_stride=1, dims=7, route=None):
    """The reference: a dict with disp [F, P, 3], msd, m4 [L + 1], msd_particle [P, L + 1], count [L + 1] in longdouble and
    the quantities the bounds need."""
    frames = np.asarray(frames)
    F, natoms = frames.shape[:2]
    L = F - 1 if max_lag is None else max_lag
    u, big = unwrap(frames, boxes, pbc, route)
    Ug, n_g, us = particles(u, natoms, idx, mass, groups)
    ua = float(np.abs(us).max()) if us.size else 0.0
    n_r = 0
    if ref_idx is not None and len(ref_idx):
        D, n_r, ur = particles(u, natoms, ref_idx, mass, np.array([0, len(ref_idx)]))
        Ug = Ug - D
        ua = max(ua, float(np.abs(ur).max()))
    P = Ug.shape[1]
    comp = dims_list(dims)
    out_msd, out_m4, count = np.zeros(L + 1, LD), np.zeros(L + 1, LD), np.zeros(L + 1, np.int64)
    per = np.zeros((P, L + 1), LD)
    for tau in range(L + 1):
        d = Ug[tau::origin_stride][: len(Ug[: F - tau: origin_stride])] - Ug[: F - tau: origin_stride]
        r2 = (d[..., comp] ** 2).sum(-1)                                   # [origins, P]
        count[tau] = r2.shape[0]
        per[:, tau] = r2.mean(0)
        out_msd[tau] = r2.mean()
        out_m4[tau] = (r2 * r2).mean()
    kappa, bvec = 1.0, 0.0
    if boxes is not None and pbc:
        bs = np.asarray(boxes, np.float64).reshape(-1, 9)
        for b in bs:
            M = box_matrix(b)
            kappa = max(kappa, float((np.abs(M) @ np.abs(np.linalg.inv(M))).sum(1).max()))
            bvec = max(bvec, float(np.sqrt((M * M).sum(0)).max()))
    return dict(disp=Ug, msd=out_msd, m4=out_m4, msd_particle=per, count=count, B=max(big, bvec), kappa=kappa, Ua=ua, n_g=n_g, n_r=n_r,
                F=F, P=P, nd=len(comp), f64_inputs=frames.dtype == np.float64)


def e_p(ref):
    c_b = 15.0 * ref["kappa"] + 8.0
    F, B, Ua = ref["F"], ref["B"], ref["Ua"]
    e = F * (c_b * U * B + U * Ua) + (ref["n_g"] + 2) * U * Ua
    if ref["n_r"]:
        e += F * (c_b * U * B + U * Ua) + (ref["n_r"] + 2) * U * Ua + U * Ua
    return e


def bounds(ref, eps_out, particle_chunk=1, nchunks=None):
    """(disp, msd, m4, msd_particle) bounds, each of the shape of its output."""
    E = e_p(ref)
    nd = ref["nd"]
    nchunks = -(-ref["P"] // particle_chunk) if nchunks is None else nchunks
    cnt = ref["count"].astype(np.float64)
    r = np.abs(ref["msd"].astype(np.float64))
    r4 = np.abs(ref["m4"].astype(np.float64))
    rp = np.abs(ref["msd_particle"].astype(np.float64))
    n_s = cnt + particle_chunk + nchunks + nd + 6
    b_disp = E + eps_out * np.abs(ref["disp"].astype(np.float64))
    b_msd = n_s * U * r + 4 * np.sqrt(nd) * E * np.sqrt(r) + 4 * nd * E * E + eps_out * r
    b_par = (cnt + nd + 6)[None, :] * U * rp + 4 * np.sqrt(nd) * E * np.sqrt(rp) + 4 * nd * E * E + eps_out * rp
    b_m4 = ((n_s + nd + 4) * U * r4 + 8 * np.sqrt(nd) * E * r4 ** 0.75 + 24 * nd * E * E * np.sqrt(r4) + 32 * nd ** 1.5 * E ** 3 * r4 ** 0.25
            + 16 * nd * nd * E ** 4 + eps_out * r4)
    return b_disp, b_msd, b_m4, b_par


def worst(err, lim):
    """the largest used fraction of a bound; an error where the bound is zero must be zero."""
    err, lim = np.asarray(err, np.float64), np.asarray(lim, np.float64)
    if err.size == 0:
        return 0.0
    assert not np.any(np.isnan(err)), "NaN where a number is expected"
    zero = lim == 0
    assert np.all(err[zero] == 0), "an error where the bound is zero"
    return float((err[~zero] / lim[~zero]).max()) if np.any(~zero) else 0.0


REPORT = {}          # output and entry -> the largest used fraction seen by check()


def check(got, ref, eps_out, particle_chunk=1, nchunks=None, what=""):
    """got: (msd, m4, msd_particle, disp), entries may be None.  Prints the used fractions before it asserts."""
    b_disp, b_msd, b_m4, b_par = bounds(ref, eps_out, particle_chunk, nchunks)
    used = {}
    for name, g, r, b in (("msd", got[0], ref["msd"], b_msd), ("m4", got[1], ref["m4"], b_m4), ("msd_particle", got[2], ref["msd_particle"], b_par),
                          ("disp", got[3], ref["disp"], b_disp)):
        if g is None:
            continue
        g = np.asarray(g)
        assert g.shape == r.shape, f"{what}: {name} has shape {g.shape}, expected {r.shape}"
        used[name] = worst(np.abs(g.astype(LD) - r).astype(np.float64), b)
        key = name + (" f32" if eps_out == EPS32 else " f64")
        REPORT[key] = max(REPORT.get(key, 0.0), used[name])
    print(f"msd bounds used {what}: " + " ".join(f"{k}={v:.3g}" for k, v in used.items()))
    for name, v in used.items():
        assert v <= 1.0, f"{what}: {name} uses {v:.3g} of its bound"
    if got[0] is not None and not np.isnan(np.asarray(got[0])[0]):
        assert np.asarray(got[0])[0] == 0, "msd[0] is exactly 0"
    return used


# ---------------------------------------------------------------- the kernels' route restated in f64 (CPU test of the bounds)

def _inverse3(M):
    m11, m21, m31, m12, m22, m32, m13, m23, m33 = (M[0, 0], M[1, 0], M[2, 0], M[0, 1], M[1, 1], M[2, 1], M[0, 2], M[1, 2], M[2, 2])
    mi1, mi2, mi3 = m22 * m33 - m32 * m23, m21 * m33 - m31 * m23, m21 * m32 - m31 * m22
    det = (m11 * mi1 - m12 * mi2) + m13 * mi3
    return np.array([[mi1 / det, (m13 * m32 - m33 * m12) / det, (m12 * m23 - m22 * m13) / det],
                     [-mi2 / det, (m11 * m33 - m31 * m13) / det, (m13 * m21 - m23 * m11) / det],
                     [mi3 / det, (m12 * m31 - m32 * m11) / det, (m11 * m22 - m21 * m12) / det]])


def _shifts(M):
    a, b, c = M[:, 0], M[:, 1], M[:, 2]
    ln = lambda v: np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    longest = max(ln((a + b) + c), ln((a + b) - c), ln((a - b) + c), ln((-a + b) + c))
    bound2 = (2.0 * (0.5 * longest)) ** 2
    out = []
    for i in (-1, 0, 1):
        for j in (-1, 0, 1):
            for k in (-1, 0, 1):
                s = (i * a + j * b) + k * c
                if (i or j or k) and (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2] < bound2:
                    out.append(s)
    return out


def _matvec(M, v):
    return np.stack([(M[r, 0] * v[:, 0] + M[r, 1] * v[:, 1]) + M[r, 2] * v[:, 2] for r in range(3)], -1)


def kernel_route(frames, idx=None, mass=None, boxes=None, pbc=7, groups=None, ref_idx=None, max_lag=None, origin_stride=1, dims=7):
    """(msd, m4, msd_particle, disp) in plain f64, operation by operation as msd.hip orders them (sequential chains)."""
    x = np.asarray(frames).astype(np.float64)
    F, natoms = x.shape[:2]
    L = F - 1 if max_lag is None else max_lag
    u = np.zeros_like(x)
    for f in range(1, F):
        d = x[f] - x[f - 1]
        if boxes is not None and pbc:
            b = np.asarray(boxes, np.float64)
            M = box_matrix(b if b.ndim == 1 else b[f])
            fr = _matvec(_inverse3(M), d)
            for k in range(3):
                if pbc >> k & 1:
                    fr[:, k] -= np.sign(fr[:, k]) * np.floor(np.abs(fr[:, k]) + 0.5)
            d = _matvec(M, fr)
            if pbc == 7 and not is_ortho(M.T.reshape(9)):
                best, best2 = d.copy(), (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                for s in _shifts(M):
                    c = d + s[None]
                    n2 = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
                    m = n2 < best2
                    best[m], best2[m] = c[m], n2[m]
                d = best
        u[f] = u[f - 1] + d

    def centre(sel, off):
        sel = np.arange(natoms) if sel is None else np.asarray(sel, np.int64)
        w = (np.ones(natoms) if mass is None else np.asarray(mass, np.float64))[sel]
        off = np.arange(len(sel) + 1) if off is None else np.asarray(off, np.int64)
        out = np.zeros((F, len(off) - 1, 3))
        for g, (a, b) in enumerate(zip(off[:-1], off[1:])):
            s, W = np.zeros((F, 3)), 0.0
            for k in range(a, b):
                s, W = s + w[k] * u[:, sel[k]], W + w[k]
            out[:, g] = s / W
        return out

    Ug = centre(idx, groups)
    if ref_idx is not None and len(ref_idx):
        Ug = Ug - centre(ref_idx, np.array([0, len(ref_idx)]))
    comp = dims_list(dims)
    P = Ug.shape[1]
    o_msd, o_m4, per = np.zeros(L + 1), np.zeros(L + 1), np.zeros((P, L + 1))
    for tau in range(L + 1):
        s2, s4, cnt = np.zeros(P), np.zeros(P), 0
        for t in range(0, F - tau, origin_stride):
            e = Ug[t + tau][:, comp] - Ug[t][:, comp]
            r2 = np.zeros(P)
            for k in range(e.shape[1]):
                r2 = r2 + e[:, k] * e[:, k]
            s2, s4, cnt = s2 + r2, s4 + r2 * r2, cnt + 1
        per[:, tau] = s2 / cnt
        a = b = 0.0
        for g in range(P):
            a, b = a + s2[g], b + s4[g]
        o_msd[tau], o_m4[tau] = a / (P * cnt), b / (P * cnt)
    return o_msd, o_m4, per, Ug


# ---------------------------------------------------------------- shared inputs

def ballistic(F, n, seed, dtype=np.float32):
    """x_k(f) = x_k(0) + v_k f on a grid of exactly representable numbers (multiples of 2^-10 below 2^13): the f32 inputs are
    exact, so msd[tau] = mean |v|^2 tau^2 exactly in the reals.  Returns (frames, v)."""
    rng = np.random.default_rng(seed)
    v = rng.integers(-8, 9, size=(n, 3)) / 1024.0
    x0 = rng.integers(0, 1024, size=(n, 3)) / 1024.0
    x = x0[None] + v[None] * np.arange(F)[:, None, None]
    fr = x.astype(np.float32)
    assert np.array_equal(fr.astype(np.float64), x)
    return fr.astype(dtype), v


def groups_unequal(n):
    """CSR of groups of sizes 1, 2, .. 9, 1, 2, .. over n atoms (the last one cut)."""
    off, k = [0], 0
    while off[-1] < n:
        off.append(min(n, off[-1] + 1 + k % 9))
        k += 1
    return np.array(off, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def frames_case(F, P=3, seed=None):
    """The walk of the frame-count tests: P single-atom particles in the orthorhombic box."""
    fr, _ = wrapped_walk(F, P, 1000 + F if seed is None else seed)
    return fr


# ---------------------------------------------------------------- the C entry spelt out, and the errors its arguments alone decide

ERR_SIZES, ERR_ZERO_MASS, ERR_NO_PBC, ERR_ZERO_LENGTH, ERR_INVERSE, ERR_INVALID, ERR_TOO_LARGE = 1, 2, 4, 5, 6, 50, 51


def raw_msd(fn, ctx, frames, real=np.float32, **kw):
    """The C entry with every argument spelt out; returns the status."""
    frames = np.ascontiguousarray(frames, dtype=real)
    F, natoms = frames.shape[:2]
    keep = []

    def addr(x, dtype):
        if x is None:
            return None
        a = np.ascontiguousarray(x, dtype=dtype)
        keep.append(a)
        return a.ctypes.data

    keep.append(frames)
    g = kw.get
    out = [g(k) for k in ("msd", "m4", "mp", "disp")]
    return fn(ctx, frames.ctypes.data, g("F", F), g("stride", 3 * natoms), g("natoms", natoms), addr(g("idx"), np.uint64), g("n", natoms),
              addr(g("mass"), real), addr(g("boxes"), real), g("box_stride", 0), g("pbc", 0), addr(g("off"), np.uint64), g("P", 0),
              addr(g("ref"), np.uint64), g("nref", 0), g("L", 0), g("os", 1), g("dims", 7),
              *(None if o is None else o.ctypes.data for o in out[:3]), g("ld", 0), None if out[3] is None else out[3].ctypes.data)


def argument_errors(fn, ctx, real=np.float32):
    """Every error of the definition's table that the arguments alone decide: (what, expected status, got status)."""
    fr = np.zeros((4, 5, 3), real)
    mp = np.zeros((5, 2), real)
    rows = [("n == 0", ERR_SIZES, dict(n=0)),
            ("ld too small", ERR_SIZES, dict(L=2, mp=mp, ld=2)),
            ("offsets decrease", ERR_SIZES, dict(off=[0, 3, 2, 5], P=3)),
            ("an empty group", ERR_SIZES, dict(off=[0, 2, 2, 5], P=3)),
            ("offsets do not end at n", ERR_SIZES, dict(off=[0, 2, 4], P=2)),
            ("max_lag >= nframes", ERR_INVALID, dict(L=4)),
            ("origin_stride == 0", ERR_INVALID, dict(os=0)),
            ("msd_dims == 0", ERR_INVALID, dict(dims=0)),
            ("msd_dims > 7", ERR_INVALID, dict(dims=8)),
            ("an index not below natoms", ERR_INVALID, dict(idx=[0, 5], n=2)),
            ("a reference index not below natoms", ERR_INVALID, dict(ref=[7], nref=1)),
            ("a stride below 3 natoms", ERR_INVALID, dict(stride=14)),
            ("natoms == 0", ERR_INVALID, dict(natoms=0, idx=[0], n=1)),
            ("pbc without boxes", ERR_NO_PBC, dict(pbc=7))]
    return [(what, want, raw_msd(fn, ctx, fr, real, **kw)) for what, want, kw in rows]
