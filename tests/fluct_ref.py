"""numpy reference of the trajectory fluctuations (molar_hip_fluct: mean structure, RMSF, positional covariance after an
optional fit), the acceptance bounds of the GPU tests, and the inputs those tests share.

The reference follows the definition in include/molar_hip.h by another route than the kernels: the rotation of a frame
comes from np.linalg.svd of the 3x3 covariance with the determinant correction (the kernels: Jacobi on Horn's 4x4 matrix), and
everything after the rotation - the fitted coordinates, the mean, the deviations, the covariance - is formed in np.longdouble
(2^-64 on x86), so the statistics of the reference carry no f64 rounding of their own.  A second rotation route, the
quaternion through np.linalg.eigh of Horn's matrix, exists only to measure the reference's own scatter (K_fit below).

Bounds (u = 2^-53, eps_out = 2^-24 for the f32 entry and 2^-53 for the f64 entry, F frames; s_i = sqrt(cov_ii), X the largest
|x - origin| of a selected atom: origin = the centre of frame 0 without a fit, the frame's own centre with one).  Derivation
for the route "z~ = fl(R (x - c)), m~ = fl(sum z~ / F), d~ = fl(z~ - m~), cov~ = fl(sum d~_i d~_j / F)":
  z~ = z + e with |e| <= e_z u X: one subtraction without a fit (e_z = 1); the subtraction, three products and two sums
       of the rotation with one (e_z = 8 covers gamma_5 sqrt(3) X and the two-norm of a row of R);
  m~ - m = mu with |mu| <= (F + 1) u X (gamma_F on the sum, one division), d~ = (d + e - mu)(1 + u);
  sum_f d_i (e_j - mu_j) / F:  the mu part vanishes exactly because the true deviations add up to zero, the e part is at
       most s_i e_z u X by Cauchy-Schwarz;  the second-order part is at most ((F + 2) u X)^2;
  the inner product itself: gamma_(F+2) sum |d_i d_j| / F <= (F + 2) u s_i s_j, and the roundings of d~ add 2 u s_i s_j.
With a fit the weighted centres c_f and c_ref are f64 sums of n terms of the size C = the largest |coordinate| of a selected
atom, formed as the kernels form them: each of 256 threads adds ceil(n / 256) terms in order, then a tree of depth 8.  A term
passes through at most N_c = ceil(n / 256) + 12 roundings (its product with the weight, the thread's chain, the tree, the
division and the same for the sum of the weights), so a centre carries up to N_c u C, which moves frame f as a whole - it
adds to e - and c_ref shifts the mean directly.  Without a fit the one origin is subtracted and added back, and its error
cancels.  With E = e_z u X (+ N_c u C with a fit) that gives
  |cov_ij - ref|   <= (F + 16) u s_i s_j + E (s_i + s_j) + ((F + 2) u X + E)^2 + 4 eps_out |ref|
  |mean - ref|     <= (F + 4) u X (+ 2 N_c u C with a fit) + eps_out |ref|
  |rmsf_k^2 - ref| <= (F + 16) u ref + 2 sqrt(3) E rmsf_k + 3 ((F + 2) u X + E)^2 + 4 eps_out ref
The issue that asked for this feature states these lines without the E and C terms; E is first order in the rounding of z
itself (x - origin is not exact in f64 when the origin carries 53 bits), does not cancel, and can exceed (F + 16) u s_i s_j
when the fluctuation s is small against the size X of the structure, so it is part of the bound here.
With a fit a rotation error dtheta_f ~ kappa u / g (g: the smallest relative gap (l1 - l2) / l1 of Horn's matrix over the
frames) moves atom i by dtheta r_i (r_i: its distance from the centre in the mean structure) and does not average out:
  cov gains K_fit u / g (r_i s_j + r_j s_i),  rmsf^2 gains K_fit u / g 2 r s,  mean gains K_fit u / g r,  R gains K_fit u / g.
K_fit is 8 times the largest discrepancy between the reference's two rotation routes over the inputs of this module, in
units of u / g, and at least 1 (k_fit(); the CPU test asserts K_fit <= 128).  The factor 8: the kernels' Jacobi route is a
third method, and the two numpy routes are both LAPACK.
The square of fit_out's rmsd is held to rmsd_matrix_ref's derived bound, (3 n + 16) u (rg2_f + rg2_ref) + 4 eps_out ref^2."""
import functools

import numpy as np

U = 2.0 ** -53
EPS64 = 2.0 ** -53
EPS32 = 2.0 ** -24
LD = np.longdouble

TILE_N_NOFIT = (1, 2, 5, 6, 21, 22, 43)          # 3n = 3, 6, 15, 18, 63, 66, 129: either side of 16, 64 and 128
TILE_N_FIT = (5, 6, 21, 22, 43)
TILE_F = (1, 2, 3, 4, 5, 16, 17, 33)


def random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return quat_to_matrix(q)


def quat_to_matrix(q):
    a, b, c, d = q
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


def random_frames(F, n, seed, sigma=0.05, size=1.0, shift=0.5, rigid=True, dtype=np.float32):
    """A seeded structure (normal cloud of n atoms, `size` nm) plus noise sigma per frame, each frame under a random proper
    rotation and a translation of `shift` nm (rigid=False: as it stands), rounded to f32."""
    rng = np.random.default_rng(seed)
    base = rng.normal(size=(n, 3)) * size
    out = np.empty((F, n, 3))
    for f in range(F):
        p = base + rng.normal(size=(n, 3)) * sigma
        out[f] = p @ random_rotation(rng).T + rng.normal(size=3) * shift if rigid else p
    return out.astype(np.float32).astype(dtype)


def _weights(natoms, idx, mass):
    idx = np.arange(natoms) if idx is None else np.asarray(idx, dtype=np.int64)
    w = np.ones(len(idx)) if mass is None else np.asarray(mass, dtype=np.float64)[idx]
    return idx, w


def horn(S):
    """Horn's 4x4 matrices of S[..., d, e] = sum w x_d y_e."""
    K = np.empty(S.shape[:-2] + (4, 4))
    xx, xy, xz = S[..., 0, 0], S[..., 0, 1], S[..., 0, 2]
    yx, yy, yz = S[..., 1, 0], S[..., 1, 1], S[..., 1, 2]
    zx, zy, zz = S[..., 2, 0], S[..., 2, 1], S[..., 2, 2]
    K[..., 0, 0] = xx + yy + zz; K[..., 0, 1] = yz - zy; K[..., 0, 2] = zx - xz; K[..., 0, 3] = xy - yx
    K[..., 1, 1] = xx - yy - zz; K[..., 1, 2] = xy + yx; K[..., 1, 3] = zx + xz
    K[..., 2, 2] = -xx + yy - zz; K[..., 2, 3] = yz + zy
    K[..., 3, 3] = -xx - yy + zz
    for i in range(4):
        for j in range(i):
            K[..., i, j] = K[..., j, i]
    return K


def rotations(x, y, w, route="svd"):
    """(R[F, 3, 3] with y ~ R x for the centred x[F, n, 3] and y[n, 3], g[F] the relative gaps of Horn's matrix)."""
    S = np.einsum("k,fkd,ke->fde", w, x, y)
    lam, vec = np.linalg.eigh(horn(S))
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(lam[:, 3] > 0, (lam[:, 3] - lam[:, 2]) / lam[:, 3], 0.0)
    if route == "eigh":
        # LAPACK's eigenvector as it is; normalised and turned into a matrix in longdouble, so that what is measured is the
        # eigen solver's scatter and not this formula's
        return np.stack([quat_to_matrix(v[:, 3].astype(LD) / np.sqrt((v[:, 3].astype(LD) ** 2).sum())) for v in vec]).astype(np.float64), g
    Uu, _, Vt = np.linalg.svd(np.swapaxes(S, 1, 2))            # sum w y x^T: R = U diag(1, 1, det) V^T
    d = np.sign(np.linalg.det(Uu @ Vt))
    D = np.zeros_like(S)
    D[:, 0, 0] = D[:, 1, 1] = 1.0
    D[:, 2, 2] = np.where(d != 0, d, 1.0)
    return polish(Uu @ D @ Vt, S), g


def _hat(v):
    z = np.zeros_like(v[..., 0])
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, -v[..., 0]], -1), np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def polish(R, S):
    """LAPACK's rotation made exact to longdouble: at the maximiser of sum w (R x) . y the matrix A = R^T sum w y x^T is
    symmetric, so Newton's step for R <- R exp([omega]) solves the linear [omega] A + A^T [omega] = A - A^T (three unknowns),
    followed by one step of R <- R (3 I - R^T R) / 2 against the loss of orthogonality.  Two rounds, all in longdouble."""
    R = R.astype(LD)
    M = np.swapaxes(S, 1, 2).astype(LD)
    eye = np.eye(3, dtype=LD)
    for _ in range(2):
        A = np.swapaxes(R, 1, 2) @ M
        rhs = A - np.swapaxes(A, 1, 2)
        b = np.stack([rhs[:, 2, 1], rhs[:, 0, 2], rhs[:, 1, 0]], -1)
        cols = []
        for k in range(3):
            G = _hat(eye[k][None]) @ A + np.swapaxes(A, 1, 2) @ _hat(eye[k][None])
            cols.append(np.stack([G[:, 2, 1], G[:, 0, 2], G[:, 1, 0]], -1))
        L = np.stack(cols, -1)                                      # L omega = b, by Cramer's rule (no longdouble solver in numpy)

        def det3(m):
            return (m[:, 0, 0] * (m[:, 1, 1] * m[:, 2, 2] - m[:, 1, 2] * m[:, 2, 1]) - m[:, 0, 1] * (m[:, 1, 0] * m[:, 2, 2] - m[:, 1, 2] * m[:, 2, 0])
                    + m[:, 0, 2] * (m[:, 1, 0] * m[:, 2, 1] - m[:, 1, 1] * m[:, 2, 0]))
        det = det3(L)
        ok = np.abs(det) > 0
        om = np.zeros_like(b)
        for k in range(3):
            Lk = L.copy()
            Lk[:, :, k] = b
            om[:, k] = np.where(ok, det3(Lk) / np.where(ok, det, 1), 0)
        H = _hat(om)
        R = R @ (eye + H + H @ H / 2)
        R = R @ (3 * eye - np.swapaxes(R, 1, 2) @ R) / 2
    return R


class Ref:
    pass


def fluct(frames, idx=None, mass=None, ref=None, fit=True, iterations=0, route="svd"):
    """The definition: Ref with mean [n, 3], rmsf [n], cov [3n, 3n], R [F, 3, 3], t [F, 3], rmsd [F] (float64, rounded from
    longdouble) and what the bounds need: g, r [3n], s [3n], X, rg2 [F], rg2_ref, F, n."""
    fr = np.asarray(frames, dtype=np.float64)
    F = fr.shape[0]
    idx_, w = _weights(fr.shape[1], idx, mass)
    n = len(idx_)
    W = w.sum()
    p = fr[:, idx_, :]
    wl = w.astype(LD)
    cl = (wl[None, :, None] * p.astype(LD)).sum(1) / wl.sum()          # the centres in longdouble: no gamma_n of the reference's own
    xl = p.astype(LD) - cl[:, None, :]
    c, x = cl.astype(np.float64), xl.astype(np.float64)
    r0 = p[0] if ref is None else np.asarray(ref, dtype=np.float64)
    out = Ref()
    out.F, out.n = F, n
    out.rg2 = (w[None, :] * (x * x).sum(-1)).sum(1) / W
    g = np.ones(F)
    for _ in range(1 + (iterations if fit else 0)):
        r0l = r0 if r0.dtype == LD else r0.astype(LD)
        crl = (wl[:, None] * r0l).sum(0) / wl.sum()
        cr = crl.astype(np.float64)
        y = (r0l - crl).astype(np.float64)
        if fit:
            R, g = rotations(x, y, w, route)
            z = np.einsum("fde,fke->fkd", R.astype(LD), xl) + crl
            t = (crl[None, :] - np.einsum("fde,fe->fd", R.astype(LD), cl)).astype(np.float64)
            R = R.astype(np.float64)
        else:
            R = np.broadcast_to(np.eye(3), (F, 3, 3)).copy()
            z = p.astype(LD)
            t = np.zeros((F, 3))
        diff = z - r0l[None]
        rmsd = np.sqrt(((w[None, :] * (diff * diff).sum(-1)).sum(1) / W).astype(np.float64))
        mean = z.sum(0) / F
        rg2_ref = float((w * (y * y).sum(-1)).sum() / W)
        if not fit:                                     # as rmsd_matrix_ref has it: without a fit both are taken about the common origin
            out.rg2 = (w[None, :] * ((p - c[0]) ** 2).sum(-1)).sum(1) / W
            rg2_ref = float((w * ((r0 - c[0]) ** 2).sum(-1)).sum() / W)
        last_ref = r0l.astype(np.float64)
        r0 = mean                                       # the next reference: the mean as it is, in longdouble
    d = (z - mean[None]).reshape(F, 3 * n)
    cov = (d.T @ d) / F
    out.mean = mean.astype(np.float64)
    out.cov = cov.astype(np.float64)
    out.rmsf = np.sqrt(((d * d).reshape(F, n, 3).sum(-1).sum(0) / F).astype(np.float64))
    out.R, out.t, out.rmsd, out.ref = R, t, rmsd, last_ref
    out.g = float(g.min()) if fit else 1.0
    out.rg2_ref = rg2_ref
    centre = out.mean.mean(0) if mass is None else (w[:, None] * out.mean).sum(0) / W
    out.r = np.repeat(np.linalg.norm(out.mean - centre, axis=1), 3)
    out.s = np.sqrt(np.diag(out.cov))
    origin = c[0][None, None, :] if not fit else c[:, None, :]
    out.X = float(np.sqrt(((p - origin) ** 2).sum(-1)).max())
    out.fit = bool(fit)
    out.cmax = float(max(np.abs(c).max(), np.abs(cr).max()))
    out.cabs = float(max(np.abs(p).max(), np.abs(last_ref).max()))
    return out


def bounds(ref, eps_out, k_fit):
    """(cov [3n, 3n], mean [n, 3], rmsf^2 [n], R scalar, rmsd^2 [F]) bounds of the module's docstring."""
    F, n, X, s = ref.F, ref.n, ref.X, ref.s
    centres = (-(-n // 256) + 12) * U * ref.cabs if ref.fit else 0.0
    E = (8.0 if ref.fit else 1.0) * U * X + centres
    second = ((F + 2) * U * X + E) ** 2
    rm = ref.rmsf
    b_cov = (F + 16) * U * np.outer(s, s) + E * (s[:, None] + s[None, :]) + second + 4 * eps_out * np.abs(ref.cov)
    b_mean = (F + 4) * U * X + 2 * centres + eps_out * np.abs(ref.mean)
    b_rmsf2 = (F + 16) * U * rm ** 2 + 2 * np.sqrt(3.0) * E * rm + 3 * second + 4 * eps_out * rm ** 2
    b_R = 0.0
    if ref.fit:
        kg = k_fit * U / max(ref.g, 1e-300)
        b_cov = b_cov + kg * (np.outer(ref.r, s) + np.outer(s, ref.r))
        ra = ref.r[::3]
        b_rmsf2 = b_rmsf2 + kg * 2 * ra * rm
        b_mean = b_mean + kg * ra[:, None]
        b_R = kg + 4 * eps_out
    b_rmsd2 = (3 * n + 16) * U * (ref.rg2 + ref.rg2_ref) + 4 * eps_out * ref.rmsd ** 2
    return b_cov, b_mean, b_rmsf2, b_R, b_rmsd2


def worst(err, lim):
    """The largest used fraction of a bound (inf where the bound is zero and the error is not)."""
    err, lim = np.broadcast_arrays(np.asarray(err, dtype=np.float64), np.asarray(lim, dtype=np.float64))
    if err.size == 0:
        return 0.0
    frac = np.where(err == 0.0, 0.0, err / np.where(lim > 0, lim, 1.0))
    frac = np.where((lim == 0) & (err > 0), np.inf, frac)
    return float(frac.max())


def check(got, ref, eps_out, k_fit, what="", limit=1.0, rotation=True):
    """Asserts every bound entry by entry on got = (mean, rmsf, cov or None, fit or None); returns the used fractions."""
    mean, rmsf, cov, fit = (None if a is None else np.asarray(a, dtype=np.float64) for a in got)
    b_cov, b_mean, b_rmsf2, b_R, b_rmsd2 = bounds(ref, eps_out, k_fit)
    used = {"mean": worst(np.abs(mean - ref.mean), b_mean), "rmsf2": worst(np.abs(rmsf ** 2 - ref.rmsf ** 2), b_rmsf2)}
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(rmsf)), f"{what}: non-finite results"
    if cov is not None:
        assert np.all(np.isfinite(cov)), f"{what}: non-finite covariance"
        used["cov"] = worst(np.abs(cov - ref.cov), b_cov)
    if fit is not None:
        used["rmsd2"] = worst(np.abs(fit[:, 12] ** 2 - ref.rmsd ** 2), b_rmsd2)
        if rotation:
            Rg = fit[:, :9].reshape(-1, 3, 3).transpose(0, 2, 1)                   # column-major records
            used["R"] = worst(np.abs(Rg - ref.R), b_R if ref.fit else 0.0)
            # t = c_ref - R c_f: the error of R times |c_f| (sqrt(3) for the three entries of a row), the f64 rounding of the
            # three products and sums on numbers of the size of the centres, and the rounding of the result
            b_t = (b_R - 4 * eps_out) * np.sqrt(3.0) * ref.cmax + 8 * U * ref.cmax + 4 * eps_out * np.abs(ref.t)
            used["t"] = worst(np.abs(fit[:, 9:12] - ref.t), b_t if ref.fit else 0.0)
    print(f"{what}: used fractions of the bounds " + ", ".join(f"{k} {v:.3g}" for k, v in used.items()))
    bad = {k: v for k, v in used.items() if not v <= limit}
    assert not bad, f"{what}: beyond the bound: {bad}"
    return used


def kernel_route(frames, idx=None, mass=None, ref=None, fit=True, iterations=0, fper=8):
    """The library's route restated in numpy f64: weighted centres, Horn's quaternion (eigh here), z' = R (x - c), the mean
    from partial sums over splits of `fper` frames added in order, the deviations about the finished mean, and the product
    accumulated in the kernel's blocks of four frames.  Returns (mean, rmsf, cov, fit[F, 13])."""
    fr = np.asarray(frames, dtype=np.float64)
    F = fr.shape[0]
    idx_, w = _weights(fr.shape[1], idx, mass)
    n = len(idx_)
    W = w.sum()
    p = fr[:, idx_, :]
    c = (w[None, :, None] * p).sum(1) / W
    r0 = p[0] if ref is None else np.asarray(ref, dtype=np.float64)
    for _ in range(1 + (iterations if fit else 0)):
        cr = (w[:, None] * r0).sum(0) / W
        y = r0 - cr
        gy = (w * (y * y).sum(-1)).sum()
        if fit:
            x = p - c[:, None, :]
            S = np.einsum("k,fkd,ke->fde", w, x, y)
            R, _ = rotations(x, y, w, "eigh")
            zp = np.einsum("fde,fke->fkd", R, x)
            o = cr
            gx = (w[None, :] * (x * x).sum(-1)).sum(1)
            d2 = gx + gy - 2 * np.einsum("fde,fed->f", R, S)
            t = cr[None, :] - np.einsum("fde,fe->fd", R, c)
        else:
            o = c[0]
            zp = p - o
            R = np.broadcast_to(np.eye(3), (F, 3, 3)).copy()
            t = np.zeros((F, 3))
            d2 = (w[None, :] * ((p - r0[None]) ** 2).sum(-1)).sum(1)
        part = [zp[f0:f0 + fper].sum(0) for f0 in range(0, F, fper)]
        m = functools.reduce(lambda a, b: a + b, part) / F
        r0 = o + m
    d = (zp - m[None]).reshape(F, 3 * n)
    cov = np.zeros((3 * n, 3 * n))
    for f0 in range(0, F, 4):
        cov += d[f0:f0 + 4].T @ d[f0:f0 + 4]
    cov /= F
    rmsf = np.sqrt((d * d).reshape(F, n, 3).sum(-1).sum(0) / F)
    rec = np.concatenate([R.transpose(0, 2, 1).reshape(F, 9), t, np.sqrt(np.maximum(d2, 0) / W)[:, None]], axis=1)
    return o + m, rmsf, cov, rec


def tile_case(F, n, fit):
    """The input of one tile-edge case of the GPU tests."""
    return random_frames(F, n, seed=100000 * int(fit) + 1000 * n + F, sigma=0.05, rigid=fit)


def named_inputs():
    """Every other input of the GPU tests that is fitted: name -> dict(frames, idx, mass, ref, iterations)."""
    rng = np.random.default_rng(77)
    out = {}
    frames = random_frames(19, 60, seed=5, sigma=0.08)
    idx = np.sort(rng.choice(60, size=37, replace=False)).astype(np.uint64)
    out["gaps"] = dict(frames=frames, idx=idx, mass=rng.uniform(1.0, 16.0, 60).astype(np.float32))
    mass = rng.uniform(1.0, 16.0, 50).astype(np.float32)
    mass[rng.choice(50, size=12, replace=False)] = 0.0
    out["zero masses"] = dict(frames=random_frames(12, 50, seed=6, sigma=0.06), mass=mass)
    out["iterated"] = dict(frames=random_frames(24, 40, seed=7, sigma=0.1), iterations=2)
    out["given reference"] = dict(frames=random_frames(8, 30, seed=8, sigma=0.05), ref=random_frames(1, 30, seed=8, sigma=0.0, rigid=False)[0])
    out["plain 257"] = dict(frames=random_frames(9, 257, seed=9, sigma=0.05))
    return out


def split_case(F, n=5):
    return random_frames(F, n, seed=4242 + F, sigma=0.05)


def route_discrepancy(frames, idx=None, mass=None, ref=None, iterations=0):
    """The largest difference between the rotations of the two routes, frame by frame in units of u / g_f."""
    a = fluct(frames, idx, mass, ref, True, iterations, "svd")
    fr = np.asarray(frames, dtype=np.float64)
    idx_, w = _weights(fr.shape[1], idx, mass)
    p = fr[:, idx_, :]
    W = w.sum()
    x = p - ((w[None, :, None] * p).sum(1) / W)[:, None, :]
    y = a.ref - (w[:, None] * a.ref).sum(0) / W
    R1, g = rotations(x, y, w, "svd")
    R2, _ = rotations(x, y, w, "eigh")
    return float((np.abs(R1 - R2).max(axis=(1, 2)) * g / U).max())


@functools.lru_cache(maxsize=None)
def split_frames(n=5):
    """(F with the frames of the covariance split over at least three workgroups, F of the same n without a split), both from
    the plan function (a host function: no GPU is needed)."""
    from molar_amd import api
    F = 256
    while api.fluct_plan(F, n, True)[1] < 3:
        F *= 2
        assert F <= 1 << 20, "the plan never splits the frames"
    small = F
    while api.fluct_plan(small, n, True)[1] > 1:
        small //= 2
    return F, small


@functools.lru_cache(maxsize=None)
def k_fit():
    """(K_fit, the largest discrepancy it comes from, the input that gave it) over the module's fitted inputs."""
    worst_units, where = 0.0, ""
    cases = [(f"tile F={F} n={n}", dict(frames=tile_case(F, n, True))) for n in TILE_N_FIT for F in TILE_F]
    cases += list(named_inputs().items())
    cases += [(f"split F={F}", dict(frames=split_case(max(split_frames()))[:F])) for F in split_frames()]
    for name, kw in cases:
        units = route_discrepancy(**kw)
        if units > worst_units:
            worst_units, where = units, name
    return max(1.0, 8.0 * worst_units), worst_units, where
