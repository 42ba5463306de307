"""numpy f64 reference of the all-pairs RMSD matrix (molar_hip_rmsd_matrix), pair by pair (a row of pairs at a time, for
speed) and WITHOUT the cancellation of the Gram route: weighted centres, np.linalg.svd of the 3x3 covariance with the determinant correction, the rotation applied,
sqrt(sum w |R x_a - x_b|^2 / sum w).  Also the acceptance bound of the GPU tests, which follows from f64 rounding alone."""
import numpy as np

EPS64 = 2.0 ** -53
EPS32 = 2.0 ** -24


def _weights(natoms, idx, mass):
    idx = np.arange(natoms) if idx is None else np.asarray(idx, dtype=np.int64)
    w = np.ones(len(idx)) if mass is None else np.asarray(mass, dtype=np.float64)[idx]
    return idx, w


def centred(frames, idx=None, mass=None):
    """(x[F, n, 3] about the weighted centres, w[n], rg2[F] = sum w |x|^2 / sum w), all float64."""
    frames = np.asarray(frames, dtype=np.float64)
    idx, w = _weights(frames.shape[1], idx, mass)
    p = frames[:, idx, :]
    W = w.sum()
    c = (w[None, :, None] * p).sum(1) / W
    x = p - c[:, None, :]
    rg2 = (w[None, :] * (x * x).sum(-1)).sum(1) / W
    return x, w, rg2


def fit_pair(xa, xb, w):
    """RMSD of the centred xa after the best PROPER rotation onto the centred xb."""
    cov = (w[:, None] * xb).T @ xa                      # sum w x_b x_a^T: R = U diag(1, 1, det) V^T maximises tr(R^T cov)
    U, _, Vt = np.linalg.svd(cov)
    d = np.sign(np.linalg.det(U @ Vt))
    R = U @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ Vt
    diff = xa @ R.T - xb
    return np.sqrt((w * (diff * diff).sum(-1)).sum() / w.sum())


class Block:
    """A centred block xb[F, n, 3] laid out for fit_row: the weighted transposes stacked [3 F, n] and the atoms first [n, F, 3]."""

    def __init__(self, xb, w):
        self.F = len(xb)
        self.wt = np.ascontiguousarray((w[None, :, None] * xb).transpose(0, 2, 1)).reshape(3 * self.F, -1)
        self.atoms_first = np.ascontiguousarray(xb.transpose(1, 0, 2))


def fit_row(xa, blk, w, first=0):
    """fit_pair of the centred xa against frames first.. of a Block at once: the same operations, two matrix products for
    the whole row (the difference R x_a - x_b is still formed atom by atom, so nothing cancels)."""
    nb = blk.F - first
    cov = (blk.wt[3 * first:] @ xa).reshape(nb, 3, 3)                  # cov[b] = sum w x_b x_a^T
    U, _, Vt = np.linalg.svd(cov)
    d = np.sign(np.linalg.det(U @ Vt))
    D = np.zeros((nb, 3, 3))
    D[:, 0, 0] = D[:, 1, 1] = 1.0
    D[:, 2, 2] = np.where(d != 0, d, 1.0)
    R = U @ D @ Vt
    diff = (xa @ R.transpose(2, 0, 1).reshape(3, 3 * nb)).reshape(-1, nb, 3) - blk.atoms_first[:, first:]      # (R_b x_a)_d = sum_e R_b[d][e] x_a[e]
    diff *= diff
    return np.sqrt(w @ diff.sum(-1) / w.sum())


def matrix(frames1, frames2=None, idx=None, mass=None, fit=True):
    """(ref[F1, F2], rg2_1[F1], rg2_2[F2]); frames2 = None: frames1 against itself.  With fit=False rg2 is taken about the
    centre of frame 0 of the first block, the origin the library subtracts."""
    f1 = np.asarray(frames1, dtype=np.float64)
    f2 = f1 if frames2 is None else np.asarray(frames2, dtype=np.float64)
    idx_, w = _weights(f1.shape[1], idx, mass)
    W = w.sum()
    out = np.zeros((f1.shape[0], f2.shape[0]))
    if fit:
        x1, _, rg1 = centred(f1, idx, mass)
        x2, _, rg2 = (x1, w, rg1) if frames2 is None else centred(f2, idx, mass)
        blk = Block(x2, w)
        for a in range(f1.shape[0]):
            if frames2 is None:                         # one block: the pairs b >= a, mirrored (the fit of a onto b and of b onto a
                out[a, a:] = fit_row(x1[a], blk, w, a)  # leave the same distance)
                out[a:, a] = out[a, a:]
            else:
                out[a] = fit_row(x1[a], blk, w)
        return out, rg1, rg2
    p1, p2 = f1[:, idx_, :], f2[:, idx_, :]
    for a in range(f1.shape[0]):
        d = p1[a][None, :, :] - p2
        out[a] = np.sqrt((w[None, :] * (d * d).sum(-1)).sum(1) / W)
    o = (w[:, None] * p1[0]).sum(0) / W
    rg1 = (w[None, :] * ((p1 - o) ** 2).sum(-1)).sum(1) / W
    rg2 = (w[None, :] * ((p2 - o) ** 2).sum(-1)).sum(1) / W
    return out, rg1, rg2


def bound(ref, rg2_1, rg2_2, n, eps_out):
    """|got^2 - ref^2| <= (3 n + 16) 2^-53 (rg2_a + rg2_b) + 4 eps_out ref^2: gamma_n on each of the 11 inner products (nine of
    the covariance, two of G), Cauchy-Schwarz on the covariance, |dK|_F <= 2 |dC|_F for Horn's matrix, Newton's 1e-15, and the
    rounding of the result to the output format."""
    return (3 * n + 16) * EPS64 * (rg2_1[:, None] + rg2_2[None, :]) + 4 * eps_out * ref * ref


def check(got, ref, rg2_1, rg2_2, n, eps_out, what=""):
    """Asserts the bound entry by entry; returns the largest used fraction of it."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.all(np.isfinite(got)), f"{what}: non-finite entries"
    err = np.abs(got * got - ref * ref)
    lim = bound(ref, rg2_1, rg2_2, n, eps_out)
    frac = np.where(err == 0.0, 0.0, err / np.where(lim > 0, lim, 1.0))
    frac = np.where((lim == 0) & (err > 0), np.inf, frac)
    worst = float(frac.max()) if frac.size else 0.0
    print(f"{what}: worst fraction of the bound {worst:.3g}")
    assert worst <= 1.0, f"{what}: {worst:.3g} of the bound at {np.unravel_index(np.argmax(frac), frac.shape)}"
    return worst


def gram_route(frames1, frames2=None, idx=None, mass=None, fit=True):
    """The library's route in numpy (Gram products, eigvalsh of Horn's matrix): what the bound is checked against on the CPU."""
    f1 = np.asarray(frames1, dtype=np.float64)
    f2 = f1 if frames2 is None else np.asarray(frames2, dtype=np.float64)
    idx_, w = _weights(f1.shape[1], idx, mass)
    W = w.sum()
    p1, p2 = f1[:, idx_, :], f2[:, idx_, :]
    if fit:
        c1 = (w[None, :, None] * p1).sum(1) / W
        c2 = (w[None, :, None] * p2).sum(1) / W
    else:
        c1 = c2 = ((w[:, None] * p1[0]).sum(0) / W)[None, :]
    q1 = np.sqrt(w)[None, :, None] * (p1 - c1[:, None, :])
    q2 = np.sqrt(w)[None, :, None] * (p2 - c2[:, None, :])
    G1, G2 = (q1 * q1).sum((1, 2)), (q2 * q2).sum((1, 2))
    S = np.einsum("akd,bke->abde", q1, q2)
    if fit:
        K = np.empty(S.shape[:2] + (4, 4))
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
        lam = np.linalg.eigvalsh(K)[..., -1]
    else:
        lam = np.trace(S, axis1=2, axis2=3)
    return np.sqrt(np.maximum(0.0, G1[:, None] + G2[None, :] - 2 * lam) / W)


def random_frames(F, natoms, seed, scale=1.0, offset=0.0, dtype=np.float32):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(F, natoms, 3)) * scale + offset).astype(dtype)


def random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    a, b, c, d = q
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


def rigid_copies(F, natoms, seed, offset=50.0, dtype=np.float32):
    """F rigid copies (random rotation and small translation) of one structure of ~1 nm extent placed `offset` nm from the
    origin, rounded to `dtype`: the copies differ from rigid images only by that rounding."""
    rng = np.random.default_rng(seed)
    base = rng.normal(size=(natoms, 3))
    out = np.empty((F, natoms, 3))
    for f in range(F):
        out[f] = base @ random_rotation(rng).T + offset + rng.normal(size=3)
    return out.astype(dtype)
