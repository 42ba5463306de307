"""numpy restatement of the per-atom volume definition of include/molar_hip.h (molar_hip_sasa_vol): the volume of each
atom's ball inside its power cell, evaluated ray by ray on the point table of the areas, for float32 and float64.  Brute
force over all j with the explicit neighbour filter, vectorised over chunks of neighbours x points; numpy evaluates each
array operation in the arrays' own precision and never contracts, which is what the definition asks for.  The min / max
over the neighbours are order-free, so no order has to be mimicked.  Shared by tests/test_sasa_vol_cpu.py and
tests/test_gpu_sasa_vol.py; keep the inputs small (2000 atoms x 192 points: about a second)."""
import numpy as np

import sasa_ref as sr  # noqa: F401  (table_formula, points and the area restatement for the callers)

CHUNK = 256


def sasa_vol_ref(xyz, vdw, probe, table, real=np.float32):
    """(volumes real[n], total float) of the atoms `xyz` (already the selection, in selection order)."""
    real = np.dtype(real).type
    c = np.ascontiguousarray(xyz, dtype=real).reshape(-1, 3)
    n = c.shape[0]
    u = np.ascontiguousarray(table, dtype=real)
    npoints = u.shape[0]
    s = np.zeros(n, np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        R = np.asarray(vdw, dtype=real) + real(probe)
        ok = np.isfinite(c).all(1) & np.isfinite(R) & (R > 0)
        R2 = R * R
        for i in np.nonzero(ok)[0]:
            d = c - c[i]                                            # c_j - c_i, component-wise
            dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            lim = R[i] + R
            nb = ok & (dd < lim * lim)
            nb[i] = False
            nb = np.nonzero(nb)[0]
            lo = np.zeros(npoints, real)
            hi = np.full(npoints, R[i], real)
            for j0 in range(0, len(nb), CHUNK):
                j = nb[j0:j0 + CHUNK]
                dj = d[j]
                cc = (((dd[j] + R2[i]) - R2[j]) * real(0.5))[:, None]
                a = (u[None, :, 0] * dj[:, None, 0] + u[None, :, 1] * dj[:, None, 1]) + u[None, :, 2] * dj[:, None, 2]
                t = cc / a
                # a > 0 and t < hi: hi = t (a NaN never compares true)
                hi = np.minimum(hi, np.where((a > 0) & ~np.isnan(t), t, real(np.inf)).min(0))
                lo = np.maximum(lo, np.where((a < 0) & ~np.isnan(t), t, real(-np.inf)).max(0))
                # a == 0 and c < 0: hi = 0; lo >= 0 and hi ends as max(hi, lo), so "= 0" and "min with 0" end alike
                hi = np.where(((a == 0) & (cc < 0)).any(0), np.minimum(hi, real(0)), hi)
            hi = np.maximum(hi, lo)
            h, l = hi.astype(np.float64), lo.astype(np.float64)
            s[i] = np.sum((h * h) * h - (l * l) * l)
    volumes = ((((4.0 * np.pi) / 3.0) * s) / float(npoints)).astype(real)
    return volumes, float(np.sum(volumes.astype(np.float64)))


def ball_below_plane(R, h):
    """Volume of the part of a ball of radius R on the near side of a plane at signed distance h from its centre."""
    if h >= R:
        return 4.0 * np.pi * R ** 3 / 3.0
    if h <= -R:
        return 0.0
    return np.pi * (R + h) ** 2 * (2.0 * R - h) / 3.0


def two_sphere_split(d, Ra, Rb):
    """Analytic volumes of two overlapping balls (centre distance d) cut at their radical plane."""
    ha = (d * d + Ra * Ra - Rb * Rb) / (2.0 * d)
    return ball_below_plane(Ra, ha), ball_below_plane(Rb, d - ha)


def union_volume_mc(xyz, R, samples, seed, block=50000):
    """(estimate, standard error) of the volume of the union of the balls from `samples` uniform points of its bounding box."""
    c = np.asarray(xyz, np.float64).reshape(-1, 3)
    R = np.asarray(R, np.float64)
    lo, hi = (c - R[:, None]).min(0), (c + R[:, None]).max(0)
    box = float(np.prod(hi - lo))
    rng = np.random.default_rng(seed)
    k = (c * c).sum(1) - R * R
    hits = 0
    for s0 in range(0, samples, block):
        p = rng.uniform(lo, hi, (min(block, samples - s0), 3))
        power = (p * p).sum(1)[:, None] - 2.0 * (p @ c.T) + k[None, :]          # |p - c_j|^2 - R_j^2
        hits += int((power < 0).any(1).sum())
    frac = hits / samples
    return box * frac, box * np.sqrt(frac * (1.0 - frac) / samples)
