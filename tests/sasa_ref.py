"""numpy restatement of the surface-area definition of include/molar_hip.h (Shrake-Rupley with every floating-point operation
fixed), for float32 and float64.  Brute force over all j with the explicit neighbour filter; numpy evaluates each array
operation in the arrays' own precision and never contracts a multiply with an add, which is what the definition asks for.
Shared by tests/test_sasa_cpu.py and tests/test_gpu_sasa.py; keep the inputs small (2000 atoms x 192 points: about a second)."""
import numpy as np


def table_formula(npoints):
    """u_k of the definition in float64."""
    k = np.arange(npoints, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / float(npoints)
    r = np.sqrt(1.0 - z * z)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)


def points(npoints, real):
    """The library's own table (the restatement takes it from there: host sin/cos may differ from numpy's in the last bit)."""
    from molar_amd import api
    return api.sasa_points(npoints, real)


def sasa_ref(xyz, vdw, probe, table, real=np.float32):
    """(exposed uint32[n], areas real[n], total float) of the atoms `xyz` (already the selection, in selection order)."""
    real = np.dtype(real).type
    c = np.ascontiguousarray(xyz, dtype=real).reshape(-1, 3)
    n = c.shape[0]
    u = np.ascontiguousarray(table, dtype=real)
    npoints = u.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        R = np.asarray(vdw, dtype=real) + real(probe)
        ok = np.isfinite(c).all(1) & np.isfinite(R) & (R > 0)
        R2 = R * R
        exposed = np.zeros(n, np.uint32)
        for i in np.nonzero(ok)[0]:
            d = c - c[i]                                            # c_j - c_i, component-wise
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            lim = R[i] + R
            nb = ok & (d2 < lim * lim)
            nb[i] = False
            nb = np.nonzero(nb)[0]
            a = R[i] * u                                            # R_i u_k
            buried = np.zeros(npoints, bool)
            for j0 in range(0, len(nb), 256):
                j = nb[j0:j0 + 256]
                t = a[None, :, :] - d[j][:, None, :]
                t2 = (t[:, :, 0] * t[:, :, 0] + t[:, :, 1] * t[:, :, 1]) + t[:, :, 2] * t[:, :, 2]
                buried |= (t2 < R2[j][:, None]).any(0)
            exposed[i] = npoints - int(buried.sum())
    Rd = np.where(ok, R, 0).astype(np.float64)
    areas = ((((4.0 * np.pi) * (Rd * Rd)) * exposed.astype(np.float64)) / float(npoints)).astype(real)
    return exposed, areas, float(np.sum(areas.astype(np.float64)))


def cap_fraction(d, Ra, Rb):
    """Exposed share of sphere a (radius Ra) with sphere b (radius Rb) at centre distance d: the analytic spherical cap."""
    if d >= Ra + Rb or d + Rb <= Ra:
        return 1.0              # disjoint, or b inside a
    if d + Ra <= Rb:
        return 0.0              # a inside b
    h = (d * d + Ra * Ra - Rb * Rb) / (2.0 * d)
    return (1.0 + h / Ra) / 2.0
