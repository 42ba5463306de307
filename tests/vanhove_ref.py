"""The reference of the van Hove tests: numpy, one lag at a time by slices of the input, the displacement in longdouble.

What the library computes (molar_hip.h): Delta_d = x_d(t + tau) - x_d(t) IN DOUBLE for the components of dims - the rounding of
that difference is part of the definition, and the reference forms it in double too -, then r2 by nd fused multiply-adds (the
first one adds to zero) and v = sqrt(r2) correctly rounded, or v = Delta_d in SIGNED mode.  The bin is
floor((v - lo) / (hi - lo) * nbins) in double.

The bound on the error of the library's v against the exact sqrt(sum Delta_d^2) of the same double Deltas:
  every fma rounds once: all terms are positive, so r2 = exact * (1 + e), |e| <= nd * U (U = 2^-53) to first order;
  sqrt halves the relative error and rounds once more: |v - v_exact| <= (nd / 2 + 1) * U * v.  VERR = (nd + 2) * U * v is used,
  twice the first-order figure.  For float inputs Delta is exact whenever the two exponents are within 29 of each other; for
  double inputs it carries one rounding - the same one in the library and here, because it is part of the definition.
  SIGNED mode, and wherever every Delta is exactly 0 (lag 0, stationary particles): v is exact, the bound is 0.
The bin formula rounds three more times (v - lo, the quotient, the product) and hi - lo once: a value within
4 * U * |v - lo| of an edge could fall on either side; FORM = 8 * U * |v - lo| is used.  The reference itself works with 64
mantissa bits: 2^-63 relative, covered by the factors of two above.

`reference` ASSERTS on its own inputs that every v is farther than VERR + FORM from the two edges of its bin (lo and hi
included) - an exact v that equals lo or hi exactly is decided the same way on both sides and is allowed.  That makes the
comparison of the integer outputs for equality fair.  No case is filtered: a case that trips the assertion has to be
re-seeded here."""
import collections
import functools

import numpy as np

U = 2.0 ** -53
ERR_INVALID, ERR_SIZES, ERR_TOO_LARGE = 1, 2, 3          # overwritten from the header by error_codes()

Ref = collections.namedtuple("Ref", ["hist", "outside", "norigins", "nvalid", "bad", "min_clearance"])
Case = collections.namedtuple("Case", ["name", "kind", "seed", "F", "natoms", "lags", "lo", "hi", "nbins", "origin_stride", "dims", "signed", "idx", "labels", "G",
                                       "pad", "plant"])


def error_codes(header_text):
    import re
    codes = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"MOLAR_HIP_ERR_(\w+)\s*=\s*(\d+)", header_text))
    return codes


def random_walk(seed, F, natoms, step=0.11):
    """Positions [F, natoms, 3] float64 of seeded Gaussian random walks that start uniformly in a cube of side 3."""
    rng = np.random.default_rng(seed)
    x0 = rng.uniform(0.0, 3.0, (1, natoms, 3))
    steps = rng.normal(0.0, step, (F, natoms, 3))
    steps[0] = 0.0
    return x0 + np.cumsum(steps, axis=0)


def stationary(seed, F, natoms):
    rng = np.random.default_rng(seed)
    return np.repeat(rng.uniform(0.0, 3.0, (1, natoms, 3)), F, axis=0)


def plant(traj, what):
    """A copy of traj with (frame, particle, component, value) planted."""
    out = np.array(traj, copy=True)
    for f, a, d, v in what:
        out[f, a, d] = v
    return out


def components(dims):
    return [d for d in range(3) if dims >> d & 1]


def reference(traj, lags, lo, hi, nbins, idx=None, labels=None, G=1, origin_stride=1, dims=7, signed=False):
    """Ref of traj [F, natoms, 3] (float32 or float64, taken exactly), see the module docstring."""
    x = np.asarray(traj).astype(np.float64)
    F = x.shape[0]
    sel = np.arange(x.shape[1]) if idx is None else np.asarray(idx, np.int64)
    comp = components(dims)
    nd = len(comp)
    assert 1 <= nd and (not signed or nd == 1)
    x = x[:, sel][:, :, comp]                                            # [F, n, nd]
    n = x.shape[1]
    lab = np.zeros(n, np.int64) if labels is None else np.asarray(labels, np.int64)
    G = 1 if labels is None else int(G)
    bad = (~np.isfinite(x)).any(axis=2).sum(axis=0).astype(np.uint32)
    ok = bad == 0
    nvalid = np.bincount(lab[ok], minlength=G).astype(np.uint64)
    L = len(lags)
    os_ = min(int(origin_stride), F)
    hist = np.zeros((G, L, nbins), np.uint64)
    outside = np.zeros((G, L), np.uint64)
    norigins = np.zeros(L, np.uint64)
    LD = np.longdouble
    llo, lhi = LD(lo), LD(hi)
    clearance = np.inf
    xs = x[:, ok]
    labs = lab[ok]
    for l, tau in enumerate(int(t) for t in lags):
        assert 0 <= tau < F
        a, b = xs[0:F - tau:os_], xs[tau:F:os_]
        norigins[l] = a.shape[0]
        assert a.shape[0] == (F - 1 - tau) // os_ + 1 and b.shape[0] == a.shape[0]
        with np.errstate(invalid="ignore"):
            delta = b - a                                                # in double: the definition
        if signed:
            v = delta[:, :, 0].astype(LD)
            exact = np.ones(v.shape, bool)
        else:
            v = np.sqrt((delta.astype(LD) ** 2).sum(axis=2))
            exact = (delta == 0.0).all(axis=2)
        verr = np.where(exact, LD(0), LD((nd + 2) * U) * np.abs(v))
        margin = verr + LD(8 * U) * np.abs(v - llo)
        inside = (v >= llo) & (v < lhi)
        pos = (v - llo) / (lhi - llo) * LD(nbins)
        bn = np.clip(np.floor(pos), 0, nbins - 1).astype(np.int64)
        e0 = llo + (lhi - llo) * bn.astype(LD) / LD(nbins)
        e1 = llo + (lhi - llo) * (bn + 1).astype(LD) / LD(nbins)
        free = exact & ((v == llo) | (v == lhi))                         # decided alike on both sides
        gap = np.where(inside, np.minimum(v - e0, e1 - v), np.where(v < llo, llo - v, v - lhi))
        tight = ~free & ~(gap > margin)
        assert not tight.any(), f"lag {tau}: {int(tight.sum())} displacements within the bound of a bin edge, e.g. v = {v[tight][0]!r}"
        rest = ~free & (margin > 0)
        if rest.any():
            clearance = min(clearance, float((gap[rest] / margin[rest]).min()))
        g = np.broadcast_to(labs[None, :], v.shape)
        np.add.at(hist, (g[inside], l, bn[inside]), 1)
        np.add.at(outside, (g[~inside], l), 1)
    assert (hist.sum(axis=2) + outside == nvalid[:, None] * norigins[None, :]).all()
    return Ref(hist, outside, norigins, nvalid, bad, clearance)


def brute_force(traj, lags, lo, hi, nbins, idx=None, labels=None, G=1, origin_stride=1, dims=7, signed=False):
    """The same counts by plain Python loops over particle, lag and origin, with math.fma-free double arithmetic: only for inputs
    whose displacements are far from every edge."""
    import math
    x = np.asarray(traj).astype(np.float64)
    F = x.shape[0]
    sel = list(range(x.shape[1])) if idx is None else [int(i) for i in idx]
    comp = components(dims)
    G = 1 if labels is None else int(G)
    L = len(lags)
    hist = np.zeros((G, L, nbins), np.uint64)
    outside = np.zeros((G, L), np.uint64)
    norigins = np.zeros(L, np.uint64)
    nvalid = np.zeros(G, np.uint64)
    bad = np.zeros(len(sel), np.uint32)
    for k, a in enumerate(sel):
        g = 0 if labels is None else int(labels[k])
        for f in range(F):
            if not all(math.isfinite(x[f, a, d]) for d in comp):
                bad[k] += 1
        if bad[k]:
            continue
        nvalid[g] += 1
        for l, tau in enumerate(int(t) for t in lags):
            t = 0
            while t + tau <= F - 1:
                d = [x[t + tau, a, c] - x[t, a, c] for c in comp]
                v = d[0] if signed else math.sqrt(sum(e * e for e in d))
                if lo <= v < hi:
                    hist[g, l, min(int(math.floor((v - lo) / (hi - lo) * nbins)), nbins - 1)] += 1
                else:
                    outside[g, l] += 1
                t += origin_stride
    for l, tau in enumerate(int(t) for t in lags):
        norigins[l] = (F - 1 - tau) // origin_stride + 1
    return Ref(hist, outside, norigins, nvalid, bad, None)


# ---------------------------------------------------------------- the cases of the GPU tests, placed by the plan

@functools.lru_cache(maxsize=None)
def plan_sizes(nbins=16):
    """(origins_per_pass, particles_per_wg, lag_tile, lds_cells) as molar_hip_vanhove_plan reports them."""
    from molar_amd import api
    p = api.vanhove_plan(100, 10, 1, 4, nbins, 3)
    return p.origins_per_pass, p.particles_per_wg, p.lag_tile, p.lds_cells


def _lags(F, *cand):
    return tuple(sorted(set(int(c) for c in cand if 0 <= c < F)))


def build_cases():
    PASS, PW, LT, CELLS = plan_sizes(16)
    LT_WIDE = plan_sizes(1000)[2]
    assert LT_WIDE < LT
    cases = []

    def add(name, F, natoms, lags, kind="walk", seed=None, lo=0.05, hi=1.3, nbins=16, os=1, dims=7, signed=False, idx=None, labels=None, G=1, pad=0, plant=()):
        cases.append(Case(name, kind, len(cases) + 100 if seed is None else seed, F, natoms, tuple(lags), lo, hi, nbins, os, dims, signed,
                          None if idx is None else tuple(idx), None if labels is None else tuple(labels), G, pad, tuple(plant)))
    # frames: 1, 2, either side of a pass, two passes and a remainder
    for F in (1, 2, PASS - 1, PASS, PASS + 1, 2 * PASS + 37):
        add(f"frames_{F}", F, 3, _lags(F, 0, 1, F - 1), hi=4.0 if F > 100 else 1.3)
    Fbig = 2 * PASS + 37
    # origin strides: 3 (not a divisor), and beyond two passes: the second pass holds no origin
    for os in (3, 2 * PASS + 5):
        add(f"stride_{os}", Fbig, 3, _lags(Fbig, 0, 1, 7, Fbig - 1), os=os, hi=4.0)
    add("lag_0_alone", PASS + 1, 3, (0,))
    add("lag_last_alone", PASS + 1, 3, (PASS,), hi=4.0)
    add("single_origin_strided", 50, 4, (0, 44, 49), os=5)
    # lag lists either side of the tile, at the widest tile and at the tile of 1000 bins
    for n_l in (LT - 1, LT, LT + 1):
        add(f"lags_{n_l}", LT + 9, 5, range(n_l))
    for n_l in (LT_WIDE - 1, LT_WIDE, LT_WIDE + 1):
        add(f"lags_{n_l}_bins_1000", LT + 9, 5, range(n_l), nbins=1000)
    for n in sorted(set((1, 63, 64, 65, PW - 1, PW, PW + 1))):
        add(f"particles_{n}", 40, n, (0, 3, 39))
    # groups: unsorted labels, empty groups first (0), in the middle (2) and last (5), one particle alone (4), group 3 across workgroups
    n_g = 2 * PW + 5
    lab = [3] * n_g
    for k in (1, 4, 9, 12, 17):
        lab[k] = 1
    lab[6] = 4
    add("groups", 40, n_g, (0, 2, 11), labels=lab, G=6)
    add("groups_sorted_two", 40, 2 * PW + 1, (1, 5), labels=[0] * (PW + 3) + [1] * (PW - 2), G=2)
    # bins: one, and the cell count G L nbins (G = L = 1) either side of the on-chip limit
    add("bins_1", 30, 4, (0, 2, 5), nbins=1, lo=0.0, hi=0.4)
    for nb in (CELLS - 1, CELLS, CELLS + 1):
        add(f"bins_{nb}", 60, 3, (3,), nbins=nb, lo=0.0, hi=1.0)
    for dims in range(1, 8):
        add(f"dims_{dims}", 30, 4, (0, 2, 5), dims=dims)
    for dims in (1, 2, 4):
        add(f"signed_{dims}", 30, 4, (0, 2, 5), dims=dims, signed=True, lo=-0.21, hi=0.19, nbins=17)
    add("outside_both_sides", 200, 6, (1, 20, 150), lo=0.2, hi=0.8)
    add("stationary", PASS + 1, 5, (0, 1), kind="still", lo=0.0, hi=1.0)
    # one particle with a NaN in the first frame, one with an inf in the last, in different groups
    add("bad_particles", 20, 9, (0, 1, 6), labels=[0, 1, 2, 0, 1, 2, 0, 1, 2], G=3, plant=((0, 1, 0, float("nan")), (19, 5, 2, float("inf"))))
    add("bad_outside_dims", 20, 5, (0, 3), dims=3, plant=((4, 2, 2, float("nan")),))
    add("index_and_pad", 45, 12, (0, 4, 44), idx=(11, 0, 7, 7, 3), pad=2, labels=[1, 0, 1, 0, 0], G=2, hi=2.5)
    return cases


@functools.lru_cache(maxsize=None)
def cases():
    return {c.name: c for c in build_cases()}


@functools.lru_cache(maxsize=None)
def case_traj(name):
    """The float32 trajectory of a case, inside a wider block when the case pads its frames (read-only)."""
    c = cases()[name]
    x = (stationary if c.kind == "still" else random_walk)(c.seed, c.F, c.natoms)
    x = plant(x, c.plant).astype(np.float32)
    if c.pad:
        wide = np.full((c.F, c.natoms + c.pad, 3), np.float32(7.5))
        wide[:, :c.natoms] = x
        x = wide[:, :c.natoms]
    x.setflags(write=False)
    return x


def case_kwargs(c):
    return dict(idx=None if c.idx is None else np.array(c.idx, np.uint64), labels=None if c.labels is None else np.array(c.labels, np.uint32),
                origin_stride=c.origin_stride, dims=c.dims, signed=c.signed)


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """Computed once, shared by the tests, left unchanged."""
    c = cases()[name]
    r = reference(case_traj(name), c.lags, c.lo, c.hi, c.nbins, G=c.G, **case_kwargs(c))
    for a in r[:5]:
        a.setflags(write=False)
    return r
