"""The frames of tests/pinned_patches.py are what they were built to be - asserted on the CPU oracle alone (f32 and f64), so that
tests/test_gpu_membrane_pinned.py compares the kernels on inputs whose patch lengths, cell sizes and reverse counts are known,
and whose results do not hang on the rounding of the inputs."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pinned_patches as pp  # noqa: E402

PRECS = ("f32", "f64")
TOL = {"f32": 2e-5, "f64": 1e-12}        # the bounds of check_smooth (test_gpu_membrane.py) and check_state (test_gpu_membrane_f64.py)
FLOATS = ("coefs", "mean_curv", "gauss_curv", "princ_curvs", "princ_dirs", "area", "normals", "head")
LARGE_K = (32 * 256 + 1, 64 * 256 + 1)   # what test_workgroup_shapes asks for on 256 compute units


@functools.lru_cache(maxsize=None)
def oracle(prec):
    from oracle.oracle import Oracle
    return Oracle(prec)


@functools.lru_cache(maxsize=None)
def frame(name, arg=None):
    if name == "length":
        return pp.length_frame(arg)
    if name == "small":
        return pp.small_frame(arg)
    if name == "large":
        return pp.large_frame(arg)
    return {"ring": pp.ring_frame, "hub": pp.hub_frame}[name]()


FRAMES = ([("length", o) for o in pp.ORDERS] + [("ring", None), ("hub", None)] + [("small", k) for k in pp.SMALL_K]
          + [("large", k) for k in LARGE_K])


def smooth(prec, f, head=None):
    o = oracle(prec)
    r = o.real
    h = f["head"].astype(r) if head is None else head
    return o.membrane_smooth(o.box_from_matrix(f["box"].astype(r)), h, f["normals"].astype(r), f["valid"], f["patch_off"], f["patch_ids"])


@functools.lru_cache(maxsize=None)
def result(prec, name, arg=None):
    return smooth(prec, frame(name, arg))


def lengths(f):
    return np.diff(f["patch_off"].astype(np.int64))


# ------------------------------------------------------------------------------------------------ what was dealt

@pytest.mark.parametrize("order", pp.ORDERS)
def test_length_frame_holds_every_length_and_group_pattern(order):
    f = frame("length", order)
    n, valid, rec = lengths(f), f["valid"].astype(bool), f["record"]
    assert np.array_equal(n, rec["np"]) and len(n) % 4 == 0
    for t in pp.LENGTH_TABLE:
        assert np.count_nonzero((n == t) & valid) >= 2, t
    assert set(n[valid]) <= set(pp.LENGTH_TABLE)
    assert np.all((n[~valid] >= 1) & (n[~valid] <= 5)) and np.all(n[valid & (n > 0)] >= 7)     # 1 .. 6 members: invalid lipids only
    g = np.where(valid, n, -n).reshape(-1, 4)
    count = lambda pred: sum(1 for q in g if pred(q))
    assert count(lambda q: len(set(q)) == 1) >= 2 * len(pp.LENGTH_TABLE)
    assert count(lambda q: tuple(q) == (7, 96, 16, 17)) >= 2
    assert count(lambda q: (q > 96).sum() == 1 and (q >= 0).all()) >= 2
    assert count(lambda q: (q < 0).sum() == 1 and (q > 96).sum() == 0) >= 2 and count(lambda q: (q < 0).sum() == 1 and (q > 96).sum() == 1) >= 1
    assert count(lambda q: (q > 96).all() and len(set(q)) > 1) >= 2
    pat = rec["pattern"].reshape(-1, 4)[:, 0]
    for p in ("equal", "7-96-16-17", "one-above-96", "one-invalid", "four-above-96"):
        assert np.count_nonzero(pat == p) >= 2, p
    po = f["patch_off"].astype(np.int64)
    for i in range(len(n)):                              # members are distinct and never the lipid itself
        p = f["patch_ids"][po[i]:po[i + 1]]
        assert len(set(p.tolist())) == len(p) and i not in p
    if order != "near":                                  # the same members as the nearest-first frame, in another order
        near = frame("length", "near")
        assert np.array_equal(near["head"], f["head"]) and np.array_equal(near["patch_off"], f["patch_off"])
        assert not np.array_equal(near["patch_ids"], f["patch_ids"])
        for i in range(len(n)):
            assert sorted(near["patch_ids"][po[i]:po[i + 1]]) == sorted(f["patch_ids"][po[i]:po[i + 1]])


@pytest.mark.parametrize("name,arg", FRAMES)
@pytest.mark.parametrize("prec", PRECS)
def test_patches_of_seven_or_more_stay_valid(prec, name, arg):
    f, w = frame(name, arg), result(prec, name, arg)
    n, entry = lengths(f), f["valid"].astype(bool)
    expect = entry & (n >= 7)
    if name == "hub":
        role = f["record"]["role"]
        expect &= role == 0
        assert not w["valid"][role != 0].any() and np.count_nonzero(role == 2) >= 8 and np.count_nonzero(role == 3) >= 8
    assert w["valid"][expect].all()
    assert not w["valid"][~entry].any() and not w["valid"][entry & (n == 0)].any()
    other = result("f64" if prec == "f32" else "f32", name, arg)
    assert np.array_equal(w["valid"], other["valid"]) and np.array_equal(w["nvert"], other["nvert"])


@pytest.mark.parametrize("prec", PRECS)
def test_cells_have_the_vertex_counts_they_were_built_for(prec):
    f, w = frame("ring"), result(prec, "ring")
    rec = f["record"]
    assert np.array_equal(np.flatnonzero(f["valid"]), rec["centres"])
    seen = set()
    for c, b in zip(rec["centres"], rec["built"]):
        assert w["nvert"][c] == (6 if b["kind"] == "transient" else b["m"]), b
        assert lengths(f)[c] == max(b["pad"], b["m"] + {"final": max(b["m"], 8), "transient": 6, "last": 8}[b["kind"]])
        seen.add((b["kind"], b["m"], b["pad"], b["form"]))
    for m in pp.FINAL_M:
        assert ("final", m, 0, "own") in seen
    for m in pp.TRANSIENT_M:
        assert ("transient", m, 0, "own") in seen
    for m in pp.LAST_M:
        assert ("last", m, 0, "own") in seen
    for kind in ("final", "transient"):
        assert all((kind, m, 0, "wave") in seen for m in pp.WAVE_M) and all((kind, 17, pad, "padded") in seen for pad in pp.PADS)
    # the wave form: four centres on the lipids 4w .. 4w + 3; on its own and padded: the three wave-mates are markers
    form = np.array([b["form"] for b in rec["built"]])
    for kind in ("final", "transient"):
        c = rec["centres"][(form == "wave") & np.array([b["kind"] == kind for b in rec["built"]])]
        assert len(c) == 4 and c[0] % 4 == 0 and np.array_equal(c, c[0] + np.arange(4))
    lone = rec["centres"][form != "wave"]
    assert np.all(lone % 4 == 0) and not f["valid"][lone[:, None] + np.arange(1, 4)].any()
    for k in pp.SMALL_K:
        fs, ws = frame("small", k), result(prec, "small", k)
        assert len(fs["valid"]) == k and fs["valid"][0] == 1 and not fs["valid"][1:].any()
        assert bool(ws["valid"][0]) == (k >= 8) and (k < 8 or ws["nvert"][0] == 7)
        assert lengths(fs)[0] == (0 if k < 8 else 7 if k < 16 else 15) and np.all((lengths(fs)[1:] >= 1) & (lengths(fs)[1:] <= 5))
    for k in LARGE_K:
        fl, wl = frame("large", k), result(prec, "large", k)
        rl = fl["record"]
        assert len(fl["valid"]) == k
        assert [int(wl["nvert"][c]) for c in rl["centres"]] == list(pp.LARGE_BUILT) == [b["m"] for b in rl["built"]]
        assert rl["centres"][0] == 0 and k // 4 < rl["centres"][1] < 3 * k // 4 and rl["centres"][3] > k - 64
        assert rl["centres"][2] == rl["centres"][1] + 16 and rl["centres"][1] // 32 == rl["centres"][2] // 32
        sheet = np.flatnonzero(rl["kind"] == 1)
        long = sheet[sheet % 29 == 0]
        assert set(rl["np"][long]) == set(pp.LARGE_CYCLE) and np.all(rl["np"][sheet[sheet % 29 != 0]] == pp.LARGE_MEMBERS)
        assert len(set((long % 64).tolist())) == 64 and fl["valid"][sheet].mean() > 0.999 and not fl["valid"][rl["kind"] == 0].any()
        beside = long[long // 64 == rl["centres"][1] // 64]                         # one 64-lane workgroup holds both
        assert len(beside) and rl["np"][beside[0]] == 97 and fl["valid"][beside[0]]


@pytest.mark.parametrize("prec", PRECS)
def test_sheet_cells_have_four_to_eight_vertices(prec):
    for order in pp.ORDERS:
        w = result(prec, "length", order)
        seen = set(w["nvert"][w["valid"].astype(bool)].tolist())
        assert {4, 5, 6, 7, 8} <= seen, seen


def test_hubs_have_the_reverse_counts_asked_for():
    f = frame("hub")
    rec = f["record"]
    rev = pp.reverse_counts(f)
    assert np.array_equal(rev[rec["hubs"]], rec["counts"])
    assert set(rec["counts"].tolist()) == set(pp.HUB_COUNTS)
    rounds = lambda c: (c + 15) // 16
    full = 0
    for w in np.unique(rec["hubs"] // 4):                # a wave of four hubs holds four different round counts
        c = rec["counts"][rec["hubs"] // 4 == w]
        if len(c) == 4:
            full += 1
            assert len(set(c.tolist())) == 4 and len(set(rounds(c).tolist())) >= 2
    assert full == 10
    assert rev[rec["role"] == 3].sum() == 0              # lifted owners are named by nobody
    po = f["patch_off"].astype(np.int64)
    owner = np.repeat(np.arange(len(rev)), np.diff(po))
    for h, c in zip(rec["hubs"], rec["counts"]):         # hubs of 15 and more: an owner of each role among the entries
        if c >= 15:
            roles = set(rec["role"][owner[f["patch_ids"] == h]].tolist())
            assert {0, 1, 2, 3} <= roles, (h, c, roles)


# ------------------------------------------------------------------------------------------------ cell sizes on the way

def local_points(f, i):
    """the members of lipid i's patch in its local frame (lipid_molecule.rs:190-196), float64"""
    n = f["normals"][i].astype(np.float64)
    c0 = np.cross(n, [1.0, 0.0, 0.0]); c1 = np.cross(n, c0)
    to_lab = np.stack([c0, c1, -n], 1)
    po = f["patch_off"].astype(np.int64)
    d = f["head"][f["patch_ids"][po[i]:po[i + 1]].astype(np.int64)].astype(np.float64) - f["head"][i].astype(np.float64)
    ext = np.diag(f["box"]).astype(np.float64)
    d -= ext * np.round(d / ext)
    return np.linalg.solve(to_lab, d.T).T


def clip_history(pts):
    """a convex polygon (the square of +-10) cut by the bisector of the origin and each point in turn: the vertex count after
    every cut and the smallest distance of a vertex from a cutting line"""
    poly = [np.array(p) for p in ((-10.0, -10.0), (10.0, -10.0), (10.0, 10.0), (-10.0, 10.0))]
    counts, margin = [], np.inf
    for p in pts:
        h = 0.5 * p[:2]
        u = h / np.linalg.norm(h)
        d = [float(v @ u - np.linalg.norm(h)) for v in poly]          # signed distance from the bisector, inside < 0
        margin = min(margin, min(abs(x) for x in d))
        new = []
        for k in range(len(poly)):
            a, b, da, db = poly[k], poly[(k + 1) % len(poly)], d[k], d[(k + 1) % len(poly)]
            if da < 0:
                new.append(a)
            if (da < 0) != (db < 0):
                new.append(a + (b - a) * (da / (da - db)))
        poly = new
        counts.append(len(poly))
    return counts, margin


def test_cells_grow_past_sixteen_vertices_exactly_where_built():
    f = frame("ring")
    rec = f["record"]
    checked = 0
    for c, b in zip(rec["centres"], rec["built"]):
        counts, margin = clip_history(local_points(f, c))
        assert counts[-1] == (6 if b["kind"] == "transient" else b["m"])
        if b["kind"] == "last":                          # the m-th vertex comes with the last member; before it, 16 at the most up to m = 17
            assert counts[-2] == b["m"] - 1 and max(counts[:-1]) == max(b["m"] - 1, 8) and margin > 1e-3, (b, counts, margin)
        elif b["kind"] == "transient" and b["m"] >= 17:
            assert max(counts) > 16 and margin > 1e-3, (b, max(counts), margin)
        elif b["m"] == 16:                               # final 16 and transient 16: at the limit, never past it
            assert max(counts) == 16 and margin > 1e-3, (b, max(counts), margin)
        elif b["kind"] == "final":
            assert (max(counts) > 16) == (b["m"] > 16) and margin > 1e-3, (b, max(counts), margin)
        else:
            assert max(counts) <= 16 and margin > 1e-3, (b, max(counts), margin)
        checked += 1
    assert checked == len(rec["built"]) >= 43
    for k in pp.SMALL_K:
        if k >= 8:
            counts, margin = clip_history(local_points(frame("small", k), 0))
            assert counts[-1] == 7 and max(counts) <= 16 and margin > 1e-3


# ------------------------------------------------------------------------------------------------ conditioning

def slots(poff, nvert, ok):
    """flat indices of the Voronoi slots and of the patch entries of the lipids `ok`"""
    po = poff.astype(np.int64)
    k = np.flatnonzero(ok)
    nv = nvert[k].astype(np.int64)
    s = np.repeat(po[k] + 4 * k - np.concatenate([[0], np.cumsum(nv)[:-1]]), nv) + np.arange(nv.sum())
    ne = po[k + 1] - po[k]
    e = np.repeat(po[k] - np.concatenate([[0], np.cumsum(ne)[:-1]]), ne) + np.arange(ne.sum())
    return s, e


def allowance_used(prec, got, want, poff):
    """the largest |got - want| of every compared float array as a fraction of what the GPU check of that precision allows:
    check_smooth |d| <= tol + tol |want|, check_state |d| <= tol |want| + tol max |want|"""
    ok = want["valid"].astype(bool)
    s, e = slots(poff, want["nvert"], ok)
    pairs = [(k, got[k][ok], want[k][ok]) for k in FLOATS] + [("voro", got["voro"][s], want["voro"][s]), ("fitted", got["fitted"][e], want["fitted"][e])]
    used = {}
    for k, g, w in pairs:
        if w.size == 0:
            continue
        g = g.astype(np.float64); w = w.astype(np.float64)
        floor = 1.0 if prec == "f32" else float(np.abs(w).max())
        frac = np.abs(g - w) / (TOL[prec] * (np.abs(w) + floor))
        used[k] = float(frac.max())
        if k == "princ_dirs":
            # The directions are the eigenvectors of the 2 x 2 shape operator: a change dW of its entries turns them by
            # dW / (k1 - k2), without bound where the principal curvatures meet - a property of the quantity, which no sheet
            # of noisy markers avoids.  What is held to the bound is the turn times the gap in 1 / nm (never more than the
            # turn itself); the plain figure is printed beside it.
            gap = np.abs(want["princ_curvs"][ok][:, 0].astype(np.float64) - want["princ_curvs"][ok][:, 1])
            used["princ_dirs x gap"] = float((frac * np.minimum(gap, 1.0)[:, None, None]).max())
    return used


@pytest.mark.parametrize("name,arg", [fa for fa in FRAMES if fa[0] != "small" or fa[1] in (8, 15, 16, 65)])
@pytest.mark.parametrize("prec", PRECS)
def test_an_ulp_of_the_markers_moves_results_by_less_than_half_the_tolerance(prec, name, arg):
    """every marker coordinate moved by -1, 0 or +1 ulp of the precision, five draws: the oracle keeps validity and vertex
    counts, and no compared float moves by more than half of what the GPU check allows (measured as that check measures)"""
    f, base = frame(name, arg), result(prec, name, arg)
    r = oracle(prec).real
    head = f["head"].astype(r)
    rng = np.random.default_rng(77)
    worst = {}
    for _ in range(5):
        step = rng.integers(-1, 2, size=head.shape)
        moved = np.where(step == 0, head, np.nextafter(head, np.where(step > 0, np.inf, -np.inf).astype(r)))
        w = smooth(prec, f, moved)
        assert np.array_equal(w["valid"], base["valid"]) and np.array_equal(w["nvert"], base["nvert"])
        ok = base["valid"].astype(bool)
        s, _ = slots(f["patch_off"], base["nvert"], ok)
        assert np.array_equal(w["neib_ids"][s], base["neib_ids"][s])
        for k, v in allowance_used(prec, w, base, f["patch_off"]).items():
            worst[k] = max(worst.get(k, 0.0), v)
    plain = worst.pop("princ_dirs")
    top = max(worst, key=worst.get)
    print(f"conditioning {name} {arg} {prec}: largest move {worst[top]:.3f} of the tolerance {TOL[prec]:g} ({top}); "
          f"principal directions {plain:.3f}, times the curvature gap {worst['princ_dirs x gap']:.2e}")
    assert worst[top] <= 0.5, worst


def test_frames_repeat_byte_for_byte():
    for a, b in ((pp.length_frame("shuffled"), pp.length_frame("shuffled")), (pp.ring_frame(), pp.ring_frame())):
        for k in ("head", "normals", "box", "valid", "patch_off", "patch_ids"):
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
