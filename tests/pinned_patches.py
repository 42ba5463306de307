"""Frames with CHOSEN patches for the membrane smoothing pass (k_membrane_fit_lanes, k_membrane_fit, k_membrane_average and
launch_fit in molar_amd/csrc/membrane.hip).  Nothing here touches the code under test: numpy alone, every coordinate from one
seeded generator.

The smoothing call takes an arbitrary patch CSR, so patch length, Voronoi cell size and reverse count (how many patch entries
name a lipid) are dictated per lipid instead of being left to a cutoff search:

    length_frame(order, seed)  patch lengths from LENGTH_TABLE, dealt to the groups of four lipids that share a wave
    ring_frame(seed)           Voronoi cells of a chosen final (3 .. 24) or transient (16, 17, 18, 24) vertex count
                               (and cells that get their last vertex from the last member of the patch)
    hub_frame(seed)            reverse counts from HUB_COUNTS, with owners that are or turn invalid
    small_frame(K)             1 .. 65 lipids: the launch edges of 4 lipids per wave, 16 per workgroup
    large_frame(K, seed)       exactly K lipids for the workgroup shapes launch_fit picks from K

Every generator returns a dict: head [K, 3] and normals [K, 3] (float32; the f64 tests widen the same values), box [3, 3],
valid [K] uint8 (validity on entry), patch_off [K + 1] and patch_ids uint64, and `record`, what every lipid was built to be.
tests/test_pinned_patches_cpu.py asserts on the oracle alone that every frame is what it says.

Clusters of ring_frame are placed on a 3 x 3 grid of sites inside a 24 nm box, several clusters to a site, and not 10 nm
apart along one axis: patches are explicit, so clusters that overlap in space never see each other, and coordinates of
hundreds of nm would cost float32 five bits (the conditioning test of the CPU module measures what an ulp of the input moves).
"""
import numpy as np

SPACING = 0.8
# patch lengths around every threshold of the pass: the 16-member rounds of the sixteen-lane kernel (15 / 16 / 17, 31 / 32 / 33,
# 47 / 48 / 49), the LDS / HBM rule of the one-lane kernel (60 | 61, and 59 .. 65 for its gathers of 4 and 2), the sixteen-lane
# kernel's LDS slice (96 | 97) and beyond
LENGTH_TABLE = (0, 7, 8, 15, 16, 17, 31, 32, 33, 47, 48, 49, 59, 60, 61, 62, 63, 64, 65, 95, 96, 97, 98, 127, 128, 129, 200)
ORDERS = ("near", "far", "shuffled")
HUB_COUNTS = (0, 1, 15, 16, 17, 31, 32, 33, 48, 49)
SMALL_K = (1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 63, 64, 65)
FINAL_M = tuple(range(3, 25))
TRANSIENT_M = (16, 17, 18, 24)
WAVE_M = (15, 16, 17, 6)
LAST_M = (15, 16, 17, 18)
PADS = (61, 97)
LARGE_CYCLE = (60, 61, 96, 97, 128)
LARGE_RINGS = (16, 17, 20)
LARGE_PAIR = 18                          # a second large cell 16 lipids behind the middle one: two LDS lanes of one workgroup
LARGE_BUILT = (16, 17, 18, 20)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _normals(n, rng, tilt=0.05):
    v = np.tile(np.array([0.0, 0.0, 1.0]), (n, 1)) + tilt * rng.normal(size=(n, 3))
    return _f32(v / np.linalg.norm(v, axis=1, keepdims=True))


def sheet(side, rng):
    """side x side markers, 0.8 nm apart, jittered by 0.2 spacings (clipped to 0.45: a marker stays in its lattice cell),
    on a gently undulating periodic surface; lipid ix * side + iy sits in lattice cell (ix, iy)"""
    L = side * SPACING
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)
    g = (ij + 0.5 + np.clip(0.2 * rng.normal(size=(side * side, 2)), -0.45, 0.45)) * SPACING
    z = 5.0 + 0.3 * np.sin(2 * np.pi * g[:, 0] / L) * np.cos(2 * np.pi * g[:, 1] / L) + 0.02 * rng.normal(size=len(g))
    return _f32(np.concatenate([g, z[:, None]], 1)), _normals(side * side, rng), np.diag([L, L, 12.0]).astype(np.float32)


def nearest_all(head, L):
    """[K, K - 1]: for every marker, all the others by in-plane minimum-image distance, nearest first"""
    xy = head[:, :2].astype(np.float64)
    d = xy[None, :, :] - xy[:, None, :]
    d -= L * np.round(d / L)
    r2 = (d * d).sum(-1)
    np.fill_diagonal(r2, np.inf)
    return np.argsort(r2, axis=1, kind="stable")[:, :-1]


def csr(patches):
    off = np.concatenate([[0], np.cumsum([len(p) for p in patches])]).astype(np.uint64)
    ids = np.concatenate([np.asarray(p, np.uint64) for p in patches] + [np.zeros(0, np.uint64)]).astype(np.uint64)
    return off, ids


def reverse_counts(frame):
    return np.bincount(frame["patch_ids"].astype(np.int64), minlength=len(frame["valid"]))


# ------------------------------------------------------------------------------------------------ patch lengths

def length_groups(ngroups, rng):
    """lengths of `ngroups` groups of four lipids (negative: invalid on entry with a patch of that many members) and the
    pattern each group was built for"""
    groups = []
    for t in LENGTH_TABLE:
        groups += [((t, t, t, t), "equal")] * 2
    groups += [((7, 96, 16, 17), "7-96-16-17")] * 2
    groups += [((8, 97, 33, 60), "one-above-96"), ((128, 15, 48, 95), "one-above-96"), ((61, 62, 200, 63), "one-above-96"),
               ((64, 65, 31, 129), "one-above-96")]
    groups += [((32, -1, 47, 49), "one-invalid"), ((-5, 7, 16, 96), "one-invalid"), ((48, 63, 65, -2), "one-invalid"),
               ((33, -4, 97, 15), "one-invalid"), ((59, 98, -3, 8), "one-invalid")]
    groups += [((97, 98, 127, 128), "four-above-96"), ((129, 200, 97, 128), "four-above-96")]
    assert len(groups) <= ngroups
    while len(groups) < ngroups:
        groups.append((tuple(int(x) for x in rng.choice(LENGTH_TABLE, 4)), "mixed"))
    return [groups[k] for k in rng.permutation(len(groups))]


def length_frame(order, seed=1):
    assert order in ORDERS
    rng = np.random.default_rng(seed)
    side = 24
    head, nrm, box = sheet(side, rng)
    K = side * side
    near = nearest_all(head, side * SPACING)
    groups = length_groups(K // 4, rng)
    lens = np.array([x for g, _ in groups for x in g], np.int64)
    pattern = np.array([p for _, p in groups for _ in range(4)])
    valid = (lens >= 0).astype(np.uint8)
    lens = np.abs(lens)
    orng = np.random.default_rng(seed + 1000)            # the member order draws from its own stream: the same sheet for every order
    patches = []
    for i in range(K):
        p = near[i, :lens[i]]
        if order == "far":
            p = p[::-1]
        elif order == "shuffled":
            p = orng.permutation(p)
        patches.append(p)
    off, ids = csr(patches)
    return dict(head=head, normals=nrm, box=box, valid=valid, patch_off=off, patch_ids=ids,
                record=dict(np=lens, pattern=pattern, order=order))


# ------------------------------------------------------------------------------------------------ cell sizes

def ring_xy(rng, m, radius, phase=0.0, radial=0.01, angular=0.02):
    a = 2 * np.pi * (np.arange(m) + angular * rng.uniform(-1, 1, m)) / m + phase
    r = radius * (1.0 + radial * rng.uniform(-1, 1, m))
    return np.stack([r * np.cos(a), r * np.sin(a)], 1)


def cluster_xy(rng, kind, m, pad=0):
    """in-plane offsets of a cluster's markers from its centre, in patch order.
    final m:     m markers at 0.8 nm (an m-vertex cell), then max(m, 8) at 1.9 nm that cut nothing;
    transient m: an m-gon at 1.6 nm (the cell holds m vertices), then a hexagon at 0.7 nm that leaves 6;
    last m:      8 markers at 1.9 nm first, then the m at 0.8 nm: the cell gets its m-th vertex from the LAST member of the
                 patch (for m = 17 the sixteen-lane kernel meets its limit when no further member could notice a lost vertex);
    pad:         markers on rings from 2.2 nm outwards until the patch has `pad` members"""
    if kind == "final":
        parts = [ring_xy(rng, m, 0.8), ring_xy(rng, max(m, 8), 1.9, phase=np.pi / max(m, 8))]
    elif kind == "last":
        parts = [ring_xy(rng, 8, 1.9, phase=np.pi / 8), ring_xy(rng, m, 0.8)]
    else:
        parts = [ring_xy(rng, m, 1.6), ring_xy(rng, 6, 0.7, phase=0.3)]
    xy = np.concatenate(parts)
    r = 2.2
    while len(xy) < pad:
        k = min(16, pad - len(xy))
        xy = np.concatenate([xy, ring_xy(rng, k, r, phase=r, radial=0.03, angular=0.2)])
        r += 0.3
    return xy


class _Builder:
    """lipids of cluster frames: centres (valid on entry, with a patch) and markers (invalid on entry, no patch)"""

    def __init__(self, rng, sites):
        self.rng, self.sites, self.nsite = rng, sites, 0
        self.pos, self.valid, self.patches, self.rec = [], [], [], []

    def _add(self, xyz, valid, rec):
        self.pos.append(xyz); self.valid.append(valid); self.patches.append([]); self.rec.append(rec)
        return len(self.pos) - 1

    def align(self, site):
        while len(self.pos) % 4:
            self._add(np.array([site[0], site[1] + 3.9, 5.0]), 0, None)

    def wave(self, clusters):
        """the centres of `clusters` (kind, m, pad) on consecutive indices from a multiple of four, their markers behind them"""
        site = self.sites[self.nsite % len(self.sites)]
        self.nsite += 1
        self.align(site)
        form = "wave" if len(clusters) > 1 else "padded" if clusters[0][2] else "own"
        centres = []
        for kind, m, pad in clusters:
            c = np.array([site[0], site[1], 5.0]) + np.append(self.rng.uniform(-0.5, 0.5, 2), 0.0)
            centres.append((self._add(c, 1, dict(kind=kind, m=m, pad=pad, form=form)), c, kind, m, pad))
        for i, c, kind, m, pad in centres:
            xy = cluster_xy(self.rng, kind, m, pad)
            # a saddle with well separated principal curvatures (0.12 and -0.06 per nm) under the markers' noise
            z = 0.06 * xy[:, 0] ** 2 - 0.03 * xy[:, 1] ** 2 + 0.02 * self.rng.normal(size=len(xy))
            for q in range(len(xy)):
                self.patches[i].append(self._add(c + np.array([xy[q, 0], xy[q, 1], z[q]]), 0, None))

    def frame(self, box):
        K = len(self.pos)
        head = _f32(np.array(self.pos))
        nrm = _normals(K, self.rng)
        off, ids = csr(self.patches)
        centres = np.array([i for i in range(K) if self.rec[i] is not None], np.int64)
        return dict(head=head, normals=nrm, box=np.asarray(box, np.float32), valid=np.array(self.valid, np.uint8), patch_off=off,
                    patch_ids=ids, record=dict(centres=centres, built=[self.rec[i] for i in centres],
                                               np=np.diff(off.astype(np.int64))))


RING_SITES = [(4.0 + 8.0 * a, 4.0 + 8.0 * b) for a in range(3) for b in range(3)]
RING_BOX = np.diag([24.0, 24.0, 12.0])


def ring_frame(seed=2):
    rng = np.random.default_rng(seed)
    b = _Builder(rng, RING_SITES)
    for m in FINAL_M:
        b.wave([("final", m, 0)])
    for m in TRANSIENT_M:
        b.wave([("transient", m, 0)])
    for kind in ("final", "transient"):
        b.wave([(kind, m, 0) for m in WAVE_M])
        for pad in PADS:
            b.wave([(kind, 17, pad)])
    b.wave([("final", 16, 61)])                      # 61 members and a cell that fits the lanes: no hand-off
    for m in LAST_M:
        b.wave([("last", m, 0)])
    return b.frame(RING_BOX)


# ------------------------------------------------------------------------------------------------ reverse counts

HUB_MEMBERS = 12


def hub_frame(seed=3):
    """the sheet with patches of the 12 nearest markers (with 8, an ulp of the markers moves the curvatures by 0.75 of the
    f32 tolerance: tests/test_pinned_patches_cpu.py); the hubs' reverse counts are set exactly by editing the other lipids' patches.
    A hub is taken out of every patch (the owner takes its next-nearest marker instead) and appended to the patches of its
    c nearest owners.  Of the owners of a hub with c >= 15, one is invalid on entry, one has a normal along x (its local
    frame is singular: the fit drops it before anything is written) and one is lifted 1.5 nm off the sheet (the fit writes
    its fitted points, then drops it for a surface more than 0.5 nm away): the average has to skip the entries of all three.
    A lifted owner is named by no patch, so that it bends nobody else's fit."""
    rng = np.random.default_rng(seed)
    side = 24
    head, nrm, box = sheet(side, rng)
    K = side * side
    near = nearest_all(head, side * SPACING)
    counts = np.full(K, -1, np.int64)
    waves = []
    for w in range(10):                                  # ten waves of four hubs with four different round counts
        first = 4 * (14 * w + 3)
        cs = [HUB_COUNTS[(w + 3 * k) % 10] for k in range(4)]
        waves.append((first, cs))
        counts[first:first + 4] = cs
    for w, c in enumerate(HUB_COUNTS):                   # and one hub among three ordinary lipids
        counts[4 * (14 * w + 10) + w % 4] = c
    hubs = np.flatnonzero(counts >= 0)
    is_hub = counts >= 0
    role = np.zeros(K, np.int64)                         # 0 ordinary, 1 invalid on entry, 2 normal along x, 3 lifted
    owners = {}
    taken = is_hub.copy()
    for h in hubs:
        own = [j for j in near[h] if not is_hub[j]][:counts[h]]
        owners[h] = own
        if counts[h] >= 15:
            free = [j for j in own if not taken[j]]
            for r, j in zip((1, 2, 3), free[1::4]):
                role[j] = r
                taken[j] = True
    lifted = role == 3
    out = is_hub | lifted                                # named by no patch of their own accord
    patches = [[j for j in near[i] if not out[j]][:HUB_MEMBERS] for i in range(K)]
    for h in hubs:
        for j in owners[h]:
            patches[j].append(h)
    valid = np.ones(K, np.uint8)
    valid[role == 1] = 0
    nrm[role == 2] = np.array([1.0, 0.0, 0.0], np.float32)
    head[lifted, 2] += np.float32(1.5)
    off, ids = csr(patches)
    return dict(head=head, normals=nrm, box=box, valid=valid, patch_off=off, patch_ids=ids,
                record=dict(hubs=hubs, counts=counts[hubs], role=role, np=np.diff(off.astype(np.int64))))


# ------------------------------------------------------------------------------------------------ launch edges

def small_frame(K):
    """K lipids.  K >= 16: a final-7 cluster (centre, 7 + 8 markers) first; 8 <= K < 16: the centre and 7 markers whose
    radii alternate by 12 % (seven markers on one circle would leave the quadric fit rank-deficient); K < 8: lipid 0 valid
    with an empty patch.  Every other lipid is invalid on entry and carries a short patch."""
    assert K >= 1
    rng = np.random.default_rng(100 + K)
    c = np.array([5.0, 5.0, 5.0])
    pos, patches = [c], [[]]
    if K >= 16:
        xy = cluster_xy(rng, "final", 7)
    elif K >= 8:
        a = 2 * np.pi * np.arange(7) / 7
        r = 0.8 * (1.0 + 0.12 * np.array([1, -1, 1, -1, 1, -1, 0]))
        xy = np.stack([r * np.cos(a), r * np.sin(a)], 1)
    else:
        xy = np.zeros((0, 2))
    for q in range(len(xy)):
        pos.append(c + np.array([xy[q, 0], xy[q, 1], 0.06 * xy[q, 0] ** 2 - 0.03 * xy[q, 1] ** 2 + 0.02 * rng.normal()]))
        patches.append([])
        patches[0].append(q + 1)
    built = 7 if len(xy) else 0
    while len(pos) < K:
        pos.append(c + np.append(rng.uniform(-3.0, 3.0, 2), 0.02 * rng.normal()))
        patches.append([])
    for i in range(1, K):                                # invalid on entry: 1 .. 5 members (as many as there are other lipids)
        n = min(1 + i % 5, K - 1)
        patches[i] = [int(x) for x in rng.permutation([j for j in range(K) if j != i])[:n]]
    valid = np.zeros(K, np.uint8)
    valid[0] = 1
    off, ids = csr(patches)
    return dict(head=_f32(np.array(pos)), normals=_normals(K, rng), box=np.diag([10.0, 10.0, 12.0]).astype(np.float32), valid=valid,
                patch_off=off, patch_ids=ids, record=dict(m=built, np=np.diff(off.astype(np.int64))))


def open_cell(head, L, rows, ids):
    """lipids whose patch leaves a sector of 150 degrees without a marker: their cell is open, or closed only far away"""
    d = head[ids][:, :, :2].astype(np.float64) - head[rows][:, None, :2].astype(np.float64)
    d -= L * np.round(d / L)
    a = np.sort(np.arctan2(d[:, :, 1], d[:, :, 0]), axis=1)
    return np.maximum(np.diff(a, axis=1).max(1), 2 * np.pi - (a[:, -1] - a[:, 0])) > np.deg2rad(150.0)


LARGE_MEMBERS = 12


def large_frame(K, seed=4):
    """exactly K lipids: ring clusters (LARGE_RINGS) at the low end, in the middle and at the high end of the index range - the
    middle one with a second cluster (LARGE_PAIR) whose centre sits 16 lipids behind its own, so that in f32, where only
    handed-over lipids reach the one-lane kernel, two lanes of one 32- or 64-lane workgroup keep their cells in LDS -, as many copies of one periodic sheet of 24 x 24 markers as fit beside them, and fillers (invalid on entry, short
    patches) for the rest.  The copies lie on top of each other in one 19.2 nm box, each with its lipids in another cyclic
    order - patches are explicit, a copy's lipids name markers of their own copy only.  One sheet of 128 x 128 markers would
    reach 100 nm, where an ulp of a float32 marker moves the fitted coefficients by more than the tolerance, and among 16 000
    random cells some Voronoi vertex always sits where two cutting lines are nearly parallel; the copies keep the frame as
    well conditioned as the one sheet, which tests/test_pinned_patches_cpu.py measures.  Sheet lipids have
    their 12 nearest markers as patch, except the lipids whose index is a multiple of 29 (coprime to 64: every thread index
    of a 64-lane workgroup is met), which cycle through LARGE_CYCLE; the few whose cell would be open are off on entry."""
    rng = np.random.default_rng(seed)
    side = 24
    tile = side * side
    L = side * SPACING
    groups = [[m] if m != LARGE_RINGS[1] else [m, LARGE_PAIR] for m in LARGE_RINGS]
    sizes = [sum(1 + m + max(m, 8) for m in g) for g in groups]
    ntiles = (K - sum(sizes) - 8) // tile
    assert ntiles >= 2
    ns = ntiles * tile
    half = tile * (ntiles // 2)
    # index layout: [cluster 0 | first sheets | cluster 1 | other sheets | fillers | cluster 2], centres on multiples of four
    start_s0 = sizes[0] + -sizes[0] % 4
    start_c1 = start_s0 + half
    start_s1 = start_c1 + sizes[1] + -sizes[1] % 4
    start_c2 = (K - sizes[2]) - (K - sizes[2]) % 4
    assert start_c2 >= start_s1 + (ns - half)
    lipid_of = np.concatenate([start_s0 + np.arange(half), start_s1 + np.arange(ns - half)])      # sheet marker -> lipid index
    head = np.zeros((K, 3), np.float32); nrm = _normals(K, rng); valid = np.zeros(K, np.uint8)
    patches = [[] for _ in range(K)]
    kind = np.zeros(K, np.int64)                         # 0 filler / cluster marker, 1 sheet, 2 cluster centre
    kind[lipid_of] = 1
    valid[lipid_of] = 1
    # multiples of 29 among the sheet lipids; one in the middle cluster's block of 64 lipids (else the first behind it) has 97
    # members: a long patch in the HBM slices and a large cell in LDS in one workgroup
    long_l = lipid_of[lipid_of % 29 == 0]
    same = np.flatnonzero(long_l // 64 == start_c1 // 64)
    after = int(same[0]) if len(same) else int(np.searchsorted(long_l, start_c1))
    length = np.full(K, LARGE_MEMBERS, np.int64)
    length[long_l] = [LARGE_CYCLE[(3 + k - after) % 5] for k in range(len(long_l))]
    h, n, box = sheet(side, rng)
    near = nearest_all(h, L)
    is_open = open_cell(h, L, np.arange(tile), near[:, :LARGE_MEMBERS])
    for t in range(ntiles):                              # lipid r of sheet t is marker (r + 17 t) mod 576 of the one sheet
        mine = lipid_of[t * tile:(t + 1) * tile]
        mark = (np.arange(tile) + 17 * t) % tile
        head[mine] = h[mark]; nrm[mine] = n[mark]
        for r in range(tile):
            patches[mine[r]] = mine[(near[mark[r], :length[mine[r]]] - 17 * t) % tile]
        valid[mine[is_open[mark]]] = 0
    centres, built = [], []
    used = kind == 1
    for k, (s, g) in enumerate(zip((0, start_c1, start_c2), groups)):
        b = _Builder(rng, [(0.25 * L * (k + 1), 0.5 * L)])
        b.wave([("final", m, 0) for m in g])
        f = b.frame(box)
        n = len(f["valid"])
        at = np.arange(n)
        if len(g) == 2:                                  # the second centre 16 lipids behind the first, not next to it
            at[[1, 16]] = [16, 1]
        head[s + at] = f["head"]; nrm[s + at] = f["normals"]; valid[s + at] = f["valid"]
        po = f["patch_off"].astype(np.int64)
        for i in range(n):
            patches[s + at[i]] = at[f["patch_ids"][po[i]:po[i + 1]].astype(np.int64)] + s
        for c, rec in zip(f["record"]["centres"], f["record"]["built"]):
            centres.append(s + at[c]); built.append(rec); kind[s + at[c]] = 2
        used[s:s + n] = True
    for i in np.flatnonzero(~used):                      # fillers and alignment gaps: beside a sheet marker, 1 .. 5 sheet markers
        j = lipid_of[rng.integers(ns)]
        head[i] = head[j] + np.array([0.1, 0.1, 0.0], np.float32)
        patches[i] = patches[j][:1 + int(i) % 5]
    off, ids = csr(patches)
    return dict(head=head, normals=nrm, box=box, valid=valid, patch_off=off, patch_ids=ids,
                record=dict(centres=np.array(centres), built=built, kind=kind, np=np.diff(off.astype(np.int64)), sheets=ntiles))
