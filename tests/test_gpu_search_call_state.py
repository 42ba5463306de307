"""A request that fails, or a request of another form, leaves nothing behind for the next one on the same context.

What one request asks of the shared search helpers (plan or not, side stream, output capacity, pairs plane only, dropping
non-finite atoms ...) travels as an argument of the call; the context keeps only what outlasts a request.  Every comparison
here is bit for bit against the same request on a freshly created Engine; the single and double lists of the sequence are
compared once against the f32 oracle as well.  The error cases are argument errors that prepare_search returns: nothing
reaches the device."""
import numpy as np
import pytest

from molar_amd import synth

pytestmark = pytest.mark.gpu

N, N2 = 4096, 512
CUTOFF = 0.8          # a cube of 4096 atoms at 100 atoms / nm^3 is 3.45 nm across: 4 x 4 x 4 cells (side stream, plan, both passes)
HIST = (0.0, 0.8, 64)


@pytest.fixture(scope="module")
def a():
    from molar_amd import build
    import molar_amd.api as api
    build.build_library()
    return api


@pytest.fixture(scope="module")
def sys_(a):
    import torch
    box = synth.box_ortho(N)
    pos = synth.frame(N, box, 0)
    pos2 = synth.frame(N2, box, 7, seed=4321)
    pos2b = synth.frame(N2, box, 8, seed=999)
    box_mid = (box * np.float32(1.3)).astype(np.float32)          # 5 x 5 x 5 cells at the same cutoff
    frames = np.stack([pos, synth.frame(N, box_mid, 1), synth.frame(N, box, 2)])
    nan = pos.copy()
    nan[1234, 1] = np.nan
    s = dict(box=box, pos=pos, pos2=pos2, nan=nan, frames=frames, boxes=np.stack([box, box_mid, box]),
             d_pos=torch.from_numpy(pos).cuda(), d_pos2=torch.from_numpy(pos2).cuda(), d_pos2b=torch.from_numpy(pos2b).cuda(),
             d_frames=torch.from_numpy(frames).cuda())
    e = a.Engine(0)
    e.search_count(a.SEARCH_SINGLE, CUTOFF, pos, box=box, pbc=7)
    dims = tuple(e.grid_dims())
    assert min(dims) >= 3
    e.search_count(a.SEARCH_SINGLE, CUTOFF, frames[1], box=box_mid, pbc=7)
    assert tuple(e.grid_dims()) != dims          # the middle frame of the block takes the frames form off its batched path
    return s


def count_fill(a, e, s, pos=None):
    cnt = e.search_count(a.SEARCH_SINGLE, CUTOFF, s["pos"] if pos is None else pos, box=s["box"], pbc=7)
    return (cnt,) + e.search_fill(cnt)


def same_list(got, want, what):
    assert got[0] == want[0] > 0, what
    assert got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes(), what


def resident_arrays(a, res, want_dist=True):
    import torch
    cnt, pp, dp = res
    pairs = a.device_view(pp, (cnt, 2), torch.int32).cpu().numpy().view(np.uint32)
    if not want_dist:
        return cnt, pairs, None
    assert dp, "the resident search must deliver distances"
    return cnt, pairs, a.device_view(dp, (cnt,), torch.float32).cpu().numpy()


def bins_tensor():
    import torch
    return torch.zeros(HIST[2], dtype=torch.int64, device="cuda")


@pytest.fixture(scope="module")
def fresh_single(a, sys_):
    return count_fill(a, a.Engine(0), sys_)


def test_failed_asynchronous_histogram_leaves_no_side_stream_or_skipped_plan(a, sys_, fresh_single):
    """(a) device bins, no count, cutoff 0: fails in prepare_search after the call asked for the side stream and for no plan."""
    e = a.Engine(0)
    with pytest.raises(a.MolarHipError):
        e.search_histogram(a.SEARCH_SINGLE, 0.0, *HIST, sys_["d_pos"], box=sys_["box"], pbc=7, bins=bins_tensor(), want_count=False)
    same_list(count_fill(a, e, sys_), fresh_single, "count + fill after the failed histogram")


def test_failed_within_set_leaves_planning_on(a, sys_, fresh_single):
    """(b) no box, no lower / upper: fails in prepare_search with planning switched off."""
    e = a.Engine(0)
    with pytest.raises(a.MolarHipError):
        e.within_set(CUTOFF, sys_["d_pos"], xyz2=sys_["d_pos2"])
    same_list(count_fill(a, e, sys_), fresh_single, "count + fill after the failed within_set")


def test_failed_resident_begin_leaves_both_tickets_and_the_distances(a, sys_):
    """(c) begin with cutoff 0 fails; both tickets stay free, their results are the plain call's, distances still come."""
    e, f = a.Engine(0), a.Engine(0)
    bad, _k0 = e.make_search_desc(a.SEARCH_SINGLE, 0.0, sys_["d_pos"], box=sys_["box"], pbc=7)
    with pytest.raises(a.MolarHipError):
        e.search_resident_begin(bad)
    want = resident_arrays(a, f.search_resident(a.SEARCH_SINGLE, CUTOFF, sys_["d_pos"], box=sys_["box"], pbc=7))
    good, _k1 = e.make_search_desc(a.SEARCH_SINGLE, CUTOFF, sys_["d_pos"], box=sys_["box"], pbc=7)
    t0 = e.search_resident_begin(good)
    t1 = e.search_resident_begin(good)
    assert {t0, t1} == {0, 1}
    for t in (t0, t1):
        same_list(resident_arrays(a, e.search_resident_end(t)), want, f"ticket {t}")
    same_list(resident_arrays(a, e.search_resident(a.SEARCH_SINGLE, CUTOFF, sys_["d_pos"], box=sys_["box"], pbc=7)), want, "plain call")


def test_synchronous_calls_between_two_tickets_in_flight(a, sys_):
    """With both tickets of search_resident_begin in flight: a count + fill of another kind and cutoff, a histogram whose edge
    table the engine has to stage, a min_max - every one of them goes through the context's bounce buffer - and then the two
    ends.  The tickets' sizes are delivered while those calls run, so nothing of a ticket may live where they stage or read
    back.  Every result is bit for bit that of the same call on a fresh Engine; the occupied cells the last search reports (the
    second ticket's: on an Engine without result buffers an end runs its search once more, knowing what the ticket's record
    said) are those a fresh Engine reports that ran only this search, until it knew them - twice."""
    s = sys_
    hist = (0.1, 0.7, 48)          # not HIST: no Engine of this test has this edge table yet
    desc = lambda eng: eng.make_search_desc(a.SEARCH_SINGLE, CUTOFF, s["d_pos"], box=s["box"], pbc=7)

    def other_count_fill(eng):
        cnt = eng.search_count(a.SEARCH_DOUBLE, 0.6, s["pos"], xyz2=s["pos2"], box=s["box"], pbc=7)
        return (cnt,) + eng.search_fill(cnt)

    def histogram(eng):
        bins, cnt = eng.search_histogram(a.SEARCH_SINGLE, CUTOFF, *hist, s["pos"], box=s["box"], pbc=7)
        return np.asarray(bins).copy(), cnt

    e = a.Engine(0)
    d, _keep = desc(e)
    t0 = e.search_resident_begin(d)
    t1 = e.search_resident_begin(d)
    assert {t0, t1} == {0, 1}
    got_double = other_count_fill(e)
    got_bins, got_cnt = histogram(e)
    got_lo, got_up = e.min_max(s["pos"])
    first = resident_arrays(a, e.search_resident_end(t0))
    second = resident_arrays(a, e.search_resident_end(t1))
    got_cells = e.search_cell_kernels()

    same_list(got_double, other_count_fill(a.Engine(0)), "count + fill between begin and end")
    want_bins, want_cnt = histogram(a.Engine(0))
    assert got_cnt == want_cnt > 0 and got_bins.dtype == want_bins.dtype and got_bins.tobytes() == want_bins.tobytes() and got_bins.any()
    want_lo, want_up = a.Engine(0).min_max(s["pos"])
    assert got_lo.tobytes() == want_lo.tobytes() and got_up.tobytes() == want_up.tobytes() and (want_up > want_lo).all()
    f = a.Engine(0)
    want = resident_arrays(a, f.search_resident(a.SEARCH_SINGLE, CUTOFF, s["d_pos"], box=s["box"], pbc=7))
    same_list(first, want, "first ticket")
    same_list(second, want, "second ticket")
    same_list(second, first, "the two tickets")
    same_list(resident_arrays(a, f.search_resident(a.SEARCH_SINGLE, CUTOFF, s["d_pos"], box=s["box"], pbc=7)), want, "the same search again")
    want_cells = f.search_cell_kernels()          # (of the second run, which knows what the first one counted)
    assert got_cells == want_cells and want_cells[1][0] > 0


def sequence(a, e, s):
    """(d) one request of every form; returns what each step produced."""
    import torch
    out = {}
    b = bins_tensor()
    e.search_histogram(a.SEARCH_SINGLE, CUTOFF, *HIST, s["d_pos"], box=s["box"], pbc=7, bins=b, want_count=False)
    e.synchronize()
    out["hist"] = b.cpu().numpy()
    e.within_hold(True)
    dev_ids = lambda n: torch.empty(n, dtype=torch.int64, device="cuda")
    # (a fill into device memory is enqueued on the engine's stream, which torch's copy does not wait for: synchronize first)
    w1 = e.within_set(CUTOFF, s["d_pos"], xyz2=s["d_pos2"], box=s["box"], pbc=7, device_out=dev_ids)
    e.synchronize()
    out["within1"] = w1.cpu().numpy()
    w2 = e.within_set(CUTOFF, s["d_pos"], xyz2=s["d_pos2b"], box=s["box"], pbc=7, device_out=dev_ids)
    e.synchronize()
    out["within2"] = w2.cpu().numpy()
    e.within_hold(False)
    c = e.search_contacts(a.SEARCH_SINGLE, CUTOFF, s["d_pos"], box=s["box"], pbc=7)
    out["contacts"] = (c.count, c.deg1.cpu().numpy())
    out["conn"] = e.search_connectivity(CUTOFF, s["d_pos"], box=s["box"], pbc=7)
    out["double"] = resident_arrays(a, e.search_resident(a.SEARCH_DOUBLE, CUTOFF, s["d_pos"], xyz2=s["d_pos2"], box=s["box"], pbc=7))
    b = bins_tensor()
    e.search_histogram_frames(a.SEARCH_SINGLE, CUTOFF, *HIST, s["d_frames"], box=s["boxes"], pbc=7, bins=b)
    e.synchronize()
    out["hist_frames"] = b.cpu().numpy()
    out["single"] = count_fill(a, e, s)
    return out


def same_sequence(got, want, what):
    for k in ("hist", "within1", "within2", "hist_frames"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes() and got[k].any(), f"{what}: {k}"
    assert got["contacts"][0] == want["contacts"][0] > 0 and got["contacts"][1].tobytes() == want["contacts"][1].tobytes(), f"{what}: contacts"
    for g, w in zip(got["conn"], want["conn"]):
        assert g.tobytes() == w.tobytes() and len(g) > 1, f"{what}: connectivity"
    same_list(got["double"], want["double"], f"{what}: resident double search")
    same_list(got["single"], want["single"], f"{what}: count + fill")


def test_requests_of_every_form_in_turn_equal_a_fresh_engine(a, sys_, orc32):
    s = sys_
    want = sequence(a, a.Engine(0), s)
    ob = orc32.box_from_matrix(s["box"])
    ref = orc32.search_single_pbc(CUTOFF, s["pos"], ob, 7, nthreads=4)
    cnt, pairs, dist = want["single"]
    assert cnt == len(ref["i"]) and np.array_equal(pairs[:, 0], ref["i"]) and np.array_equal(pairs[:, 1], ref["j"]) and np.array_equal(dist, ref["d"])
    ref = orc32.search_double_pbc(CUTOFF, s["pos"], s["pos2"], ob, 7, nthreads=4)
    cnt, pairs, dist = want["double"]
    assert cnt == len(ref["i"]) and np.array_equal(pairs[:, 0], ref["i"]) and np.array_equal(pairs[:, 1], ref["j"]) and np.array_equal(dist, ref["d"])
    e = a.Engine(0)
    for rnd in range(2):             # the second round starts from whatever the first left
        same_sequence(sequence(a, e, s), want, f"round {rnd}")


NO_SEARCH = 52          # MOLAR_HIP_ERR_NO_SEARCH


def single_frame_histograms(a, e, s, which, box):
    """The frames `which` of the block one by one through the single-frame histogram, summed into one set of device bins."""
    b = bins_tensor()
    for k in which:
        e.search_histogram(a.SEARCH_SINGLE, CUTOFF, *HIST, s["d_frames"][k], box=box[k] if box.ndim == 3 else box, pbc=7, bins=b, want_count=False)
    e.synchronize()
    return b.cpu().numpy()


def no_cached_search(a, e):
    for call in (e.grid_dims, lambda: e.search_fill(1)):
        with pytest.raises(a.MolarHipError) as err:
            call()
        assert err.value.code == NO_SEARCH


def test_batched_frames_leave_the_cached_search_shape_alone(a, sys_, fresh_single):
    """A batched frames call describes its frames by shapes of its own: search_cell_kernels() keeps answering for the context's
    last search proper - also when the group's grid (5 x 5 x 5 under box_mid) is not that search's (4 x 4 x 4).  The group is
    frames 0 and 2 of the block, which share `box`: two frames of one shape, everything in device memory."""
    s = sys_
    box_mid = s["boxes"][1]
    e = a.Engine(0)
    assert count_fill(a, e, s)[0] == fresh_single[0] and e.grid_dims() == (4, 4, 4)
    before = e.search_cell_kernels()
    pair = s["d_frames"][::2]                     # frames 0 and 2, a strided view
    for box in (s["box"], box_mid):
        want = single_frame_histograms(a, a.Engine(0), s, (0, 2), box)
        b = bins_tensor()
        e.search_histogram_frames(a.SEARCH_SINGLE, CUTOFF, *HIST, pair, box=box, pbc=7, bins=b)
        e.synchronize()
        got = b.cpu().numpy()
        assert got.tobytes() == want.tobytes() and got.any()
        assert e.search_cell_kernels() == before
        no_cached_search(a, e)
        same_list(count_fill(a, e, s), fresh_single, "count + fill after the batched frames call")
        assert e.search_cell_kernels()[0] == before[0]
        before = e.search_cell_kernels()          # (the second count knows the grid's occupied cells from the first)


def test_frames_that_give_up_batching_leave_nothing_behind(a, sys_):
    """The three-frame block whose middle frame has other grid dims leaves the batched path after its dims loop and is walked
    frame by frame: those are searches proper, so the context then answers for the last of them, as an Engine does that was
    handed the three frames singly - and a count + fill on another box equals a fresh Engine's."""
    s = sys_
    box_mid = s["boxes"][1]
    e, g = a.Engine(0), a.Engine(0)
    for eng in (e, g):
        count_fill(a, eng, s)
    want = single_frame_histograms(a, g, s, (0, 1, 2), s["boxes"])
    b = bins_tensor()
    e.search_histogram_frames(a.SEARCH_SINGLE, CUTOFF, *HIST, s["d_frames"], box=s["boxes"], pbc=7, bins=b)
    e.synchronize()
    got = b.cpu().numpy()
    assert got.tobytes() == want.tobytes() and got.any()
    assert e.search_cell_kernels() == g.search_cell_kernels()
    no_cached_search(a, e)

    def on_mid(eng):
        cnt = eng.search_count(a.SEARCH_SINGLE, CUTOFF, s["frames"][1], box=box_mid, pbc=7)
        return (cnt,) + eng.search_fill(cnt)
    same_list(on_mid(e), on_mid(a.Engine(0)), "count + fill on another box after the frames call")
    assert e.grid_dims() == (5, 5, 5)


def test_membrane_frame_then_a_search_with_a_nan_coordinate(a, sys_):
    """(e) the membrane's marker search drops non-finite atoms from its grid and fills the pairs plane only; a plain search
    behind it on the same context bins a NaN atom the way the reference does and delivers distances."""
    from molar_amd import membrane as mb
    xyz, box, first, tpl, masses = mb.build_bilayer(20, 3000)
    e, f = a.Engine(0), a.Engine(0)
    res = []
    for eng in (e, f):
        m = mb.Membrane(eng, len(xyz), first, tpl, masses, mb.MembraneOptions(cutoff=1.5, order_type=1))
        assert m.fusable()
        res.append(m.compute_end(m.compute_begin(xyz.copy(), box)))
    for k in ("patch_off", "patch_ids", "normals", "valid"):
        assert np.ascontiguousarray(res[0][k]).tobytes() == np.ascontiguousarray(res[1][k]).tobytes(), k
    assert len(res[0]["patch_ids"]) > 0
    want = count_fill(a, a.Engine(0), sys_, pos=sys_["nan"])
    same_list(count_fill(a, e, sys_, pos=sys_["nan"]), want, "count + fill of a frame with a NaN after the membrane frame")


# ---- the lane of a grid build: stream, scan scratch and sort scratch travel together
# A pipelined resident search on an Engine that owns its stream builds its grid on the side stream, with that stream's scratch;
# count + fill on another Engine builds the same grid on the main stream.  Two shapes reach the per-stream scratch:
#  * more than 8191 cells: the cell counts are scanned in tiles, whose block sums live in the stream's scan scratch;
#  * more than 384 atoms per cell on average: the cell order comes from the device sort and its scratch.
N_CELLS, RC_CELLS = 30000, 0.3        # box_ortho: 100 atoms / nm^3, 6.69 nm across: 22 x 22 x 22 cells
N_SORT, RC_SORT = 1000, 1.2           # 2.15 nm across: one cell of 1000 atoms


@pytest.fixture(scope="module")
def lanes(a):
    """The frames of the two shapes on host and device, and what count + fill of ONE fresh Engine (grids on the main stream)
    gives for each, with the grid it came to."""
    import torch
    f = {}
    box = synth.box_ortho(N_CELLS)
    f["A"] = dict(box=box, rc=RC_CELLS, pos=synth.frame(N_CELLS, box, 0))
    f["B"] = dict(box=box, rc=RC_CELLS, pos=synth.frame(N_CELLS, box, 1))
    box = synth.box_ortho(N_SORT)
    f["C"] = dict(box=box, rc=RC_SORT, pos=synth.frame(N_SORT, box, 2))
    main = a.Engine(0)
    for v in f.values():
        v["d_pos"] = torch.from_numpy(v["pos"]).cuda()
        cnt = main.search_count(a.SEARCH_SINGLE, v["rc"], v["pos"], box=v["box"], pbc=7)
        v["want"] = (cnt,) + main.search_fill(cnt)
        v["dims"] = main.grid_dims()
    return f


def pipelined(a, e, lanes, names):
    """The frames `names` through search_resident_begin / _end on `e`, two in flight; each result against the main-stream one."""
    descs = {k: e.make_search_desc(a.SEARCH_SINGLE, lanes[k]["rc"], lanes[k]["d_pos"], box=lanes[k]["box"], pbc=7) for k in set(names)}
    for k in range(0, len(names), 2):
        pair = names[k:k + 2]
        tickets = [e.search_resident_begin(descs[name][0]) for name in pair]
        assert sorted(tickets) == [0, 1]
        for name, t in zip(pair, tickets):
            same_list(resident_arrays(a, e.search_resident_end(t)), lanes[name]["want"], f"frame {name}, step {k}")


def against_oracle(orc32, v):
    ref = orc32.search_single_pbc(v["rc"], v["pos"], orc32.box_from_matrix(v["box"]), 7, nthreads=4)
    cnt, pairs, dist = v["want"]
    assert cnt == len(ref["i"]) and np.array_equal(pairs[:, 0], ref["i"]) and np.array_equal(pairs[:, 1], ref["j"]) and np.array_equal(dist, ref["d"])


def test_tile_scan_of_a_grid_built_on_the_side_stream(a, lanes, orc32):
    assert int(np.prod(lanes["A"]["dims"])) + 1 > 8192 and lanes["B"]["dims"] == lanes["A"]["dims"]
    pipelined(a, a.Engine(0), lanes, "ABAB")
    against_oracle(orc32, lanes["A"])


def test_device_sort_of_a_grid_built_on_the_side_stream(a, lanes, orc32):
    """Alternating with a frame of many cells: the scan and sort scratch of the side stream have been sized by the other shape
    before they are used again."""
    assert N_SORT > 384 * int(np.prod(lanes["C"]["dims"]))
    pipelined(a, a.Engine(0), lanes, "CACA")
    against_oracle(orc32, lanes["C"])


def test_empty_vdw_request_between_ordinary_ones(a, sys_, fresh_single):
    """A vdW request with an empty second set comes to nothing: count 0, a grid of one cell, an empty fill - through count,
    through the resident call and through the fused histogram - and the Engine answers the ordinary request as a fresh one does."""
    s = sys_
    empty = dict(xyz2=s["pos2"], idx2=np.zeros(1, np.uint64)[:0], vdw1=np.full(N, 0.15, np.float32), vdw2=np.ones(1, np.float32),
                 box=s["box"], pbc=7)
    e = a.Engine(0)
    same_list(count_fill(a, e, s), fresh_single, "count + fill before")
    assert e.grid_dims() == (4, 4, 4)
    assert e.search_count(a.SEARCH_DOUBLE_VDW, None, s["pos"], **empty) == 0
    assert e.grid_dims() == (1, 1, 1)
    pairs, dist = e.search_fill(0)
    assert pairs.shape == (0, 2) and dist.shape == (0,)
    same_list(count_fill(a, e, s), fresh_single, "count + fill after the empty vdW count")
    assert e.search_resident(a.SEARCH_DOUBLE_VDW, None, s["pos"], **empty)[0] == 0
    assert e.grid_dims() == (1, 1, 1)
    same_list(count_fill(a, e, s), fresh_single, "count + fill after the empty resident vdW search")
    bins, cnt = e.search_histogram(a.SEARCH_DOUBLE_VDW, None, *HIST, s["pos"], **empty)
    assert cnt == 0 and not np.asarray(bins).any()
    assert e.grid_dims() == (1, 1, 1)
    same_list(count_fill(a, e, s), fresh_single, "count + fill after the empty vdW histogram")


# ---- the consumers of the search keep their states apart: within.hip, connectivity.hip, contacts.hip
# `within` as a set, SearchConnectivity and the contacts / clusters calls each keep what outlasts a call in a state of their own
# behind one pointer of the context, made on first use.  Sizes are those of sys_; the partner-list path of `within` needs a
# second set of at least 4682 atoms (the branch is n2 * 28 <= 2^17), so one more frame of 5000 atoms in the same box.
N2_PARTNERS = 5000


def test_calls_on_states_that_were_never_created(a):
    import ctypes as C
    from molar_amd import _lib
    e = a.Engine(0)
    ids, off = np.zeros(4, np.uint64), np.zeros(4, np.uint64)
    assert e.lib.molar_hip_within_fill(e.ctx, ids.ctypes.data) == NO_SEARCH
    assert _lib.last_error() == "no cached within set: call molar_hip_within_count first"
    assert e.lib.molar_hip_search_connectivity_fill(e.ctx, off.ctypes.data, ids.ctypes.data) == NO_SEARCH
    assert _lib.last_error() == "no cached connectivity: call molar_hip_search_connectivity first"
    out4 = (C.c_uint64 * 4)(7, 7, 7, 7)
    assert e.lib.molar_hip_search_clusters_counters(e.ctx, 0, out4) == 0 and list(out4) == [0, 0, 0, 0]
    assert e.lib.molar_hip_within_hold(e.ctx, 1) == 0 and e.lib.molar_hip_within_hold(e.ctx, 0) == 0
    e.close()


def within_and_connectivity(a, e, s, second, between):
    """within_count .. within_fill (to host and to device memory) and search_connectivity .. _fill by raw calls, with
    `between` run inside each pair."""
    import ctypes as C
    import torch
    d, _k = e.make_search_desc(a.SEARCH_WITHIN, CUTOFF, s["pos"], xyz2=second, box=s["box"], pbc=7)
    cnt = C.c_uint64(0)
    assert e.lib.molar_hip_within_count(e.ctx, C.byref(d), C.byref(cnt)) == 0
    between()
    ids = np.empty(cnt.value, np.uint64)
    assert e.lib.molar_hip_within_fill(e.ctx, ids.ctypes.data) == 0
    dev = torch.empty(cnt.value, dtype=torch.int64, device="cuda")
    assert e.lib.molar_hip_within_fill(e.ctx, dev.data_ptr()) == 0
    e.synchronize()
    d, _k = e.make_search_desc(a.SEARCH_SINGLE, CUTOFF, s["pos"], box=s["box"], pbc=7, ids_local=True)
    rows, ent = C.c_uint64(0), C.c_uint64(0)
    assert e.lib.molar_hip_search_connectivity(e.ctx, C.byref(d), C.byref(rows), C.byref(ent)) == 0
    between()
    off, nb = np.empty(rows.value + 1, np.uint64), np.empty(max(ent.value, 1), np.uint64)
    assert e.lib.molar_hip_search_connectivity_fill(e.ctx, off.ctypes.data, nb.ctypes.data) == 0
    return ids, dev.cpu().numpy().view(np.uint64), off, nb[:ent.value]


@pytest.mark.parametrize("n2", [N2, N2_PARTNERS], ids=["small_list", "partner_lists"])
def test_a_cached_result_survives_the_other_consumers(a, sys_, n2):
    s = sys_
    assert N2 * 28 <= 2 ** 17 < N2_PARTNERS * 28
    second = s["pos2"] if n2 == N2 else synth.frame(n2, s["box"], 9, seed=77)
    e = a.Engine(0)

    def others():
        c = e.search_contacts(a.SEARCH_SINGLE, CUTOFF, s["pos2"], box=s["box"], pbc=7)
        k = e.search_clusters(CUTOFF, s["pos2"], box=s["box"], pbc=7)
        assert c.count > 0 and 0 < k.ncomponents < N2
    got = within_and_connectivity(a, e, s, second, others)
    want = within_and_connectivity(a, a.Engine(0), s, second, lambda: None)
    for g, w, name in zip(got, want, ("ids", "ids left on the device", "offsets", "neighbours")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes() and len(w) > 1, name
    assert got[0].tobytes() == got[1].tobytes() and np.all(np.diff(got[0].astype(np.int64)) > 0)


def csr_in_push_order(ref, rows):
    """SearchConnectivity::from_iter (connectivity.rs:19-35): pair p pushes j onto i's list (entry 2p), i onto j's (2p + 1)"""
    npairs = len(ref["i"])
    row = np.empty(2 * npairs, np.uint64); nb = np.empty(2 * npairs, np.uint64)
    row[0::2], row[1::2] = ref["i"], ref["j"]
    nb[0::2], nb[1::2] = ref["j"], ref["i"]
    order = np.argsort(row, kind="stable")
    off = np.searchsorted(row[order], np.arange(rows + 1, dtype=np.uint64)).astype(np.uint64)
    return off, nb[order]


def test_one_csr_home_for_both_precisions(a, sys_, orc32, orc64):
    """The f64 entry and the f32 entry build their CSR in the same place and the one _fill copies it out: first the f64 lists,
    then, after an f32 request on another cutoff, the f32 lists."""
    s = sys_
    e = a.Engine(0)
    pos64, box64 = s["pos"].astype(np.float64), s["box"].astype(np.float64)
    off, nb = e.search_connectivity_f64(CUTOFF, pos64, box=box64, pbc=7)
    woff, wnb = csr_in_push_order(orc64.search_single_pbc(CUTOFF, pos64, orc64.box_from_matrix(box64), 7, nthreads=4), N)
    assert len(wnb) > N and np.array_equal(off, woff) and np.array_equal(nb, wnb)
    off, nb = e.search_connectivity(0.6, s["pos"], box=s["box"], pbc=7)
    woff32, wnb32 = csr_in_push_order(orc32.search_single_pbc(0.6, s["pos"], orc32.box_from_matrix(s["box"]), 7, nthreads=4), N)
    assert N < len(wnb32) < len(wnb) and np.array_equal(off, woff32) and np.array_equal(nb, wnb32)


def test_engines_that_used_every_consumer_close_cleanly(a, sys_, fresh_single):
    """Three times: an Engine that has made every state - the `within` set, the connectivity CSR, the contacts and clusters
    calls' second context and work areas, a cached search - is closed; every release path and the buffers that free themselves
    run once per cycle.  A fresh Engine then answers as ever."""
    s = sys_
    labels = (np.arange(N) % 8).astype(np.uint32)
    for _ in range(3):
        e = a.Engine(0)
        assert len(e.within_set(CUTOFF, s["pos"], xyz2=s["pos2"], box=s["box"], pbc=7)) > 0
        assert len(e.search_connectivity(CUTOFF, s["pos"], box=s["box"], pbc=7)[1]) > 0
        c = e.search_contacts(a.SEARCH_SINGLE, CUTOFF, s["pos"], box=s["box"], pbc=7, group1=labels, ngroups1=8)
        assert c.count > 0 and np.asarray(c.map).any()
        assert e.search_clusters(CUTOFF, s["pos"], box=s["box"], pbc=7).ncomponents >= 1
        blk = e.search_clusters_frames(CUTOFF, s["frames"][:2], box=s["boxes"][:2], pbc=7)
        assert len(blk.ncomponents) == 2 and min(blk.ncomponents) >= 1
        assert count_fill(a, e, s)[0] == fresh_single[0]
        e.close()
        assert e.ctx is None
    same_list(count_fill(a, a.Engine(0), s), fresh_single, "count + fill after three engines were closed")
