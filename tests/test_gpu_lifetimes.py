"""molar_hip_lifetimes and molar_hip_hbonds_frames_lifetimes against the dense numpy restatement of tests/lifetimes_ref.py.
Every result is an integer and every comparison is equality.  Sizes are small (R <= 300, F <= 260; 12 rows of up to 1100
frames where the intermittent kernel's unrolled loop begins) and sit on the edges of the 64-bit words, of the split of a lag
into a word shift and a bit shift, and of the launch shapes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lifetimes_ref as lr  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES, INVALID_ARGUMENT, TOO_LARGE, NO_SEARCH = 1, 50, 51, 52       # MOLAR_HIP_ERR_*
NAMES = ("inter", "cont", "run_hist", "events", "longest", "present")
SPLIT_LAGS = (0, 1, 62, 63, 64, 65, 127, 128, 129)


@pytest.fixture(scope="module")
def eng():
    from molar_amd import build
    from molar_amd.api import Engine
    build.build_library()
    return Engine(0)


def host(x):
    """a result as the numpy array the reference gives (int64 / int32 tensors hold the same bits)"""
    if x is None:
        return None
    if type(x).__module__.startswith("torch"):
        x = x.cpu().numpy()
        return x.view(np.uint64 if x.dtype == np.int64 else np.uint32)
    return x


def same(res, ref, names=NAMES, lags=None):
    for name in names:
        got, want = host(getattr(res, name)), ref[name]
        assert got is not None and got.shape == want.shape and got.dtype == want.dtype, name
        if lags is not None and name in ("inter", "cont"):
            got, want = got[:, list(lags)], want[:, list(lags)]
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5].tolist())
    assert np.array_equal(res.count, ref["count"])


def run_and_compare(eng, off, rows, R, **kw):
    ref = lr.reference(off, rows, R, **kw)
    kw = dict(kw)
    groups = kw.pop("groups", None)
    res = eng.lifetimes(off, rows, R, groups=groups, **kw)
    same(res, ref)
    return res, ref


@pytest.mark.parametrize("F", [1, 2, 63, 64, 65, 127, 128, 129, 257])
def test_word_edges(eng, F):
    h, off, rows = lr.case(24, F, seed=F, empty_frames=(3, 64))
    res, ref = run_and_compare(eng, off, rows, 24, max_lag=F - 1)
    assert int(ref["present"][1]) == F - sum(t < F for t in (3, 64)) and int(ref["present"][0]) == 0


def test_lags_across_the_word_and_bit_shift(eng):
    F, R = 260, 300
    h, off, rows = lr.case(R, F, seed=11, p_on=0.05, p_off=0.02)
    ref = lr.reference(off, rows, R, max_lag=F - 1)
    res = eng.lifetimes(off, rows, R, max_lag=F - 1)
    same(res, ref, ("inter", "cont"), lags=SPLIT_LAGS)
    assert all(int(ref["inter"][0, tau]) > 0 for tau in SPLIT_LAGS)       # the lags are compared on something
    same(res, ref)
    # a shorter curve is the head of the longer one, for every largest lag on the split
    for L in (62, 63, 64, 65, 127, 128):
        part = eng.lifetimes(off, rows, R, max_lag=L, want=("inter", "cont"))
        assert np.array_equal(part.inter, ref["inter"][:, :L + 1]) and np.array_equal(part.cont, ref["cont"][:, :L + 1])


@pytest.mark.parametrize("F", [384, 385, 448, 1100])
def test_rows_of_more_words_than_a_step(eng, F):
    # The intermittent kernel takes the words of a row four at a time for the four lag words of a wave together once a row has
    # seven words or more (F >= 385), and the rest word by word: 384 frames stay below that, 385 and 448 take one step with
    # and without words left over, 1100 frames (18 words) several steps and every count of left-over words.
    R = 12
    h, off, rows = lr.case(R, F, seed=F, p_on=0.1, p_off=0.1)
    run_and_compare(eng, off, rows, R, max_lag=F - 1)
    run_and_compare(eng, off, rows, R, max_lag=F - 1, origin_stride=5, gap=2, groups=(np.arange(R) % 2).astype(np.uint32), ngroups=2)


@pytest.mark.parametrize("stride", [1, 3, 7, 64, 65, 130, 135])
def test_origin_strides(eng, stride):
    F = 130
    h, off, rows = lr.case(40, F, seed=stride, p_on=0.1, p_off=0.05)
    run_and_compare(eng, off, rows, 40, max_lag=F - 1, origin_stride=stride)
    groups = (np.arange(40) % 3).astype(np.uint32)
    run_and_compare(eng, off, rows, 40, max_lag=70, origin_stride=stride, groups=groups, ngroups=3, gap=2)


@pytest.mark.parametrize("gap", [0, 1, 2, 63, 64, 200])
def test_gaps(eng, gap):
    F = 200
    h, off, rows = lr.case(30, F, seed=5, p_on=0.03, p_off=0.3)
    res, ref = run_and_compare(eng, off, rows, 30, max_lag=F - 1, gap=gap)
    # the hand-made rows hold what the gaps are about: bits 63 and 65 (one frame between them, across the word boundary), 62 and
    # 65, 0 and 64 (63 between), 0 and 65 (64 between), and 63 and 64, with nothing between the words
    hand = lr.hand_rows(F)
    for r, (a, b) in ((10, (63, 65)), (11, (62, 65)), (12, (0, 64)), (13, (0, 65))):
        assert h[r].sum() == 2 and h[r, a] and h[r, b]
        assert int(ref["present"][r]) == (b - a + 1 if b - a - 1 <= gap else 2)
    assert h[9, 63] and h[9, 64] and int(ref["longest"][9]) == 2 and np.array_equal(h[:len(hand)], hand)


@pytest.mark.parametrize("R", [1, 63, 64, 65, 255, 256, 257])
def test_row_counts(eng, R):
    h, off, rows = lr.case(R, 70, seed=R)
    run_and_compare(eng, off, rows, R, max_lag=69)
    run_and_compare(eng, off, rows, R, max_lag=69, origin_stride=4, gap=1, groups=(np.arange(R) % 5).astype(np.uint32), ngroups=5)


@pytest.mark.parametrize("E", [0, 1, 63, 64, 65])
def test_entry_counts(eng, E):
    R, F = 5, 70
    rng = np.random.default_rng(E)
    h = np.zeros(R * F, bool)
    h[rng.choice(R * F, E, replace=False)] = True
    off, rows = lr.sparse(h.reshape(R, F), rng)
    assert rows.shape[0] == E
    run_and_compare(eng, off, rows, R, max_lag=F - 1)
    run_and_compare(eng, off, rows, R, max_lag=F - 1, gap=3, origin_stride=2)


def test_full_and_empty_and_runs_of_64_and_65(eng):
    F = 257
    for fill in (False, True):
        hh = np.full((3, F), fill)
        off, rows = lr.sparse(hh)
        res, ref = run_and_compare(eng, off, rows, 3, max_lag=F - 1)
        assert int(res.run_hist[0, F]) == (3 if fill else 0) and int(res.run_hist.sum()) == (3 if fill else 0)
    h, off, rows = lr.case(24, F, seed=2)
    res, ref = run_and_compare(eng, off, rows, 24, max_lag=F - 1)
    assert int(ref["longest"][5]) == 64 and int(ref["longest"][6]) == 65 and int(ref["longest"][7]) == 64      # rows (1, 65), (3, 68), (0, 64)
    assert int(ref["longest"][4]) == 10 and h[4, 63] and h[4, 64]                                                # a run across a word boundary
    assert rows.shape[0] > int(h.sum())                                                                          # rows named more than once in a frame


def test_groups(eng):
    R, F = 65, 100
    h, off, rows = lr.case(R, F, seed=8)
    one, ref_one = run_and_compare(eng, off, rows, R, max_lag=F - 1)
    zeros = eng.lifetimes(off, rows, R, groups=np.zeros(R, np.uint32), ngroups=1, max_lag=F - 1)
    for name in NAMES:
        assert np.array_equal(getattr(one, name), getattr(zeros, name)), name
    # several groups, group 2 of 4 without a row
    labels = np.random.default_rng(1).choice([0, 1, 3], R).astype(np.uint32)
    res, ref = run_and_compare(eng, off, rows, R, max_lag=F - 1, groups=labels, ngroups=4, gap=1)
    assert not res.inter[2].any() and not res.cont[2].any() and not res.run_hist[2].any() and res.inter[3].any()
    assert np.array_equal(res.inter.sum(axis=0), lr.reference(off, rows, R, max_lag=F - 1, gap=1)["inter"][0])
    # every row its own group
    res, ref = run_and_compare(eng, off, rows, R, max_lag=F - 1, groups=np.arange(R, dtype=np.uint32)[::-1].copy(), ngroups=R, origin_stride=3)
    assert np.array_equal(res.run_hist.sum(axis=1).astype(np.uint32), res.events[::-1])


def test_each_output_alone_and_twice_the_same_bytes(eng):
    R, F = 100, 140
    h, off, rows = lr.case(R, F, seed=21)
    kw = dict(max_lag=100, origin_stride=3, gap=1, groups=(np.arange(R) % 4).astype(np.uint32), ngroups=4)
    ref = lr.reference(off, rows, R, **kw)
    allof = eng.lifetimes(off, rows, R, **kw)
    same(allof, ref)
    again = eng.lifetimes(off, rows, R, **kw)
    for name in NAMES:
        assert getattr(allof, name).tobytes() == getattr(again, name).tobytes(), name
    for name in NAMES:
        alone = eng.lifetimes(off, rows, R, want=(name,), **kw)
        same(alone, ref, (name,))
        assert all(getattr(alone, other) is None for other in NAMES if other != name)
    # stride 1 takes another route to the continuous curve: alone (its own histogram) and beside run_hist (the caller's)
    kw["origin_stride"] = 1
    ref = lr.reference(off, rows, R, **kw)
    same(eng.lifetimes(off, rows, R, want=("cont",), **kw), ref, ("cont",))
    same(eng.lifetimes(off, rows, R, want=("cont", "run_hist"), **kw), ref, ("cont", "run_hist"))


def test_device_memory(eng):
    import torch
    R, F = 70, 129
    h, off, rows = lr.case(R, F, seed=4)
    labels = (np.arange(R) % 3).astype(np.uint32)
    kw = dict(max_lag=F - 1, origin_stride=2, gap=2)
    ref = lr.reference(off, rows, R, groups=labels, ngroups=3, **kw)
    off_t = torch.from_numpy(off.astype(np.int64)).cuda()
    rows_t = torch.from_numpy(rows.astype(np.int32)).cuda()
    labels_t = torch.from_numpy(labels.astype(np.int32)).cuda()
    res = eng.lifetimes(off_t, rows_t, R, groups=labels_t, ngroups=3, **kw)
    assert all(getattr(res, name).is_cuda for name in NAMES)
    same(res, ref)
    # device rows with host offsets and host labels: outputs follow the rows
    res = eng.lifetimes(off, rows_t, R, groups=labels, ngroups=3, **kw)
    assert res.inter.is_cuda
    same(res, ref)


def call(eng, off, rows, F, R, groups=None, G=0, L=0, stride=1, gap=0, outs=None):
    outs = outs or [np.full(32, 77, np.uint64) for _ in range(3)] + [np.full(32, 77, np.uint32) for _ in range(3)]
    addr = lambda a: None if a is None else (a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)
    rc = eng.lib.molar_hip_lifetimes(eng.ctx, addr(off), addr(rows), F, R, addr(groups), G, L, stride, gap, *[o.ctypes.data for o in outs])
    return rc, all((o == 77).all() for o in outs)


def test_errors_write_nothing(eng):
    import torch
    off = np.array([0, 2, 3, 3, 5], np.uint64)
    rows = np.array([0, 1, 1, 0, 2], np.uint32)
    ok = lambda **kw: call(eng, kw.pop("off", off), kw.pop("rows", rows), kw.pop("F", 4), kw.pop("R", 3), **kw)
    assert ok(L=3)[0] == 0
    assert ok(L=4) == (INVALID_ARGUMENT, True)                                        # max_lag >= nframes
    assert ok(stride=0) == (INVALID_ARGUMENT, True)
    assert ok(off=np.array([1, 2, 3, 3, 5], np.uint64)) == (INVALID_ARGUMENT, True)   # offsets that do not start at 0
    assert ok(off=np.array([0, 3, 2, 3, 5], np.uint64)) == (INVALID_ARGUMENT, True)   # ... that decrease
    assert ok(R=2) == (INVALID_ARGUMENT, True)                                        # a row == nrows, host memory
    assert ok(groups=np.array([0, 1, 2], np.uint32), G=2) == (INVALID_ARGUMENT, True)
    assert ok(groups=np.array([0, 1, 2], np.uint32), G=0) == (INVALID_ARGUMENT, True)
    assert ok(R=0) == (SIZES, True) and ok(F=0, off=np.array([0], np.uint64)) == (SIZES, True)
    # 2^32 entries or more are refused before a row is read; one entry fewer passes that check (and is refused for its null rows)
    assert ok(off=np.array([0, 0, 0, 0, 2 ** 32], np.uint64), L=3) == (TOO_LARGE, True)
    assert ok(off=np.array([0, 0, 0, 0, 2 ** 33 + 5], np.uint64), L=3) == (TOO_LARGE, True)
    assert call(eng, np.array([0, 0, 0, 0, 2 ** 32 - 1], np.uint64), None, 4, 3, L=3) == (INVALID_ARGUMENT, True)
    # the same from device memory: judged on the device, a normal return
    rows_t = torch.from_numpy(rows.astype(np.int32)).cuda()
    off_t = torch.from_numpy(off.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    assert call(eng, off_t, rows_t, 4, 2, L=3) == (INVALID_ARGUMENT, True)            # a row == nrows
    assert call(eng, off_t, rows_t, 4, 3, L=3)[0] == 0
    bad = torch.tensor([0, 1, 3], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert call(eng, off, rows_t, 4, 3, groups=bad, G=3, L=3) == (INVALID_ARGUMENT, True)
    assert call(eng, torch.tensor([0, 3, 2, 3, 5], dtype=torch.int64, device="cuda"), rows_t, 4, 3, L=3) == (INVALID_ARGUMENT, True)
    from molar_amd._lib import MolarHipError
    with pytest.raises(MolarHipError) as err:
        eng.lifetimes(off, rows_t, 2)
    assert err.value.code == INVALID_ARGUMENT and "nrows" in str(err.value)


def test_chain_from_hbonds_frames(eng):
    import hbonds_ref as hr
    from molar_amd._lib import MolarHipError
    from molar_amd.api import Engine
    fresh = Engine(0)
    outs = [np.zeros(4, np.uint64)]
    assert fresh.lib.molar_hip_hbonds_frames_lifetimes(fresh.ctx, None, 1, 0, 1, 0, outs[0].ctypes.data, None, None, None, None, None) == NO_SEARCH
    fresh.close()
    b = hr.frames_case("block17")
    blk = eng.hbonds_frames(b["frames"], b["donors"], (b["hoff"], b["hidx"]), b["acceptors"], box=b["boxes"], pbc=7)
    R, F = blk.table.shape[0], blk.frame_offsets.shape[0] - 1
    assert F == 17 and R > 100
    labels = (blk.table[:, 0] % 3).astype(np.uint32)                # by the donor
    for kw in (dict(), dict(gap=1, origin_stride=2, max_lag=9, groups=labels, ngroups=3)):
        ref = lr.reference(blk.frame_offsets, blk.bond_of_entry, R, **kw)
        chained = blk.lifetimes(**kw)
        same(chained, ref)
        direct = eng.lifetimes(blk.frame_offsets, blk.bond_of_entry, R, **kw)
        for name in NAMES:
            assert np.array_equal(getattr(chained, name), getattr(direct, name)), name
    assert np.array_equal(blk.lifetimes(want="present").present, blk.occupancy)
    # another block of another size replaces this one: the first block's call is refused and nothing is written under its name,
    # the second block's call is its own
    small = eng.hbonds_frames(b["frames"][:5], b["donors"], (b["hoff"], b["hidx"]), b["acceptors"], box=b["boxes"][:5], pbc=7)
    assert small.table.shape[0] != R and small.frame_offsets.shape[0] == 6
    with pytest.raises(MolarHipError) as err:
        blk.lifetimes()
    assert err.value.code == NO_SEARCH
    same(small.lifetimes(), lr.reference(small.frame_offsets, small.bond_of_entry, small.table.shape[0]))
    again = eng.hbonds_frames(b["frames"], b["donors"], (b["hoff"], b["hidx"]), b["acceptors"], box=b["boxes"], pbc=7)
    with pytest.raises(MolarHipError):
        small.lifetimes()                       # a larger block in its place
    with pytest.raises(MolarHipError):
        blk.lifetimes()                         # the same frames again are another block all the same
    same(again.lifetimes(), lr.reference(blk.frame_offsets, blk.bond_of_entry, R))
    blk = again
    # a single-frame call replaces the block: the chained call is refused
    one = hr.frame_of(b, 0)
    eng.hbonds(one["xyz"], one["donors"], (one["hoff"], one["hidx"]), one["acceptors"], box=one["box"], pbc=one["pbc"])
    with pytest.raises(MolarHipError) as err:
        blk.lifetimes()
    assert err.value.code == NO_SEARCH
