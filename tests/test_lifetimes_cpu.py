"""Lifetime correlations without a GPU: the numpy reference of tests/lifetimes_ref.py against a literal loop over single frames,
the identities that tie the curves to the run-length histogram, lifetime_curves, and the plan entry's numbers."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lifetimes_ref as lr  # noqa: E402

NAMES = ("inter", "cont", "run_hist", "events", "longest", "present")


@pytest.mark.parametrize("R,F,stride,gap,grouped", [(1, 1, 1, 0, False), (3, 7, 1, 0, False), (6, 20, 1, 1, True), (5, 19, 3, 2, True),
                                                    (4, 12, 5, 0, False), (6, 16, 20, 16, True), (2, 2, 1, 1, False), (6, 20, 7, 3, True)])
def test_reference_is_the_literal_definition(R, F, stride, gap, grouped):
    rng = np.random.default_rng(100 * R + F)
    h = lr.markov(R, F, 0.3, 0.3, seed=R + F)
    h[0] = False
    if R > 1:
        h[1] = True
    off, rows = lr.sparse(h, rng, duplicates=1)
    groups, G = (rng.integers(0, 3, R).astype(np.uint32), 4) if grouped else (None, None)
    want = lr.literal(off, rows, R, groups, G, F - 1, stride, gap)
    got = lr.reference(off, rows, R, groups, G, F - 1, stride, gap)
    for name in NAMES:
        assert np.array_equal(got[name], want[name]), name
    t = np.arange(0, F, stride)
    assert [int(c) for c in got["count"]] == [int((t + tau <= F - 1).sum()) for tau in range(F)]


@pytest.mark.parametrize("gap", [0, 2])
def test_curves_follow_from_the_run_histogram_at_stride_one(gap):
    h, off, rows = lr.case(40, 150, seed=3)
    ref = lr.reference(off, rows, 40, max_lag=149, gap=gap)
    hist = ref["run_hist"][0].astype(np.int64)
    ell = np.arange(151)
    for tau in range(150):
        assert int(ref["cont"][0, tau]) == int((hist * np.maximum(0, ell - tau)).sum())
    assert int(ref["inter"][0, 0]) == int(ref["cont"][0, 0]) == int((ell * hist).sum()) == int(ref["present"].sum())
    assert hist[0] == 0 and int(hist.sum()) == int(ref["events"].sum())


def test_lifetime_curves_on_two_rows():
    from molar_amd.api import Lifetimes, lifetime_count, lifetime_curves
    # row 0: present in frames 0, 1, 2 of 4; row 1: present in frames 0 and 2
    off, rows = lr.sparse(np.array([[1, 1, 1, 0], [1, 0, 1, 0]], bool))
    ref = lr.reference(off, rows, 2)
    assert ref["inter"].tolist() == [[5, 2, 2, 0]] and ref["cont"].tolist() == [[5, 2, 1, 0]]
    count = lifetime_count(4, 3, 1)
    assert count.tolist() == [4, 3, 2, 1] and np.array_equal(count, ref["count"])
    res = Lifetimes(ref["inter"], ref["cont"], None, None, None, None, count, 4, 1)
    c = lifetime_curves(res, dt=2.0)
    # (x / count) / (x[0] / count[0]) in float64
    ci = np.array([[1.0, (2 / 3) / (5 / 4), (2 / 2) / (5 / 4), 0.0]])
    cc = np.array([[1.0, (2 / 3) / (5 / 4), (1 / 2) / (5 / 4), 0.0]])
    assert np.array_equal(c.tau, [0.0, 2.0, 4.0, 6.0])
    assert np.allclose(c.c_inter, ci, rtol=1e-15, atol=0) and np.allclose(c.c_cont, cc, rtol=1e-15, atol=0)
    trap = lambda y: 2.0 * (y[0] / 2 + y[1] + y[2] + y[3] / 2)
    assert np.allclose(c.tau_inter, [trap(ci[0])], rtol=1e-15) and np.allclose(c.tau_cont, [trap(cc[0])], rtol=1e-15)
    # an empty group: 0 / 0 is NaN, not an error
    empty = Lifetimes(np.zeros((1, 4), np.uint64), None, None, None, None, None, count, 4, 1)
    ce = lifetime_curves(empty)
    assert np.isnan(ce.c_inter).all() and ce.c_cont is None and ce.tau_cont is None


def test_plan_numbers():
    from molar_amd.api import lifetimes_plan
    # regions one after the other, each rounded up to 256 bytes: 16 bytes of flags, rows x (words + 1) x 8 of bits, words x 8 of
    # origin masks, and with want_cont groups x (frames + 1) x 8 of histogram
    assert lifetimes_plan(1, 1, 1, want_cont=False) == (256 + 256 + 256, 1)
    assert lifetimes_plan(64, 3, 1, want_cont=False) == (256 + 256 + 256, 1)
    assert lifetimes_plan(65, 100, 1, want_cont=False) == (256 + 2560 + 256, 2)
    assert lifetimes_plan(65, 100, 1, want_cont=True) == (256 + 2560 + 256 + 768, 2)
    assert lifetimes_plan(4096, 200000, 3, want_cont=True) == (256 + 200000 * 65 * 8 + 512 + 98304 + 256, 64)
    assert lifetimes_plan(0, 10) == (0, 0) and lifetimes_plan(10, 0)[0] == 0
    # it grows with rows x ceil(frames / 64)
    prev = 0
    for R, F in ((100, 64), (100, 65), (1000, 65), (1000, 4096), (100000, 4096), (100000, 65536)):
        ws, words = lifetimes_plan(F, R, 1, want_cont=False)
        assert words == (F + 63) // 64 and ws > prev and ws >= R * (words + 1) * 8
        prev = ws
