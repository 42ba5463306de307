"""Van Hove on the GPU (molar_hip_vanhove / _f64: the check, the sort by label, the gather, the pair kernel with its on-chip and
its in-memory counts) against the longdouble numpy reference of tests/vanhove_ref.py.  Every output is an integer and is compared
for EQUALITY: the reference asserts on its own inputs that no displacement is within the derived bound of a bin edge, so no
case is left out.  Both entries see the same numbers (f32 inputs, cast to f64 for the f64 entry), from host and from device
memory.  The shapes stand either side of every size molar_hip_vanhove_plan reports (vanhove_ref.build_cases)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vanhove_ref as vr  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ("hist", "outside", "norigins", "nvalid", "bad")


@pytest.fixture(autouse=True)
def plain_plan(monkeypatch):
    monkeypatch.delenv("MOLAR_HIP_VANHOVE_ONCHIP", raising=False)
    monkeypatch.delenv("MOLAR_HIP_VANHOVE_COMBINE", raising=False)


@pytest.fixture(scope="module")
def eng():
    from molar_amd import api
    return api.Engine()


@pytest.fixture(scope="module")
def m64(eng):
    from molar_amd import api
    return api.MeasureF64(eng)


def traj_as(name, real):
    """The case's trajectory in `real`, inside its wider block when the case pads its frames."""
    c = vr.cases()[name]
    x = vr.case_traj(name)
    if real == np.float32:
        return x
    return np.asarray(x.base, real)[:, :c.natoms] if c.pad else np.asarray(x, real)


def call(entry, name, real, device=False, **over):
    c = vr.cases()[name]
    x = traj_as(name, real)
    kw = vr.case_kwargs(c)
    lags = np.array(c.lags, np.uint64)
    if device:
        import torch
        wide = torch.as_tensor(np.array(x.base if c.pad else x)).cuda()
        x = wide[:, :c.natoms] if c.pad else wide
        kw["idx"] = None if kw["idx"] is None else torch.as_tensor(kw["idx"].astype(np.int64)).cuda()
        kw["labels"] = None if kw["labels"] is None else torch.as_tensor(kw["labels"].astype(np.int32)).cuda()
        lags = torch.as_tensor(lags.astype(np.int64)).cuda()
    kw.update(over)
    return entry.van_hove(x, lags, (c.lo, c.hi), c.nbins, ngroups=c.G if c.labels is not None else None, **kw)


def host(a):
    if a is None:
        return None
    if type(a).__module__.startswith("torch"):
        a = a.cpu().numpy()
        return a.astype(np.uint32) if a.dtype == np.int32 else a.astype(np.uint64)
    return a


def check(eng, got, ref, what):
    eng.synchronize()
    for nm in NAMES:
        g = host(getattr(got, nm))
        r = getattr(ref, nm)
        assert g.dtype == r.dtype and g.shape == r.shape, (what, nm)
        assert np.array_equal(g, r), (what, nm, int((g != r).sum()), "entries differ")
    h, o, nv, no = host(got.hist), host(got.outside), host(got.nvalid), host(got.norigins)
    assert (h.sum(axis=2) + o == nv[:, None] * no[None, :]).all(), (what, "the count identity")


@pytest.mark.parametrize("name", sorted(vr.cases()))
def test_counts_equal_the_reference(eng, m64, name):
    ref = vr.case_ref(name)
    c = vr.cases()[name]
    check(eng, call(eng, name, np.float32), ref, (name, "f32 host"))
    check(eng, call(m64, name, np.float64), ref, (name, "f64 host"))
    got = call(eng, name, np.float32, device=True)
    assert all(type(getattr(got, nm)).__module__.startswith("torch") and getattr(got, nm).is_cuda for nm in NAMES), "device in, device out"
    check(eng, got, ref, (name, "f32 device"))
    check(eng, call(m64, name, np.float64, device=True), ref, (name, "f64 device"))
    assert np.array_equal(got.edges, c.lo + (c.hi - c.lo) * np.arange(c.nbins + 1) / c.nbins)


def test_both_routes_of_the_counts_agree(eng, monkeypatch):
    """The on-chip histogram and the atomics straight to memory on one input, at the limit and in a tile of many lags; and the
    combining of equal cells of a wave switched on."""
    from molar_amd import api
    PASS, PW, LT, CELLS = vr.plan_sizes(16)
    for name in (f"bins_{CELLS}", f"bins_{CELLS - 1}", f"lags_{LT + 1}", "groups", "stationary", "signed_1"):
        c = vr.cases()[name]
        assert api.vanhove_plan(c.F, c.natoms, c.G, len(c.lags), c.nbins, 3).on_chip == 1
        ref = vr.case_ref(name)
        monkeypatch.setenv("MOLAR_HIP_VANHOVE_ONCHIP", "0")
        assert api.vanhove_plan(c.F, c.natoms, c.G, len(c.lags), c.nbins, 3).on_chip == 0
        check(eng, call(eng, name, np.float32), ref, (name, "in memory"))
        monkeypatch.delenv("MOLAR_HIP_VANHOVE_ONCHIP")
        monkeypatch.setenv("MOLAR_HIP_VANHOVE_COMBINE", "1")
        check(eng, call(eng, name, np.float32), ref, (name, "combined"))
        monkeypatch.delenv("MOLAR_HIP_VANHOVE_COMBINE")
    assert api.vanhove_plan(60, 3, 1, 1, CELLS + 1, 3).on_chip == 0, "one bin more goes to memory by itself"


def test_bad_particles_leave_the_others_alone(eng):
    name = "bad_particles"
    c = vr.cases()[name]
    got = call(eng, name, np.float32)
    assert got.bad.tolist() == [0, 1, 0, 0, 0, 1, 0, 0, 0] and got.nvalid.tolist() == [3, 2, 2]
    keep = np.array([0, 2, 3, 4, 6, 7, 8], np.uint64)
    without = eng.van_hove(vr.case_traj(name), np.array(c.lags, np.uint64), (c.lo, c.hi), c.nbins, idx=keep, labels=np.array(c.labels, np.uint32)[keep.astype(np.int64)],
                           ngroups=c.G)
    assert without.bad.sum() == 0
    assert np.array_equal(got.hist, without.hist) and np.array_equal(got.outside, without.outside) and np.array_equal(got.nvalid, without.nvalid)


def test_the_same_call_gives_the_same_bytes_and_want_and_out(eng):
    name = "groups"
    c = vr.cases()[name]
    a, b = call(eng, name, np.float32), call(eng, name, np.float32)
    assert all(getattr(a, nm).tobytes() == getattr(b, nm).tobytes() for nm in NAMES)
    part = call(eng, name, np.float32, want=("outside", "nvalid"))
    assert part.hist is None and part.norigins is None and part.bad is None
    assert np.array_equal(part.outside, a.outside) and np.array_equal(part.nvalid, a.nvalid)
    only_hist = call(eng, name, np.float32, want=("hist",))
    assert np.array_equal(only_hist.hist, a.hist) and only_hist.outside is None
    out = (np.full(a.hist.shape, 9, np.uint64), None, None, None, np.full(a.bad.shape, 9, np.uint32))
    given = call(eng, name, np.float32, out=out)
    assert given.hist is out[0] and given.bad is out[4] and np.array_equal(out[0], a.hist) and np.array_equal(out[4], a.bad)


def test_device_arguments_are_judged_before_anything_is_written(eng):
    import torch
    from molar_amd import api
    x = torch.zeros((6, 5, 3), dtype=torch.float32, device="cuda")
    good = dict(lags=torch.tensor([0, 2], device="cuda"), idx=torch.tensor([0, 1, 4], device="cuda"), labels=torch.tensor([0, 1, 1], dtype=torch.int32, device="cuda"))
    bad = dict(lags=(torch.tensor([0, 6], device="cuda"), torch.tensor([2, 2], device="cuda")), idx=(torch.tensor([0, 1, 5], device="cuda"),),
               labels=(torch.tensor([0, 2, 1], dtype=torch.int32, device="cuda"),))
    for key, values in bad.items():
        for v in values:
            kw = dict(good)
            kw[key] = v
            out = (torch.full((2, 2, 4), 9, dtype=torch.int64, device="cuda"), torch.full((2, 2), 9, dtype=torch.int64, device="cuda"),
                   torch.full((2,), 9, dtype=torch.int64, device="cuda"), torch.full((2,), 9, dtype=torch.int64, device="cuda"),
                   torch.full((3,), 9, dtype=torch.int32, device="cuda"))
            with pytest.raises(api.MolarHipError) as e:
                eng.van_hove(x, kw["lags"], (0.0, 1.0), 4, idx=kw["idx"], labels=kw["labels"], ngroups=2, out=out)
            assert e.value.code == vr.error_codes(open(os.path.join(os.path.dirname(__file__), "..", "include", "molar_hip.h")).read())["INVALID_ARGUMENT"]
            eng.synchronize()
            assert all(bool((o == 9).all()) for o in out), (key, "an output was touched after an error")
    ok = eng.van_hove(x, good["lags"], (0.0, 1.0), 4, idx=good["idx"], labels=good["labels"], ngroups=2)
    eng.synchronize()
    assert ok.hist[:, :, 0].cpu().tolist() == [[6, 4], [12, 8]]


def wrapped_walks(seed, F, natoms, box, drift):
    rng = np.random.default_rng(seed)
    x = vr.random_walk(seed, F, natoms, step=0.08) + drift * np.arange(F)[:, None, None]
    boxes = np.zeros((F, 9))
    scale = 1.0 + 0.01 * rng.uniform(-1, 1, F)
    for d in range(3):
        boxes[:, 4 * d] = box[d] * scale
    return x, boxes


@pytest.mark.parametrize("per_frame", (False, True))
def test_frames_chain_equals_the_reference_on_the_engines_own_disp(eng, m64, per_frame):
    F, natoms = 60, 24
    x, boxes = wrapped_walks(11, F, natoms, (2.0, 2.2, 1.9), 0.01)
    if not per_frame:
        boxes = boxes[:1].repeat(F, axis=0)
    wrapped = (x - np.floor(x / boxes[:, None, [0, 4, 8]]) * boxes[:, None, [0, 4, 8]]).astype(np.float32)
    bx = boxes.astype(np.float32) if per_frame else boxes[0].astype(np.float32)
    idx = np.arange(2, 22, dtype=np.uint64)
    groups = np.array([0, 3, 6, 10, 11, 15, 20], np.uint64)                  # six particles of 3, 3, 4, 1, 4, 5 atoms
    mass = np.random.default_rng(2).uniform(1.0, 16.0, natoms).astype(np.float32)
    ref_idx = np.array([0, 1, 22, 23], np.uint64)
    labels = np.array([1, 0, 1, 1, 0, 1], np.uint32)
    lags = np.array([0, 1, 5, 30, 59], np.uint64)
    rng_, nbins = (0.013, 0.9), 12
    for entry, real in ((eng, np.float32), (m64, np.float64)):
        fr, b = np.asarray(wrapped, real), np.asarray(bx, real)
        disp = entry.msd(fr, idx=idx, mass=np.asarray(mass, real), boxes=b, groups=groups, ref_idx=ref_idx, disp=True, msd=False, m4=False).disp
        assert disp.shape == (F, 6, 3)
        ref = vr.reference(disp, lags, rng_[0], rng_[1], nbins, labels=labels, G=2)
        got = entry.van_hove_frames(fr, lags, rng_, nbins, idx=idx, boxes=b, mass=np.asarray(mass, real), groups=groups, ref_idx=ref_idx, labels=labels, ngroups=2)
        check(eng, got, ref, ("frames", real, per_frame))
        assert ref.hist.sum() > 0 and ref.nvalid.tolist() == [2, 4]
        import torch
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()      # noqa: E731
        dev = entry.van_hove_frames(t(fr), t(lags.astype(np.int64)), rng_, nbins, idx=t(idx.astype(np.int64)), boxes=t(b), mass=t(np.asarray(mass, real)),
                                    groups=t(groups.astype(np.int64)), ref_idx=t(ref_idx.astype(np.int64)), labels=t(labels.astype(np.int32)), ngroups=2)
        assert all(getattr(dev, nm).is_cuda for nm in NAMES), "torch in, device tensors out"
        check(eng, dev, ref, ("frames on the device", real, per_frame))
