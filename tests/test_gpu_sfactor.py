"""Static structure factors on the GPU (molar_hip_sfactor / _f64: the partition by label, the gram kernel on the f64 matrix
cores with operands formed on chip, the fold of the K splits, the products and the shells) against the longdouble numpy
reference of tests/sfactor_ref.py, output by output within the bounds derived there; integers and NaN positions for
equality.  Both entries see the same numbers (f32 inputs, cast to f64 for the f64 entry), so one reference serves both, and
every reference is computed once.  atom_chunk is overridden to 64 and frame_block to 2, so that the small shapes stand
either side of every size molar_hip_sfactor_plan reports.  The largest used fraction of each bound is printed by the last
test."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sfactor_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu
ALL = ("rho", "frame_ok", "rho_mean", "sab", "shell", "shell_count")
FRACTIONS = {}


@pytest.fixture(autouse=True)
def small_plan(monkeypatch):
    monkeypatch.setenv("MOLAR_HIP_SFACTOR_ATOM_CHUNK", str(sr.ATOM_CHUNK))
    monkeypatch.setenv("MOLAR_HIP_SFACTOR_FRAME_BLOCK", str(sr.FRAME_BLOCK))


@pytest.fixture(scope="module")
def eng():
    from molar_amd import api
    return api.Engine()


@pytest.fixture(scope="module")
def m64(eng):
    from molar_amd import api
    return api.MeasureF64(eng)


def grid_of(case):
    from molar_amd import api
    return api.sfactor_grid(case.hmax, case.qmin, case.dq, case.nshells)


def call(entry, case, real, want=ALL, inputs=None, out=None):
    frames, boxes, idx, weight, labels = sr.case_inputs(case) if inputs is None else inputs
    return entry.structure_factor(np.asarray(frames, real), grid_of(case), idx=idx, weight=None if weight is None else np.asarray(weight, real),
                                  labels=labels, ngroups=case.G if labels is not None else None, boxes=np.asarray(boxes, real), want=want, out=out)


def check(got, ref, what):
    """Every output given within its bound, integers equal; the fractions used are kept for the last test."""
    for name, bound in (("rho", ref.b_rho), ("rho_mean", ref.b_mean), ("sab", ref.b_sab), ("shell", ref.b_shell)):
        g = getattr(got, name)
        if g is None:
            continue
        frac = sr.fraction(g, getattr(ref, name), bound)
        print(f"{what}: {name} uses {frac:.3f} of its bound")
        FRACTIONS[name] = max(FRACTIONS.get(name, 0.0), frac)
        assert frac <= 1.0, (what, name, frac)
    if got.frame_ok is not None:
        assert np.array_equal(got.frame_ok, ref.frame_ok), what
    if got.shell_count is not None:
        assert np.array_equal(got.shell_count, ref.shell_count), what


def both(eng, m64, case, inputs=None, ref=None):
    out = []
    for entry, real, eps in ((eng, np.float32, sr.EPS32), (m64, np.float64, sr.EPS64)):
        if inputs is None:
            r = sr.case_reference(case, eps)
        else:
            r = sr.reference(*inputs, case.G, case.hmax, case.qmin, case.dq, case.nshells, sr.ATOM_CHUNK, eps) if ref is None else ref[eps]
        got = call(entry, case, real, inputs=inputs)
        check(got, r, f"{case.name} {np.dtype(real).name}")
        out.append(got)
    return out


def same_bits(a, b, names=ALL):
    for n in names:
        x, y = getattr(a, n), getattr(b, n)
        if x is None or y is None:
            continue
        x, y = np.asarray(x), np.asarray(y)
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), n


def test_the_shapes_cross_every_size_of_the_plan():
    from molar_amd import api
    _, layout, rb, cb, ac, ks, fb = api.sfactor_plan(3, 131, api.sfactor_grid((2, 2, 2)))
    assert (rb, cb, ac, fb) == (sr.ROW_BLOCK, sr.COL_BLOCK, sr.ATOM_CHUNK, sr.FRAME_BLOCK) and ks == 3
    assert sorted(c.natoms for c in sr.ATOM_CASES) == [1, 3, 4, 5, ac - 1, ac, ac + 1, 2 * ac + 3]
    shapes = {(lay, R, Cn) for lay, _, R, Cn in (sr.layout_of(c.hmax) for c in sr.SHAPE_CASES)}
    for lay, rows in ((0, (1, 15, 16, 17, rb - 1, rb + 1)), (1, (15, 17, rb - 1, rb + 1))):
        assert set(rows) <= {R for l, R, _ in shapes if l == lay}, (lay, shapes)
    assert {1, 15, 16, 17, cb + 1} <= {Cn for _, _, Cn in shapes}
    assert sr.layout_of((20, 0, 0))[0] == 0 and api.sfactor_plan(1, 9, api.sfactor_grid((20, 0, 0)))[1] == 0
    assert sorted(c.F for c in sr.FRAME_CASES) == [1, fb, fb + 1]
    for c in sr.ALL_CASES:
        Q = (c.hmax[0] + 1) * (2 * c.hmax[1] + 1) * (2 * c.hmax[2] + 1)
        assert c.natoms * Q * c.F <= 2 * 10 ** 7


@pytest.mark.parametrize("case", sr.ALL_CASES, ids=lambda c: c.name)
def test_every_output_within_its_bound(eng, m64, case):
    both(eng, m64, case)


def test_shells_fill_and_stay_empty():
    for case in sr.FRAME_CASES[-1:] + sr.GROUP_CASES:
        ref = sr.case_reference(case, sr.EPS32)
        assert (ref.shell_count > 0).any(), case.name
        if case.nshells > 1:
            assert (ref.shell_count == 0).any() and np.all(np.isnan(ref.shell[:, ref.shell_count == 0])), case.name


def test_frame_stride_and_rho_row_stride(eng, m64):
    case = sr.GROUP_CASES[0]
    frames, boxes, idx, weight, labels = sr.case_inputs(case)
    Q = 4 * 5 * 5
    for entry, real in ((eng, np.float32), (m64, np.float64)):
        plain = call(entry, case, real)
        wide = np.full((case.F, case.natoms + 3, 3), np.nan, real)
        wide[:, :case.natoms] = frames
        rho = np.full((case.F, case.G, Q + 2, 2), -7.0, real)
        got = call(entry, case, real, inputs=(wide[:, :case.natoms], boxes, idx, weight, labels), out=(rho[:, :, :Q], None, None, None, None, None))
        same_bits(plain, got)
        assert np.all(rho[:, :, Q:] == -7.0), "the rest of a row is not touched"


def test_each_output_alone_equals_all_together(eng):
    case = sr.GROUP_CASES[1]
    full = call(eng, case, np.float32)
    for name in ALL:
        alone = call(eng, case, np.float32, want=(name,))
        assert all((getattr(alone, n) is None) == (n != name) for n in ALL)
        same_bits(full, alone, (name,))


def test_device_memory_on_both_sides(eng, m64):
    import torch
    case = sr.GROUP_CASES[0]
    frames, boxes, idx, weight, labels = sr.case_inputs(case)
    for entry, real in ((eng, np.float32), (m64, np.float64)):
        host = call(entry, case, real)
        dev = lambda a, dt=None: None if a is None else torch.as_tensor(np.asarray(a, dt), device="cuda")
        g = entry.structure_factor(dev(frames, real), grid_of(case), idx=dev(idx, np.int64), weight=dev(weight, real), labels=dev(labels, np.int32),
                                   ngroups=case.G, boxes=dev(boxes, real), want=ALL)
        # device frames and results with host idx, weight and labels
        mixed = entry.structure_factor(dev(frames, real), grid_of(case), idx=idx, weight=None if weight is None else np.asarray(weight, real), labels=labels,
                                       ngroups=case.G, boxes=np.asarray(boxes, real), want=ALL)
        eng.synchronize()
        for got in (g, mixed):
            assert all(r.is_cuda for r in got[:6])
            as_host = type(host)(*(r.cpu().numpy() for r in got[:6]), got.grid)
            assert as_host.frame_ok.dtype == np.int32 and as_host.shell_count.dtype == np.int64
            same_bits(host, as_host, ("rho", "rho_mean", "sab", "shell"))
            assert np.array_equal(as_host.frame_ok, host.frame_ok) and np.array_equal(as_host.shell_count, host.shell_count.astype(np.int64))


def test_a_frame_that_is_not_finite(eng, m64):
    for case in (sr.GROUP_CASES[1], sr.GROUP_CASES[0]):             # per-frame boxes, one box
        frames, boxes, idx, weight, labels = sr.case_inputs(case)
        sel = np.arange(case.natoms) if idx is None else idx.astype(np.int64)
        bad = frames.copy()
        bad[1, sel[3], 1] = np.inf
        out = both(eng, m64, case, inputs=(bad, boxes, idx, weight, labels))
        keep = [0, 2]
        bk = np.asarray(boxes)[keep] if np.asarray(boxes).ndim == 2 else boxes
        for entry, real, got in ((eng, np.float32, out[0]), (m64, np.float64, out[1])):
            assert list(got.frame_ok) == [1, 0, 1] and np.all(np.isnan(got.rho[1]))
            without = call(entry, case, real, inputs=(np.ascontiguousarray(frames[keep]), bk, idx, weight, labels))
            assert np.array_equal(got.rho[keep], without.rho), "the other frames, bit for bit"
            same_bits(got, without, ("rho_mean", "sab", "shell", "shell_count"))
        # an atom outside the selection may hold anything
        if idx is not None:
            other = np.setdiff1d(np.arange(case.natoms), sel)[0]
            odd = frames.copy()
            odd[:, other] = np.nan
            same_bits(call(eng, case, np.float32), call(eng, case, np.float32, inputs=(odd, boxes, idx, weight, labels)))
        none = frames.copy()
        none[:, sel[0], 0] = np.nan
        for got in both(eng, m64, case, inputs=(none, boxes, idx, weight, labels)):
            assert not got.frame_ok.any() and not got.shell_count.any()
            for name in ("rho", "rho_mean", "sab", "shell"):
                assert np.all(np.isnan(getattr(got, name))), name


def test_the_same_call_gives_the_same_bits(eng, m64):
    for case in (sr.ATOM_CASES[-1], sr.GROUP_CASES[0], sr.GROUP_CASES[2]):
        for entry, real in ((eng, np.float32), (m64, np.float64)):
            same_bits(call(entry, case, real), call(entry, case, real))


def test_frame_block_does_not_change_the_bits(eng, monkeypatch):
    case = sr.FRAME_CASES[-1]
    a = call(eng, case, np.float32)
    monkeypatch.setenv("MOLAR_HIP_SFACTOR_FRAME_BLOCK", "1")
    b = call(eng, case, np.float32)
    monkeypatch.delenv("MOLAR_HIP_SFACTOR_FRAME_BLOCK")
    same_bits(a, b)
    same_bits(a, call(eng, case, np.float32))


def test_cubic_lattice_known_answer(eng, m64):
    from molar_amd import api
    c, hmax = 3, (6, 3, 4)
    m, _ = api.sfactor_miller(hmax)
    x = sr.cubic_lattice(c)[None]
    bragg = np.all(m % c == 0, axis=1)
    for entry, real, tol in ((eng, np.float32, 1e-4), (m64, np.float64, 1e-11)):
        got = entry.structure_factor(np.asarray(x, real), api.sfactor_grid(hmax), boxes=np.asarray(sr.ORTHO, real), want=("rho", "sab"))
        rho = got.rho[0, 0, :, 0].astype(np.float64) + 1j * got.rho[0, 0, :, 1]
        # positions rounded to Real move a phase by 2 pi |m| eps: 27 atoms, |m|_1 <= 13
        assert np.abs(rho[bragg] - c ** 3).max() < tol * c ** 3 and np.abs(rho[~bragg]).max() < tol * c ** 3
        assert np.abs(api.sfactor_normalize(got.sab, n=c ** 3)[0][bragg] - c ** 3).max() < 2 * tol * c ** 3


def test_device_side_errors_touch_no_output(eng):
    import torch
    from molar_amd import api
    case = sr.GROUP_CASES[0]
    frames, boxes, idx, weight, labels = sr.case_inputs(case)
    dev = lambda a, dt: torch.as_tensor(np.asarray(a, dt), device="cuda")
    Q, P = 4 * 5 * 5, 6
    shapes = ((case.F, case.G, Q, 2), (case.F,), (case.G, Q, 2), (P, Q), (P, case.nshells), (case.nshells,))
    dts = (torch.float32, torch.int32, torch.float32, torch.float32, torch.float32, torch.int64)
    bad_idx = idx.astype(np.int64).copy()
    bad_idx[5] = case.natoms
    bad_lab = labels.astype(np.int32).copy()
    bad_lab[7] = case.G
    bad_w = weight.copy()
    bad_w[idx[2]] = np.inf
    for what, kw in (("index", dict(idx=dev(bad_idx, np.int64))), ("label", dict(labels=dev(bad_lab, np.int32))), ("weight", dict(weight=dev(bad_w, np.float32)))):
        args = dict(idx=dev(idx, np.int64), weight=dev(weight, np.float32), labels=dev(labels, np.int32))
        args.update(kw)
        out = tuple(torch.full(s, 7, dtype=d, device="cuda") for s, d in zip(shapes, dts))
        with pytest.raises(api.MolarHipError) as e:
            eng.structure_factor(dev(frames, np.float32), grid_of(case), ngroups=case.G, boxes=dev(boxes, np.float32), want=ALL, out=out, **args)
        assert e.value.code == sr.ERR_INVALID, what
        eng.synchronize()
        assert all(bool((o == 7).all()) for o in out), what
    # a box without an inverse, found on the device
    flat = np.array(boxes, np.float32).copy()
    flat[6:9] = flat[3:6]
    with pytest.raises(api.MolarHipError) as e:
        call(eng, case, np.float32, inputs=(frames, flat, idx, weight, labels))
    assert e.value.code == sr.ERR_INVERSE
    flat[6:9] = 0.0
    with pytest.raises(api.MolarHipError) as e:
        call(eng, case, np.float32, inputs=(frames, flat, idx, weight, labels))
    assert e.value.code == sr.ERR_ZERO_LENGTH


def test_print_the_largest_used_fraction_of_each_bound():
    assert set(FRACTIONS) == {"rho", "rho_mean", "sab", "shell"}
    for name, frac in sorted(FRACTIONS.items()):
        print(f"sfactor: {name} used at most {frac:.3f} of its bound")
        assert frac <= 1.0
