"""The bin edges of the f64 fused histogram (molar_hip_histogram_edges_f64: host arithmetic, no GPU) against the f64
Histogram1D::add_one (molar_membrane/src/stats.rs:29-35): numpy float64 and the f64 build of the CPU checker."""
import numpy as np
import pytest

INVALID_ARGUMENT = 50          # MOLAR_HIP_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def lib():
    from molar_amd import _lib, build
    build.build_library()
    return _lib.load()


def formula(d2, hmin, hmax, nbins):
    """The f64 bin of the squared distance: floor(n * (sqrt(d2) - min) / (max - min)), IEEE double like the checker's C."""
    d = np.sqrt(np.asarray(d2, np.float64))
    return np.floor(np.float64(nbins) * (d - np.float64(hmin)) / (np.float64(hmax) - np.float64(hmin)))


@pytest.mark.parametrize("hmin,hmax,nbins", [(0.0, 1.2, 1200), (0.35, 0.9, 450), (-0.2, 0.7, 350), (0.0, 0.6, 1), (0.1, 2.5, 8192)])
def test_histogram_edges_f64_are_the_formula(lib, orc64, hmin, hmax, nbins):
    from molar_amd import api
    e = api.histogram_edges_f64(hmin, hmax, nbins)
    assert e.dtype == np.float64 and e.shape == (nbins + 1,)
    assert np.all(np.diff(e) >= 0) and e[0] >= 0
    rng = np.random.default_rng(5)
    x = rng.uniform(0, 1.1 * max(hmax, 0.1), 40000) ** 2
    # squared distances on and next to the edges themselves
    x = np.concatenate([x, e, np.nextafter(e, -1.0), np.nextafter(e, np.inf)])
    x = x[x >= 0]
    fb = formula(x, hmin, hmax, nbins)
    ok = (fb >= 0) & (fb < nbins)
    want = orc64.histogram_add(hmin, hmax, nbins, np.sqrt(x)).astype(np.int64)
    assert np.array_equal(np.bincount(fb[ok].astype(np.int64), minlength=nbins), want)
    tb = np.searchsorted(e, x, side="right") - 1          # largest b with e[b] <= x
    assert np.array_equal(tb[ok], fb[ok].astype(np.int64))
    assert np.all((tb[~ok] < 0) | (tb[~ok] >= nbins))


@pytest.mark.parametrize("hmin,hmax,nbins", [(0.0, 1.2, 1200), (-0.2, 0.7, 350), (0.1, 2.5, 8192), (0.749999, 0.75, 8192)])
def test_histogram_edges_f64_are_tight(lib, hmin, hmax, nbins):
    """Each edge reaches its bin, and the next double below each positive edge bins lower."""
    from molar_amd import api
    e = api.histogram_edges_f64(hmin, hmax, nbins)
    b = np.arange(nbins + 1)
    assert np.all(formula(e, hmin, hmax, nbins) >= b)
    pos = e > 0
    below = np.nextafter(e[pos], -1.0)
    assert np.all(formula(below, hmin, hmax, nbins) < b[pos])
    # bins that start below d = 0 share the edge 0
    if hmin < 0:
        assert e[0] == 0.0 and e[int(np.floor(nbins * -hmin / (hmax - hmin)))] == 0.0


def test_histogram_edges_f64_differ_from_f32(lib):
    """The f64 table is its own: at C4's binning it is not the f32 table widened."""
    from molar_amd import api
    e64 = api.histogram_edges_f64(0.0, 1.2, 1200)
    e32 = api.histogram_edges(0.0, 1.2, 1200).astype(np.float64)
    assert np.count_nonzero(e64 != e32) > 1000


def test_histogram_edges_f64_rejects_degenerate_ranges(lib):
    from molar_amd import api
    from molar_amd._lib import MolarHipError
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (float("-inf"), 1.0), (float("nan"), 1.0), (0.0, float("nan")),
                   (-1.0e308, 1.0e308)):
        with pytest.raises(MolarHipError) as e:
            api.histogram_edges_f64(lo, hi, 10)
        assert e.value.code == INVALID_ARGUMENT
    with pytest.raises(MolarHipError) as e:
        api.histogram_edges_f64(0.0, 1.0, 0)
    assert e.value.code == INVALID_ARGUMENT

