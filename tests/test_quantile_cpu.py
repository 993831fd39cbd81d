"""histogram_quantile without a GPU: the oracle against scipy.stats.binned_statistic's median and against a sort-and-index
restatement of numpy's five methods, argument errors raised before any device work, the new C symbol with the ABI still 11,
and the xarray wrapper's labels (compute swapped for the oracle)."""
import importlib
import os
import sys

import numpy as np
import pytest

import quantile_oracle as qo
from xhistogram_amd import _native, core

try:
    import xarray as xr  # noqa: F401
except ImportError:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "doubles"))
    import xarray as xr  # the double

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ("linear", "lower", "higher", "midpoint", "nearest")


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_median_matches_scipy_binned_statistic(seed):
    """to the last bit: scipy's median (np.median) averages the two middle values, np.nanquantile interpolates between them"""
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(seed)
    n = 3000
    x = rng.uniform(-0.2, 1.2, n)
    y = rng.uniform(0, 1, n)
    v = np.round(rng.standard_normal(n), 2)  # (ties)
    e = np.linspace(0, 1, 13)
    got = qo.histogram_quantile(x, values=v, q=0.5, bins=[e])
    want = stats.binned_statistic(x, v, statistic="median", bins=e).statistic
    np.testing.assert_allclose(got, want, rtol=4e-16, atol=1e-300)
    got2 = qo.histogram_quantile(x, y, values=v, q=[0.5], bins=[e, e[::2]])
    want2 = stats.binned_statistic_2d(x, y, v, statistic="median", bins=[e, e[::2]]).statistic
    np.testing.assert_allclose(got2[0], want2, rtol=4e-16, atol=1e-16, equal_nan=True)


def _sorted_index(vals, q, method):
    """numpy's arithmetic restated on a sorted array: what the GPU's finalize step computes from two order statistics"""
    a = np.sort(vals[~np.isnan(vals)])
    n = len(a)
    if n == 0:
        return np.nan
    x = (n - 1) * q
    vi = {"linear": x, "lower": np.floor(x), "higher": np.ceil(x), "midpoint": 0.5 * (np.floor(x) + np.ceil(x)),
          "nearest": np.around(x)}[method]
    if method in ("lower", "higher", "nearest"):
        return a[int(vi)]
    above = vi >= n - 1
    r = n - 1 if above else int(np.floor(vi))
    lo, hi = a[r], a[r] if above else a[r + 1]
    gamma = (vi + 1.0 if above else vi - np.floor(vi)) if method == "linear" else (0.0 if vi == np.floor(vi) else 0.5)
    with np.errstate(invalid="ignore"):
        diff = hi - lo
        return hi - diff * (1.0 - gamma) if gamma >= 0.5 else lo + diff * gamma


@pytest.mark.parametrize("method", METHODS)
def test_finalize_arithmetic_restates_nanquantile(method):
    """the two-order-statistics form the kernels use equals np.nanquantile bit for bit, on hard data"""
    rng = np.random.default_rng(5)
    cases = [np.array([1.0]), np.array([np.inf, np.inf]), np.array([-np.inf, 1.0]), np.array([-0.0, 0.0, -0.0]),
             np.array([np.inf]), np.array([1.0, np.inf]), np.array([np.nan, 2.0, 3.0]), np.array([3.0, 3.0, 3.0, 3.0]),
             np.nextafter(1.0, 2.0) ** np.arange(7), rng.standard_normal(101), np.round(rng.standard_normal(64), 1)]
    for vals in cases:
        for q in (0.0, 1.0, 0.5, 0.1, 0.25, 0.75, 0.9, 1.0 / 3.0):
            with np.errstate(invalid="ignore"):
                want = np.nanquantile(vals, q, method=method)
            np.testing.assert_array_equal(_sorted_index(vals, q, method), want, err_msg="%s q=%r %r" % (method, q, vals))


def test_argument_errors_come_before_any_device_work():
    x = np.linspace(0, 1, 10)
    e = np.linspace(0, 1, 5)
    with pytest.raises(TypeError):
        core.histogram_quantile(x, q=0.5, bins=e)  # values are required
    with pytest.raises(TypeError):
        core.histogram_quantile(x, values=None, q=0.5, bins=e)
    with pytest.raises(TypeError, match="complex"):
        core.histogram_quantile(x, values=x + 1j, q=0.5, bins=e)
    for bad in (-0.1, 1.5, np.nan, [0.5, 2.0], [np.nan]):
        with pytest.raises(ValueError, match=r"Quantiles must be in the range \[0, 1\]"):
            core.histogram_quantile(x, values=x, q=bad, bins=e)
        with pytest.raises(ValueError, match=r"Quantiles must be in the range \[0, 1\]"):
            np.nanquantile(x, bad)  # (the same error as numpy's)
    with pytest.raises(ValueError):
        core.histogram_quantile(x, values=x, q=[[0.5]], bins=e)
    with pytest.raises(ValueError, match="linear.*lower.*higher.*midpoint.*nearest"):
        core.histogram_quantile(x, values=x, q=0.5, bins=e, method="hazen")
    with pytest.raises(TypeError):
        core.histogram_quantile(x, values=x, q=0.5, bins=e, weights=x)
    with pytest.raises(TypeError):
        core.histogram_quantile(x, values=x, q=0.5, bins=e, density=True)
    assert "histogram_quantile" in core.__all__


def test_symbol_and_abi_version():
    assert _native.ABI_VERSION == 11
    assert "xhist_plan_execute_quantile" in _native.EXPORTS
    header = open(os.path.join(ROOT, "include", "xhist_amd.h")).read()
    assert "#define XHIST_ABI_VERSION 11" in header and "xhist_plan_execute_quantile(" in header
    for i, m in enumerate(METHODS):
        assert "#define XHIST_Q_%s %d" % (m.upper(), i) in header
    assert _native.QUANTILE_METHODS == METHODS
    lib = _native.load()
    assert lib.xhist_abi_version() == 11
    assert len(lib.xhist_plan_execute_quantile.argtypes) == 11
    assert callable(getattr(_native.Plan, "execute_quantile"))


xhx = importlib.import_module("xhistogram_amd.xarray")


def _oracle_quantile(*args, values, q, bins=None, range=None, axis=None, method="linear", block_size="auto"):
    bins = [bins] * len(args) if isinstance(bins, np.ndarray) else list(bins)
    return qo.histogram_quantile(*args, values=values, q=q, bins=bins, axis=axis, method=method), bins


def test_xarray_wrapper_labels(monkeypatch):
    monkeypatch.setattr(core, "histogram_quantile", _oracle_quantile)
    assert "histogram_quantile" in xhx.__all__
    rng = np.random.default_rng(7)
    dims, shape = ("t", "y", "x"), (2, 3, 40)
    coords = {d: np.arange(n) * 1.0 for d, n in zip(dims, shape)}
    T = xr.DataArray(rng.uniform(0, 1, shape), dims=dims, coords=coords, name="T", attrs={"units": "K"})
    S = xr.DataArray(rng.uniform(0, 1, shape), dims=dims, coords=coords, name="S")
    V = xr.DataArray(rng.standard_normal(shape), dims=dims, coords=coords, name="temp")
    bins = [np.linspace(0, 1, 5), np.linspace(0, 1, 4)]
    qs = [0.1, 0.5, 0.9]
    r = xhx.histogram_quantile(T, S, values=V, q=qs, bins=bins, dim=("y", "x"), method="nearest")
    assert r.name == "temp_quantile"
    assert r.dims == ("quantile", "t", "T_bin", "S_bin")
    np.testing.assert_array_equal(r["quantile"].values, qs)
    np.testing.assert_array_equal(r["T_bin"].values, 0.5 * (bins[0][:-1] + bins[0][1:]))
    np.testing.assert_array_equal(r["t"].values, coords["t"])
    assert r["T_bin"].attrs == {"units": "K"}
    want = qo.histogram_quantile(T.values, S.values, values=V.values, q=qs, bins=bins, axis=(1, 2), method="nearest")
    np.testing.assert_array_equal(r.values, want)
    # a scalar q: no quantile dimension, a scalar quantile coordinate; a nameless values array broadcast over a dim it lacks
    W = xr.DataArray(rng.standard_normal(shape[1:]), dims=dims[1:])
    m = xhx.histogram_quantile(T, values=W, q=0.5, bins=[bins[0]])
    assert m.name == "values_quantile" and m.dims == ("T_bin",)
    assert "quantile" in m.coords and float(m["quantile"].values) == 0.5
    with pytest.raises(TypeError):
        xhx.histogram_quantile(T, values=V.values, q=0.5, bins=[bins[0]])
