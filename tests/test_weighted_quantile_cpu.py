"""histogram_weighted_quantile without a GPU: the oracle against numpy, a restatement of the kernels' select arithmetic (most
significant digit first over order-preserving keys, `below`, C / W >= q, the positive-sum rule, the fallback to the last bucket of
positive weight) against the oracle bit for bit on hard data, argument errors raised before any device work, the new C symbol
with the ABI still 11, and the xarray wrapper's labels (compute swapped for the oracle)."""
import importlib
import os
import sys

import numpy as np
import pytest

import exact_weights as xw
import weighted_quantile_oracle as wqo
from xhistogram_amd import _native, core

try:
    import xarray as xr  # noqa: F401
except ImportError:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "doubles"))
    import xarray as xr  # the double

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEFORE_ONE = float(np.nextafter(1.0, 0.0))


def _keys(v):
    """extrema_key64: unsigned order is the total order of float64 with -0.0 < +0.0"""
    b = np.asarray(v, np.float64).view(np.uint64)
    neg = (b >> np.uint64(63)).astype(bool)
    return np.where(neg, ~b, b | np.uint64(1 << 63))


def _value(k):
    k = np.uint64(k)
    b = k ^ (np.uint64(1 << 63) if (int(k) >> 63) else np.uint64(0xFFFFFFFFFFFFFFFF))
    return float(np.array([b], np.uint64).view(np.float64)[0])


def _radix_select(v, w, q, d, rng):
    """the radix family on one bin: pass 0 (min, max, W), qw_init, then digit passes and qw_select; the bucket sums of every
    pass are taken in a shuffled order of the samples, as atomics take them"""
    keep = ~np.isnan(v)
    v, w = v[keep], w[keep]
    if v.size == 0:
        return np.nan
    p = rng.permutation(v.size)
    W = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for x in w[p]:
            W += x if x >= 0 else np.nan
    if not (W > 0 and np.isfinite(W)):
        return np.nan
    k = _keys(v)
    mn, mx = int(k.min()), int(k.max())
    if mn == mx:
        return _value(mn)
    nfix = 64 - (mn ^ mx).bit_length()
    pre = mn >> (64 - nfix) << (64 - nfix) if nfix else 0
    below = 0.0
    ki = [int(x) for x in k]
    while nfix < 64:
        dd = min(d, 64 - nfix)
        shift = 64 - nfix - dd
        sums = np.zeros(1 << dd)
        for i in rng.permutation(v.size):  # the digit pass
            if w[i] > 0 and (ki[i] >> (64 - nfix) if nfix else 0) == (pre >> (64 - nfix) if nfix else 0):
                sums[(ki[i] >> shift) & ((1 << dd) - 1)] += w[i]
        cum, under, dig, found = 0.0, 0.0, 0, False
        for j in range(1 << dd):  # qw_select
            if found or not sums[j] > 0:
                continue
            dig, under = j, cum
            cum += sums[j]
            found = (below + cum) / W >= q
        below += under
        nfix += dd
        pre |= dig << (64 - nfix)
    return _value(pre)


def _short_walk(v, w, q):
    """the short-row family on one bin: the sorted run walked with one sequential running sum"""
    keep = ~np.isnan(v)
    v, w = v[keep], w[keep]
    o = np.argsort(_keys(v), kind="stable")
    v, w = v[o], w[o]
    W, good = 0.0, v.size > 0
    with np.errstate(invalid="ignore", over="ignore"):
        for x in w:
            W += x if x >= 0 else np.nan
    if not (good and W > 0 and np.isfinite(W)):
        return np.nan
    cum, last = 0.0, 0
    for i in range(v.size):
        cum += w[i]
        if w[i] > 0:
            last = i
            if cum / W >= q:
                break
    return float(v[last])


def _hard_cases(rng):
    z = lambda n, frac=0.3: np.where(rng.random(n) < frac, 0.0, xw.f64(rng, n))  # noqa: E731
    cases = [
        ("single value", np.array([1.5]), xw.f64(rng, 1)),
        ("all equal", np.full(9, 3.0), z(9, 0.2) + np.r_[xw.f64(rng, 1), np.zeros(8)]),
        ("infinities", np.array([-np.inf, 1.0, np.inf, np.inf, -2.0]), xw.f64(rng, 5)),
        ("ties", np.round(rng.standard_normal(64), 1), z(64) + np.r_[np.zeros(63), xw.f64(rng, 1)]),
        ("zero weights at both ends", np.arange(10.0), np.r_[0.0, 0.0, xw.f64(rng, 6), 0.0, 0.0]),
        ("NaN values", np.array([np.nan, 2.0, 3.0, np.nan, 1.0]), np.r_[1e300, xw.f64(rng, 4)]),
        ("a bin of zero weight", np.arange(5.0), np.zeros(5)),
        ("close keys", (np.float64(1.5).view(np.uint64) + rng.integers(0, 1 << 11, 40).astype(np.uint64)).view(np.float64), z(40) + np.r_[xw.f64(rng, 1), np.zeros(39)]),
        ("mixed signs", rng.standard_normal(101), z(101) + np.r_[xw.f64(rng, 1), np.zeros(100)]),
        ("eighths", np.round(rng.standard_normal(33), 1), np.round(z(33) * 8) / 8 + np.r_[0.5, np.zeros(32)]),
        ("empty", np.array([np.nan, np.nan]), np.ones(2)),
        ("a NaN weight", np.arange(4.0), np.array([0.5, np.nan, 0.5, 0.75])),
        ("a negative weight", np.arange(4.0), np.array([0.5, -0.75, 0.5, 0.75])),
        ("an infinite weight", np.arange(4.0), np.array([0.5, np.inf, 0.5, 0.75])),
    ]
    return cases


def _qs(v, w):
    """0, 1, the float before 1, 1e-300, 1/3, and the cdf's own steps (hit exactly)"""
    qs = [0.0, 1.0, BEFORE_ONE, 1e-300, 1.0 / 3.0, 0.5]
    keep = ~np.isnan(v)
    if keep.any() and np.all(w[keep] >= 0) and w[keep].sum() > 0 and np.isfinite(w[keep].sum()):
        o = np.argsort(v[keep], kind="stable")
        cdf = np.cumsum(w[keep][o])
        cdf = cdf / cdf[-1]
        qs += [float(c) for c in cdf[:: max(1, len(cdf) // 6)]]
    return qs


def _same(got, want, what):
    if np.isnan(want):
        assert np.isnan(got), what
    elif want == 0:
        assert got == 0, what  # (zeros compare by value: numpy keeps the input order of -0.0 and +0.0)
    else:
        assert np.float64(got).view(np.int64) == np.float64(want).view(np.int64), (what, got, want)


@pytest.mark.parametrize("d", [4, 5, 8])
def test_select_arithmetic_restates_the_oracle_bit_for_bit(d):
    rng = np.random.default_rng(11 + d)
    n = 0
    for name, v, w in _hard_cases(rng):
        for q in _qs(v, w):
            want = wqo.bin_quantiles(v, w, [q])[0]
            _same(_radix_select(v, w, q, d, rng), want, "radix d=%d %s q=%r" % (d, name, q))
            _same(_short_walk(v, w, q), want, "short %s q=%r" % (name, q))
            n += 1
    assert n > 100


def test_oracle_against_numpy_and_its_nan_rules():
    rng = np.random.default_rng(3)
    x = rng.uniform(-0.2, 1.2, 4000)
    v = np.round(rng.standard_normal(4000), 1)
    v[rng.random(4000) < 0.02] = np.nan
    w = np.where(rng.random(4000) < 0.3, 0.0, xw.f64(rng, 4000))
    e = np.linspace(0, 1, 9)
    qs = [0.0, 0.1, 0.5, 0.9, 1.0]
    got, counts = wqo.histogram_weighted_quantile(x, values=v, weights=w, q=qs, bins=[e], return_counts=True)
    assert got.shape == (5, 8) and counts.shape == (8,)
    for b in range(8):
        inb = (x >= e[b]) & ((x < e[b + 1]) | ((b == 7) & (x == e[-1]))) & ~np.isnan(v)
        assert counts[b] == inb.sum()
        np.testing.assert_array_equal(got[:, b], np.quantile(v[inb], qs, weights=w[inb], method="inverted_cdf"))
    # a NaN or negative weight makes its own bin NaN, and no other; a bin of zero weight is NaN
    for bad in (np.nan, -0.5):
        w2 = w.copy()
        i = np.flatnonzero((x >= e[2]) & (x < e[3]) & ~np.isnan(v))[0]
        w2[i] = bad
        g2 = wqo.histogram_weighted_quantile(x, values=v, weights=w2, q=qs, bins=[e])
        assert np.isnan(g2[:, 2]).all()
        np.testing.assert_array_equal(np.delete(g2, 2, axis=1), np.delete(got, 2, axis=1))
    w3 = np.where((x >= e[4]) & (x < e[5]), 0.0, w)
    g3 = wqo.histogram_weighted_quantile(x, values=v, weights=w3, q=0.5, bins=[e])
    assert g3.shape == (8,) and np.isnan(g3[4]) and not np.isnan(np.delete(g3, 4)).any()
    # rows and axes
    xr_ = rng.uniform(0, 1, (3, 50))
    g4 = wqo.histogram_weighted_quantile(xr_, values=xr_, weights=np.ones(50), q=[0.5], bins=[e], axis=1)
    assert g4.shape == (1, 3, 8)


def test_argument_errors_come_before_any_device_work():
    x = np.linspace(0, 1, 10)
    e = np.linspace(0, 1, 5)
    f = core.histogram_weighted_quantile
    with pytest.raises(TypeError):
        f(x, weights=x, q=0.5, bins=e)  # values are required
    with pytest.raises(TypeError):
        f(x, values=x, q=0.5, bins=e)  # weights are required
    with pytest.raises(TypeError):
        f(x, values=None, weights=x, q=0.5, bins=e)
    with pytest.raises(TypeError):
        f(x, values=x, weights=None, q=0.5, bins=e)
    with pytest.raises(TypeError, match="complex"):
        f(x, values=x, weights=x + 1j, q=0.5, bins=e)
    with pytest.raises(TypeError, match="complex"):
        f(x, values=x + 1j, weights=x, q=0.5, bins=e)
    for bad in (-0.1, 1.5, np.nan, [0.5, 2.0]):
        with pytest.raises(ValueError, match=r"Quantiles must be in the range \[0, 1\]"):
            f(x, values=x, weights=x, q=bad, bins=e)
    with pytest.raises(ValueError):
        f(x, values=x, weights=x, q=[[0.5]], bins=e)
    for m in ("linear", "lower", "hazen", None):
        with pytest.raises(ValueError, match="Only method 'inverted_cdf' supports weights"):
            f(x, values=x, weights=x, q=0.5, bins=e, method=m)
    with pytest.raises(ValueError, match="Only method 'inverted_cdf' supports weights"):
        np.quantile(x, 0.5, weights=x, method="linear")  # (numpy's wording)
    assert "histogram_weighted_quantile" in core.__all__
    # the unweighted function still refuses weights, with the error type it had
    with pytest.raises(TypeError):
        core.histogram_quantile(x, values=x, q=0.5, bins=e, weights=x)


def test_symbol_and_abi_version():
    assert _native.ABI_VERSION == 11
    assert "xhist_plan_execute_quantile_weighted" in _native.EXPORTS
    header = open(os.path.join(ROOT, "include", "xhist_amd.h")).read()
    assert "#define XHIST_ABI_VERSION 11" in header and "xhist_plan_execute_quantile_weighted(" in header
    lib = _native.load()
    assert lib.xhist_abi_version() == 11
    assert len(lib.xhist_plan_execute_quantile_weighted.argtypes) == 11
    assert len(lib.xhist_plan_execute_quantile.argtypes) == 11
    assert callable(getattr(_native.Plan, "execute_quantile_weighted"))
    assert "xhist_plan_execute_quantile_weighted" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "xhist_quantile_w" in open(os.path.join(ROOT, "xhistogram_amd", "csrc", "build.sh")).read()


xhx = importlib.import_module("xhistogram_amd.xarray")


def _oracle(*args, values, weights, q, bins=None, range=None, axis=None, method="inverted_cdf", block_size="auto"):
    bins = [bins] * len(args) if isinstance(bins, np.ndarray) else list(bins)
    return wqo.histogram_weighted_quantile(*args, values=values, weights=weights, q=q, bins=bins, axis=axis), bins


def test_xarray_wrapper_labels(monkeypatch):
    monkeypatch.setattr(core, "histogram_weighted_quantile", _oracle)
    assert "histogram_weighted_quantile" in xhx.__all__
    rng = np.random.default_rng(7)
    dims, shape = ("t", "y", "x"), (2, 3, 40)
    coords = {d: np.arange(n) * 1.0 for d, n in zip(dims, shape)}
    T = xr.DataArray(rng.uniform(0, 1, shape), dims=dims, coords=coords, name="T", attrs={"units": "K"})
    S = xr.DataArray(rng.uniform(0, 1, shape), dims=dims, coords=coords, name="S")
    V = xr.DataArray(rng.standard_normal(shape), dims=dims, coords=coords, name="temp")
    A = xr.DataArray(xw.f64(rng, shape[1:]), dims=dims[1:], coords={d: coords[d] for d in dims[1:]}, name="area")
    bins = [np.linspace(0, 1, 5), np.linspace(0, 1, 4)]
    qs = [0.1, 0.5, 0.9]
    r = xhx.histogram_weighted_quantile(T, S, values=V, weights=A, q=qs, bins=bins, dim=("y", "x"))
    assert r.name == "temp_weighted_quantile"
    assert r.dims == ("quantile", "t", "T_bin", "S_bin")
    np.testing.assert_array_equal(r["quantile"].values, qs)
    np.testing.assert_array_equal(r["T_bin"].values, 0.5 * (bins[0][:-1] + bins[0][1:]))
    np.testing.assert_array_equal(r["t"].values, coords["t"])
    assert r["T_bin"].attrs == {"units": "K"}
    want = wqo.histogram_weighted_quantile(T.values, S.values, values=V.values, weights=A.values, q=qs, bins=bins, axis=(1, 2))
    np.testing.assert_array_equal(r.values, want)
    # a scalar q: no quantile dimension, a scalar quantile coordinate; a nameless values array
    W = xr.DataArray(rng.standard_normal(shape[1:]), dims=dims[1:])
    m = xhx.histogram_weighted_quantile(T, values=W, weights=A, q=0.5, bins=[bins[0]])
    assert m.name == "values_weighted_quantile" and m.dims == ("T_bin",)
    assert "quantile" in m.coords and float(m["quantile"].values) == 0.5
    with pytest.raises(TypeError):
        xhx.histogram_weighted_quantile(T, values=V, weights=A.values, q=0.5, bins=[bins[0]])
