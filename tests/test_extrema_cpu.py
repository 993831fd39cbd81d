"""histogram_extrema without a GPU: the oracle against a per-bin loop, the key order, the host combine of dask partials,
argument errors raised before any device work, and the xarray wrapper's labels (compute swapped for the oracle)."""
import importlib
import os
import sys

import numpy as np
import pytest

import extrema_oracle as eo
from xhistogram_amd import core

try:
    import xarray as xr  # noqa: F401
except ImportError:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "doubles"))
    import xarray as xr  # the double

SPECIAL = np.array([-np.inf, -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 2.2e-308, 1.0, 1e300, np.inf])


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _same(got, want):
    """bit for bit, NaN where NaN"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(nan_g, nan_w)
    np.testing.assert_array_equal(_bits(got[~nan_g]), _bits(want[~nan_w]))


def _values(rng, n):
    v = rng.standard_normal(n)
    pick = rng.integers(0, 4, n)
    v = np.where(pick == 0, SPECIAL[rng.integers(0, len(SPECIAL), n)], v)
    v[rng.random(n) < 0.1] = np.nan
    return v


@pytest.mark.parametrize("seed", range(6))
def test_oracle_matches_the_per_bin_loop(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 300))
    D = 1 + seed % 2
    edges = [np.sort(rng.uniform(-2, 2, int(rng.integers(2, 9)))) for _ in range(D)]
    samples = []
    for e in edges:
        x = rng.uniform(-2.5, 2.5, n)
        on_edge = rng.random(n) < 0.2
        x[on_edge] = e[rng.integers(0, len(e), int(on_edge.sum()))]
        x[rng.random(n) < 0.05] = np.nan
        samples.append(x)
    v = _values(rng, n)
    v[:5] = [-0.0, 0.0, -0.0, np.nan, 0.0]
    lo, hi = eo.extrema_rows([s[None, :] for s in samples], edges, v[None, :])
    dlo, dhi = eo.definitional(samples, edges, v)
    _same(lo[0], dlo)
    _same(hi[0], dhi)


def test_oracle_zeros_and_all_nan_bins():
    edges = [np.array([0.0, 1.0, 2.0, 3.0])]
    x = np.array([0.5, 0.5, 1.5, 1.5, 2.5, 3.0])
    v = np.array([0.0, -0.0, np.nan, np.nan, 5e-324, -np.inf])
    lo, hi = eo.extrema_rows([x[None]], edges, v[None])
    _same(lo[0], [-0.0, np.nan, -np.inf])
    _same(hi[0], [0.0, np.nan, 5e-324])
    assert np.signbit(lo[0, 0]) and not np.signbit(hi[0, 0])


def test_key_transform_orders_totally():
    k = core.extrema_keys(SPECIAL)
    assert np.all(np.diff(k.astype(object)) > 0), "keys must increase strictly along -inf < ... < -0 < +0 < ... < inf"
    np.testing.assert_array_equal(k, eo.key(SPECIAL))
    _same(core._extrema_values(k), SPECIAL)
    rng = np.random.default_rng(3)
    a = rng.standard_normal(1000) * 10.0 ** rng.integers(-300, 300, 1000)
    order = np.argsort(core.extrema_keys(a), kind="stable")
    assert np.all(np.diff(a[order]) >= 0)
    # the empty markers (~0 for a minimum, 0 for a maximum) are keys of NaN bit patterns only
    assert np.isnan(core._extrema_values(np.array([0xFFFFFFFFFFFFFFFF, 0], np.uint64))).all()


def test_dask_combine_on_numpy_partials():
    rng = np.random.default_rng(5)
    edges = [np.linspace(-1, 1, 6)]
    x = rng.uniform(-1.2, 1.2, (4, 3, 50))
    v = _values(rng, x.size).reshape(x.shape)
    v[0, 0, :] = np.nan  # a block whose values are all NaN
    parts = [eo.histogram_extrema(x[i], values=v[i], bins=edges, axis=1) for i in range(4)]
    plo = np.stack([p[0] for p in parts])[:, :, None, :]  # (block, kept, reduced of extent 1, bins)
    phi = np.stack([p[1] for p in parts])[:, :, None, :]
    lo, hi = core.combine_extrema(plo, phi, axis=(0, 2))
    want = eo.histogram_extrema(np.moveaxis(x, 0, 1).reshape(3, -1), values=np.moveaxis(v, 0, 1).reshape(3, -1), bins=edges, axis=1)
    _same(lo.reshape(3, 5), want[0])
    _same(hi.reshape(3, 5), want[1])
    # -0.0 and +0.0 in different partials: the key order decides, not fmin / fmax
    lo, hi = core.combine_extrema(np.array([[0.0], [-0.0], [np.nan]]), np.array([[-0.0], [0.0], [np.nan]]), axis=0)
    assert np.signbit(lo[0, 0]) and not np.signbit(hi[0, 0])
    lo, hi = core.combine_extrema(np.array([[np.nan], [np.nan]]), np.array([[np.nan], [np.nan]]), axis=0)
    assert np.isnan(lo).all() and np.isnan(hi).all()
    pair = core._extrema_pair_reduce(np.stack([plo, phi]), axis=(1, 3), keepdims=False)
    _same(pair[0], want[0])
    _same(pair[1], want[1])


def test_argument_errors_come_before_any_device_work():
    x = np.linspace(0, 1, 10)
    e = np.linspace(0, 1, 5)
    with pytest.raises(TypeError):
        core.histogram_extrema(x, bins=e)  # values are required
    with pytest.raises(TypeError):
        core.histogram_extrema(x, values=None, bins=e)
    with pytest.raises(TypeError, match="complex"):
        core.histogram_extrema(x, values=x + 1j, bins=e)
    with pytest.raises(TypeError):
        core.histogram_extrema(x, values=x, bins=e, density=True)
    with pytest.raises(TypeError):
        core.histogram_extrema(x, values=x.astype("datetime64[s]"), bins=e)
    assert "histogram_extrema" in core.__all__


xhx = importlib.import_module("xhistogram_amd.xarray")


def _oracle_extrema(*args, values, bins=None, range=None, axis=None, block_size="auto"):
    bins = [bins] * len(args) if isinstance(bins, np.ndarray) else list(bins)
    lo, hi = eo.histogram_extrema(*args, values=values, bins=bins, axis=axis)
    return lo, hi, bins


def test_xarray_wrapper_labels(monkeypatch):
    monkeypatch.setattr(core, "histogram_extrema", _oracle_extrema)
    rng = np.random.default_rng(7)
    dims, shape = ("t", "y", "x"), (2, 3, 40)
    coords = {d: np.arange(n) * 1.0 for d, n in zip(dims, shape)}
    T = xr.DataArray(rng.uniform(0, 1, shape), dims=dims, coords=coords, name="T", attrs={"units": "K"})
    S = xr.DataArray(rng.uniform(0, 1, shape), dims=dims, coords=coords, name="S")
    V = xr.DataArray(rng.standard_normal(shape), dims=dims, coords=coords, name="flux")
    bins = [np.linspace(0, 1, 5), np.linspace(0, 1, 4)]
    vmin, vmax = xhx.histogram_extrema(T, S, values=V, bins=bins, dim=("y", "x"))
    assert vmin.name == "flux_min" and vmax.name == "flux_max"
    assert vmin.dims == vmax.dims == ("t", "T_bin", "S_bin")
    np.testing.assert_array_equal(vmin["T_bin"].values, 0.5 * (bins[0][:-1] + bins[0][1:]))
    np.testing.assert_array_equal(vmax["S_bin"].values, 0.5 * (bins[1][:-1] + bins[1][1:]))
    assert vmin["T_bin"].attrs == {"units": "K"}
    np.testing.assert_array_equal(vmin["t"].values, coords["t"])
    want = eo.histogram_extrema(T.values, S.values, values=V.values, bins=bins, axis=(1, 2))
    _same(vmin.values, want[0])
    _same(vmax.values, want[1])
    # a nameless values array, values broadcast over a dim they lack, everything reduced
    W = xr.DataArray(rng.standard_normal(shape[1:]), dims=dims[1:])
    vmin, vmax = xhx.histogram_extrema(T, values=W, bins=[bins[0]])
    assert vmin.name == "values_min" and vmax.name == "values_max"
    assert vmin.dims == ("T_bin",)
    want = eo.histogram_extrema(T.values, values=np.broadcast_to(W.values, shape), bins=[bins[0]])
    _same(vmin.values, want[0])
    _same(vmax.values, want[1])
    with pytest.raises(TypeError):
        xhx.histogram_extrema(T, values=V.values, bins=[bins[0]])
