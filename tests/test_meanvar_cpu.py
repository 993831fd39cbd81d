"""histogram_mean_var without a GPU: the oracle against np.nanmean / np.nanvar per bin, the host merge of dask partials
(core.combine_mean_var) against the oracle, argument errors raised before any device work, the new C symbol, and the
xarray wrapper's labels (compute swapped for the oracle)."""
import importlib
import os
import sys

import numpy as np
import pytest

import meanvar_oracle as mo
from xhistogram_amd import _native, core

try:
    import xarray as xr  # noqa: F401
except ImportError:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "doubles"))
    import xarray as xr  # the double

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _per_bin_loop(samples, edges, v, ddof):
    """np.nanmean / np.nanvar over the values of each bin of one row, bins found by a loop"""
    nbs = [len(e) - 1 for e in edges]
    groups = {}
    for i in range(len(v)):
        idx = []
        for s, e in zip(samples, edges):
            x = s[i]
            if not (x >= e[0] and x <= e[-1]):
                idx = None
                break
            idx.append(next(k for k in range(len(e) - 1) if e[k] <= x and (x < e[k + 1] or k == len(e) - 2)))
        if idx is not None:
            groups.setdefault(tuple(idx), []).append(v[i])
    cnt = np.zeros(nbs, np.int64)
    mean = np.full(nbs, np.nan)
    var = np.full(nbs, np.nan)
    with np.errstate(invalid="ignore", divide="ignore"), _quiet():
        for k, vals in groups.items():
            vals = np.asarray(vals)
            good = vals[~np.isnan(vals)]
            cnt[k] = len(good)
            if len(good):
                mean[k] = np.nanmean(vals)
            if len(good) > ddof:
                var[k] = np.nanvar(vals, ddof=ddof)
    return cnt, mean, var


class _quiet:
    def __enter__(self):
        import warnings

        self._w = warnings.catch_warnings()
        self._w.__enter__()
        warnings.simplefilter("ignore")

    def __exit__(self, *a):
        self._w.__exit__(*a)


@pytest.mark.parametrize("seed", range(6))
def test_oracle_matches_nanmean_nanvar(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 400))
    D = 1 + seed % 2
    ddof = seed % 3
    edges = [np.sort(rng.uniform(-2, 2, int(rng.integers(2, 9)))) for _ in range(D)]
    samples = []
    for e in edges:
        x = rng.uniform(-2.5, 2.5, n)
        on_edge = rng.random(n) < 0.2
        x[on_edge] = e[rng.integers(0, len(e), int(on_edge.sum()))]
        x[rng.random(n) < 0.05] = np.nan
        samples.append(x)
    v = rng.standard_normal(n) * 3 + 10
    v[rng.random(n) < 0.1] = np.nan
    if seed >= 4:  # infinities: the mean is +-inf or NaN, the variance NaN
        v[rng.random(n) < 0.05] = np.inf
        v[rng.random(n) < 0.03] = -np.inf
    want = _per_bin_loop(samples, edges, v, ddof)
    for exact in (False, True):
        cnt, mean, m2 = mo.mean_var_rows([s[None, :] for s in samples], edges, v[None, :], exact=exact)
        np.testing.assert_array_equal(cnt[0], want[0])
        np.testing.assert_allclose(mean[0], want[1], rtol=1e-13, atol=0, equal_nan=True)
        np.testing.assert_allclose(mo.var_of(cnt, m2, ddof)[0], want[2], rtol=1e-11, atol=1e-300, equal_nan=True)


def test_oracle_exact_mode_on_exactly_summable_data():
    """values k * 2^-10 with a power-of-two count per bin: the fsum mode and the kernels' formula agree bit for bit"""
    rng = np.random.default_rng(1)
    nb = 16
    edges = [np.arange(nb + 1, dtype=np.float64)]
    counts = 2 ** rng.integers(0, 8, nb)
    x = np.repeat(np.arange(nb) + 0.5, counts)
    v = rng.integers(-4095, 4096, len(x)) * 2.0**-10
    perm = rng.permutation(len(x))
    x, v = x[perm], v[perm]
    a = mo.mean_var_rows([x[None]], edges, v[None], exact=True)
    b = mo.mean_var_rows([x[None]], edges, v[None], exact=False)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    np.testing.assert_array_equal(a[2], b[2])


def test_oracle_cancellation_shows_the_naive_formula_fails():
    """1e8 + N(0, 1): the oracle keeps the variance; sum(v^2)/n - mean^2 is off by O(1)"""
    rng = np.random.default_rng(2)
    v = 1e8 + rng.standard_normal(100_000)
    x = np.full(v.shape, 0.5)
    cnt, mean, m2 = mo.mean_var_rows([x[None]], [np.array([0.0, 1.0])], v[None])
    var = m2[0, 0] / cnt[0, 0]
    np.testing.assert_allclose(var, np.var(v - 1e8), rtol=1e-9)
    naive = np.mean(v * v) - np.mean(v) ** 2
    assert abs(naive - var) > 0.01


def _partials(rng, n_parts, empty):
    nb = 5
    edges = [np.linspace(-1, 1, nb + 1)]
    parts = []
    allv, allx = [], []
    for i in range(n_parts):
        k = 0 if i in empty else int(rng.integers(1, 300))
        x = rng.uniform(-1.2, 1.2, k)
        v = rng.standard_normal(k) * 2 + 50
        v[rng.random(k) < 0.1] = np.nan
        allx.append(x)
        allv.append(v)
        parts.append(mo.mean_var_rows([x[None]], edges, v[None]))
    want = mo.mean_var_rows([np.concatenate(allx)[None]], edges, np.concatenate(allv)[None])
    return parts, want


@pytest.mark.parametrize("seed", range(5))
def test_combine_mean_var_against_the_oracle(seed):
    rng = np.random.default_rng(10 + seed)
    n_parts = int(rng.integers(1, 7))
    empty = set(rng.choice(n_parts, int(rng.integers(0, n_parts)), replace=False).tolist()) if n_parts > 1 else set()
    parts, want = _partials(rng, n_parts, empty)
    n = np.stack([p[0] for p in parts])  # (part, row of extent 1, bins)
    mean = np.stack([p[1] for p in parts])
    m2 = np.stack([p[2] for p in parts])
    cn, cm, cq = core.combine_mean_var(n, mean, m2, axis=0)
    assert cn.shape == (1, 1, 5)
    np.testing.assert_array_equal(cn[0], want[0])
    np.testing.assert_allclose(cm[0], want[1], rtol=1e-13, equal_nan=True)
    np.testing.assert_allclose(cq[0], want[2], rtol=1e-10, atol=1e-12, equal_nan=True)
    # the same partials on two reduced axes (C order) and through the dask reduction step
    if n_parts % 2 == 0:
        n2, m_2, q2 = (a.reshape((2, n_parts // 2) + a.shape[1:]) for a in (n, mean, m2))
        cn2, cm2, cq2 = core.combine_mean_var(n2, m_2, q2, axis=(0, 1))
        np.testing.assert_array_equal(cn2.reshape(cn.shape), cn)
        np.testing.assert_allclose(cm2.reshape(cm.shape), cm, rtol=1e-14, equal_nan=True)
    out = core._mean_var_aggregate(np.stack([n, mean, m2]).astype(np.float64), axis=(1,), keepdims=False, ddof=1)
    np.testing.assert_array_equal(out[0], want[0])
    np.testing.assert_allclose(out[2], mo.var_of(want[0], want[2], 1), rtol=1e-10, atol=1e-12, equal_nan=True)


def test_combine_mean_var_all_empty():
    z = np.zeros((3, 2))
    nan = np.full((3, 2), np.nan)
    cn, cm, cq = core.combine_mean_var(z, nan, nan, axis=0)
    assert (cn == 0).all() and np.isnan(cm).all() and np.isnan(cq).all()


def test_argument_errors_come_before_any_device_work():
    x = np.linspace(0, 1, 10)
    e = np.linspace(0, 1, 5)
    with pytest.raises(TypeError):
        core.histogram_mean_var(x, bins=e)  # values are required
    with pytest.raises(TypeError):
        core.histogram_mean_var(x, values=None, bins=e)
    with pytest.raises(TypeError, match="complex"):
        core.histogram_mean_var(x, values=x + 1j, bins=e)
    with pytest.raises(TypeError):
        core.histogram_mean_var(x, values=x.astype("datetime64[s]"), bins=e)
    for bad in (-1, 1.0, 0.5, "1", None, True):
        with pytest.raises(ValueError, match="ddof"):
            core.histogram_mean_var(x, values=x, bins=e, ddof=bad)
    with pytest.raises(ValueError):
        core.histogram_mean_var(x, values=x, bins=[e, e])  # two bin arrays for one input
    with pytest.raises(TypeError):
        core.histogram_mean_var(x, values=x, bins=e, density=True)
    assert "histogram_mean_var" in core.__all__


def test_symbol_and_abi_version():
    assert _native.ABI_VERSION == 11
    assert "xhist_plan_execute_mean_var" in _native.EXPORTS
    header = open(os.path.join(ROOT, "include", "xhist_amd.h")).read()
    assert "#define XHIST_ABI_VERSION 11" in header and "xhist_plan_execute_mean_var(" in header
    lib = _native.load()
    assert lib.xhist_abi_version() == 11
    assert len(lib.xhist_plan_execute_mean_var.argtypes) == 10
    assert callable(getattr(_native.Plan, "execute_mean_var"))


xhx = importlib.import_module("xhistogram_amd.xarray")


def _oracle_mean_var(*args, values, bins=None, range=None, axis=None, ddof=0, block_size="auto"):
    bins = [bins] * len(args) if isinstance(bins, np.ndarray) else list(bins)
    cnt, mean, var = mo.histogram_mean_var(*args, values=values, bins=bins, axis=axis, ddof=ddof)
    return cnt, mean, var, bins


def test_xarray_wrapper_labels(monkeypatch):
    monkeypatch.setattr(core, "histogram_mean_var", _oracle_mean_var)
    rng = np.random.default_rng(7)
    dims, shape = ("t", "y", "x"), (2, 3, 40)
    coords = {d: np.arange(n) * 1.0 for d, n in zip(dims, shape)}
    T = xr.DataArray(rng.uniform(0, 1, shape), dims=dims, coords=coords, name="T", attrs={"units": "K"})
    S = xr.DataArray(rng.uniform(0, 1, shape), dims=dims, coords=coords, name="S")
    V = xr.DataArray(rng.standard_normal(shape), dims=dims, coords=coords, name="flux")
    bins = [np.linspace(0, 1, 5), np.linspace(0, 1, 4)]
    cnt, mean, var = xhx.histogram_mean_var(T, S, values=V, bins=bins, dim=("y", "x"), ddof=1)
    assert (cnt.name, mean.name, var.name) == ("flux_count", "flux_mean", "flux_var")
    assert cnt.dims == mean.dims == var.dims == ("t", "T_bin", "S_bin")
    np.testing.assert_array_equal(mean["T_bin"].values, 0.5 * (bins[0][:-1] + bins[0][1:]))
    np.testing.assert_array_equal(var["S_bin"].values, 0.5 * (bins[1][:-1] + bins[1][1:]))
    assert cnt["T_bin"].attrs == {"units": "K"}
    np.testing.assert_array_equal(mean["t"].values, coords["t"])
    want = mo.histogram_mean_var(T.values, S.values, values=V.values, bins=bins, axis=(1, 2), ddof=1)
    np.testing.assert_array_equal(cnt.values, want[0])
    np.testing.assert_array_equal(mean.values, want[1])
    np.testing.assert_array_equal(var.values, want[2])
    # a nameless values array, values broadcast over a dim they lack, everything reduced
    W = xr.DataArray(rng.standard_normal(shape[1:]), dims=dims[1:])
    cnt, mean, var = xhx.histogram_mean_var(T, values=W, bins=[bins[0]])
    assert (cnt.name, mean.name, var.name) == ("values_count", "values_mean", "values_var")
    assert var.dims == ("T_bin",)
    # keep_coords: a non-dimension coordinate on a kept dim survives
    c2 = dict(coords, label=(("t",), np.array([10.0, 20.0])), area=(("t", "x"), np.ones((2, 40))))
    T2 = xr.DataArray(T.values, dims=dims, coords=c2, name="T")
    kept = xhx.histogram_mean_var(T2, values=V, bins=[bins[0]], dim=("y", "x"), keep_coords=True)
    dropped = xhx.histogram_mean_var(T2, values=V, bins=[bins[0]], dim=("y", "x"))
    assert all("label" in a.coords and "area" not in a.coords for a in kept)  # (area spans a reduced dim)
    np.testing.assert_array_equal(kept[1]["label"].values, [10.0, 20.0])
    assert not any("label" in a.coords for a in dropped)
    with pytest.raises(TypeError):
        xhx.histogram_mean_var(T, values=V.values, bins=[bins[0]])
