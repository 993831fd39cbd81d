"""histogram_argextrema without a GPU: the oracle against a per-bin loop and against np.nanargmin / np.nanargmax, the
-0.0 / +0.0 rule, the column order of the reduced axes, argument errors raised before any device work, the C ABI's symbol,
the stats tables, and the xarray wrapper's names and unravelling (compute swapped for the oracle)."""
import importlib
import os
import sys

import numpy as np
import pytest

import argextrema_oracle as ao
import extrema_oracle as eo
from xhistogram_amd import _native, core

try:
    import xarray as xr  # noqa: F401
except ImportError:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "doubles"))
    import xarray as xr  # the double

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECIAL = np.array([-np.inf, -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 2.2e-308, 1.0, 1e300, np.inf])


def _same(got, want):
    """bit for bit, NaN where NaN"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64))


def _inputs(rng, n, D, ties):
    edges = [np.sort(rng.uniform(-2, 2, int(rng.integers(2, 9)))) for _ in range(D)]
    samples = []
    for e in edges:
        x = rng.uniform(-2.5, 2.5, n)
        on_edge = rng.random(n) < 0.2
        x[on_edge] = e[rng.integers(0, len(e), int(on_edge.sum()))]
        x[rng.random(n) < 0.05] = np.nan
        samples.append(x)
    v = rng.integers(-2, 3, n).astype(np.float64) if ties else rng.standard_normal(n)
    pick = rng.random(n) < 0.25
    v[pick] = SPECIAL[rng.integers(0, len(SPECIAL), int(pick.sum()))]
    v[rng.random(n) < 0.1] = np.nan
    return samples, edges, v


@pytest.mark.parametrize("seed", range(8))
def test_oracle_matches_the_per_bin_loop(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 300))
    samples, edges, v = _inputs(rng, n, 1 + seed % 2, ties=seed % 4 < 2)
    v[:5] = [0.0, -0.0, 0.0, np.nan, -0.0][: min(5, n)]
    got = ao.argextrema_rows([s[None, :] for s in samples], edges, v[None, :])
    want = ao.definitional(samples, edges, v)
    np.testing.assert_array_equal(got[0][0], want[0])
    np.testing.assert_array_equal(got[1][0], want[1])
    _same(got[2][0], want[2])
    _same(got[3][0], want[3])
    # ... and its values are histogram_extrema's
    lo, hi = eo.extrema_rows([s[None, :] for s in samples], edges, v[None, :])
    _same(got[2], lo)
    _same(got[3], hi)


@pytest.mark.parametrize("seed", range(4))
def test_oracle_matches_nanargmin_per_bin_without_signed_zeros(seed):
    rng = np.random.default_rng(20 + seed)
    n = 500
    e = np.linspace(-2, 2, 7)
    x = rng.uniform(-2.3, 2.3, n)
    v = rng.integers(-3, 4, n).astype(np.float64) + 0.5  # many ties, no zero of either sign
    v[rng.random(n) < 0.1] = np.nan
    amin, amax, lo, hi = (o[0] for o in ao.argextrema_rows([x[None]], [e], v[None]))
    code = np.searchsorted(e, x, side="right") - 1
    code[x == e[-1]] = len(e) - 2
    for b in range(len(e) - 1):
        pos = np.flatnonzero((code == b) & (x >= e[0]) & (x <= e[-1]) & ~np.isnan(v))
        if not pos.size:
            assert amin[b] == amax[b] == -1 and np.isnan(lo[b]) and np.isnan(hi[b])
            continue
        assert amin[b] == pos[np.nanargmin(v[pos])] and amax[b] == pos[np.nanargmax(v[pos])]
        assert lo[b] == v[amin[b]] and hi[b] == v[amax[b]]


def test_zeros_follow_the_total_order():
    e = np.array([0.0, 1.0, 2.0])
    x = np.array([0.5, 0.5, 0.5, 0.5, 1.5, 1.5])
    v = np.array([0.0, -0.0, 0.0, -0.0, -0.0, -0.0])
    amin, amax, lo, hi = (o[0] for o in ao.argextrema_rows([x[None]], [e], v[None]))
    # +0.0 first, -0.0 after it: argmin is the first -0.0, argmax the first +0.0 (np.nanargmin would say 0 for both)
    np.testing.assert_array_equal(amin, [1, 4])
    np.testing.assert_array_equal(amax, [0, 4])
    assert np.signbit(lo[0]) and not np.signbit(hi[0]) and np.signbit(hi[1])


def test_positions_do_not_depend_on_the_order_axis_lists():
    rng = np.random.default_rng(3)
    x = rng.uniform(-1.2, 1.2, (4, 3, 5))
    v = rng.integers(0, 3, x.shape).astype(np.float64)
    e = [np.linspace(-1, 1, 4)]
    a = ao.histogram_argextrema(x, values=v, bins=e, axis=(0, 2))
    b = ao.histogram_argextrema(x, values=v, bins=e, axis=(2, 0))
    for p, q in zip(a, b):
        np.testing.assert_array_equal(p, q)
    # the position is the C-order flat index over (axis 0, axis 2)
    for j in range(3):
        sub = v[:, j, :]
        for b_ in range(3):
            if a[0][j, b_] >= 0:
                i0, i2 = np.unravel_index(a[0][j, b_], (4, 5))
                assert sub[i0, i2] == a[2][j, b_]
    # axis=None: the flat index into the array
    full = ao.histogram_argextrema(x, values=v, bins=e)
    ok = full[0] >= 0
    np.testing.assert_array_equal(v.reshape(-1)[full[0][ok]], full[2][ok])


def test_value_views_can_insist_on_ascending_axes():
    """_value_views(ordered=True) keeps the reduced axes ascending; the default may permute them"""
    import inspect

    sig = inspect.signature(core._value_views)
    assert sig.parameters["ordered"].default is False and sig.parameters["ordered"].kind is inspect.Parameter.KEYWORD_ONLY
    a = np.asfortranarray(np.zeros((3, 4)))
    assert core._reduced_order(a, [0, 1]) == [1, 0]  # (what other statistics may do to a Fortran-ordered array)
    assert core._collapse(a, None, True, [0, 1]) is None  # ascending order: no single strided dimension, hence the copy


def test_argument_errors_come_before_any_device_work():
    x = np.linspace(0, 1, 10)
    e = np.linspace(0, 1, 5)
    with pytest.raises(TypeError):
        core.histogram_argextrema(x, bins=e)  # values are required
    with pytest.raises(TypeError):
        core.histogram_argextrema(x, values=None, bins=e)
    with pytest.raises(TypeError, match="complex"):
        core.histogram_argextrema(x, values=x + 1j, bins=e)
    with pytest.raises(TypeError):
        core.histogram_argextrema(x, values=x, bins=e, density=True)
    with pytest.raises(TypeError):
        core.histogram_argextrema(x, values=x, bins=e, weights=x)
    with pytest.raises(TypeError):
        core.histogram_argextrema(x, values=x.astype("datetime64[s]"), bins=e)
    assert "histogram_argextrema" in core.__all__
    assert not hasattr(core, "combine_argextrema")


class _Chunked:
    """just enough of a dask array for the front of the call: its chunks along each axis"""
    def __init__(self, shape, chunks):
        self.shape, self.ndim, self.chunks, self.dtype = shape, len(shape), chunks, np.dtype(np.float64)


def test_dask_with_a_chunked_reduced_axis_is_refused_before_any_compute(monkeypatch):
    """the front of the call stubbed to hand over chunked arrays (this interpreter has no dask; with the real thing:
    tests/argextrema_dask_script.py): nothing is uploaded, nothing computed"""
    monkeypatch.setattr(core, "_values_blockwise", lambda *a, **k: pytest.fail("a graph was built"))
    monkeypatch.setattr(core, "_upload_host", lambda *a, **k: pytest.fail("device work"))
    arr = _Chunked((4, 6), ((2, 2), (3, 3)))
    monkeypatch.setattr(core, "_values_call", lambda *a, **k: ("dask", [arr, arr], None, [np.linspace(0, 1, 3)], [1], (1,)))
    with pytest.raises(ValueError, match="positions of several chunks cannot be merged: rechunk the reduced axes"):
        core.histogram_argextrema(arr, values=arr, bins=[np.linspace(0, 1, 3)], axis=1)


def test_symbol_and_abi_version():
    assert _native.ABI_VERSION == 11
    assert "xhist_plan_execute_argextrema" in _native.EXPORTS
    header = open(os.path.join(ROOT, "include", "xhist_amd.h")).read()
    assert "#define XHIST_ABI_VERSION 11" in header and "xhist_plan_execute_argextrema(" in header
    lib = _native.load()
    assert lib.xhist_abi_version() == 11
    assert len(lib.xhist_plan_execute_argextrema.argtypes) == 9
    assert callable(getattr(_native.Plan, "execute_argextrema"))


def test_the_statistic_is_an_entry_of_the_stats_table():
    """(vmin, vmax, argmin, argmax): the two positions int64, the columns in ascending axis order, and no dask step, since
    positions of several chunks are not merged"""
    st = core._VALUE_STATS["argextrema"]
    assert (st.k, st.ints, st.extras, st.method, st.ptrs) == (4, (2, 3), 0, "execute_argextrema", (0, 2))
    assert st.ordered is True and st.reduce is None
    assert [name for name, s in core._VALUE_STATS.items() if s.ordered] == ["argextrema"]


xhx = importlib.import_module("xhistogram_amd.xarray")


def _oracle_argextrema(*args, values, bins=None, range=None, axis=None, block_size="auto"):
    bins = [bins] * len(args) if isinstance(bins, np.ndarray) else list(bins)
    return ao.histogram_argextrema(*args, values=values, bins=bins, axis=axis) + (bins,)


def test_xarray_wrapper_names_and_unravelling(monkeypatch):
    monkeypatch.setattr(core, "histogram_argextrema", _oracle_argextrema)
    rng = np.random.default_rng(7)
    dims, shape = ("t", "y", "x"), (2, 3, 40)
    coords = {d: np.arange(n) * 1.0 for d, n in zip(dims, shape)}
    T = xr.DataArray(rng.uniform(0, 1, shape), dims=dims, coords=coords, name="T", attrs={"units": "K"})
    S = xr.DataArray(rng.uniform(0, 1, shape), dims=dims, coords=coords, name="S")
    V = xr.DataArray(rng.integers(0, 4, shape).astype(np.float64), dims=dims, coords=coords, name="flux")
    bins = [np.linspace(0, 1, 5), np.linspace(0, 1, 4)]
    out = xhx.histogram_argextrema(T, S, values=V, bins=bins, dim=("x", "y"))  # (listed unsorted)
    assert sorted(out) == sorted(["flux_min", "flux_max", "flux_argmin_y", "flux_argmin_x", "flux_argmax_y", "flux_argmax_x"])
    for name, da in out.items():
        assert da.name == name and da.dims == ("t", "T_bin", "S_bin")
        np.testing.assert_array_equal(da["T_bin"].values, 0.5 * (bins[0][:-1] + bins[0][1:]))
        np.testing.assert_array_equal(da["t"].values, coords["t"])
    assert out["flux_min"]["T_bin"].attrs == {"units": "K"}
    want = ao.histogram_argextrema(T.values, S.values, values=V.values, bins=bins, axis=(1, 2))
    _same(out["flux_min"].values, want[2])
    _same(out["flux_max"].values, want[3])
    for which, flat in (("argmin", want[0]), ("argmax", want[1])):
        iy, ix = out["flux_%s_y" % which].values, out["flux_%s_x" % which].values
        assert iy.dtype == np.int64 and ix.dtype == np.int64
        empty = flat < 0
        np.testing.assert_array_equal(iy[empty], -1)
        np.testing.assert_array_equal(ix[empty], -1)
        np.testing.assert_array_equal(iy[~empty] * shape[2] + ix[~empty], flat[~empty])
        # what isel takes: the value at (t, iy, ix) is the bin's extreme
        t_idx = np.broadcast_to(np.arange(shape[0])[:, None, None], flat.shape)
        vals = V.values[t_idx[~empty], iy[~empty], ix[~empty]]
        np.testing.assert_array_equal(vals, (want[2] if which == "argmin" else want[3])[~empty])
    # a nameless values array broadcast over a dim it lacks, everything reduced: three index arrays per extreme, one empty bin
    W = xr.DataArray(rng.standard_normal(shape[1:]), dims=dims[1:])
    e1 = np.array([0.0, 0.5, 1.0, 2.0])  # (nothing above 1: the last bin is empty)
    out = xhx.histogram_argextrema(T, values=W, bins=[e1])
    assert sorted(out) == sorted(["values_min", "values_max"] + ["values_%s_%s" % (w, d) for w in ("argmin", "argmax") for d in dims])
    want = ao.histogram_argextrema(T.values, values=np.broadcast_to(W.values, shape), bins=[e1])
    assert want[0][-1] == -1
    for which, flat in (("argmin", want[0]), ("argmax", want[1])):
        got = [out["values_%s_%s" % (which, d)].values for d in dims]
        assert all(g.shape == (3,) and g.dtype == np.int64 for g in got)
        assert [int(g[-1]) for g in got] == [-1, -1, -1]
        np.testing.assert_array_equal(np.ravel_multi_index([g[:-1] for g in got], shape), flat[:-1])
    assert "histogram_argextrema" in xhx.__all__
    with pytest.raises(TypeError):
        xhx.histogram_argextrema(T, values=V.values, bins=[bins[0]])
