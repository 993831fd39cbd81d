"""histogram_mean_var with weights on an MI355X: the weighted passes (mvw_* kernels of xhist_meanvar_w.hip) against the weighted
oracle (tests/meanvar_weighted_oracle.py).

On exactly summable data (values on values_exact.grid, integer weights 0..7) W and the mean are checked bit for bit, and so is
the variance where W is a power of two up to 2^8; elsewhere it stays within the oracle's float64 bound.  Every case also checks
its describe() line against test_gpu_values_census.predict("mean_var", ...): the weighted slots have the unweighted sizes, so
the choice is the same, with the fast family given up when the weights' dtype or layout disqualifies it.

The cases here have one copy of their slots or are checked against an rtol where they have more, one row chunk, and no case on
an LDS border, with tables read through L2, in a datetime or uint64 domain, or with weights laid out otherwise than the values
beyond test_fast_fallback_and_views.  Those launch variants, each held to the exact oracle, are the cases of
tests/test_gpu_values_census_streams.py, which borrows check_exact, as_unweighted_line, int_weights and run_w from here."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import meanvar_weighted_oracle as mwo
import values_exact as vx
from test_gpu_census import edges_of
from test_gpu_parity import _plan_for, xh  # noqa: F401  (xh: the module fixture)
from test_gpu_values_census import (FORM_EDGES, HOME_BINS, _cus, _domain_edges, assert_variant, float_samples, grid_values,
                                    int_samples, predict)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F64, F32 = np.float64, np.float32
PY39 = "/opt/conda/bin/python3.9"
SCRIPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "meanvar_weighted_dask_script.py")


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def run_w(core, xs, v, w, edges, axis=1, ddof=0):
    wsum, mean, var, _ = core.histogram_mean_var(*xs, values=v, weights=w, bins=edges, axis=axis, ddof=ddof)
    torch.cuda.synchronize()
    return _np(wsum), _np(mean), _np(var)


def as_unweighted_line(desc):
    """a weighted describe() line in the unweighted line's words, for test_gpu_values_census.assert_variant"""
    assert desc.startswith("mean_var_w pass1=mvw_sum_"), desc
    assert " pass2=mvw_dev_" in desc, desc
    return desc.replace("mean_var_w ", "mean_var ").replace("mvw_", "mv_")


def check_exact(xl, edges, vl, wl, got, ddof=0, what=""):
    """W and mean bit for bit; var bit for bit where W is a power of two <= 2^8, else within the oracle's bound"""
    W, mean, m2 = mwo.mean_var_w_rows(xl, edges, vl, wl, exact=True)
    gW, gm, gv = (np.asarray(a).reshape(W.shape) for a in got)
    np.testing.assert_array_equal(gW, W, err_msg=what)
    np.testing.assert_array_equal(gm, mean, err_msg=what)
    var, lim, pow2 = mwo.var_bound(W, m2, mwo.m2_bound(xl, edges, vl, wl, mean), ddof)
    np.testing.assert_array_equal(gv[pow2], var[pow2], err_msg=what)
    rest = (W > ddof) & ~pow2
    assert np.all(np.abs(gv[rest] - var[rest]) <= lim[rest]), what
    np.testing.assert_array_equal(np.isnan(gv), np.isnan(var), err_msg=what)
    return W


def int_weights(rng, shape, dt):
    return rng.integers(0, 8, shape).astype(dt)


# ---------------------------------------------------------------------------------------------------------------------
# every fast form: f32 / f64 x D 1 / 2 x SCAN 1 / 2 / arith
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("sdt", ["f64", "f32"])
@pytest.mark.parametrize("form", ["k1", "k2", "arith"])
def test_fast_forms(xh, form, sdt, D):
    (kind, nb1, nb2), fine, arith = FORM_EDGES[form]
    st = F64 if sdt == "f64" else F32
    if form == "arith" and st == F32 and D == 1:
        nb1 = (6_000,)  # (float32 fine tables are smaller: at 5000 bins they still fit next to the slots)
    seed = 700 + 10 * ["k1", "k2", "arith"].index(form) + 2 * D + (st == F32)
    edges = [edges_of(kind, nb, seed=seed + d) for d, nb in enumerate(nb1 if D == 1 else nb2)]
    rng = np.random.default_rng(seed)
    xs = float_samples(edges, 3, 20_011, st, seed)
    v = grid_values(rng, xs[0].shape, st)
    w = int_weights(rng, xs[0].shape, st)
    xd = [_dev(x) for x in xs]
    got = run_w(xh, xd, _dev(v), _dev(w), edges)
    plan = _plan_for(xh, xd, edges)
    want = predict("mean_var", _cus(), edges, 0, st, st, 3, 20_011, fine, arith)
    assert (want["scan"] == 5) == (form == "arith"), want
    assert_variant(as_unweighted_line(plan.describe()), want)
    check_exact(xs, edges, v, w, got, what="%s %s D=%d" % (form, sdt, D))
    # w == 1: W is the count, the mean the unweighted call's bit for bit, and so is the variance where both are exact (counts
    # 2^j <= 2^8); elsewhere both calls round their sums of d*d, in orders of their own
    ones = run_w(xh, xd, _dev(v), _dev(np.ones_like(w)), edges, ddof=1)
    cnt, mean, var, _ = xh.histogram_mean_var(*xd, values=_dev(v), bins=edges, axis=1, ddof=1)
    cnt, var = _np(cnt), _np(var)
    np.testing.assert_array_equal(ones[0], cnt.astype(F64))
    np.testing.assert_array_equal(ones[1], _np(mean))
    lg = np.log2(np.maximum(cnt, 1))
    pow2 = (cnt > 1) & (cnt <= mwo.POW2_EXACT) & (lg == np.round(lg))
    np.testing.assert_array_equal(ones[2][pow2], var[pow2])
    np.testing.assert_allclose(ones[2], var, rtol=1e-12, atol=0)


def test_frequency_weights_equal_repeated_samples(xh):
    """integer weights m in 0..7 == the unweighted call on np.repeat'ed samples and values"""
    rng = np.random.default_rng(11)
    edges = [np.linspace(-3, 3, 41)]
    x = rng.standard_normal(50_000)
    v = vx.grid(rng, x.shape)
    m = rng.integers(0, 8, x.shape)
    W, mean, var, _ = xh.histogram_mean_var(x, values=v, weights=m, bins=edges)
    cnt, mean_r, var_r, _ = xh.histogram_mean_var(np.repeat(x, m), values=np.repeat(v, m), bins=edges)
    np.testing.assert_array_equal(W, cnt.astype(F64))
    np.testing.assert_array_equal(mean, mean_r)
    lg = np.log2(np.maximum(cnt, 1))
    pow2 = (cnt > 0) & (cnt <= mwo.POW2_EXACT) & (lg == np.round(lg))
    np.testing.assert_array_equal(var[pow2], var_r[pow2])
    check_exact([x[None, :]], edges, v[None, :], m[None, :].astype(F64), (W[None], mean[None], var[None]))


# ---------------------------------------------------------------------------------------------------------------------
# the generic family: CMP 0 / 1 / 3, slots in LDS or sums in global memory
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("home", ["lds", "global_tables_lds"])
@pytest.mark.parametrize("dom", ["f64", "i64", "mixed"])
def test_generic_domain_and_home(xh, dom, home):
    rng = np.random.default_rng(80 + 3 * ["f64", "i64", "mixed"].index(dom) + ["lds", "global_tables_lds"].index(home))
    nb = HOME_BINS[home] if dom != "mixed" else max(2, HOME_BINS[home] // 6)
    edges = _domain_edges(dom, nb, rng)
    n_rows, n_cols = 2, 20_011
    cmp = {"f64": 0, "i64": 1, "mixed": 3}[dom]
    xs = []
    for d, e in enumerate(edges):
        if np.asarray(e).dtype.kind == "f":
            xs += float_samples([e], n_rows, n_cols, F64, 17 + d)
        else:
            xs += int_samples([e], n_rows, n_cols, None, 17 + d)
    v = grid_values(rng, (n_rows, n_cols), F32 if dom == "f64" else F64)
    w = int_weights(rng, (n_rows, n_cols), np.int32 if dom == "i64" else F64)
    xd = [_dev(x) for x in xs]
    got = run_w(xh, xd, _dev(v), _dev(w), edges)
    plan = _plan_for(xh, xd, edges)
    want = predict("mean_var", _cus(), edges, cmp, xs[0].dtype, v.dtype, n_rows, n_cols, False)
    got_v = assert_variant(as_unweighted_line(plan.describe()), want)
    assert got_v["slots"] == ("lds" if home == "lds" else "global")
    check_exact(xs, edges, v, w, got, what="%s %s" % (dom, home))


def test_1024_x_1024_bins(xh):
    rng = np.random.default_rng(5)
    edges = [np.linspace(-4, 4, 1025)] * 2
    xs = [rng.standard_normal((1, 1 << 20)) for _ in range(2)]
    v = vx.grid(rng, xs[0].shape)
    w = int_weights(rng, xs[0].shape, F64)
    xd = [_dev(x) for x in xs]
    got = run_w(xh, xd, _dev(v), _dev(w), edges)
    assert "slots=global" in _plan_for(xh, xd, edges).describe()
    check_exact(xs, edges, v, w, got, what="1024x1024")


# ---------------------------------------------------------------------------------------------------------------------
# row shapes, views and the fast family's fallback
# ---------------------------------------------------------------------------------------------------------------------
def _case(xh, xs_host, v_host, w_host, edges, axis, xs_dev, v_dev, w_dev, family, ddof=0):
    """one N-D call against the exact oracle, and the family its describe() names"""
    got = xh.histogram_mean_var(*xs_dev, values=v_dev, weights=w_dev, bins=edges, axis=axis, ddof=ddof)[:3]
    torch.cuda.synchronize()
    desc = _plan_for(xh, xs_dev, edges).describe()
    assert family is None or ("pass1=mvw_sum_%s " % family) in desc, desc
    want = mwo.histogram_mean_var_w(*xs_host, values=v_host, weights=w_host, bins=edges, axis=axis, ddof=ddof, exact=True)
    np.testing.assert_array_equal(_np(got[0]), want[0])
    np.testing.assert_array_equal(_np(got[1]), want[1])
    np.testing.assert_allclose(_np(got[2]), want[2], rtol=1e-13, atol=0)


def test_fast_fallback_and_views(xh):
    rng = np.random.default_rng(21)
    edges = [np.linspace(-3, 3, 61)]
    x = rng.standard_normal((4, 30_001))
    v = vx.grid(rng, x.shape)
    w = int_weights(rng, x.shape, F64)
    xd, vd = _dev(x), _dev(v)
    _case(xh, [x], v, w, edges, 1, [xd], vd, _dev(w), "fast")
    _case(xh, [x], v, w.astype(F32), edges, 1, [xd], vd, _dev(w.astype(F32)), "generic")  # weights of another dtype
    wide = _dev(np.repeat(w, 2, axis=1))[:, ::2]  # column stride 2 (the view layer may hand over a copy: either family)
    _case(xh, [x], v, w, edges, 1, [xd], vd, wide, None)
    wcol = int_weights(rng, (4, 1), F64)  # column stride 0: a weight per row
    _case(xh, [x], v, wcol, edges, 1, [xd], vd, _dev(wcol).expand(4, 30_001), "generic")
    # unaligned row starts: every row begins one element past a 16-byte boundary
    xb, vb, wb = (np.concatenate([np.zeros((4, 1)), a], axis=1) for a in (x, v, w))
    _case(xh, [x], v, w, edges, 1, [_dev(xb)[:, 1:]], _dev(vb)[:, 1:], _dev(wb)[:, 1:], "fast")
    # mixed dtypes of values and weights
    _case(xh, [x], v.astype(F32), w.astype(np.int16), edges, 1, [xd], _dev(v.astype(F32)), _dev(w.astype(np.int16)), "generic")


def test_broadcast_cell_area_and_grouped_rows(xh):
    """(lat, lon) cell areas over (time, lat, lon): row stride 0 keeps the fast family; grouped rows over lat"""
    rng = np.random.default_rng(31)
    edges = [np.linspace(-3, 3, 51)]
    x = rng.standard_normal((6, 40, 72)).astype(F32)
    v = vx.grid(rng, x.shape, F32)
    area = rng.integers(1, 8, (40, 72)).astype(F32)
    xd, vd, ad = _dev(x), _dev(v), _dev(area)
    _case(xh, [x], v, area, edges, (1, 2), [xd], vd, ad.expand(6, 40, 72), "fast")
    _case(xh, [x], v, area, edges, (1,), [xd], vd, ad.expand(6, 40, 72), "generic")  # grouped rows: (time, LAT, lon)


# ---------------------------------------------------------------------------------------------------------------------
# random data, cancellation, special values
# ---------------------------------------------------------------------------------------------------------------------
def _volume_weights(rng, shape):
    return 10.0 ** rng.uniform(6, 12, shape)


def test_random_against_fsum(xh):
    rng = np.random.default_rng(41)
    edges = [np.linspace(-3, 3, 31)]
    x = rng.standard_normal((2, 200_003))
    v = 3.0 + rng.standard_normal(x.shape)
    w = _volume_weights(rng, x.shape)
    gW, gm, gv = run_w(xh, [_dev(x)], _dev(v), _dev(w), edges)
    W, mean, m2 = mwo.mean_var_w_rows([x], edges, v, w, exact=False)
    ok = W > 0
    n = int(x.size)
    np.testing.assert_allclose(gW[ok], W[ok], rtol=mwo.gamma(n), atol=0)
    # mean: S and W each within g(n) relative (all terms of W positive; |S| <= sum |w v|)
    sabs = mwo.mean_var_w_rows([x], edges, np.abs(v), w, exact=False)[1] * W
    assert np.all(np.abs(gm[ok] - mean[ok]) <= 4 * mwo.gamma(n + 2) * sabs[ok] / W[ok])
    # M2 of the kernel's own mean: the exact M2 of its terms, within the oracle's bound
    exact_m2 = np.zeros_like(W)
    ok2, flat, _ = mwo._flat_bins([x], edges)
    flat = (flat + np.arange(2)[:, None] * 30)[ok2]
    vv, ww = v[ok2], w[ok2]
    d = vv - gm.reshape(-1)[flat]
    for k in np.unique(flat):
        sel = flat == k
        wd = ww[sel] * d[sel]
        q, s = math.fsum(wd * d[sel]), math.fsum(wd)
        exact_m2.reshape(-1)[k] = max(0.0, q - s * s / W.reshape(-1)[k])
    b = mwo.m2_bound([x], edges, v, w, gm)
    assert np.all(np.abs(gv[ok] * W[ok] - exact_m2[ok]) <= b[ok] + 4 * mwo.U * exact_m2[ok])
    np.testing.assert_allclose(gv[ok], (m2 / W)[ok], rtol=1e-9)


def test_cancellation_large_offset(xh):
    """values at 1e8 with a spread of 1: the two-pass variance keeps its digits; sum(w v^2) / W - mean^2 loses them"""
    rng = np.random.default_rng(51)
    edges = [np.linspace(-3, 3, 21)]
    x = rng.standard_normal(400_000)
    v = 1e8 + rng.standard_normal(x.shape)
    w = _volume_weights(rng, x.shape)
    _, _, var = run_w(xh, [_dev(x)], _dev(v), _dev(w), edges, axis=None)
    W, mean, m2 = mwo.mean_var_w_rows([x[None]], edges, v[None], w[None], exact=False)
    want = (m2 / W)[0]
    np.testing.assert_allclose(var, want, rtol=1e-6)
    h = xh.histogram_two_weights(x, weights=(w * v * v, w * v), bins=edges)
    hw = xh.histogram(x, weights=w, bins=edges)[0]
    naive = h[0] / hw - (h[1] / hw) ** 2
    assert np.max(np.abs(naive - want)) > 0.1, np.max(np.abs(naive - want))


def test_special_values(xh):
    edges = [np.array([0.0, 1.0, 2.0, 3.0, 4.0])]
    x = np.array([0.5, 0.5, 1.5, 1.5, 2.5, 2.5, 3.5, 3.5, 9.0])
    v = np.array([1.0, np.nan, 2.0, 4.0, 1.0, 3.0, 5.0, 7.0, 1.0])
    w = np.array([2.0, np.nan, 1.0, np.nan, 0.0, 0.0, 1.0, 1.0, 5.0])
    W, mean, var, _ = xh.histogram_mean_var(x, values=v, weights=w, bins=edges, ddof=1)
    # bin 0: the NaN value is ignored with its NaN weight; bin 1: a NaN weight -> NaN; bin 2: zero weights; bin 3: W = 2 > ddof
    np.testing.assert_array_equal(W, [2.0, np.nan, 0.0, 2.0])
    np.testing.assert_array_equal(mean, [1.0, np.nan, np.nan, 6.0])
    np.testing.assert_array_equal(var, [0.0, np.nan, np.nan, 2.0])


def test_special_values_var(xh):
    edges = [np.array([0.0, 1.0, 2.0, 3.0])]
    x = np.array([0.5, 1.5, 1.5, 2.5])
    v = np.array([3.0, 1.0, 5.0, 2.0])
    w = np.array([1.0, 0.5, 1.5, 0.0])
    W, mean, var, _ = xh.histogram_mean_var(x, values=v, weights=w, bins=edges, ddof=1)
    np.testing.assert_array_equal(W, [1.0, 2.0, 0.0])
    np.testing.assert_array_equal(mean, [3.0, 4.0, np.nan])
    np.testing.assert_array_equal(var, [np.nan, 6.0, np.nan])  # W <= ddof; M2 = 0.5*9 + 1.5*1 = 6, 6 / (2 - 1); W == 0
    for xe, ve, we in ((np.zeros(0), np.zeros(0), np.zeros(0)), (np.full(5, 9.0), np.ones(5), np.ones(5))):
        W, mean, var, _ = xh.histogram_mean_var(xe, values=ve, weights=we, bins=edges)
        np.testing.assert_array_equal(W, np.zeros(3))
        assert np.isnan(mean).all() and np.isnan(var).all()


def test_tutorial_identity(xh):
    """the volume-weighted mean oxygen of each T-S class == histogram(masked, weights=O2 dV) / histogram(masked, weights=dV)"""
    rng = np.random.default_rng(61)
    T = rng.uniform(-2, 32, (12, 30, 40))
    S = rng.uniform(31, 38, (12, 30, 40))
    o2 = vx.grid(rng, T.shape)
    o2[rng.random(T.shape) < 0.3] = np.nan
    dvol = rng.integers(1, 8, (1, 30, 40)).astype(F64)  # broadcast over depth
    bins = [np.arange(-2, 32, 0.1), np.arange(31, 38, 0.025)]
    W, mean, var, _ = xh.histogram_mean_var(T, S, values=o2, weights=dvol, bins=bins)
    keep = ~np.isnan(o2)
    Tm, Sm = np.where(keep, T, np.nan), np.where(keep, S, np.nan)
    dv = np.broadcast_to(dvol, T.shape)
    hv = xh.histogram(Tm, Sm, weights=dv, bins=bins)[0]
    ho = xh.histogram(Tm, Sm, weights=np.where(keep, o2, 0.0) * dv, bins=bins)[0]
    np.testing.assert_array_equal(W, hv)
    with np.errstate(invalid="ignore", divide="ignore"):
        np.testing.assert_array_equal(mean, np.where(hv != 0, ho / hv, np.nan))


# ---------------------------------------------------------------------------------------------------------------------
# backends
# ---------------------------------------------------------------------------------------------------------------------
def _delay():
    """tens of milliseconds of GPU work on the current stream"""
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(50_000_000)
        return
    a = torch.randn(4096, 4096, device="cuda")
    for _ in range(20):
        a = torch.tanh(a @ a)


def test_backends(xh):
    from xhistogram_amd.devicearray import DeviceArray

    rng = np.random.default_rng(71)
    edges = [np.linspace(-3, 3, 25)]
    x = rng.standard_normal((5, 3000))
    v = vx.grid(rng, x.shape)
    w = int_weights(rng, (1, 3000), F64)
    want = mwo.histogram_mean_var_w(x, values=v, weights=w, bins=edges, axis=1, exact=True)
    got_np = xh.histogram_mean_var(x, values=v, weights=w, bins=edges, axis=1)
    for a, b in zip(got_np[:2], want[:2]):
        assert isinstance(a, np.ndarray) and a.dtype == F64
        np.testing.assert_array_equal(a, b)
    # torch: issued on the current stream.  The values and weights the call reads are written on a side stream `s` behind a
    # long wait, over NaN placeholders; a call issued on any other stream (torch's are non-blocking, so the null stream too)
    # would read the placeholders and give NaN in every bin
    xd, v_src, w_src = _dev(x), _dev(v), _dev(w)
    vd = torch.full(v_src.shape, float("nan"), dtype=torch.float64, device="cuda")
    wd = torch.full(w_src.shape, float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        _delay()
        vd.copy_(v_src)
        wd.copy_(w_src)
        got_t = xh.histogram_mean_var(xd, values=vd, weights=wd, bins=edges, axis=1)
        done = torch.cuda.Event()
        done.record(s)
    done.synchronize()
    for a, b in zip(got_t[:2], want[:2]):
        assert a.device.type == "cuda" and a.dtype == torch.float64
        np.testing.assert_array_equal(_np(a), b)
    got_d = xh.histogram_mean_var(DeviceArray.from_numpy(x, 0), values=DeviceArray.from_numpy(v, 0), weights=DeviceArray.from_numpy(w, 0),
                                  bins=edges, axis=1)
    for a, b in zip(got_d[:2], want[:2]):
        np.testing.assert_array_equal(np.asarray(a), b)
    np.testing.assert_allclose(got_d[2], want[2], rtol=1e-13)


def test_xarray(xh):
    try:
        import xarray as xr
    except ImportError:  # the small double of tests/doubles, as tests/test_xarray_wrapper.py uses it
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "doubles"))
        import xarray as xr
    from xhistogram_amd import xarray as xhx

    rng = np.random.default_rng(81)
    coords = {"time": np.arange(4), "lat": np.arange(6) * 1.5, "lon": np.arange(8) * 2.0}
    T = xr.DataArray(rng.uniform(0, 10, (4, 6, 8)), dims=("time", "lat", "lon"), name="T", coords=coords)
    o2 = xr.DataArray(vx.grid(rng, (4, 6, 8)), dims=("time", "lat", "lon"), name="o2", coords=coords)
    area = xr.DataArray(rng.integers(1, 8, (6, 8)).astype(F64), dims=("lat", "lon"), coords={"lat": coords["lat"], "lon": coords["lon"]})
    edges = np.linspace(0, 10, 6)
    W, mean, var = xhx.histogram_mean_var(T, values=o2, weights=area, bins=[edges], dim=["lat", "lon"], keep_coords=True)
    assert (W.name, mean.name, var.name) == ("o2_sum_of_weights", "o2_mean", "o2_var")
    assert tuple(W.dims) == ("time", "T_bin")
    np.testing.assert_array_equal(np.asarray(W.coords["time"].values), coords["time"])
    np.testing.assert_array_equal(np.asarray(W.coords["T_bin"].values), 0.5 * (edges[:-1] + edges[1:]))
    want = mwo.histogram_mean_var_w(T.values, values=o2.values, weights=area.values[None], bins=[edges], axis=(1, 2), exact=True)
    np.testing.assert_array_equal(np.asarray(W.values), want[0])
    np.testing.assert_array_equal(np.asarray(mean.values), want[1])
    cnt = xhx.histogram_mean_var(T, values=o2, bins=[edges], dim=["lat", "lon"])[0]
    assert cnt.name == "o2_count"


def test_dask_chunked_equals_unchunked():
    env = dict(os.environ)
    sys_cxx = "/usr/lib/x86_64-linux-gnu/libstdc++.so.6"  # (as tests/test_dask_branch.py: conda's libstdc++ is older)
    if os.path.exists(sys_cxx):
        env["LD_PRELOAD"] = (sys_cxx + ":" + env["LD_PRELOAD"]) if env.get("LD_PRELOAD") else sys_cxx
    r = subprocess.run([PY39, "-W", "ignore", SCRIPT], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "MEANVAR-W-DASK-OK" in r.stdout


# ---------------------------------------------------------------------------------------------------------------------
# size: 2^28 float64 samples against a torch restatement
# ---------------------------------------------------------------------------------------------------------------------
def test_2_28_samples(xh):
    n = 1 << 28
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
    v = 5.0 + torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
    w = torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
    edges = np.linspace(-4, 4, 101)
    W, mean, var, _ = xh.histogram_mean_var(x, values=v, weights=w, bins=[edges])
    e = torch.as_tensor(edges, device="cuda")
    b = torch.bucketize(x, e, right=True) - 1
    b = torch.where(x == e[-1], torch.full_like(b, 99), b)
    ok = (b >= 0) & (b < 100)
    b, vv, ww = b[ok], v[ok], w[ok]
    rW = torch.zeros(100, dtype=torch.float64, device="cuda").index_add_(0, b, ww)
    rS = torch.zeros(100, dtype=torch.float64, device="cuda").index_add_(0, b, ww * vv)
    rm = rS / rW
    d = vv - rm[b]
    rQ = torch.zeros(100, dtype=torch.float64, device="cuda").index_add_(0, b, ww * d * d)
    np.testing.assert_allclose(_np(W), _np(rW), rtol=1e-10)
    np.testing.assert_allclose(_np(mean), _np(rm), rtol=1e-10)
    np.testing.assert_allclose(_np(var), _np(rQ / rW), rtol=1e-8)
