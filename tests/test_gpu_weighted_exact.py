"""Every weighted kernel bit for bit: weights whose float64 sums are exact in any order (tests/exact_weights.py), so the GPU's
result must carry the bits np.bincount's does — no tolerance.  A weight rounded to float32, a float32 accumulator, a packed
record of less than 24 stored bits, one weighted sample lost or counted twice: each changes bins that the 1e-6 comparisons of
the rest of the suite cannot see.

(a) the census cover's weighted cases and the census's other families, (b) weights of both signs over the partitioned homes,
(c) the exchange mode at C5's shape, (d) the public API's paths that reshape or transform weights, (e) subnormal weights."""
import os
import sys

import numpy as np
import pytest

import exact_weights as ew
from oracle import oracle_np as onp
from test_gpu_census import (F32, F64, HOMES, _ST, _WT, _cases, _fresh, _generic_integer_domains, _int64_domain, _key,
                             _mixed_dtypes, _run_case, _selected_keys, _small_samples, _two_weights, edges_of)
from test_gpu_parity import _dev, _plan_for, _run, xh  # noqa: F401  (xh: the module fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _case_plan(core, st, case, seed):
    """the plan a _run_case call used (same edges: edges_of is deterministic in its seed)"""
    edges = [edges_of(case["kind"], nb, seed=seed + d) for d, nb in enumerate(case["nbs"])]
    cmp_domain, conv, _ = core._compare_domain([np.dtype(st)] * len(edges), edges)
    return core._get_plan(conv, cmp_domain, 0)


# ---------------------------------------------------------------------------------------------------------------------
# (a) the census cover's weighted cases, and the families of _run_general
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("wt", ["f32", "f64"])
@pytest.mark.parametrize("st", ["f64", "f32"])
def test_census_cover_weighted_cases_bitwise(xh, st, wt, D):
    """the weighted cases of tests/golden/census_cases.json (every home, every digitize form, float32 and float64 weights): the
    same samples, edges and plan parameters as test_gpu_census, exactly summable weights, bit for bit"""
    keep = _selected_keys()
    n = 0
    for i, case in enumerate(_cases(_ST[st], _WT[wt], D)):
        if keep is not None and _key(st, wt, D, case) not in keep:
            continue
        _run_case(xh, _ST[st], _WT[wt], D, case, seed=1000 * D + 17 * i, make_w=ew.make(_WT[wt]))
        n += 1
    assert n > 0


@pytest.mark.parametrize("dtype", ["int32", "int64", "int16", "uint8", "float16"])
def test_small_samples_bitwise(xh, dtype):
    _small_samples(xh, dtype, make_w=ew.make(F64))


def test_int64_domain_and_generic_bitwise(xh):
    _int64_domain(xh, make_w=ew.make(F64))
    _generic_integer_domains(xh, make_w=ew.make(F64, signs="both"))


@pytest.mark.parametrize("D", [1, 2, 3])
def test_mixed_dtypes_bitwise(xh, D):
    _mixed_dtypes(xh, D, make_w=ew.make(F64))


@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("wt", ["f32", "f64"])
@pytest.mark.parametrize("st", ["f64", "f32"])
def test_two_weights_bitwise(xh, st, wt, D):
    _two_weights(xh, st, wt, D, make_w=ew.make(_WT[wt], signs="both"))


# ---------------------------------------------------------------------------------------------------------------------
# (b) both signs over the partitioned homes: the exact-record passes (and the packed attempt discarded inside one call)
# ---------------------------------------------------------------------------------------------------------------------
PARTITIONED = ("route", "route_rows", "route_spl4", "three_pass", "sliced", "global_big")


@pytest.mark.parametrize("wt", ["f32", "f64"])
@pytest.mark.parametrize("home", PARTITIONED)
def test_partitioned_homes_both_signs_bitwise(xh, home, wt):
    n = 0
    for D in (1, 2, 3):
        for i, case in enumerate(_cases(F64, _WT[wt], D)):
            if case["home"] != home or case["kind"] not in ("lin", "k1") or case["params"] != HOMES[home]["params"]:
                continue
            seed = 7000 + 100 * D + i
            try:
                _run_case(xh, F64, _WT[wt], D, case, seed, make_w=ew.make(_WT[wt], signs="both"))
            finally:
                _fresh(_case_plan(xh, F64, case, seed))  # (forgets "both signs": later modules still select the packed kernels)
            n += 1
    assert n >= 3


# ---------------------------------------------------------------------------------------------------------------------
# (c) the exchange mode at C5's shape, forced
# ---------------------------------------------------------------------------------------------------------------------
C5_EDGES = [np.linspace(-4, 4, 1025), np.linspace(-4, 4, 1025)]


@pytest.mark.parametrize("n", [4, 4095, 4096, 4097, 1_000_003, 3_000_001])
def test_exchange_mode_c5_shape_bitwise(xh, n):
    """packed8 records with weights of one sign, exact12 with both: bitwise against the oracle, and bitwise between the
    exchange kernel and the classic passes"""
    rng = np.random.default_rng(900 + n % 97)
    x, y = rng.standard_normal((1, n)), rng.standard_normal((1, n))
    for signs, more, tag in (("one", {"records48": 0}, "exchange_records=packed8"), ("both", {"records48": -1}, "exchange_records=exact12")):
        w = ew.f64(rng, (1, n), signs)
        want = onp.bincount_rows([x, y], C5_EDGES, w)
        got, desc = _run(xh, [x, y], C5_EDGES, w, True, partition=1, exchange=1, **more)
        assert "exchange=forced" in desc and tag in desc, desc
        ew.assert_bits_equal(got, want, desc)
        classic, desc = _run(xh, [x, y], C5_EDGES, w, True, partition=1, exchange=-1, **more)
        assert "exchange=no" in desc, desc
        ew.assert_bits_equal(got, classic, "exchange against classic")
    if n == 1_000_003:  # both signs without asking for exact records: the packed attempt is discarded, the exact passes of the call finish it
        try:
            got, desc = _run(xh, [x, y], C5_EDGES, w, True, partition=1, exchange=1, records48=0)
        finally:  # (the plan's note of both signs arrives with the call's end: forget it after that, for the modules that follow)
            torch.cuda.synchronize()
            _plan_for(xh, [_dev(x), _dev(y)], C5_EDGES).set_param("records48", 0)
        ew.assert_bits_equal(got, want, desc)


# ---------------------------------------------------------------------------------------------------------------------
# (d) the public API's paths that reshape or transform weights
# ---------------------------------------------------------------------------------------------------------------------
def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def test_resident_fast_path_and_device_arrays(xh):
    """the headline call (1-D float64 samples, float64 weights, 100 bins: hist_fast<double, double, ...>) on torch tensors and
    on DeviceArray inputs, float32 alike, numpy in / numpy out"""
    from xhistogram_amd.devicearray import DeviceArray

    rng = np.random.default_rng(31)
    e = np.linspace(-4, 4, 101)
    for dt, mk in ((np.float64, ew.make(F64)), (np.float32, ew.make(F32)), (np.float64, ew.make(F64, signs="both"))):
        for n in (1, 4095, 1_000_003):
            x = rng.standard_normal(n).astype(dt)
            x[::997] = np.nan
            w = mk(rng, (n,))
            want, _ = onp.histogram(x, bins=e, weights=w)
            for conv in (_dev, DeviceArray.from_numpy, lambda a: a):
                got, _ = xh.histogram(conv(x), bins=e, weights=conv(w))
                ew.assert_bits_equal(_np(got), want, "%s %d %s" % (dt.__name__, n, conv))


@pytest.mark.parametrize("resident", [False, True], ids=["host", "device"])
def test_weights_broadcast_along_reduced_axes_bitwise(xh, resident):
    """weights constant along reduced axes (applied to counts), the stride-0 slab, weights already broadcast, non-adjacent
    reduced axes in two steps, and block_size chunks"""
    rng = np.random.default_rng(32)
    conv = _dev if resident else (lambda a: a)
    t = rng.standard_normal((6, 40, 700))
    t[0, 3, :5] = np.nan
    e = np.linspace(-3, 3, 31)

    def check(args, w, axis, bins=e, **kw):
        want, _ = onp.histogram(*args, bins=bins, weights=w, axis=axis)
        got, _ = xh.histogram(*[conv(a) for a in args], bins=bins, weights=conv(w), axis=axis, **kw)
        ew.assert_bits_equal(_np(got), want, "w %s axis %s %s" % (np.shape(w), axis, kw))

    w_lat = ew.f64(rng, (1, 40, 1))
    for axis in ((1, 2), None, (2,), (0, 2), (0, 1, 2)):
        check([t], w_lat, axis)
    check([t], ew.f64(rng, (6, 1, 1), "both"), (1, 2))
    check([t], ew.f64(rng, (700,)), (1, 2))
    check([t], np.broadcast_to(w_lat, t.shape), (1, 2))
    check([t, rng.standard_normal(t.shape)], w_lat, (1, 2), bins=[np.linspace(-3, 3, 9), np.linspace(-3, 3, 7)])
    if resident:
        got, _ = xh.histogram(_dev(t), bins=e, weights=_dev(w_lat).expand(t.shape), axis=(1, 2))
        ew.assert_bits_equal(_np(got), onp.histogram(t, bins=e, weights=w_lat, axis=(1, 2))[0], "expanded")
    # the slab: (lat, lon) weights against (time, lat, lon), read with stride 0 along time
    s = rng.standard_normal((48, 36, 72)).astype(np.float32)
    for w, axis in ((ew.f64(rng, (36, 72)), (1, 2)), (ew.f64(rng, (1, 36, 1), "both"), (0, 1)), (ew.f32(rng, (72,)), 2)):
        check([s], w, axis)
    # non-adjacent reduced axes: a histogram over the last block of adjacent axes, then a sum of the rest
    q = rng.standard_normal((5, 8, 6, 300)).astype(np.float32)
    for arr, axis in ((rng.standard_normal((9, 30, 700)), (0, 2)), (q, (0, 3)), (q, (1, 3)), (q, (0, 2, 3))):
        check([arr], ew.f64(rng, arr.shape, "both"), axis)
    # block_size chunks
    w = ew.f64(rng, t.shape)
    for bs in (1, 2, 5, None, "auto"):
        check([t], w, 2, block_size=bs)
        check([t], w, (1, 2), block_size=bs)


@pytest.mark.parametrize("resident", [False, True], ids=["host", "device"])
def test_two_weights_and_the_xarray_pair_bitwise(xh, resident):
    rng = np.random.default_rng(33)
    conv = _dev if resident else (lambda a: a)
    x = rng.standard_normal(700_001)
    x[::1001] = np.nan
    e = np.linspace(-4, 4, 101)
    wa, wb = ew.f64(rng, x.shape, "both"), ew.f64(rng, x.shape)
    ha, hb, _ = xh.histogram_two_weights(conv(x), bins=e, weights=(conv(wa), conv(wb)))
    ew.assert_bits_equal(_np(ha), onp.histogram(x, bins=e, weights=wa)[0], "first of the pair")
    ew.assert_bits_equal(_np(hb), onp.histogram(x, bins=e, weights=wb)[0], "second of the pair")
    t = rng.standard_normal((5, 7, 3001))
    ta, tb = ew.f64(rng, t.shape), ew.f64(rng, (1, 7, 3001), "both")
    for axis in (2, (1, 2), 0):
        ha, hb, _ = xh.histogram_two_weights(conv(t), bins=np.linspace(-3, 3, 21), weights=(conv(ta), conv(tb)), axis=axis)
        ew.assert_bits_equal(_np(ha), onp.histogram(t, bins=np.linspace(-3, 3, 21), weights=ta, axis=axis)[0], "axis %s" % (axis,))
        ew.assert_bits_equal(_np(hb), onp.histogram(t, bins=np.linspace(-3, 3, 21), weights=tb, axis=axis)[0], "axis %s" % (axis,))
    try:
        import xarray as xr
    except ImportError:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "doubles"))
        import xarray as xr  # the double tests/test_xarray_wrapper.py uses
    import importlib

    xhx = importlib.import_module("xhistogram_amd.xarray")
    s = rng.standard_normal((6, 40, 50)).astype(np.float32)
    da = xr.DataArray(conv(s), dims=["time", "lat", "lon"], name="T")
    w = ew.f64(rng, (40, 50))
    sw = ew.f64(rng, s.shape, "both")
    bins = np.linspace(-4, 4, 51)
    num, den = xhx.histogram(da, bins=[bins], dim=["lat", "lon"],
                             weights=(xr.DataArray(conv(sw), dims=["time", "lat", "lon"], name="Tw"), xr.DataArray(conv(w), dims=["lat", "lon"], name="w")))
    ew.assert_bits_equal(_np(num.values), onp.histogram(s, bins=bins, axis=(1, 2), weights=sw)[0], "xarray pair, first")
    ew.assert_bits_equal(_np(den.values), onp.histogram(s, bins=bins, axis=(1, 2), weights=np.broadcast_to(w, s.shape))[0], "xarray pair, second")


def _assert_ulps(got, want, ulps, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    diff = np.abs(got[ok] - want[ok])
    tol = ulps * np.spacing(np.abs(want[ok]))
    assert (diff <= tol).all(), "%s: %d bins beyond %d ulp, worst %.3g ulp" % (what, (diff > tol).sum(), ulps, (diff / np.maximum(tol / ulps, 5e-324)).max())


@pytest.mark.parametrize("resident", [False, True], ids=["host", "device"])
def test_density_within_two_ulp_of_the_normalised_exact_histogram(xh, resident):
    """density=True for counts and for exact weights: at most 2 ulp per bin from oracle_np.density_normalise applied to the exact
    histogram"""
    rng = np.random.default_rng(34)
    conv = _dev if resident else (lambda a: a)
    t = rng.standard_normal((6, 40, 700))
    u = rng.standard_normal(t.shape)
    e1 = np.linspace(-3, 3, 31)
    e2 = [np.linspace(-3, 3, 9), np.sort(rng.uniform(-3, 3, 12))]
    for args, bins, edges in (([t], e1, [e1]), ([t, u], e2, e2)):
        for w, axis in ((None, (1, 2)), (ew.f64(rng, t.shape), (1, 2)), (ew.f64(rng, t.shape), None), (ew.f64(rng, (1, 40, 1)), (1, 2)),
                        (ew.f64(rng, t.shape), (0, 2))):
            h, _ = onp.histogram(*args, bins=bins, weights=w, axis=axis)
            want = onp.density_normalise(h, edges)
            got, _ = xh.histogram(*[conv(a) for a in args], bins=bins, weights=None if w is None else conv(w), axis=axis, density=True)
            _assert_ulps(_np(got), want, 2, "D=%d w=%s axis=%s" % (len(args), None if w is None else w.shape, axis))


# ---------------------------------------------------------------------------------------------------------------------
# (e) subnormal weights: (2^24 + k) * 2^-1065, sums exact — does any family flush them?
#
# Measured on gfx950: no.  ds_add_f64 (LDS homes, lane copies, flat rows, the partitioned adding-up pass), global_atomic_add_f64
# (force_global, flushes into the output) and the exact records of the routing and exchange passes keep every subnormal bit.
# What does not is the PACKED record (pack48 / exch_pack_fast): it rounds the weight's bit pattern to 36 stored mantissa bits, and
# a subnormal has fewer significant bits than stored ones — (2^24 + k) * 2^-1065 keeps 18 of its 25 (relative error up to 2^-18
# per weight instead of 2^-37; below 2^-1058 a weight rounds to 0 or 2^-1058).  Weights of one sign take packed records by
# default beyond LDS; a fix would need a per-weight test in the routing and exchange passes, so those two subcases are expected
# to fail (README, accuracy).
# ---------------------------------------------------------------------------------------------------------------------
SUB = -1040
_PACKED_SUBNORMAL = pytest.mark.xfail(strict=True, reason="packed records round a subnormal weight's bit pattern to 36 stored bits: 18 of its 25 significant bits are kept")
_SUB_HOMES = {"lds": "lds", "global": "global", "lanes": "lanes", "flat_rows": "flat_rows", "partitioned_packed": "route",
              "exact_route": "route_exact"}


@pytest.mark.parametrize("family,signs", [pytest.param(f, s, marks=_PACKED_SUBNORMAL if (f, s) == ("partitioned_packed", "one") else ())
                                          for f in sorted(_SUB_HOMES) for s in ("one", "both")])
def test_subnormal_weights(xh, family, signs):
    """LDS, global, lane, flat-row, packed-record (one sign) and exact-record (both signs, or records48 = -1) homes"""
    home = _SUB_HOMES[family]
    n = 0
    for D in (1, 2):
        for i, case in enumerate(_cases(F64, F64, D)):
            if case["home"] != home or case["kind"] not in ("lin", "k1") or case["params"] != HOMES[home]["params"]:
                continue
            seed = 8000 + 100 * D + i
            try:
                _run_case(xh, F64, F64, D, case, seed, make_w=ew.make(F64, signs=signs, scale_log2=SUB))
            finally:
                _fresh(_case_plan(xh, F64, case, seed))
            n += 1
    assert n >= 2


@pytest.mark.parametrize("records", [pytest.param("packed8", marks=_PACKED_SUBNORMAL), "exact12"])
def test_subnormal_weights_exchange(xh, records):
    rng = np.random.default_rng(35)
    n = 1_000_003
    x, y = rng.standard_normal((1, n)), rng.standard_normal((1, n))
    w = ew.f64(rng, (1, n), "one" if records == "packed8" else "both", scale_log2=SUB)
    more = {"records48": 0 if records == "packed8" else -1}
    got, desc = _run(xh, [x, y], C5_EDGES, w, True, partition=1, exchange=1, **more)
    assert "exchange=forced" in desc and "exchange_records=" + records in desc, desc
    ew.assert_bits_equal(got, onp.bincount_rows([x, y], C5_EDGES, w), desc)
