"""histogram_weighted_quantile on the MI355X against tests/weighted_quantile_oracle.py (np.nanquantile with weights and
method="inverted_cdf" per bin), bit for bit on exactly summable weights (tests/exact_weights.py, about 30 % of them zero; zero
results compare by value): both families (the radix select of long rows, the LDS sort of short rows, on both sides of the
bound), every digitize form of the fast family in both of its passes, the generic family's three compare domains with slots in
LDS and sums in global memory, weights that send fast-shaped inputs to the generic family (stride 0, another dtype), rows / axes
/ views, row chunks of the radix scratch, groups of q values, hard data, poisoned bins, and the numpy, torch and DeviceArray
backends.  Weights with full mantissas are held to the bound derived from the any-order summation error.  Between them the cases
select every kernel of xhist_quantile_w.hip (the census of the -m gpu session holds them to that); describe() shows the path."""
import math
import os
import subprocess

import numpy as np
import pytest

import exact_weights as xw
import weighted_quantile_oracle as wqo

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BEFORE_ONE = float(np.nextafter(1.0, 0.0))
QS = (0.0, 1.0, 0.5, [0.1, 0.25, 0.5, 0.75, 0.9], [1e-300, BEFORE_ONE, 1.0 / 3.0])


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from xhistogram_amd import _native

    if _native.device_count() < 1:
        pytest.skip("no MI355X visible")


DESCS = []


@pytest.fixture(autouse=True)
def _record_describe(monkeypatch):
    """the describe() line of the plan after every execute_quantile_weighted, for the path assertions"""
    from xhistogram_amd import _native

    orig = _native.Plan.execute_quantile_weighted

    def wrapped(self, *a, **kw):
        orig(self, *a, **kw)
        DESCS.append(self.describe())

    monkeypatch.setattr(_native.Plan, "execute_quantile_weighted", wrapped)
    DESCS.clear()
    yield


def _core():
    from xhistogram_amd import core

    return core


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _assert_same(got, want, what=""):
    """bit for bit, zero results by value (numpy keeps the input order of -0.0 and +0.0, the library orders -0.0 < +0.0)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape, (got.dtype, got.shape, want.shape, what)
    xw.assert_bits_equal(np.where(got == 0, 0.0, got), np.where(want == 0, 0.0, want), what)


def _check(args, values, weights, bins, q=0.5, axis=None, path=(), wdt=np.float64):
    got, edges = _core().histogram_weighted_quantile(*args, values=values, weights=weights, q=q, bins=bins, axis=axis)
    want, counts = wqo.histogram_weighted_quantile(*[_np(a) for a in args], values=_np(values), weights=_np(weights), q=q,
                                                   bins=[_np(e) for e in edges], axis=axis, return_counts=True)
    xw.assert_summable(counts, wdt)
    _assert_same(_np(got), want, "q=%r %s" % (q, DESCS[-1:] if DESCS else ""))
    for p in path:
        assert DESCS and p in DESCS[-1], (p, DESCS[-1:] if DESCS else None)
    return got


def _inside(edges, n, rng):
    """n samples spread over the edges' range, some on the edges themselves"""
    e = np.asarray(edges, np.float64)
    x = rng.uniform(e[0], e[-1], n)
    on = rng.random(n) < 0.05
    x[on] = e[rng.integers(0, len(e), on.sum())]
    return x


def _weights(rng, shape, dt=np.float64, zeros=0.3):
    """exactly summable weights of `dt`, about `zeros` of them 0"""
    w = xw.f32(rng, shape) if np.dtype(dt) == np.float32 else xw.f64(rng, shape).astype(dt)
    w[rng.random(shape) < zeros] = 0
    return w


def _case(rng, edges, n, sdt=np.float64, vdt=np.float64, wdt=None, shape=None):
    """samples inside the edges (2 % outside, 1 % NaN), values with ties, +-0, +-inf and 1 % NaN, exact weights with zeros"""
    shape = shape or (n,)
    sdts = sdt if isinstance(sdt, (list, tuple)) else [sdt] * len(edges)
    xs = []
    for e, dt in zip(edges, sdts):
        x = _inside(e, int(np.prod(shape)), rng).reshape(shape)
        if np.dtype(dt).kind == "f":
            x[rng.random(shape) < 0.02] = np.asarray(e, np.float64)[-1] + 1.0
            x[rng.random(shape) < 0.01] = np.nan
        xs.append(x.astype(dt))
    v = np.round(rng.standard_normal(shape) * 4.0, 1)
    sp = rng.random(shape)
    v[sp < 0.01] = -0.0
    v[(sp >= 0.01) & (sp < 0.015)] = np.inf
    v[(sp >= 0.015) & (sp < 0.02)] = -np.inf
    if np.dtype(vdt).kind == "f":
        v[(sp >= 0.02) & (sp < 0.03)] = np.nan
        v = v.astype(vdt)
    else:
        v = np.nan_to_num(v, posinf=7.0, neginf=-7.0).astype(vdt)
    return xs, v, _weights(rng, shape, wdt or np.float64)


def _cuda(a):
    return torch.as_tensor(a).cuda()


LIN = np.linspace(-2.0, 3.0, 101)
TWO = np.sort(np.r_[np.linspace(-2.0, 3.0, 81), 0.0001])  # one bucket with two edges: the two-edge scan
L5 = np.linspace(-2.0, 3.0, 5)
LONG = 6000  # columns of a radix-family row (the short-row family takes rows of at most 2048)


# ---- 1. the fast family: every digitize form in both passes -------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["one", "two"])
@pytest.mark.parametrize("D", [1, 2])
def test_fast_table_forms(dt, kind, D):
    rng = np.random.default_rng(10 * D + (dt == np.float32) + 3 * (kind == "two"))
    first = LIN if kind == "one" else TWO
    edges = [first] if D == 1 else [first, L5]
    xs, v, w = _case(rng, edges, 3 * LONG, sdt=dt, vdt=dt, wdt=dt)
    scan = 1 if kind == "one" else 2
    for q in (0.5, [0.1, 0.25, 0.5, 0.75, 0.9]):
        _check([_cuda(x) for x in xs], _cuda(v), _cuda(w), edges, q=q, wdt=dt,
               path=("family=radix", "window=fast/lds", "digits=fast/lds", "scan=%d/%d" % (scan, scan)))
    # several rows, one kept axis
    xr_, vr, wr = _case(rng, edges, 0, sdt=dt, vdt=dt, wdt=dt, shape=(3, LONG))
    _check([_cuda(x) for x in xr_], _cuda(vr), _cuda(wr), edges, q=[0.25, 0.75], axis=1, wdt=dt, path=("family=radix", "window=fast"))


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("D", [1, 2])
def test_fast_arith_forms(dt, D):
    """arithmetic edges whose tables do not fit LDS next to the slots: 1070 bins (the digit pass: 152-byte slots at d = 4 take
    162 640 of the 163 776 bytes) and 6800 bins (the window pass: 24-byte slots; the digits then sum in global memory)"""
    rng = np.random.default_rng(40 + D + (dt == np.float32))
    e1070 = [np.linspace(-1.0, 2.0, 1071)] if D == 1 else [np.linspace(-1.0, 2.0, 3), np.linspace(-1.0, 2.0, 536)]
    xs, v, w = _case(rng, e1070, 8 * LONG, sdt=dt, vdt=dt, wdt=dt)
    _check([_cuda(x) for x in xs], _cuda(v), _cuda(w), e1070, q=0.5, wdt=dt, path=("family=radix", "digits=fast/lds", "scan=", "/5", "d=4"))
    e6800 = [np.linspace(-1.0, 2.0, 6801)] if D == 1 else [np.linspace(-1.0, 2.0, 5), np.linspace(-1.0, 2.0, 1701)]
    xs, v, w = _case(rng, e6800, 8 * LONG, sdt=dt, vdt=dt, wdt=dt)
    _check([_cuda(x) for x in xs], _cuda(v), _cuda(w), e6800, q=0.75, wdt=dt,
           path=("family=radix", "window=fast/lds", "scan=5/", "digits=generic/global"))


# ---- 2. the generic family: compare domains, LDS and global homes -----------------------------------------------------------
@pytest.mark.parametrize("dom", ["f64", "i64", "mixed"])
def test_generic_domains_lds_and_global(dom):
    rng = np.random.default_rng(50 + ["f64", "i64", "mixed"].index(dom))
    if dom == "f64":  # float64 samples, float32 values: the generic family in the float64 domain
        small, big = [LIN], [np.linspace(-2.0, 3.0, 1025)] * 2
        sdt, vdt = np.float64, np.float32
    elif dom == "i64":
        small = [np.arange(0, 2000, 17, dtype=np.int64)]
        big = [np.arange(0, 2050, 2, dtype=np.int64), np.arange(0, 1025, dtype=np.int64)]
        sdt, vdt = np.int64, np.float64
    else:
        small, big = [np.linspace(-2.0, 3.0, 41), np.arange(0, 100, 9, dtype=np.int64)], [np.linspace(-2.0, 3.0, 1025), np.arange(0, 1025, dtype=np.int64)]
        sdt, vdt = [np.float32, np.int64], np.int32
    xs, v, w = _case(rng, small, 2 * LONG, sdt=sdt, vdt=vdt)
    _check(xs, v, w, small, q=[0.1, 0.5, 0.9], path=("family=radix", "window=generic/lds", "digits=generic/lds"))
    # 1024 x 1024 bins: records and sums in global memory
    xs, v, w = _case(rng, big, 2 * LONG, sdt=sdt, vdt=vdt)
    _check(xs, v, w, big, q=0.5, path=("family=radix", "window=generic/global", "digits=generic/global"))
    # the short-row family in the same domain
    xs, v, w = _case(rng, small, 0, sdt=sdt, vdt=vdt, shape=(7, 900))
    _check(xs, v, w, small, q=[0.25, 0.75], axis=1, path=("family=short",))


def test_datetime_samples():
    rng = np.random.default_rng(60)
    te = np.arange(np.datetime64("2020-01-01"), np.datetime64("2021-02-01"), np.timedelta64(10, "D")).astype("datetime64[s]")
    t = te[0] + (rng.uniform(0, 1, 2 * LONG) * (te[-1] - te[0]).astype(np.int64)).astype("timedelta64[s]")
    v = np.round(rng.standard_normal(2 * LONG), 2)
    _check([t], v, _weights(rng, 2 * LONG), [te], q=[0.1, 0.5, 0.9], path=("family=radix", "cmp=1"))


def test_weights_that_take_the_generic_family():
    """samples and values the fast family would take, with weights it does not: a cell area broadcast along the reduced axis
    (column stride 0), and weights of another dtype (float32 next to float64 samples, int32 counts)"""
    rng = np.random.default_rng(65)
    x = rng.uniform(-2.2, 3.2, (4, LONG))
    v = np.round(rng.standard_normal((4, LONG)), 1)
    # the same data with weights of the sample dtype: the fast family
    _check([_cuda(x)], _cuda(v), _cuda(_weights(rng, (4, LONG))), [LIN], q=0.5, axis=1, path=("window=fast/lds", "digits=fast/lds"))
    per_row = _weights(rng, (4, 1), zeros=0.0)
    _check([_cuda(x)], _cuda(v), _cuda(per_row), [LIN], q=[0.25, 0.5], axis=1, path=("window=generic/lds", "digits=generic/lds"))
    _check([_cuda(x)], _cuda(v), _cuda(_weights(rng, (4, LONG), np.float32)), [LIN], q=0.5, axis=1, wdt=np.float32,
           path=("window=generic/lds", "digits=generic/lds"))
    wi = rng.integers(0, 4, (4, LONG)).astype(np.int32)
    _check([_cuda(x)], _cuda(v), _cuda(wi), [LIN], q=[0.1, 0.9], axis=1, path=("window=generic/lds", "digits=generic/lds"))
    # a (lat, lon) weight broadcast over rows (row stride 0, unit column stride) stays fast
    area = _weights(rng, (LONG,))
    _check([_cuda(x)], _cuda(v), _cuda(area), [LIN], q=0.5, axis=1, path=("window=fast/lds", "digits=fast/lds"))


# ---- 3. hard data, every q, both families ------------------------------------------------------------------------------------
def _hard(n_cols, rng):
    """one row of n_cols samples over 10 bins of [0, 10): bin 0 every value equal, bin 1 one value, bin 2 two, bin 3 empty,
    bin 4 +-0 mixed, bin 5 +-inf with finite values, bin 6 values 1 + k ulp, bin 7 keys sharing 52 leading bits, bin 8 heavy
    ties, bin 9 random with zero weights on its smallest and largest values; NaN values everywhere, NaN and out-of-range
    samples"""
    x = np.empty(n_cols)
    v = np.empty(n_cols)
    rest = n_cols - 3
    per = rest // 7
    layout = [(0, per), (1, 1), (2, 2), (4, per), (5, per), (6, per), (7, per), (8, per), (9, rest - 6 * per)]
    i = 0
    for b, k in layout:
        x[i:i + k] = b + rng.uniform(0.0, 0.999, k)
        if b == 0:
            v[i:i + k] = 2.5
        elif b == 1:
            v[i:i + k] = -3.0
        elif b == 2:
            v[i:i + k] = [np.inf, np.inf]
        elif b == 4:
            v[i:i + k] = np.where(rng.random(k) < 0.5, -0.0, 0.0)
        elif b == 5:
            v[i:i + k] = rng.choice([-np.inf, np.inf, 1.0, -2.0], k)
        elif b == 6:
            v[i:i + k] = np.nextafter(1.0, 2.0) ** rng.integers(0, 9, k)
        elif b == 7:
            v[i:i + k] = (np.float64(1.5).view(np.uint64) + rng.integers(0, 1 << 11, k).astype(np.uint64)).view(np.float64)
        elif b == 8:
            v[i:i + k] = rng.integers(-2, 3, k).astype(np.float64)
        else:
            v[i:i + k] = rng.standard_normal(k)
        i += k
    w = _weights(rng, n_cols)
    w[0] = 0.75  # (bin 0 keeps a positive weight)
    w[per] = 0.75  # bin 1's one value
    in9 = np.flatnonzero(x >= 9)
    order = in9[np.argsort(v[in9])]
    w[order[:5]] = 0.0
    w[order[-5:]] = 0.0
    nanv = rng.random(n_cols) < 0.03
    nanv[:per + 3] = False
    v[nanv & (x >= 3)] = np.nan
    x[rng.random(n_cols) < 0.02] = 11.0
    x[rng.random(n_cols) < 0.01] = np.nan
    p = rng.permutation(n_cols)
    return x[p], v[p], w[p]


@pytest.mark.parametrize("n_cols,family", [(LONG, "radix"), (2000, "short")])
def test_hard_data_every_q(n_cols, family):
    rng = np.random.default_rng(70 + n_cols)
    x, v, w = _hard(n_cols, rng)
    e = np.arange(11.0)
    for q in QS:
        _check([_cuda(x)], _cuda(v), _cuda(w), [e], q=q, path=("family=" + family,))
    # the cdf's own steps, hit exactly: q = C / W of some values of bin 9
    xn, vn, wn = x.copy(), v.copy(), w.copy()
    in9 = (xn >= 9) & (xn < 10) & ~np.isnan(vn)
    o = np.argsort(vn[in9], kind="stable")
    cdf = np.cumsum(wn[in9][o])
    cdf = cdf / cdf[-1]
    _check([_cuda(x)], _cuda(v), _cuda(w), [e], q=cdf[[7, len(cdf) // 3, len(cdf) // 2, -8]], path=("family=" + family,))
    # float32 values and weights of the same data
    _check([_cuda(x.astype(np.float32))], _cuda(v.astype(np.float32)), _cuda(_weights(rng, n_cols, np.float32)), [e], q=[0.0, 0.5, 1.0],
           wdt=np.float32, path=("family=" + family,))


@pytest.mark.parametrize("n_cols,family", [(LONG, "radix"), (1500, "short")])
def test_all_values_equal_empty_bins_and_bins_of_zero_weight(n_cols, family):
    rng = np.random.default_rng(80)
    x = rng.uniform(0, 4, n_cols)
    e = np.linspace(0, 8, 9)  # bins 4..7 empty
    w = _weights(rng, n_cols)
    w[(x >= 2) & (x < 3)] = 0.0  # bin 2: values, but no weight
    for v in (np.full(n_cols, 7.25), np.full(n_cols, -0.0), np.full(n_cols, np.nan), rng.standard_normal(n_cols)):
        got = _check([x], v, w, [e], q=[0.0, 0.5, 1.0], path=("family=" + family,))
        assert np.isnan(got[:, 2]).all() and np.isnan(got[:, 4:]).all()


def test_poisoned_bins():
    """a NaN weight and a negative weight, each in a bin of its own: those bins are NaN, their neighbours are unchanged; a NaN
    value with a huge weight contributes nothing; an infinite weight makes W infinite, hence NaN"""
    rng = np.random.default_rng(85)
    for n_cols, family in ((LONG, "radix"), (1800, "short")):
        x = rng.uniform(0, 10, n_cols)
        v = np.round(rng.standard_normal(n_cols), 1)
        w = _weights(rng, n_cols)
        e = np.arange(11.0)
        q = [0.1, 0.5, 0.9]
        clean = _np(_check([_cuda(x)], _cuda(v), _cuda(w), [e], q=q, path=("family=" + family,)))
        assert not np.isnan(clean).any()
        w2, v2 = w.copy(), v.copy()
        w2[np.flatnonzero((x >= 2) & (x < 3))[0]] = np.nan
        w2[np.flatnonzero((x >= 5) & (x < 6))[0]] = -0.25
        w2[np.flatnonzero((x >= 8) & (x < 9))[0]] = np.inf
        i = np.flatnonzero((x >= 6) & (x < 7))[0]
        v2[i], w2[i] = np.nan, 1e300
        got = _np(_check([_cuda(x)], _cuda(v2), _cuda(w2), [e], q=q, path=("family=" + family,)))
        for b in (2, 5, 8):
            assert np.isnan(got[:, b]).all()
        rest = [b for b in range(10) if b not in (2, 5, 6, 8)]
        np.testing.assert_array_equal(got[:, rest], clean[:, rest])
        assert not np.isnan(got[:, 6]).any()


# ---- 4. rows, axes, grouped rows, broadcast values, the bound, row chunks -----------------------------------------------------
def test_rows_axes_and_views():
    rng = np.random.default_rng(90)
    x = rng.uniform(-2.2, 3.2, (3, LONG, 4))
    v = np.round(rng.standard_normal((3, LONG, 4)), 1)
    w = _weights(rng, (3, LONG, 4))
    _check([_cuda(x)], _cuda(v), _cuda(w), [LIN], q=[0.25, 0.5], axis=1, path=("family=radix",))  # a middle axis: grouped rows
    _check([_cuda(x)], _cuda(v), _cuda(w), [LIN], q=0.5, axis=(0, 1), path=("family=radix",))
    _check([x], v, w, [LIN], q=0.9, axis=None, path=("family=radix",))
    # a leading (time) axis: the short-row family, several rows per workgroup; weights of full shape, then (lat, lon) weights
    xt = rng.uniform(-2.2, 3.2, (365, 12, 30)).astype(np.float32)
    vt = np.round(rng.standard_normal((365, 12, 30)), 1).astype(np.float32)
    wt = _weights(rng, (365, 12, 30), np.float32)
    e50 = [np.linspace(-2, 3, 51)]
    _check([_cuda(xt)], _cuda(vt), _cuda(wt), e50, q=[0.1, 0.5, 0.9], axis=0, wdt=np.float32, path=("family=short", "rows_per_wg=5"))
    _check([_cuda(xt)], _cuda(vt), _cuda(wt[0]), e50, q=0.5, axis=0, wdt=np.float32, path=("family=short",))
    # values and weights broadcast along the rows
    vb = np.round(rng.standard_normal(LONG), 1)
    _check([_cuda(x[:, :, 0])], _cuda(vb), _cuda(w[0, :, 0]), [LIN], q=0.5, axis=1, path=("family=radix",))
    # a strided view of the weights
    _check([_cuda(x[:, :, 0])], _cuda(v[:, :, 1]), _cuda(w)[:, :, 2], [LIN], q=0.5, axis=1, path=("family=radix",))


@pytest.mark.parametrize("n_cols,family", [(2048, "short"), (2049, "radix")])
def test_short_row_bound(n_cols, family):
    rng = np.random.default_rng(100 + n_cols)
    x = rng.uniform(-2.2, 3.2, (5, n_cols))
    v = np.round(rng.standard_normal((5, n_cols)), 2)
    w = _weights(rng, (5, n_cols))
    _check([_cuda(x)], _cuda(v), _cuda(w), [LIN], q=[0.0, 0.1, 0.5, 0.9, 1.0], axis=1, path=("family=" + family,))


def test_row_chunks():
    """9000 rows of 4200 values, 100 bins, two quantiles: the radix scratch (344 bytes per (row, bin): two targets at d = 4) takes
    two chunks of 7803 rows; the rows at the chunk border and at the ends against the oracle, the others by the histogram's
    counts"""
    rng = np.random.default_rng(110)
    x = rng.uniform(-2.2, 3.2, (9000, 4200)).astype(np.float32)
    v = np.round(rng.standard_normal((9000, 4200)), 1).astype(np.float32)
    w = _weights(rng, (9000, 4200), np.float32, zeros=0.1)
    got, _ = _core().histogram_weighted_quantile(_cuda(x), values=_cuda(v), weights=_cuda(w), q=[0.25, 0.5], bins=[LIN], axis=1)
    assert "family=radix" in DESCS[-1] and "group=2" in DESCS[-1] and "chunks=2 " in DESCS[-1], DESCS[-1]
    g = _np(got)
    for r0 in (0, 7753, 8900):
        want = wqo.histogram_weighted_quantile(x[r0:r0 + 100], values=v[r0:r0 + 100], weights=w[r0:r0 + 100], q=[0.25, 0.5], bins=[LIN],
                                               axis=1)
        _assert_same(g[:, r0:r0 + 100], want, "rows %d.." % r0)
    wsum, _ = _core().histogram(_cuda(x), weights=_cuda(w.astype(np.float64)), bins=[LIN], axis=1)
    np.testing.assert_array_equal(np.isnan(g[0]), _np(wsum) == 0)


# ---- 5. many q values: groups of targets ------------------------------------------------------------------------------------
def test_many_q_groups():
    rng = np.random.default_rng(120)
    x = rng.uniform(-2.2, 3.2, 3 * LONG)
    v = np.round(rng.standard_normal(3 * LONG), 2)
    w = _weights(rng, 3 * LONG)
    q = np.linspace(0, 1, 11)
    _check([_cuda(x)], _cuda(v), _cuda(w), [LIN], q=q, path=("family=radix",))
    assert int(DESCS[-1].split("groups=")[1].split()[0]) >= 2
    _check([_cuda(x[:2000])], _cuda(v[:2000]), _cuda(w[:2000]), [LIN], q=q, path=("family=short", "groups=2"))


# ---- 6. weights with full mantissas: the derived bound ------------------------------------------------------------------------
@pytest.mark.parametrize("n_cols,family", [(40000, "radix"), (2048, "short")])
def test_full_mantissa_weights_within_the_summation_bound(n_cols, family):
    """For every (row, bin, q), with L = sum w[v < r], U = sum w[v <= r] and W by math.fsum: L / W < q + tol and
    U / W >= q - tol, tol = 2 gamma(n_b) + 2^-51 (the any-order summation bound once for C and once for W, plus the roundings
    of the division and of the comparison), and r is a value of the bin with positive weight.  No bin is left out."""
    rng = np.random.default_rng(140 + n_cols)
    rows = 3
    x = rng.uniform(-2.2, 3.2, (rows, n_cols))
    v = np.round(rng.standard_normal((rows, n_cols)), 2)
    w = rng.random((rows, n_cols))
    w[rng.random((rows, n_cols)) < 0.2] = 0.0
    qs = [0.0, 0.1, 1.0 / 3.0, 0.5, 0.9, BEFORE_ONE, 1.0]
    got, _ = _core().histogram_weighted_quantile(_cuda(x), values=_cuda(v), weights=_cuda(w), q=qs, bins=[LIN], axis=1)
    assert "family=" + family in DESCS[-1], DESCS[-1]
    g = _np(got)
    code = np.digitize(x, LIN, right=False) - 1
    code[x == LIN[-1]] = 99
    checked = 0
    for r in range(rows):
        for b in range(100):
            inb = code[r] == b
            vb, wb = v[r][inb], w[r][inb]
            if vb.size == 0 or not (wb > 0).any():
                assert np.isnan(g[:, r, b]).all(), (r, b)
                continue
            W = math.fsum(wb)
            tol = 2.0 * float(xw.gamma(vb.size)) + 2.0 ** -51
            for i, q in enumerate(qs):
                res = g[i, r, b]
                print("row %d bin %d q %r: result %r" % (r, b, q, res)) if checked < 3 else None
                at = vb == res
                assert at.any() and (wb[at] > 0).any(), (r, b, q, res)
                L = math.fsum(wb[vb < res])
                U = math.fsum(wb[vb <= res])
                assert L / W < q + tol and U / W >= q - tol, (r, b, q, res, L / W, U / W, tol)
                checked += 1
    assert checked >= rows * 90 * len(qs)


# ---- 7. backends --------------------------------------------------------------------------------------------------------------
def test_backends():
    from xhistogram_amd import core
    from xhistogram_amd.devicearray import DeviceArray

    rng = np.random.default_rng(130)
    x = rng.uniform(-2.2, 3.2, (4, LONG))
    v = np.round(rng.standard_normal(x.shape), 1)
    w = _weights(rng, x.shape)
    kw = dict(q=[0.25, 0.75], bins=[LIN], axis=1)
    a, ea = core.histogram_weighted_quantile(x, values=v, weights=w, **kw)
    b, _ = core.histogram_weighted_quantile(_cuda(x), values=_cuda(v), weights=_cuda(w), **kw)
    c, _ = core.histogram_weighted_quantile(DeviceArray.from_numpy(x), values=DeviceArray.from_numpy(v), weights=DeviceArray.from_numpy(w), **kw)
    assert isinstance(a, np.ndarray) and isinstance(c, np.ndarray) and b.is_cuda and b.dtype == torch.float64
    assert a.shape == (2, 4, 100)
    np.testing.assert_array_equal(_np(b), a)
    np.testing.assert_array_equal(c, a)
    _assert_same(a, wqo.histogram_weighted_quantile(x, values=v, weights=w, **kw))
    m, _ = core.histogram_weighted_quantile(x, values=v, weights=w, q=0.5, bins=[LIN], axis=1)
    assert m.shape == (4, 100)
    # torch on a side stream: asynchronous, the result follows the stream's order
    s = torch.cuda.Stream()
    xc, vc, wc = _cuda(x), _cuda(v), _cuda(w)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        t, _ = core.histogram_weighted_quantile(xc, values=vc, weights=wc, q=0.5, bins=[LIN], axis=1)
    s.synchronize()
    np.testing.assert_array_equal(_np(t), m)
    # int bins: the edges of the unweighted histogram; unit weights give the unweighted inverted_cdf
    r, e2 = core.histogram_weighted_quantile(x, values=v, weights=np.ones(x.shape[1]), q=0.5, bins=20)
    np.testing.assert_array_equal(e2[0], np.histogram_bin_edges(x, bins=20))
    _assert_same(r, wqo.histogram_weighted_quantile(x, values=v, weights=np.ones(x.shape), q=0.5, bins=e2))


# ---- 8. dask ------------------------------------------------------------------------------------------------------------------
PY39 = "/opt/conda/bin/python3.9"
SCRIPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "weighted_quantile_dask_script.py")


def _have_dask_python():
    return os.path.exists(PY39) and subprocess.run([PY39, "-c", "import dask.array, numpy"], capture_output=True).returncode == 0


@pytest.mark.skipif(not _have_dask_python(), reason="no interpreter with dask in this image")
def test_dask_blocks_complete_along_the_reduced_axes():
    env = dict(os.environ)
    sys_cxx = "/usr/lib/x86_64-linux-gnu/libstdc++.so.6"  # (as tests/test_dask_branch.py: conda's libstdc++ is older)
    if os.path.exists(sys_cxx):
        env["LD_PRELOAD"] = (sys_cxx + ":" + env["LD_PRELOAD"]) if env.get("LD_PRELOAD") else sys_cxx
    r = subprocess.run([PY39, "-W", "ignore", SCRIPT], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "WEIGHTED-QUANTILE-DASK-OK" in r.stdout
