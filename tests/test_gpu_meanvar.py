"""histogram_mean_var on the MI355X.  Bit for bit against tests/meanvar_oracle.py (exact mode) on data whose sums are exact in
any order — every bin holds a power-of-two number of values k * 2^-10, |k| < 2^12 — over sample and value dtypes, D = 1..3,
edge kinds, LDS and beyond-LDS homes, row shapes and views, and ddof; random data against the exactly rounded oracle;
cancellation; special values; the counting and ratio-of-histograms properties; the three in-memory backends; a 2^28-sample
case against a torch restatement; and dask in the conda interpreter.  Between them the cases select every kernel of
xhist_meanvar.hip (the census of the -m gpu session holds them to that), and describe() shows each family and home reached."""
import os
import subprocess

import numpy as np
import pytest

import meanvar_oracle as mo

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from xhistogram_amd import _native

    if _native.device_count() < 1:
        pytest.skip("no MI355X visible")


DESCS = []


@pytest.fixture(autouse=True)
def _record_describe(monkeypatch):
    """the describe() line of the plan after every execute_mean_var, for the path assertions"""
    from xhistogram_amd import _native

    orig = _native.Plan.execute_mean_var

    def wrapped(self, *a, **kw):
        orig(self, *a, **kw)
        DESCS.append(self.describe())

    monkeypatch.setattr(_native.Plan, "execute_mean_var", wrapped)
    DESCS.clear()
    yield


def _core():
    from xhistogram_amd import core

    return core


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _same(got, want):
    got, want = np.asarray(_np(got)), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.dtype.kind == "i":
        assert got.dtype == np.int64, got.dtype
        np.testing.assert_array_equal(got, want)
        return
    got, want = got.astype(np.float64), want.astype(np.float64)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64))


def _check(args, values, bins, axis=None, ddof=0, path=None, **kw):
    """bit for bit against the exact-mode oracle; `path`: substrings the describe() line must hold"""
    cnt, mean, var, edges = _core().histogram_mean_var(*args, values=values, bins=bins, axis=axis, ddof=ddof, **kw)
    want = mo.histogram_mean_var(*[_np(a) for a in args], values=_np(values), bins=[_np(e) for e in edges], axis=axis, ddof=ddof,
                                 exact=True)
    _same(cnt, want[0])
    _same(mean, want[1])
    _same(var, want[2])
    for p in path or ():
        assert DESCS and p in DESCS[-1], (p, DESCS[-1:] or None)
    return cnt, mean, var, edges


FAST = ("pass1=mv_sum_fast slots=lds", "pass2=mv_dev_fast slots=lds")
GEN_LDS = ("pass1=mv_sum_generic slots=lds", "pass2=mv_dev_generic slots=lds")
GEN_GLOBAL = ("pass1=mv_sum_generic slots=global", "pass2=mv_dev_generic slots=global")


def _inside(edges, k):
    """a point inside bin k of each edge array (float: the middle; integer / datetime: the lower edge)"""
    e = np.asarray(edges)
    if e.dtype.kind in "iuM":
        return e[k]
    return 0.5 * (e[k] + e[k + 1])


def _exact_case(rng, edges, shape_rows=None, max_log2=6, empty_frac=0.2, sdt=None, vdt=np.float64, vscale=2.0**-10,
                extra=True):
    """samples that fill every non-empty bin with 2^j values k * vscale (|k| < 2^12), shuffled, plus samples that do not count
    (outside the edges, NaN samples, NaN values).  One row of N samples, or rows x N (each row its own counts)."""
    rows = 1 if shape_rows is None else shape_rows
    nbs = [len(e) - 1 for e in edges]
    n_bins = int(np.prod(nbs))
    xs_rows, v_rows = [], []
    for _ in range(rows):
        reps = np.where(rng.random(n_bins) < empty_frac, 0, 2 ** rng.integers(0, max_log2 + 1, n_bins))
        flat = np.repeat(np.arange(n_bins), reps)
        idx = np.unravel_index(flat, nbs)
        xs = [_inside(e, i) for e, i in zip(edges, idx)]
        k = rng.integers(-4095, 4096, len(flat))
        v = k * vscale if np.dtype(vdt).kind == "f" else k
        if extra:
            m = max(8, len(flat) // 20)
            for d, e in enumerate(edges):
                e = np.asarray(e)
                if e.dtype.kind == "f":
                    out = np.where(rng.random(m) < 0.5, e[0] - 1.0, e[-1] + 1.0)
                    out[: m // 4] = np.nan
                else:
                    out = np.where(rng.random(m) < 0.5, e[0] - (e[1] - e[0]), e[-1] + (e[1] - e[0]))
                xs[d] = np.concatenate([xs[d], out])
            v = np.concatenate([v, rng.integers(-4095, 4096, m) * (vscale if np.dtype(vdt).kind == "f" else 1)])
            if np.dtype(vdt).kind == "f":  # NaN values on counted samples: dropped, the count falls
                nanv = max(4, len(flat) // 50)
                pick = rng.integers(0, n_bins, nanv)
                pidx = np.unravel_index(pick, nbs)
                for d, e in enumerate(edges):
                    xs[d] = np.concatenate([xs[d], _inside(e, pidx[d])])
                v = np.concatenate([v, np.full(nanv, np.nan)])
        perm = rng.permutation(len(v))
        xs_rows.append([x[perm] for x in xs])
        v_rows.append(v[perm].astype(vdt))
    if rows > 1:  # rows of one length: the shorter ones padded with samples past the last edge, which do not count
        n = max(len(v) for v in v_rows)
        for r in range(rows):
            k = n - len(v_rows[r])
            for d, e in enumerate(edges):
                e = np.asarray(e)
                xs_rows[r][d] = np.concatenate([xs_rows[r][d], np.full(k, e[-1] + (e[-1] - e[0]), e.dtype)])
            v_rows[r] = np.concatenate([v_rows[r], np.zeros(k, v_rows[r].dtype)])
        xs = [np.stack([r[d] for r in xs_rows]) for d in range(len(edges))]
        v = np.stack(v_rows)
    else:
        xs, v = xs_rows[0], v_rows[0]
    if sdt is not None:
        xs = [x.astype(t) for x, t in zip(xs, sdt if isinstance(sdt, (list, tuple)) else [sdt] * len(xs))]
    return xs, v


def _assert_pow2_counts(cnt):
    c = np.asarray(_np(cnt)).ravel()
    c = c[c > 0]
    assert np.all((c & (c - 1)) == 0), "the exact-data construction needs power-of-two counts"


LIN = np.linspace(-2.0, 3.0, 101)
TWO = np.sort(np.r_[np.linspace(-2.0, 3.0, 81), 0.0001])  # one bucket with two edges: the two-edge scan
L41 = np.linspace(-2.0, 3.0, 41)


# ---- 1. bit for bit on exactly summable data -----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["one", "two", "arith"])
@pytest.mark.parametrize("D", [1, 2])
def test_fast_path_forms(dt, kind, D):
    """the vector fast path: float32 / float64 samples with values of the same type, one or two inputs, every digitize form"""
    rng = np.random.default_rng(100 * (dt == np.float32) + 10 * ["one", "two", "arith"].index(kind) + D)
    if kind == "arith":  # linspace edges whose tables do not fit LDS next to the 24-byte slots: the table-free digitize
        edges = [np.linspace(-1.0, 2.0, 6801)] if D == 1 else [np.linspace(-1.0, 2.0, 4), np.linspace(-1.0, 2.0, 2251)]
        scan = "scan=5"
    else:
        edges = ([LIN] if D == 1 else [LIN, L41]) if kind == "one" else ([TWO] if D == 1 else [TWO, L41])
        scan = "scan=%d" % (1 if kind == "one" else 2)
    xs, v = _exact_case(rng, edges, max_log2=4 if kind == "arith" else 7, sdt=dt, vdt=dt)
    cnt, *_ = _check([torch.as_tensor(x).cuda() for x in xs], torch.as_tensor(v).cuda(), edges, path=FAST + (scan,))
    _assert_pow2_counts(cnt)
    # several rows, one kept axis, ddof 1
    xr_, vr = _exact_case(rng, edges, shape_rows=3, max_log2=3, sdt=dt, vdt=dt)
    _check([torch.as_tensor(x).cuda() for x in xr_], torch.as_tensor(vr).cuda(), edges, axis=1, ddof=1, path=FAST)


@pytest.mark.parametrize("sdt", [np.float64, np.float32, np.int32, "mixed"])
@pytest.mark.parametrize("vdt", [np.float64, np.float32, np.int32])
def test_dtypes(sdt, vdt):
    """sample dtypes x value dtypes through numpy inputs; a value dtype other than the samples' takes the generic family"""
    rng = np.random.default_rng(11)
    if sdt == np.int32:
        edges = [np.arange(0, 200, 7).astype(np.int32)]
        xs, v = _exact_case(rng, edges, vdt=vdt)
        xs = [x.astype(np.int32) for x in xs]
    elif sdt == "mixed":
        edges = [LIN, L41]
        xs, v = _exact_case(rng, edges, sdt=[np.float32, np.float64], vdt=vdt)
    else:
        edges = [LIN]
        xs, v = _exact_case(rng, edges, sdt=sdt, vdt=vdt)
    fast = sdt in (np.float64, np.float32) and np.dtype(vdt) == np.dtype(sdt)
    for ddof in (0, 1):
        _check(xs, v, edges, ddof=ddof, path=FAST if fast else GEN_LDS)


def test_three_inputs_and_random_edges():
    rng = np.random.default_rng(12)
    e3 = [np.linspace(-2, 3, 11), np.geomspace(0.01, 30.0, 9), np.arange(-2, 3, 0.5)]
    xs, v = _exact_case(rng, e3, sdt=[np.float32, np.float64, np.float16])
    _check(xs, v, e3, path=GEN_LDS)
    er = np.sort(rng.uniform(-2, 3, 300))  # random non-uniform edges (crowded buckets: the binary search)
    xs, v = _exact_case(rng, [er])
    _check(xs, v, [er], path=("slots=lds",))
    _check([torch.as_tensor(x).cuda() for x in xs], torch.as_tensor(v).cuda(), [er], ddof=1, path=("slots=lds",))


def test_datetime_and_per_input_domains():
    rng = np.random.default_rng(13)
    te = np.arange(np.datetime64("2020-01-01"), np.datetime64("2021-02-01"), np.timedelta64(10, "D")).astype("datetime64[s]")
    xs, v = _exact_case(rng, [te])
    _check(xs, v, [te], path=GEN_LDS)  # the int64 domain, slots in LDS
    xs, v = _exact_case(rng, [te, LIN])
    _check(xs, v, [te, LIN], path=GEN_LDS)  # per-input domains
    # beyond LDS: int64 domain and per-input domains with their sums in global memory
    big_t = (np.datetime64("2020-01-01") + np.arange(1025).astype("timedelta64[D]")).astype("datetime64[s]")
    ei = np.arange(1025, dtype=np.int64)
    xs, v = _exact_case(rng, [big_t, ei], max_log2=1, empty_frac=0.5, extra=False)
    _check(xs, v, [big_t, ei], path=GEN_GLOBAL)
    el = np.linspace(0, 1, 1025)
    xs, v = _exact_case(rng, [big_t, el], max_log2=1, empty_frac=0.5, extra=False)
    _check(xs, v, [big_t, el], path=GEN_GLOBAL)


def test_beyond_lds_1024_squared():
    """1024 x 1024 bins: the generic family with its sums in global memory, pass 2 reading the means through L2"""
    rng = np.random.default_rng(14)
    e = [np.linspace(-4, 4, 1025)] * 2
    xs, v = _exact_case(rng, e, max_log2=2, empty_frac=0.3)
    cnt, *_ = _check([torch.as_tensor(x).cuda() for x in xs], torch.as_tensor(v).cuda(), e, path=GEN_GLOBAL)
    _assert_pow2_counts(cnt)
    xs, v = _exact_case(rng, e, max_log2=2, empty_frac=0.3, sdt=np.float32, vdt=np.int32)  # integer values
    _check([torch.as_tensor(x).cuda() for x in xs], torch.as_tensor(v).cuda(), e, ddof=1, path=GEN_GLOBAL)


def _close(args, values, bins, axis=None, ddof=0):
    """against the exactly rounded oracle, for reductions whose bins hold counts that are not powers of two"""
    cnt, mean, var, edges = _core().histogram_mean_var(*args, values=values, bins=bins, axis=axis, ddof=ddof)
    want = mo.histogram_mean_var(*[_np(a) for a in args], values=_np(values), bins=[_np(e) for e in edges], axis=axis, ddof=ddof)
    np.testing.assert_array_equal(_np(cnt), want[0])
    np.testing.assert_allclose(_np(mean), want[1], rtol=1e-12, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(_np(var), want[2], rtol=1e-10, atol=1e-12, equal_nan=True)


def test_row_shapes_and_views():
    rng = np.random.default_rng(15)
    # six rows of exact data, each folded into (m, 40): reducing (1, 2) keeps the rows, every count a power of two
    xs, v = _exact_case(rng, [LIN], shape_rows=6, max_log2=3)
    m = -(-xs[0].shape[1] // 40)
    pad = m * 40 - xs[0].shape[1]
    a = np.concatenate([xs[0], np.full((6, pad), 9.0)], axis=1).reshape(6, m, 40)
    vv = np.concatenate([v, np.zeros((6, pad))], axis=1).reshape(a.shape)
    t, tv = torch.as_tensor(a).cuda(), torch.as_tensor(vv).cuda()
    _check([a], vv, [LIN], axis=(1, 2), path=FAST)
    _check([t], tv, [LIN], axis=(1, 2), ddof=1, path=FAST)
    _check([t.permute(2, 1, 0)], tv.permute(2, 1, 0), [LIN], axis=(0, 1))  # non-contiguous views, the rows last
    # strided samples and values (column stride 2): the even columns hold the rows, the odd ones samples that do not count
    a2 = np.stack([a, np.full(a.shape, -9.0)], axis=3).reshape(6, m, 80)
    v2 = np.stack([vv, np.ones(vv.shape)], axis=3).reshape(a2.shape)
    t2, tv2 = torch.as_tensor(a2).cuda(), torch.as_tensor(v2).cuda()
    _check([t2[..., ::2]], tv2[..., ::2], [LIN], axis=(1, 2), path=GEN_LDS)
    # values broadcast with stride 0 (exact data without NaN values: every counted sample counts) — across the rows, and
    # along them (one value per row: every bin's mean is that value, its variance 0)
    xs, _ = _exact_case(rng, [LIN], shape_rows=6, max_log2=3, extra=False)
    ncol = xs[0].shape[1]
    vb = rng.integers(-4095, 4096, (1, ncol)) * 2.0**-10
    _check([xs[0]], vb, [LIN], axis=1)
    _check([torch.as_tensor(xs[0]).cuda()], torch.as_tensor(vb).cuda(), [LIN], axis=1, ddof=1)
    vr = rng.integers(-4095, 4096, (6, 1)) * 2.0**-10
    _check([torch.as_tensor(xs[0]).cuda()], torch.as_tensor(vr).cuda(), [LIN], axis=1, path=GEN_LDS)
    # other reductions of the folded rows: counts of any size, against the exactly rounded oracle
    for axis in (None, (2,), (0,), (0, 2)):
        _close([a], vv, [LIN], axis=axis)
        _close([t], tv, [LIN], axis=axis, ddof=1)


# ---- 2. random data against the exactly rounded oracle -------------------------------------------------------------------
@pytest.mark.parametrize("per_bin", [10, 10_000, 1_000_000])
def test_random_data_against_fsum(per_bin):
    rng = np.random.default_rng(20 + len(str(per_bin)))
    nb = 8
    edges = np.linspace(0.0, float(nb), nb + 1)
    n = per_bin * nb
    x = rng.uniform(0.0, float(nb), n)
    mu = 3.0 * (1 + np.arange(nb))  # each bin's mean at least one standard deviation away from zero
    sd = 1.0 + np.arange(nb) * 0.5
    b = np.minimum(x.astype(np.int64), nb - 1)
    v = mu[b] + sd[b] * rng.standard_normal(n)
    cnt, mean, var, _ = _core().histogram_mean_var(torch.as_tensor(x).cuda(), values=torch.as_tensor(v).cuda(), bins=[edges], ddof=1)
    want = mo.histogram_mean_var(x, values=v, bins=[edges], ddof=1)
    np.testing.assert_array_equal(_np(cnt), want[0])
    np.testing.assert_allclose(_np(mean), want[1], rtol=1e-10, atol=0)
    np.testing.assert_allclose(_np(var), want[2], rtol=1e-9, atol=0)


# ---- 3. cancellation ---------------------------------------------------------------------------------------------------
def test_cancellation_large_offset():
    """values 1e8 + N(0, 1): sum(v^2)/n - mean^2 is off by O(1) here (the squares near 1e16 keep no digit of the spread).  The
    two-pass form stays within 1e-6: v - mean is exact (Sterbenz), and the sum(d) term corrects the rounding of the mean."""
    rng = np.random.default_rng(30)
    n = 4_000_000
    x = rng.uniform(0, 4, n)
    v = 1e8 + rng.standard_normal(n)
    edges = np.linspace(0, 4, 5)
    cnt, mean, var, _ = _core().histogram_mean_var(x, values=v, bins=[edges])
    want = mo.histogram_mean_var(x, values=v, bins=[edges])
    np.testing.assert_array_equal(cnt, want[0])
    np.testing.assert_allclose(mean, want[1], rtol=1e-14)
    np.testing.assert_allclose(var, want[2], rtol=1e-6)
    naive = np.array([np.mean(v[(x >= k) & (x < k + 1)] ** 2) - np.mean(v[(x >= k) & (x < k + 1)]) ** 2 for k in range(4)])
    assert np.max(np.abs(naive - want[2])) > 1e-2  # (what the three-histogram recipe would have given)


# ---- 4. special values --------------------------------------------------------------------------------------------------
def test_special_values_and_empty_inputs():
    e = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.0])
    x = np.array([0.5, 0.5, 0.5, 1.5, 1.5, 2.5, 2.5, 3.5, 4.5, 4.5, np.nan, 9.0])
    v = np.array([1.0, np.nan, 3.0, np.inf, 2.0, np.inf, -np.inf, -0.0, -0.0, -0.0, 1.0, 1.0])
    for dt in (np.float64, np.float32):
        cnt, mean, var, _ = _core().histogram_mean_var(x.astype(dt), values=v.astype(dt), bins=[e])
        np.testing.assert_array_equal(cnt, [2, 2, 2, 1, 2])  # the NaN value drops from bin 0
        np.testing.assert_array_equal(mean, [2.0, np.inf, np.nan, 0.0, 0.0])  # (np.nanmean / np.nanvar, bin by bin)
        np.testing.assert_array_equal(var, [1.0, np.nan, np.nan, 0.0, 0.0])
        assert not np.signbit(var[3]) and not np.signbit(var[4])
        cnt, mean, var, _ = _core().histogram_mean_var(x.astype(dt), values=v.astype(dt), bins=[e], ddof=1)
        np.testing.assert_array_equal(np.isnan(var), [False, True, True, True, False])  # n <= ddof: NaN
        np.testing.assert_array_equal(var[[0, 4]], [2.0, 0.0])
        cnt, mean, var, _ = _core().histogram_mean_var(x.astype(dt), values=v.astype(dt), bins=[e], ddof=2)
        assert np.isnan(var).all()
    cnt, mean, var, _ = _core().histogram_mean_var(np.zeros(0), values=np.zeros(0), bins=[e])
    assert cnt.shape == (5,) and (cnt == 0).all() and np.isnan(mean).all() and np.isnan(var).all()
    cnt, mean, var, _ = _core().histogram_mean_var(np.zeros((0, 5)), values=np.zeros((0, 5)), bins=[e], axis=1)
    assert cnt.shape == mean.shape == var.shape == (0, 5)


# ---- 5. properties -----------------------------------------------------------------------------------------------------
def test_properties_and_backends():
    from xhistogram_amd import core
    from xhistogram_amd.devicearray import DeviceArray

    rng = np.random.default_rng(17)
    x = rng.uniform(-2.2, 3.2, (4, 100_000))
    x[rng.random(x.shape) < 0.01] = np.nan
    v = 5.0 + rng.standard_normal(x.shape)  # no NaN values
    a = core.histogram_mean_var(x, values=v, bins=[LIN], axis=1)
    b = core.histogram_mean_var(torch.as_tensor(x).cuda(), values=torch.as_tensor(v).cuda(), bins=[LIN], axis=1)
    c = core.histogram_mean_var(DeviceArray.from_numpy(x), values=DeviceArray.from_numpy(v), bins=[LIN], axis=1)
    assert all(isinstance(t, np.ndarray) for t in a[:3] + c[:3]) and all(t.is_cuda for t in b[:3])
    assert a[0].dtype == np.int64 and b[0].dtype == torch.int64 and a[1].dtype == a[2].dtype == np.float64
    for got in (b, c):
        np.testing.assert_array_equal(_np(got[0]), a[0])
        np.testing.assert_allclose(_np(got[1]), a[1], rtol=1e-13)
        np.testing.assert_allclose(_np(got[2]), a[2], rtol=1e-11)
    counts, _ = core.histogram(x, bins=[LIN], axis=1)
    np.testing.assert_array_equal(a[0], counts)
    s_v, s_1, _ = core.histogram_two_weights(x, bins=[LIN], axis=1, weights=(v, np.ones_like(v)))
    np.testing.assert_allclose(a[1], s_v / s_1, rtol=1e-10)
    want = mo.histogram_mean_var(x, values=v, bins=[LIN], axis=1)
    np.testing.assert_allclose(a[2], want[2], rtol=1e-9)
    # int / estimator bins: the edges of the unweighted histogram
    xc = np.where(np.isnan(x), 0.5, x)  # (numpy's range detection refuses NaN)
    for bins in (50, "sturges"):
        _, _, _, edges = core.histogram_mean_var(xc, values=v, bins=bins)
        _, want_e = core.histogram(xc, bins=bins)
        np.testing.assert_array_equal(edges[0], want_e[0])


# ---- 6. size ------------------------------------------------------------------------------------------------------------
def test_2_28_float64_samples_against_torch():
    from xhistogram_amd import core

    n = 1 << 28
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    x = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
    v = torch.randn(n, dtype=torch.float64, device="cuda", generator=g) + 10.0
    cnt, mean, var, edges = core.histogram_mean_var(x, values=v, bins=[LIN])
    assert "pass1=mv_sum_fast" in DESCS[-1]
    e = torch.as_tensor(edges[0], device="cuda")
    idx = torch.bucketize(x, e, right=True) - 1
    idx = torch.where(x == e[-1], torch.full_like(idx, len(LIN) - 2), idx)
    ok = (x >= e[0]) & (x <= e[-1])
    del x
    idx, vv = idx[ok], v[ok]
    del ok, v
    nb = len(LIN) - 1
    tc = torch.bincount(idx, minlength=nb)
    ts = torch.zeros(nb, dtype=torch.float64, device="cuda").scatter_add_(0, idx, vv)
    tm = ts / tc.to(torch.float64)
    d = vv - tm[idx]
    tsd = torch.zeros(nb, dtype=torch.float64, device="cuda").scatter_add_(0, idx, d)
    ts2 = torch.zeros(nb, dtype=torch.float64, device="cuda").scatter_add_(0, idx, d * d)
    tm2 = (ts2 - tsd * tsd / tc.to(torch.float64)).clamp_min(0)
    torch.testing.assert_close(cnt, tc, rtol=0, atol=0)
    torch.testing.assert_close(mean, tm, rtol=1e-10, atol=0)
    torch.testing.assert_close(var, tm2 / tc.to(torch.float64), rtol=1e-9, atol=0)


# ---- 7. dask ------------------------------------------------------------------------------------------------------------
PY39 = "/opt/conda/bin/python3.9"
SCRIPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "meanvar_dask_script.py")


def _have_dask_python():
    return os.path.exists(PY39) and subprocess.run([PY39, "-c", "import dask.array, numpy"], capture_output=True).returncode == 0


@pytest.mark.skipif(not _have_dask_python(), reason="no interpreter with dask in this image")
def test_dask_chunked_equals_unchunked():
    env = dict(os.environ)
    sys_cxx = "/usr/lib/x86_64-linux-gnu/libstdc++.so.6"  # (as tests/test_dask_branch.py: conda's libstdc++ is older)
    if os.path.exists(sys_cxx):
        env["LD_PRELOAD"] = (sys_cxx + ":" + env["LD_PRELOAD"]) if env.get("LD_PRELOAD") else sys_cxx
    r = subprocess.run([PY39, "-W", "ignore", SCRIPT], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "MEANVAR-DASK-OK" in r.stdout
