"""histogram_cov on an MI355X: the kernels of xhist_cov.hip against tests/cov_exact.py and tests/cov_oracle.py.

On exactly summable data (both value arrays on values_exact.grid, NaNs put independently into each) the count is checked
against the oracle's and the histogram's, both means bit for bit, and M2_a, C_ab, M2_b bit for bit where the count is a power
of two up to 2^9 and within cov_exact's float64 bounds elsewhere.  Every census case also checks its whole describe() line
against test_gpu_values_census.predict, a restatement of choose_values / values_geometry, with the slot sizes of the two cov
passes (24 and 56 bytes, copies) registered in that module's tables from here.  Between them the fast-form and generic cases
select all 36 binning kernels of xhist_cov.hip plus its moments_mean and moments_finalize (tests/test_zz_gpu_census_total.py
holds the session to that).

What the launcher decides at run time inside one kernel symbol is not covered here: every census case of this file has one
copy of its slots, one row chunk and dense arrays.  The copies of the 24 / 56-byte slots, the LDS borders, the tables read
through L2, the datetime and uint64 domains, more than two sample arrays, segments and ragged tiles, a layout per stream through
the C ABI and the row chunks (where the plane distance differs from the chunk's rows) are the cases of
tests/test_gpu_values_census_streams.py, which borrows predict_cov, assert_cov_variant, check_exact, nan_grid and run_cov
from here."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cov_exact as cx
import cov_oracle as co
import meanvar_oracle as mo
import test_gpu_values_census as tvc
import values_exact as vx
from test_gpu_census import edges_of
from test_gpu_parity import _plan_for, xh  # noqa: F401  (xh: the module fixture)
from test_gpu_values_census import FORM_EDGES, HOME_BINS, _cus, _domain_edges, float_samples, grid_values, int_samples

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F64, F32 = np.float64, np.float32
PY39 = "/opt/conda/bin/python3.9"
SCRIPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cov_dask_script.py")
SLOT1, SLOT2 = 24, 56  # a bin's LDS slot in the two passes (MomentSumSlot<2, .>, MomentDevSlot<2> of xhist_moments.hip.h)
tvc.SLOTS.setdefault("cov", ((SLOT1, SLOT2), (SLOT1, SLOT2)))
tvc.COPIES.setdefault("cov", True)


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def run_cov(core, xs, a, b, edges, axis=1, ddof=0):
    out = core.histogram_cov(*xs, values=(a, b), bins=edges, axis=axis, ddof=ddof)[:6]
    torch.cuda.synchronize()
    return tuple(_np(o) for o in out)


def predict_cov(cus, edges, cmp, sdt, vdt, n_rows, n_cols, fine=True, arith=False, layout_fast=True):
    """test_gpu_values_census.predict for the cov slots; that function reports one pass's LDS bytes for statistics it does not
    know to have two, so the second pass's are restated here: the same tables and copies, 56-byte slots"""
    want = tvc.predict("cov", cus, edges, cmp, sdt, vdt, n_rows, n_cols, fine, arith, layout_fast)
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    first = want["lds_bytes"][0]
    in_lds = want["slots"] == "lds"
    want["lds_bytes"] = [first, first + (n_bins * (SLOT2 - SLOT1) * want["copies"] if in_lds else 0) if first else 0]
    return want


def assert_cov_variant(desc, want):
    """a cov describe() line in the mean_var line's words, for test_gpu_values_census.assert_variant"""
    assert desc.startswith("cov pass1=cov_sum_") and " pass2=cov_dev_" in desc, desc
    return tvc.assert_variant(desc.replace("cov pass1=cov_sum_", "mean_var pass1=mv_sum_").replace("cov_dev_", "mv_dev_"), want)


def _flat(samples, edges):
    """(counted mask, flat bin index over rows) of [R, C] host samples in the compare domain numpy's promotion gives"""
    cmp_s, cmp_e = [], []
    for s, e in zip(samples, edges):
        s, e = np.asarray(s), np.asarray(e)
        if s.dtype.kind == "f" or e.dtype.kind == "f":
            s, e = s.astype(F64), e.astype(F64)
        cmp_s.append(s)
        cmp_e.append(e)
    ok, flat, nbs = mo._flat_bins(cmp_s, cmp_e)
    m, n_bins = samples[0].shape[0], int(np.prod(nbs))
    return ok, flat + (np.arange(m, dtype=np.int64) * n_bins)[:, None], m * n_bins


def check_exact(core, xs_host, edges, a, b, got, xs_dev=None, ddof=0, what=""):
    """got = (count, mean_a, mean_b, var_a, var_b, cov_ab) of [R, C] host samples and values (a, b broadcastable to them)"""
    ok, flat, size = _flat(xs_host, edges)
    a = np.broadcast_to(np.asarray(a), ok.shape)
    b = np.broadcast_to(np.asarray(b), ok.shape)
    cnt, (ma, mb), moments, bounds, exact = cx.expected(flat[ok], a[ok], b[ok], size)
    got_cnt = np.asarray(got[0]).reshape(-1)
    assert got_cnt.dtype == np.int64
    np.testing.assert_array_equal(got_cnt, cnt, err_msg="count " + what)
    hist = np.bincount(flat[ok], minlength=size)
    dropped = np.bincount(flat[ok & (np.isnan(a.astype(F64)) | np.isnan(b.astype(F64)))], minlength=size)
    np.testing.assert_array_equal(got_cnt + dropped, hist, err_msg="count + pairs with a NaN " + what)
    if xs_dev is not None:
        h, _ = core.histogram(*xs_dev, bins=edges, axis=1)
        np.testing.assert_array_equal(_np(h).reshape(-1), hist, err_msg="histogram count " + what)
    tvc._bits(got[1], ma, "mean_a " + what)
    tvc._bits(got[2], mb, "mean_b " + what)
    cx.assert_moments((got[3], got[5], got[4]), moments, bounds, exact, cnt=cnt, ddof=ddof, what=what)
    return cnt, exact


def nan_grid(rng, shape, dt, seed_shift=0):
    """grid values with NaNs of their own (float dtypes)"""
    return grid_values(np.random.default_rng(int(rng.integers(1 << 30)) + seed_shift), shape, dt)


# ---------------------------------------------------------------------------------------------------------------------
# every fast form: f32 / f64 x D 1 / 2 x SCAN 1 / 2 / arith
# ---------------------------------------------------------------------------------------------------------------------
# arithmetic edges: the fine tables and the 56-byte slots together exceed 160 KiB while the slots alone fit (n_bins <= 2925)
ARITH_BINS = ((2_900,), (3, 960))


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("sdt", ["f64", "f32"])
@pytest.mark.parametrize("form", ["k1", "k2", "arith"])
def test_fast_forms(xh, form, sdt, D):
    (kind, nb1, nb2), fine, arith = FORM_EDGES[form]
    if form == "arith":
        nb1, nb2 = ARITH_BINS
    st = F64 if sdt == "f64" else F32
    seed = 900 + 10 * ["k1", "k2", "arith"].index(form) + 2 * D + (st == F32)
    edges = [edges_of(kind, nb, seed=seed + d) for d, nb in enumerate(nb1 if D == 1 else nb2)]
    rng = np.random.default_rng(seed)
    xs = float_samples(edges, 3, 20_011, st, seed)
    a, b = nan_grid(rng, xs[0].shape, st), nan_grid(rng, xs[0].shape, st)
    xd = [_dev(x) for x in xs]
    got = run_cov(xh, xd, _dev(a), _dev(b), edges, ddof=D - 1)
    desc = _plan_for(xh, xd, edges).describe()
    want = predict_cov(_cus(), edges, 0, st, st, 3, 20_011, fine, arith)
    assert want["family"] == "fast" and (want["scan"] == 5) == (form == "arith"), want
    hit = assert_cov_variant(desc, want)
    assert (" scan=5 " in desc) == (form == "arith") and hit["D"] == D
    check_exact(xh, xs, edges, a, b, got, xs_dev=xd, ddof=D - 1, what="%s %s D=%d" % (form, sdt, D))


# ---------------------------------------------------------------------------------------------------------------------
# the generic family: CMP 0 / 1 / 3, slots in LDS or sums in global memory
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("home", ["lds", "global_tables_lds"])
@pytest.mark.parametrize("dom", ["f64", "i64", "mixed"])
def test_generic_domain_and_home(xh, dom, home):
    rng = np.random.default_rng(120 + 3 * ["f64", "i64", "mixed"].index(dom) + ["lds", "global_tables_lds"].index(home))
    nb = HOME_BINS[home] if dom != "mixed" else max(2, HOME_BINS[home] // 6)
    edges = _domain_edges(dom, nb, rng)
    n_rows, n_cols = 2, 20_011
    cmp = {"f64": 0, "i64": 1, "mixed": 3}[dom]
    xs = []
    for d, e in enumerate(edges):
        if np.asarray(e).dtype.kind == "f":
            xs += float_samples([e], n_rows, n_cols, F64, 27 + d)
        else:
            xs += int_samples([e], n_rows, n_cols, None, 27 + d)
    # f64: float64 samples with values of another dtype; i64: integer a next to a float64 b
    a = nan_grid(rng, (n_rows, n_cols), F32 if dom == "f64" else F64)
    b = nan_grid(rng, (n_rows, n_cols), F32 if dom == "f64" else F64)
    if dom == "i64":
        a = vx.grid(rng, (n_rows, n_cols), np.int32)
    xd = [_dev(x) for x in xs]
    got = run_cov(xh, xd, _dev(a), _dev(b), edges, ddof=1)
    want = predict_cov(_cus(), edges, cmp, xs[0].dtype, a.dtype, n_rows, n_cols, False)
    hit = assert_cov_variant(_plan_for(xh, xd, edges).describe(), want)
    assert hit["family"] == "generic" and hit["slots"] == ("lds" if home == "lds" else "global") and hit["cmp"] == cmp
    check_exact(xh, xs, edges, a, b, got, xs_dev=xd, ddof=1, what="%s %s" % (dom, home))


def test_1024_x_1024_bins(xh):
    """beyond LDS: 2^20 bins, every sum a float64 atomic in global memory"""
    rng = np.random.default_rng(5)
    edges = [np.linspace(-4, 4, 1025)] * 2
    xs = [rng.standard_normal((1, 1 << 20)) for _ in range(2)]
    a, b = nan_grid(rng, xs[0].shape, F64), nan_grid(rng, xs[0].shape, F64)
    xd = [_dev(x) for x in xs]
    got = run_cov(xh, xd, _dev(a), _dev(b), edges)
    assert "slots=global" in _plan_for(xh, xd, edges).describe()
    check_exact(xh, xs, edges, a, b, got, what="1024x1024")


# ---------------------------------------------------------------------------------------------------------------------
# identities
# ---------------------------------------------------------------------------------------------------------------------
def test_identities(xh):
    rng = np.random.default_rng(11)
    edges = [edges_of("k1", 300, seed=11)]
    xs = float_samples(edges, 3, 20_011, F64, 11)
    a = nan_grid(rng, xs[0].shape, F64)
    b = vx.grid(rng, xs[0].shape)  # NaN-free
    xd, ad, bd = [_dev(x) for x in xs], _dev(a), _dev(b)
    # cov(a, a): the three moments are one (three sums of the same terms, each in an order of its own: bit for bit where the
    # sums are exact, to the weighted test's rtol elsewhere)
    n, ma, mb, va, vb, cab = run_cov(xh, xd, ad, ad, edges)
    tvc._bits(ma, mb, "mean of (a, a)")
    same = vx.m2_exact(n)
    np.testing.assert_array_equal(va[same], vb[same])
    np.testing.assert_array_equal(cab[same], va[same])
    np.testing.assert_allclose(vb, va, rtol=1e-12, atol=0)
    np.testing.assert_allclose(cab, va, rtol=1e-12, atol=0)
    # a NaN-free b: count and mean_a are histogram_mean_var's bit for bit, var_a on power-of-two counts
    n, ma, mb, va, vb, cab = run_cov(xh, xd, ad, bd, edges, ddof=1)
    cnt, mean, var, _ = xh.histogram_mean_var(*xd, values=ad, bins=edges, axis=1, ddof=1)
    cnt, mean, var = _np(cnt), _np(mean), _np(var)
    np.testing.assert_array_equal(n, cnt)
    tvc._bits(ma, mean, "mean_a against histogram_mean_var")
    pow2 = vx.m2_exact(cnt) & (cnt > 1)
    assert pow2.any()
    np.testing.assert_array_equal(va[pow2], var[pow2])
    np.testing.assert_allclose(va, var, rtol=1e-12, atol=0)
    # cov(a, b) == cov(b, a) where the sums are exact
    n2, mb2, ma2, vb2, va2, cba = run_cov(xh, xd, bd, ad, edges, ddof=1)
    np.testing.assert_array_equal(n2, n)
    tvc._bits(ma2, ma, "mean_a, swapped")
    tvc._bits(mb2, mb, "mean_b, swapped")
    np.testing.assert_array_equal(cba[pow2], cab[pow2])
    np.testing.assert_array_equal(va2[pow2], va[pow2])
    np.testing.assert_array_equal(vb2[pow2], vb[pow2])


def test_negative_covariance_stays_negative(xh):
    edges = [np.array([0.0, 1.0, 2.0])]
    x = np.array([0.5, 0.5, 0.5, 0.5, 1.5, 1.5])
    a = np.array([1.0, 2.0, 3.0, 4.0, 1.0, 3.0])
    b = np.array([8.0, 6.0, 4.0, 2.0, 1.0, 5.0])
    n, ma, mb, va, vb, cab, _ = xh.histogram_cov(x, values=(a, b), bins=edges)
    np.testing.assert_array_equal(n, [4, 2])
    np.testing.assert_array_equal(ma, [2.5, 2.0])
    np.testing.assert_array_equal(mb, [5.0, 3.0])
    np.testing.assert_array_equal(va, [1.25, 1.0])
    np.testing.assert_array_equal(vb, [5.0, 4.0])
    np.testing.assert_array_equal(cab, [-2.5, 2.0])  # bin 0: b = 10 - 2 a
    # ddof = 1 is np.cov's default; correlation and slope follow from the outputs
    n, ma, mb, va, vb, cab, _ = xh.histogram_cov(x, values=(a, b), bins=edges, ddof=1)
    np.testing.assert_allclose(cab[0], np.cov(a[:4], b[:4])[0, 1], rtol=1e-15)
    np.testing.assert_allclose(cab / np.sqrt(va * vb), [-1.0, 1.0], rtol=1e-14)
    np.testing.assert_allclose(cab / va, [-2.0, 2.0], rtol=1e-14)


# ---------------------------------------------------------------------------------------------------------------------
# cancellation
# ---------------------------------------------------------------------------------------------------------------------
def test_cancellation_large_offsets(xh):
    """a = 1e8 + grid, b = -1e8 + grid: the two-pass co-moment stays within cov_exact's bound; sum(a b) / n - mean_a mean_b
    evaluated in float64 loses every digit"""
    rng = np.random.default_rng(51)
    edges = [np.linspace(-3, 3, 21)]
    x = rng.standard_normal((1, 100_003))
    ga = vx.grid(rng, x.shape)
    gb = np.round((-0.5 * ga + 0.25 * vx.grid(rng, x.shape)) / vx.SCALE) * vx.SCALE
    a, b = 1e8 + ga, -1e8 + gb  # (exact: multiples of 2^-10 below 2^27)
    got = run_cov(xh, [_dev(x)], _dev(a), _dev(b), edges)
    ok, flat, size = _flat([x], edges)
    n = np.bincount(flat[ok], minlength=size)
    np.testing.assert_array_equal(got[0].reshape(-1), n)
    cab = got[5].reshape(-1)
    naive = np.zeros(size)
    for k in range(size):
        sel = (flat == k) & ok
        av, bv = a[sel], b[sel]
        ma, mb = got[1].reshape(-1)[k], got[2].reshape(-1)[k]
        c_star, bound = cx.c_star_and_bound(av, bv, ma, mb)  # the exact co-moment of the terms the kernel adds, its own means
        assert abs(cab[k] * n[k] - c_star) <= bound + 3 * vx.U * abs(c_star), (k, cab[k] * n[k], c_star, bound)
        # against the truth, the covariance of the offsets' remainders (means of the small numbers are accurate)
        true = np.mean((ga[sel] - ga[sel].mean()) * (gb[sel] - gb[sel].mean()))
        assert abs(cab[k] - true) <= 1e-6 * abs(true), (k, cab[k], true)
        naive[k] = np.sum(av * bv) / n[k] - (np.sum(av) / n[k]) * (np.sum(bv) / n[k])
    assert (cab < 0).all()
    assert np.max(np.abs(naive - cab)) > 0.1, np.max(np.abs(naive - cab))


# ---------------------------------------------------------------------------------------------------------------------
# special values
# ---------------------------------------------------------------------------------------------------------------------
def test_special_values(xh):
    nan, inf = np.nan, np.inf
    edges = [np.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.0])]
    #             bin 0: only incomplete pairs | bin 1: n = 1 | bin 2: an inf in a | bin 3: -inf in b | bin 4: empty
    x = np.array([0.5, 0.5, 0.5, 1.5, 1.5, 2.5, 2.5, 2.5, 3.5, 3.5, 9.0])
    a = np.array([1.0, nan, nan, 2.0, nan, 1.0, inf, 3.0, 1.0, 2.0, 1.0])
    b = np.array([nan, 2.0, nan, 7.0, 1.0, 1.0, 2.0, 3.0, -inf, 2.0, 1.0])
    for ddof in (0, 1):
        n, ma, mb, va, vb, cab, _ = xh.histogram_cov(x, values=(a, b), bins=edges, ddof=ddof)
        np.testing.assert_array_equal(n, [0, 1, 3, 2, 0])
        np.testing.assert_array_equal(ma, [nan, 2.0, inf, 1.5, nan])
        np.testing.assert_array_equal(mb, [nan, 7.0, 2.0, -inf, nan])
        zero = 0.0 if ddof == 0 else nan  # n = 1: moments 0, NaN once n <= ddof
        np.testing.assert_array_equal(va, [nan, zero, nan, 0.5 / (2 - ddof), nan])
        np.testing.assert_array_equal(vb, [nan, zero, 2.0 / (3 - ddof), nan, nan])
        np.testing.assert_array_equal(cab, [nan, zero, nan, nan, nan])
    h, _ = xh.histogram(x, bins=edges)
    np.testing.assert_array_equal(h, [3, 2, 3, 2, 0])
    # empty inputs, and inputs with no counted sample
    for xe in (np.zeros(0), np.full(5, 9.0)):
        out = xh.histogram_cov(xe, values=(np.ones(xe.shape), np.ones(xe.shape)), bins=edges)
        np.testing.assert_array_equal(out[0], np.zeros(5, np.int64))
        assert out[0].dtype == np.int64 and all(np.isnan(o).all() for o in out[1:6])


# ---------------------------------------------------------------------------------------------------------------------
# layouts and backends
# ---------------------------------------------------------------------------------------------------------------------
def _moment_atol(cnt):
    """what two float64 evaluations of a variance or covariance of grid values may differ by when their sums round in orders
    of their own: each sum of n terms is within g(n) of its exact value relative to the sum of the terms' magnitudes, at most
    16 n (|d| < 4 on the grid), and the division by n - ddof >= n / 2 keeps twice that per side"""
    return 4.0 * vx.gamma(max(int(np.max(cnt, initial=1)), 1)) * 16.0


def _case(xh, xs_host, a_host, b_host, edges, axis, xs_dev, a_dev, b_dev, family, ddof=0):
    """one N-D call against the exact-mode oracle, and the family its describe() names"""
    got = xh.histogram_cov(*xs_dev, values=(a_dev, b_dev), bins=edges, axis=axis, ddof=ddof)[:6]
    torch.cuda.synchronize()
    desc = _plan_for(xh, xs_dev, edges).describe()
    assert family is None or ("pass1=cov_sum_%s " % family) in desc, desc
    want = co.histogram_cov(*xs_host, values=(a_host, b_host), bins=edges, axis=axis, ddof=ddof, exact=True)
    for i in range(3):
        np.testing.assert_array_equal(_np(got[i]), want[i])
    for i in range(3, 6):
        np.testing.assert_allclose(_np(got[i]), want[i], rtol=0, atol=_moment_atol(want[0]))


def test_layouts(xh):
    rng = np.random.default_rng(21)
    edges = [np.linspace(-3, 3, 61)]
    x = rng.standard_normal((4, 30_001))
    a, b = nan_grid(rng, x.shape, F64), nan_grid(rng, x.shape, F64)
    xd, ad, bd = _dev(x), _dev(a), _dev(b)
    _case(xh, [x], a, b, edges, 1, [xd], ad, bd, "fast")
    _case(xh, [x], a, b.astype(F32), edges, 1, [xd], ad, _dev(b.astype(F32)), "generic")  # b of another dtype than a
    brow = vx.grid(rng, (1, 30_001))  # b broadcast across rows (row stride 0): the fast layout
    _case(xh, [x], a, brow, edges, 1, [xd], ad, _dev(brow).expand(4, 30_001), "fast", ddof=1)
    bcol = vx.grid(rng, (4, 1))  # b broadcast along rows (column stride 0): one value per row, the generic family
    _case(xh, [x], a, bcol, edges, 1, [xd], ad, _dev(bcol).expand(4, 30_001), "generic")
    # unaligned row starts: every row begins one element past a 16-byte boundary
    xb, ab, bb = (np.concatenate([np.zeros((4, 1)), t], axis=1) for t in (x, a, b))
    off = [_dev(t)[:, 1:] for t in (xb, ab, bb)]
    assert all(t.data_ptr() % 16 for t in off)
    _case(xh, [x], a, b, edges, 1, off[:1], off[1], off[2], "fast")
    # a leading-axis reduction, and a reduction over everything
    x3 = rng.standard_normal((50, 6, 40))
    a3, b3 = nan_grid(rng, x3.shape, F64), nan_grid(rng, x3.shape, F64)
    _case(xh, [x3], a3, b3, edges, (0,), [_dev(x3)], _dev(a3), _dev(b3), None, ddof=1)
    _case(xh, [x3], a3, b3, edges, None, [_dev(x3)], _dev(a3), _dev(b3), "fast")


def _delay():
    """tens of milliseconds of GPU work on the current stream"""
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(50_000_000)
        return
    t = torch.randn(4096, 4096, device="cuda")
    for _ in range(20):
        t = torch.tanh(t @ t)


def test_backends(xh):
    from xhistogram_amd.devicearray import DeviceArray

    rng = np.random.default_rng(71)
    edges = [np.linspace(-3, 3, 25)]
    x = rng.standard_normal((5, 3000))
    a = nan_grid(rng, x.shape, F64)
    b = vx.grid(rng, (1, 3000))
    want = co.histogram_cov(x, values=(a, b), bins=edges, axis=1, exact=True)
    got_np = xh.histogram_cov(x, values=(a, b), bins=edges, axis=1)
    assert got_np[0].dtype == np.int64 and all(isinstance(g, np.ndarray) and g.dtype == F64 for g in got_np[1:6])
    for g, w in zip(got_np[:3], want[:3]):
        np.testing.assert_array_equal(g, w)
    for g, w in zip(got_np[3:6], want[3:]):
        np.testing.assert_allclose(g, w, rtol=0, atol=_moment_atol(want[0]))
    # torch: issued on the current stream.  The values the call reads are written on a side stream behind a long wait, over
    # NaN placeholders; a call issued on any other stream would read the placeholders and count nothing
    xd, a_src, b_src = _dev(x), _dev(a), _dev(np.broadcast_to(b, x.shape))
    ad = torch.full(a_src.shape, float("nan"), dtype=torch.float64, device="cuda")
    bd = torch.full(b_src.shape, float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        _delay()
        ad.copy_(a_src)
        bd.copy_(b_src)
        got_t = xh.histogram_cov(xd, values=(ad, bd), bins=edges, axis=1)
        done = torch.cuda.Event()
        done.record(s)
    done.synchronize()
    assert got_t[0].dtype == torch.int64 and all(t.device.type == "cuda" and t.dtype == torch.float64 for t in got_t[1:6])
    got_d = xh.histogram_cov(DeviceArray.from_numpy(x, 0), values=(DeviceArray.from_numpy(a, 0), DeviceArray.from_numpy(b, 0)),
                             bins=edges, axis=1)
    for other in (got_t, got_d):
        for g, w in zip(other[:3], got_np[:3]):
            np.testing.assert_array_equal(_np(g), w)
        for g, w in zip(other[3:6], got_np[3:6]):
            np.testing.assert_allclose(_np(g), w, rtol=0, atol=_moment_atol(want[0]), equal_nan=True)


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
    o2 = xr.DataArray(nan_grid(rng, (4, 6, 8), F64), dims=("time", "lat", "lon"), name="o2", coords=coords)
    w = xr.DataArray(vx.grid(rng, (6, 8)), dims=("lat", "lon"), name="w", coords={"lat": coords["lat"], "lon": coords["lon"]})
    edges = np.linspace(0, 10, 6)
    out = xhx.histogram_cov(T, values=(o2, w), bins=[edges], dim=["lat", "lon"], keep_coords=True)
    assert list(out) == ["o2_w_count", "o2_mean", "w_mean", "o2_var", "w_var", "o2_w_cov"]
    assert all(tuple(v.dims) == ("time", "T_bin") for v in out.values())
    np.testing.assert_array_equal(np.asarray(out["o2_w_cov"].coords["time"].values), coords["time"])
    np.testing.assert_array_equal(np.asarray(out["o2_w_cov"].coords["T_bin"].values), 0.5 * (edges[:-1] + edges[1:]))
    want = co.histogram_cov(T.values, values=(o2.values, w.values[None]), bins=[edges], axis=(1, 2), exact=True)
    for g, wv in zip(list(out.values())[:3], want[:3]):
        np.testing.assert_array_equal(np.asarray(g.values), wv)
    for g, wv in zip(list(out.values())[3:], want[3:]):
        np.testing.assert_allclose(np.asarray(g.values), wv, rtol=0, atol=_moment_atol(want[0]))


def test_dask_chunked_equals_unchunked():
    env = dict(os.environ)
    sys_cxx = "/usr/lib/x86_64-linux-gnu/libstdc++.so.6"  # (as tests/test_dask_branch.py: conda's libstdc++ is older)
    if os.path.exists(sys_cxx):
        env["LD_PRELOAD"] = (sys_cxx + ":" + env["LD_PRELOAD"]) if env.get("LD_PRELOAD") else sys_cxx
    r = subprocess.run([PY39, "-W", "ignore", SCRIPT], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "COV-DASK-OK" in r.stdout
