"""histogram_skew_kurt without a GPU: the oracle (tests/skew_kurt_oracle.py) against scipy, the claims of
tests/skew_kurt_exact.py in exact arithmetic for every shape tests/test_gpu_skew_kurt.py uses, the bounds, the merge of dask's
partials, and the surface (names, header, ABI, argument errors, the xarray wrapper, the loud failure without a device)."""
import importlib
import math
import os
import pickle
import sys
from fractions import Fraction

import numpy as np
import pytest
import scipy.stats

import skew_kurt_exact as sx
import skew_kurt_oracle as so
import test_gpu_skew_kurt as tg
import values_exact as vx
from skew_kurt_exact import Err
from xhistogram_amd import _native, core

try:
    import xarray as xr  # noqa: F401
except ImportError:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "doubles"))
    import xarray as xr  # the double

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32 = np.float64, np.float32
U = vx.U


# ---------------------------------------------------------------------------------------------------------------------
# the oracle against scipy
# ---------------------------------------------------------------------------------------------------------------------
def _scipy_bound(vals, bias, fisher):
    """what scipy.stats.skew / kurtosis may differ by from the exact statistics of `vals` (float64, no NaN), as (skew, kurt):
    scipy takes m_k = mean((v - mean)^k) about ITS mean m^ = vals.mean(): about the true mean mu the central sums move by
    e = mu - m^ exactly as sum((d + e)^k) expands (M2: n e^2; M3: 3 e M2 + n e^3; M4: 4 e M3 + 6 e^2 M2 + n e^4, bounded with
    |M3| <= A3), each term d^k carries k roundings and numpy's sum of n terms is within g(n) A_k whatever its order.  Those go
    into skew_kurt_exact's running error bounds through the public formulas (skew_kurt_exact.outputs).  scipy evaluates the
    same quantities in an order of its own (m2**1.5, (n^2 - 1) m4 / m2^2 - 3 (n - 1)^2): fewer than 16 more operations, each
    within u of quantities no larger than |g| + 3 after the scaling by 1 / n, so 64 u (|val| + 3) is added and the bound doubled."""
    n = len(vals)
    mu = float(Fraction(sum(Fraction(float(v)) for v in vals), n))
    m_hat = float(np.mean(vals))
    e = abs(mu - m_hat) + U * abs(mu)
    d = vals - m_hat
    sums = []
    for k in (2, 3, 4):
        t = d ** k
        A = math.fsum(np.abs(t))
        sums.append((math.fsum(t), vx.gamma(n + 2 * k + 2) * A + U * A, A))
    (s2, e2, _), (s3, e3, A3), (s4, e4, _) = sums
    m2 = Err(s2, e2 + n * e * e)
    m3 = Err(s3, e3 + 3 * e * s2 + n * e ** 3)
    m4 = Err(s4, e4 + 4 * e * A3 + 6 * e * e * s2 + n * e ** 4)
    _, skew, kurt = sx.outputs(float(n), m2, m3, m4, 0, bias, fisher)
    return (2 * float(skew.err) + 64 * U * (abs(float(skew.val)) + 3), 2 * float(kurt.err) + 64 * U * (abs(float(kurt.val)) + 3))


def _bins_of(x, edges):
    nb = len(edges) - 1
    idx = np.searchsorted(edges, x, side="right") - 1
    idx[x == edges[-1]] = nb - 1
    return idx, (x >= edges[0]) & (x <= edges[-1])


MEASURED = []  # (oracle - scipy) / bound of every bin compared, for the figures in the docstring below


@pytest.mark.parametrize("fisher", [True, False])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("seed", range(4))
def test_oracle_matches_scipy(seed, bias, fisher):
    """scipy.stats.skew / kurtosis (1.15, nan_policy="omit") over the values of each bin with more than 3 of them, both `bias`
    and both `fisher` settings, within _scipy_bound.  Measured on these 16 cases, 72 bins (oracle minus scipy): at most 5.0e-15
    absolute in skew and 4.5e-15 in kurt (values 10 + 3 N(0, 1), up to a few hundred per bin), at most 0.062 and 0.018 of the
    bound: scipy's own rounding is a few ulps of its results, the bound allows for sums of n terms in any order."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(300, 1500))
    edges = np.sort(rng.uniform(-2, 2, int(rng.integers(4, 9))))
    x = rng.uniform(-2.3, 2.3, n)
    on = rng.random(n) < 0.1
    x[on] = edges[rng.integers(0, len(edges), int(on.sum()))]
    x[:3] = [edges[0], edges[-1], np.nan]
    v = rng.standard_normal(n) * 3 + 10 + rng.exponential(2.0, n) * (seed % 2)
    v[rng.random(n) < 0.06] = np.nan
    got = so.histogram_skew_kurt(x, values=v, bins=[edges], bias=bias, fisher=fisher)
    idx, inside = _bins_of(x, edges)
    compared = 0
    for k in range(len(edges) - 1):
        vals = v[inside & (idx == k)]
        cnt = int((~np.isnan(vals)).sum())
        assert got[0][k] == cnt
        if cnt <= 3:
            continue
        ws = float(scipy.stats.skew(vals, bias=bias, nan_policy="omit"))
        wk = float(scipy.stats.kurtosis(vals, fisher=fisher, bias=bias, nan_policy="omit"))
        bs, bk = _scipy_bound(vals[~np.isnan(vals)], bias, fisher)
        assert abs(got[3][k] - ws) <= bs and abs(got[4][k] - wk) <= bk, (k, got[3][k] - ws, bs, got[4][k] - wk, bk)
        MEASURED.append((abs(got[3][k] - ws), abs(got[4][k] - wk), abs(got[3][k] - ws) / bs, abs(got[4][k] - wk) / bk))
        # the variance, as np.nanvar gives it
        np.testing.assert_allclose(got[2][k], np.nanvar(vals), rtol=1e-12)
        compared += 1
    assert compared >= 3


def test_oracle_small_counts_and_weights():
    """bias=False: NaN where x <= 2 (skew) and x <= 3 (kurt), where scipy keeps the biased value; a constant bin is NaN; the
    weighted oracle with integer weights is the oracle of the repeated samples, value for value"""
    nan = np.nan
    edges = [np.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.0])]
    x = np.array([0.5, 1.5, 1.5, 2.5, 2.5, 2.5, 3.5, 3.5, 3.5, 3.5, 4.5, 4.5])
    v = np.array([1.0, 1.0, 4.0, 1.0, 2.0, 6.0, 1.0, 2.0, 4.0, 9.0, 5.0, 5.0])
    n, mean, var, skew, kurt = so.histogram_skew_kurt(x, values=v, bins=edges, bias=False, ddof=1)
    np.testing.assert_array_equal(n, [1, 2, 3, 4, 2])
    np.testing.assert_array_equal(np.isnan(var), [True, False, False, False, False])
    np.testing.assert_array_equal(np.isnan(skew), [True, True, False, False, True])
    np.testing.assert_array_equal(np.isnan(kurt), [True, True, True, False, True])
    np.testing.assert_allclose(skew[2:4], [scipy.stats.skew(v[3:6], bias=False), scipy.stats.skew(v[6:10], bias=False)], rtol=1e-14)
    np.testing.assert_allclose(kurt[3], scipy.stats.kurtosis(v[6:10], bias=False), rtol=1e-13)
    assert scipy.stats.skew(v[1:3], bias=False) == 0.0  # (scipy: the biased value at n = 2; here NaN)
    biased = so.histogram_skew_kurt(x, values=v, bins=edges)
    np.testing.assert_array_equal(np.isnan(biased[3]), [True, False, False, False, True])  # n = 1 and 5, 5: constant bins
    np.testing.assert_array_equal(biased[4][1], -2.0)
    # integer weights == repeated samples
    rng = np.random.default_rng(5)
    xs = rng.uniform(-0.2, 5.2, 400)
    vs = rng.standard_normal(400) + 3
    vs[::19] = nan
    w = rng.integers(0, 6, 400).astype(F64)
    for bias, fisher, ddof in ((True, True, 0), (False, False, 1)):
        a = so.histogram_skew_kurt(xs, values=vs, weights=w, bins=edges, bias=bias, fisher=fisher, ddof=ddof)
        b = so.histogram_skew_kurt(np.repeat(xs, w.astype(int)), values=np.repeat(vs, w.astype(int)), bins=edges, bias=bias,
                                   fisher=fisher, ddof=ddof)
        np.testing.assert_array_equal(a[0], b[0].astype(F64))
        for p, q in zip(a[1:], b[1:]):
            np.testing.assert_array_equal(p, q)
    # a NaN weight makes its own bin NaN, weights that sum to 0 give NaN moments
    w2 = np.ones(12)
    w2[1] = nan
    w2[10:] = 0.0
    W, mean, var, skew, kurt = so.histogram_skew_kurt(x, values=v, weights=w2, bins=edges)
    np.testing.assert_array_equal(W, [1.0, nan, 3.0, 4.0, 0.0])
    assert np.isnan(mean[1]) and np.isnan(skew[1]) and np.isnan(mean[4]) and not np.isnan(skew[2])


# ---------------------------------------------------------------------------------------------------------------------
# the narrow grid's claims, in exact arithmetic, for every shape of the GPU module
# ---------------------------------------------------------------------------------------------------------------------
CASES = tg.cases()


def _exact_bin_claims(vals, w, x):
    """one bin of the bit-for-bit path in rational arithmetic: the mean, d, every term and every partial sum are float64"""
    j = int(x).bit_length() - 1
    assert 1 << j == int(x) and 1 <= j <= 5
    fv = [Fraction(float(v)) for v in vals]
    fw = [Fraction(1)] * len(vals) if w is None else [Fraction(float(t)) for t in w]
    mean = sum(a * b for a, b in zip(fw, fv)) / int(x)
    assert Fraction(float(mean)) == mean
    d = [a - mean for a in fv]
    scale = 1 if all(abs(a) < 4 for a in fv) else 16  # (integer values: the same bits, 2^4 times the size)
    unit = Fraction(scale, 1 << (4 + j))
    assert all((t / unit).denominator == 1 and abs(t) < 8 * scale for t in d)
    assert sum(a * b for a, b in zip(fw, d)) == 0  # D = 0
    t = [a * b for a, b in zip(fw, d)]
    sums = []
    for k in (1, 2, 3, 4):
        if k > 1:
            t = [a * b for a, b in zip(t, d)]
        uk = unit ** k
        assert all(Fraction(float(a)) == a for a in t)  # every term is a float64
        assert sum(abs(a) for a in t) / uk < (1 << 53)  # so is every partial sum, in any order: multiples of uk below 2^53 uk
        sums.append(sum(t))
    return float(mean), [float(s) for s in sums[1:]]


@pytest.mark.parametrize("name", list(CASES))
def test_every_gpu_shape_has_exact_bins_and_they_are_exact(name):
    edges, xs, v, w = CASES[name]
    ok, flat, size = tg.flat_of(xs, edges)
    vb = np.broadcast_to(np.asarray(v), ok.shape).astype(F64)
    wb = np.broadcast_to(np.asarray(w), ok.shape).astype(F64)
    assert sx.on_narrow(vb) and xs[0].shape[1] <= 10_000  # (small rows: the GPU cases take seconds)
    for weights in (None, wb):
        x, mean, moments, bounds, exact = sx.expected(flat[ok], vb[ok], size, None if weights is None else weights[ok])
        assert exact.any(), "no bin on the bit-for-bit path"
        assert np.all(bounds[:, exact] == 0) and np.all(bounds[:, ~exact & (x != 0)] >= 0)
        keep = ok & ~np.isnan(vb)
        for k in np.flatnonzero(exact)[:40]:
            sel = keep & (flat == k)
            m, s = _exact_bin_claims(vb[sel], None if weights is None else weights[sel], x[k])
            assert m == mean[k] and s == list(moments[:, k]), (k, m, mean[k], s, moments[:, k])
            # the oracle from the raw values says the same, value for value
            assert so.bin_moments(vb[sel], None if weights is None else weights[sel])[2:] == tuple(moments[:, k])


def test_exact_counts_are_the_issue_s():
    assert sx.X_EXACT == (2, 4, 8, 16, 32) and sx.K_MAX == 64 and sx.SCALE == 2.0 ** -4 and sx.W_MAX == 7
    np.testing.assert_array_equal(sx.exact_x([0, 1, 2, 3, 4, 8, 16, 32, 64, 6.0, np.nan]), [0, 0, 1, 0, 1, 1, 1, 1, 0, 0, 0])
    rng = np.random.default_rng(0)
    assert sx.on_narrow(sx.narrow(rng, 1000)) and sx.on_narrow(sx.narrow(rng, 1000, F32)) and vx.on_grid(sx.narrow(rng, 1000))
    assert not sx.on_narrow(np.array([4.5])) and not sx.on_narrow(np.array([64.0])) and not sx.on_narrow(np.array([2.0 ** -5]))
    # x = 64 would need 28 + 5 * 6 = 58 bits: such a bin takes the bound
    v = sx.narrow(rng, 64)
    assert not sx.expected(np.zeros(64, np.int64), v, 1)[4][0]


# ---------------------------------------------------------------------------------------------------------------------
# the bounds
# ---------------------------------------------------------------------------------------------------------------------
def _kernel_moments(vals, mean, x, w, rng, pieces=1, acc=F64):
    """the kernel's computation in one random order: the terms added in `acc` within `pieces` interleaved partial sums (the
    copies and workgroups), those then added in float64, then the finalize step in float64"""
    terms = sx.kernel_terms(vals, mean, w)
    order = rng.permutation(len(vals))
    sums = []
    for t in terms:
        t = t[order]
        parts = []
        for p in range(pieces):
            s = np.zeros((), acc)
            for a in t[p::pieces]:
                s = (s + np.asarray(a, acc)).astype(acc)
            parts.append(float(s))
        tot = 0.0
        for p in rng.permutation(pieces):
            tot += parts[p]
        sums.append(tot)
    D, Q2, Q3, Q4 = sums
    delta = D / x
    d2 = delta * delta
    d3 = d2 * delta
    d4 = d2 * d2
    r2 = Q2 - D * D / x
    r4 = ((Q4 - (4.0 * delta) * Q3) + (6.0 * d2) * Q2) - (3.0 * x) * d4
    return max(0.0, r2), (Q3 - (3.0 * delta) * Q2) + (2.0 * x) * d3, max(0.0, r4)


def _bin(rng, n, weighted, offset=0.0):
    v = np.clip(np.round((sx.narrow(rng, n) * 0.3 + offset) / sx.SCALE), -63, 63) * sx.SCALE
    w = rng.integers(0, 8, n).astype(F64) if weighted else None
    if w is not None:
        w[0] = 7.0
        if sx.exact_x(w.sum()):
            w[0] = 6.0
    return v, w


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", [3, 5, 7, 100, 999, 4097])
def test_bound_holds_for_float64_sums_in_many_orders(n, weighted):
    rng = np.random.default_rng(n + weighted)
    for offset in (0.0, 2.5, -3.0):  # (means far from zero: skewed by the clip, either sign of M3)
        v, w = _bin(rng, n, weighted, offset)
        x, mean, star, bounds, exact = sx.expected(np.zeros(n, np.int64), v, 1, w)
        assert not exact[0] and np.all(bounds[:, 0] > 0)
        for pieces in (1, 2, 16, 256):
            for _ in range(4):
                got = _kernel_moments(v, mean[0], float(x[0]), w, rng, pieces)
                for g, s, b in zip(got, star[:, 0], bounds[:, 0]):
                    assert abs(g - s) <= b, (n, offset, pieces, g, s, abs(g - s), b)
        # the outputs' bounds follow: the same sums through the public formulas
        want, wb = sx.expected_outputs(x, star, bounds, 1, False, True)
        m = [np.array([g]) for g in got]
        outs = so.outputs(x.astype(F64), *m, ddof=1, bias=False, fisher=True)
        for g, s, b in zip(outs, want, wb):
            assert np.isnan(s[0]) or abs(g[0] - s[0]) <= b[0], (g, s, b)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", [100, 999, 20_000])
def test_bound_is_broken_by_float32_sums(n, weighted):
    """t3 / t4 accumulated in float32 (what an accumulator of 24 bits would give): beyond the bound by orders of magnitude;
    and the bound is a small multiple of n u sum |t_k|, what float64 sums may move, not a loose tolerance"""
    rng = np.random.default_rng(100 + n + weighted)
    v, w = _bin(rng, n, weighted, 1.0)
    x, mean, star, bounds, exact = sx.expected(np.zeros(n, np.int64), v, 1, w)
    assert not exact[0]
    errs = np.array([np.abs(np.array(_kernel_moments(v, mean[0], float(x[0]), w, rng, 4, F32)) - star[:, 0]) for _ in range(4)])
    assert errs[:, 1].max() > 1000 * bounds[1, 0] and errs[:, 2].max() > 1000 * bounds[2, 0], (errs, bounds[:, 0])
    A = [float(np.sum(np.abs(t))) for t in sx.kernel_terms(v, mean[0], w)]
    assert bounds[1, 0] <= 16 * n * U * A[2] and bounds[2, 0] <= 16 * n * U * A[3], (bounds[:, 0], A)


def test_assert_within_catches_what_it_should():
    rng = np.random.default_rng(3)
    flat = np.repeat(np.arange(12), rng.integers(0, 70, 12))
    v = sx.narrow_nan(rng, flat.size)
    x, mean, star, bounds, exact = sx.expected(flat, v, 12)
    np.testing.assert_array_equal(x, np.bincount(flat[~np.isnan(v)], minlength=12))
    sx.assert_within(star[1], star[1], bounds[1], exact)
    j = int(np.flatnonzero(~exact & (x > 2))[0])
    bad = star[1].copy()
    bad[j] -= 4 * bounds[1][j]
    with pytest.raises(AssertionError, match="bound"):
        sx.assert_within(bad, star[1], bounds[1], exact)
    with pytest.raises(AssertionError, match="integers"):
        sx.expected(flat, v, 12, np.full(flat.size, 0.5))
    with pytest.raises(AssertionError, match="narrow"):
        sx.expected(flat, v + 2.0 ** -7, 12)


# ---------------------------------------------------------------------------------------------------------------------
# combine_skew_kurt
# ---------------------------------------------------------------------------------------------------------------------
N_BINS = 9


def _partials(rng, n_parts, weighted, empty=()):
    """narrow-grid data of N_BINS bins split into n_parts: the parts' correctly rounded (x, mean, M2, M3, M4) [5, parts, bins]
    and the whole's [5, bins]"""
    n = 600
    flat = rng.integers(0, N_BINS, n)
    v = sx.narrow(rng, n) + np.where(rng.random(n) < 0.3, 1.5, 0.0)
    w = rng.integers(0, 8, n).astype(F64) if weighted else None
    part = rng.integers(0, n_parts, n)
    part[np.isin(part, empty)] = next(p for p in range(n_parts + 1) if p not in empty) if len(empty) < n_parts else -1

    def moments(sel):
        out = np.full((5, N_BINS), np.nan)
        out[0] = 0.0
        for k in range(N_BINS):
            s = sel & (flat == k)
            out[:, k] = so.bin_moments(v[s], None if w is None else w[s])
        return out

    parts = np.stack([moments(part == p) for p in range(n_parts)], axis=1)
    return parts, moments(part >= 0)


def _merge_err(parts, present):
    """core._pebay_update, as core._merge_partials walks it, restated per bin on skew_kurt_exact.Err scalars, in its order of operations: val is what core must
    give bit for bit; err bounds the distance of the exact merge of the exact partials (each within u of its float64) from
    val, the roundings of every step included"""
    n_parts, n_bins = parts.shape[1:]
    out = np.full((5, n_bins), np.nan)
    errs = np.zeros((5, n_bins))
    for b in range(n_bins):
        cx, run = 0.0, None
        for k in range(n_parts):
            xb = float(parts[0, k, b])
            if not present(xb):
                continue
            new = [Err(parts[i, k, b], U * abs(parts[i, k, b])) for i in range(1, 5)]
            if not present(cx):
                cx, run = xb, new
                continue
            tot = cx + xb
            (cm, c2, c3, c4), (mb, q2, q3, q4) = run, new
            X, B, T = Err(cx), Err(xb), Err(tot)
            d = mb - cm
            n2 = c2 + q2 + d * d * X * B / T
            n3 = c3 + q3 + d * d * d * X * B * (X - B) / (T * T) + 3.0 * d * (X * q2 - B * c2) / T
            n4 = (c4 + q4 + d * d * d * d * X * B * (X * X - X * B + B * B) / (T * T * T)
                  + 6.0 * d * d * (X * X * q2 + B * B * c2) / (T * T) + 4.0 * d * (X * q3 - B * c3) / T)
            run = [cm + d * B / T, n2, n3, n4]
            cx = tot
        out[0, b] = cx
        if run is not None:
            out[1:, b] = [float(r.val) for r in run]
            errs[1:, b] = [float(r.err) * sx.WIDEN for r in run]
    return out, errs


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n_parts,empty", [(2, ()), (3, ()), (7, ()), (3, (1,)), (7, (0, 3, 6)), (2, (0, 1))])
def test_combine_skew_kurt(n_parts, empty, weighted):
    """the data of the narrow grid split into 2, 3 and 7 parts and merged: x, mean and M2 are combine_mean_var's bit for bit,
    all five are the scalar restatement's bit for bit, x is the whole's exactly, and the mean, M2, M3 and M4 of the whole are
    within the restatement's bound.  (A merged mean divides by counts that are no powers of two, so against the whole it is
    held to that bound, which is a few ulps.)  Empty partials are skipped; all partials empty gives NaN."""
    rng = np.random.default_rng(400 + 10 * n_parts + len(empty) + weighted)
    parts, whole = _partials(rng, n_parts, weighted, empty)
    combine = core.combine_weighted_skew_kurt if weighted else core.combine_skew_kurt
    mv = core.combine_weighted_mean_var if weighted else core.combine_mean_var
    got = combine(*[p[:, None] for p in parts], axis=0)
    assert all(g.shape == (1, 1, N_BINS) and g.dtype == F64 for g in got)
    for g, m in zip(got[:3], mv(*[p[:, None] for p in parts[:3]], axis=0)):
        assert np.array_equal(g.view(np.int64), np.asarray(m).view(np.int64))
    val, err = _merge_err(parts, core._weighed if weighted else core._counted)
    for i in range(5):
        g = got[i].reshape(-1)
        assert np.array_equal(np.isnan(g), np.isnan(val[i])) and np.array_equal(g[~np.isnan(g)], val[i][~np.isnan(g)]), i
    np.testing.assert_array_equal(got[0].reshape(-1), whole[0])
    if len(empty) == n_parts:
        assert not got[0].any() and all(np.isnan(g).all() for g in got[1:])
        return
    for i in range(1, 5):
        sx.assert_within(got[i], whole[i], err[i] + U * np.abs(whole[i]), None, "merged moment %d" % i)
        assert np.all(err[i] <= 1e-10 * (1 + np.abs(whole[i])))
    # through the dask step and its last step
    out = (core._skew_kurt_w_reduce if weighted else core._skew_kurt_reduce)(parts, axis=(1,), keepdims=False)
    for i in range(5):
        assert np.array_equal(out[i], got[i].reshape(-1), equal_nan=True)
    last = (core._skew_kurt_w_reduce if weighted else core._skew_kurt_reduce)(parts, axis=(1,), keepdims=False, final=(1, False, False))
    want = so.outputs(out[0], out[2], out[3], out[4], 1, False, False)
    for i, wv in zip((2, 3, 4), want):
        np.testing.assert_allclose(last[i], wv, rtol=1e-14, equal_nan=True)


def test_combine_nan_and_zero_partials():
    """a partial with W == 0 is skipped; a NaN weighted partial (a NaN W) spreads; every partial empty: x 0, the rest NaN"""
    nan = np.nan
    w = np.array([[2.0, 0.0, nan, 0.0], [2.0, 3.0, 1.0, 0.0]])
    m = np.array([[1.0, nan, nan, nan], [3.0, 5.0, 1.0, nan]])
    q = np.array([[0.5, nan, nan, nan], [0.5, 2.0, 1.0, nan]])
    got = core.combine_weighted_skew_kurt(w, m, q, 0.25 * q, 3 * q, axis=0)
    np.testing.assert_array_equal(got[0][0], [4.0, 3.0, nan, 0.0])
    np.testing.assert_array_equal(got[1][0], [2.0, 5.0, nan, nan])
    np.testing.assert_array_equal(got[2][0], [0.5 + 0.5 + 4.0 * 2 * 2 / 4, 2.0, nan, nan])
    # d = 2, na = nb = 2: M3 = M3a + M3b + 0 + 3 d (na M2b - nb M2a) / n = 0.25; M4 = 3 + 8 d^4 / 64 ... written out:
    np.testing.assert_array_equal(got[3][0], [0.125 + 0.125 + 0.0 + 3.0 * 2.0 * (2 * 0.5 - 2 * 0.5) / 4, 0.5, nan, nan])
    np.testing.assert_array_equal(got[4][0], [1.5 + 1.5 + 16.0 * 2 * 2 * (4 - 4 + 4) / 64 + 6.0 * 4.0 * (4 * 0.5 + 4 * 0.5) / 16
                                              + 4.0 * 2.0 * (2 * 0.125 - 2 * 0.125) / 4, 6.0, nan, nan])
    cnt = core.combine_skew_kurt(np.nan_to_num(w), m, q, q, q, axis=0)
    np.testing.assert_array_equal(cnt[0][0], [4.0, 3.0, 1.0, 0.0])
    np.testing.assert_array_equal(cnt[1][0], [2.0, 5.0, 1.0, nan])
    for f in (core._skew_kurt_reduce, core._skew_kurt_w_reduce):
        assert pickle.loads(pickle.dumps(f)).keywords == f.keywords and f.func is core._moment_reduce
    assert core._skew_kurt_w_reduce.keywords["present"] is core._weighed and core._skew_kurt_reduce.keywords["present"] is core._counted


# ---------------------------------------------------------------------------------------------------------------------
# arguments and wiring
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_device_work():
    x = np.linspace(0, 1, 10)
    e = np.linspace(0, 1, 5)
    f = core.histogram_skew_kurt
    with pytest.raises(TypeError):
        f(x, bins=e)  # values are required
    with pytest.raises(TypeError, match="needs values"):
        f(x, values=None, bins=e)
    with pytest.raises(TypeError, match="complex"):
        f(x, values=x + 1j, bins=e)
    with pytest.raises(TypeError, match="complex"):
        f(x, values=x, weights=x + 1j, bins=e)
    with pytest.raises(TypeError):
        f(x, values=x.astype("datetime64[s]"), bins=e)
    for bad in (-1, 1.0, 0.5, "1", None, True):
        with pytest.raises(ValueError, match="ddof"):
            f(x, values=x, bins=e, ddof=bad)
    for bad in (0, 1, None, "yes", 1.0):
        with pytest.raises(TypeError, match="bias"):
            f(x, values=x, bins=e, bias=bad)
        with pytest.raises(TypeError, match="fisher"):
            f(x, values=x, bins=e, fisher=bad)
    with pytest.raises(TypeError, match="sample"):
        f(values=x, bins=e)  # no samples
    for name in ("histogram_skew_kurt", "combine_skew_kurt", "combine_weighted_skew_kurt"):
        assert name in core.__all__
    st = core._VALUE_STATS["skew_kurt"]
    assert (st.k, st.ints, st.extras, st.method, st.ptrs) == (5, (0,), 0, "execute_skew_kurt", (0, 1, 2))
    st = core._VALUE_STATS["skew_kurt_w"]
    assert (st.k, st.ints, st.extras, st.method, st.ptrs) == (5, (), 1, "execute_skew_kurt_weighted", (0, 1, 2))
    doc = f.__doc__
    assert "histogram_mean_var" in doc and "scipy keeps the biased value" in doc and "block_size" in doc


def test_no_gpu_means_loud_failure():
    if _native.device_count() > 0:
        pytest.skip("a GPU is visible here")
    x = np.linspace(0, 1, 10)
    for w in (None, x):
        with pytest.raises(RuntimeError):
            core.histogram_skew_kurt(x, values=x, weights=w, bins=np.linspace(0, 1, 5))


def test_symbols_and_abi_version():
    assert _native.ABI_VERSION == 11
    header = open(os.path.join(ROOT, "include", "xhist_amd.h")).read()
    assert "#define XHIST_ABI_VERSION 11" in header
    lib = _native.load()
    assert lib.xhist_abi_version() == 11
    for name, n_args in (("xhist_plan_execute_skew_kurt", 10), ("xhist_plan_execute_skew_kurt_weighted", 11)):
        assert name in _native.EXPORTS and (name + "(") in header
        assert len(getattr(lib, name).argtypes) == n_args
    assert callable(_native.Plan.execute_skew_kurt) and callable(_native.Plan.execute_skew_kurt_weighted)


xhx = importlib.import_module("xhistogram_amd.xarray")


def _oracle_sk(*args, values, weights=None, bins=None, range=None, axis=None, ddof=0, bias=True, fisher=True, block_size="auto"):
    bins = [bins] * len(args) if isinstance(bins, np.ndarray) else list(bins)
    return so.histogram_skew_kurt(*args, values=values, weights=weights, bins=bins, axis=axis, ddof=ddof, bias=bias, fisher=fisher) + (bins,)


def test_xarray_wrapper_names(monkeypatch):
    monkeypatch.setattr(core, "histogram_skew_kurt", _oracle_sk)
    rng = np.random.default_rng(7)
    dims, shape = ("t", "y", "x"), (2, 3, 40)
    coords = {d: np.arange(n) * 1.0 for d, n in zip(dims, shape)}
    T = xr.DataArray(rng.uniform(0, 1, shape), dims=dims, coords=coords, name="T", attrs={"units": "K"})
    S = xr.DataArray(rng.uniform(0, 1, shape), dims=dims, coords=coords, name="S")
    A = xr.DataArray(rng.standard_normal(shape), dims=dims, coords=coords, name="sst")
    Wt = xr.DataArray(rng.integers(1, 5, shape[1:]).astype(F64), dims=dims[1:], name="area")  # broadcast over t
    bins = [np.linspace(0, 1, 4), np.linspace(0, 1, 3)]
    for wts, first in ((None, "sst_count"), (Wt, "sst_sum_of_weights")):
        out = xhx.histogram_skew_kurt(T, S, values=A, weights=wts, bins=bins, dim=("y", "x"), ddof=1, bias=False, fisher=False)
        assert isinstance(out, tuple) and [o.name for o in out] == [first, "sst_mean", "sst_var", "sst_skew", "sst_kurt"]
        assert all(tuple(o.dims) == ("t", "T_bin", "S_bin") for o in out)
        np.testing.assert_array_equal(out[3]["T_bin"].values, 0.5 * (bins[0][:-1] + bins[0][1:]))
        assert out[1]["T_bin"].attrs == {"units": "K"}
        want = so.histogram_skew_kurt(T.values, S.values, values=A.values, weights=None if wts is None else wts.values[None], bins=bins,
                                      axis=(1, 2), ddof=1, bias=False, fisher=False)
        for g, wv in zip(out, want):
            np.testing.assert_array_equal(np.asarray(g.values), wv)
    out = xhx.histogram_skew_kurt(T, values=xr.DataArray(A.values, dims=dims), bins=[bins[0]])  # nameless, everything reduced
    assert [o.name for o in out] == ["values_count", "values_mean", "values_var", "values_skew", "values_kurt"]
    assert tuple(out[4].dims) == ("T_bin",)
    with pytest.raises(TypeError):
        xhx.histogram_skew_kurt(T, values=A.values, bins=[bins[0]])
    with pytest.raises(TypeError):
        xhx.histogram_skew_kurt(T, values=A, weights=Wt.values, bins=[bins[0]])
    assert "histogram_skew_kurt" in xhx.__all__


def test_census_predictions_of_the_gpu_cases():
    """what the GPU module expects of the launcher, restated without a GPU: the forms, the copies of the 40-byte slot (C2's 100
    bins get 4, C4's 50 get 8), both sides of its borders, and the slots registered in the census tables"""
    assert tg.tvc.SLOTS["skew_kurt"] == ((16, 40), (16, 40)) and tg.tvc.COPIES["skew_kurt"] is True
    cus = 256
    for form in tg.FORMS:
        for sdt in ("f64", "f32"):
            for D in (1, 2):
                edges, xs, v, w, fine, arith = tg.form_data(form, sdt, D)
                want = tg.predict_sk(cus, edges, 0, xs[0].dtype, v.dtype, *tg.FORM_SHAPE, fine, arith)
                assert want["family"] == "fast" and (want["scan"] == 5) == (form == "arith"), (form, sdt, D, want)
                assert want["lds_bytes"][1] - want["lds_bytes"][0] == 24 * want["copies"] * int(np.prod([len(e) - 1 for e in edges]))
    for nb, copies in tg.COPIES:
        for sdt in (F64, F32):
            assert tg.predict_sk(cus, [np.linspace(0, 1, nb + 1)], 0, sdt, sdt, 8, 9 * nb + 1, True, True)["copies"] == copies
    assert dict(tg.COPIES)[100] == 4 and dict(tg.COPIES)[50] == 8
    for i, (border, nb, kind, other, family, home) in enumerate(tg.BORDERS):
        edges, xs, v, w = tg.border_data(i)
        want = tg.predict_sk(cus, edges, 0, F64, v.dtype, *tg.BORDER_SHAPE, True, kind == "lin")
        assert (want["family"], want["slots"]) == (family, home), (tg.BORDERS[i], want)
    for dom in tg.DOMS:
        for home in tg.HOMES:
            edges, xs, v, w, cmp = tg.generic_data(dom, home)
            want = tg.predict_sk(cus, edges, cmp, xs[0].dtype, v.dtype, *xs[0].shape, False)
            assert want["family"] == "generic" and want["slots"] == ("lds" if home == "lds" else "global") and want["cmp"] == cmp
    for form, (st, D, T) in tg.TILE_FORMS.items():
        assert T == 256 * (16 // np.dtype(st).itemsize) * (4 if D == 1 else 8 // (16 // np.dtype(st).itemsize))
        assert tg.tile_cols(form) == (T - 1, T, T + 1)
