"""Weights whose float64 sums are exact, and the comparisons that go with them.

A float64 weight w = +-(2^24 + k) * 2^-25, k in [0, 2^24), has 25 significant bits and lies in [0.5, 1).  Every partial sum of
at most 2^28 of them in one bin is a multiple of 2^-25 below 2^28 in magnitude: it fits 53 bits, so ANY order of float64
additions (LDS atomics, lane copies, workgroup flushes, partial histograms, two-step reductions, all-reduces; mixed signs
included) gives the bits np.bincount gives.  25 bits is more than float32 holds (rounding a weight to float32 changes about half
of them) and no more than the 36 a packed record keeps (packed records carry these weights exactly).  Scaled by 2^-1040 the same
weights are subnormal multiples of 2^-1065 and their sums stay exact: a direct test of flush-to-zero.

float32 weights (2^23 + k) * 2^-24 summed in float64 are exact up to 2^29 samples per bin; a float32 accumulator breaks them.

So every weighted result on such weights is compared with `assert_bits_equal`: the standard int64 counts are held to.  For weights
with full mantissas `assert_within_f64_bound` states what float64 summation in another order may differ by."""
import numpy as np

F64_LIMIT = 1 << 28  # samples per bin below which sums of `f64` weights are exact
F32_LIMIT = 1 << 29  # ... of `f32` weights, summed in float64


def f64(rng, shape, signs="one", scale_log2=0):
    """float64 weights +-(2^24 + k) * 2^-25 (times 2^scale_log2); signs="one": all positive, "both": random signs"""
    k = rng.integers(0, 1 << 24, shape, dtype=np.int64)
    w = np.ldexp((k + (1 << 24)).astype(np.float64), -25 + scale_log2)
    if signs == "both":
        w = np.where(rng.integers(0, 2, shape).astype(bool), -w, w)
    elif signs != "one":
        raise ValueError(signs)
    return w


def f32(rng, shape, signs="one"):
    """float32 weights +-(2^23 + k) * 2^-24: 24 significant bits, [0.5, 1)"""
    k = rng.integers(0, 1 << 23, shape, dtype=np.int64)
    w = np.ldexp((k + (1 << 23)).astype(np.float64), -24).astype(np.float32)
    if signs == "both":
        w = np.where(rng.integers(0, 2, shape).astype(bool), -w, w)
    elif signs != "one":
        raise ValueError(signs)
    return w


def make(dtype, signs="one", scale_log2=0):
    """a weights factory (rng, shape) -> array of `dtype` for the runners of test_gpu_census"""
    if np.dtype(dtype) == np.float32:
        assert scale_log2 == 0
        return lambda rng, shape: f32(rng, shape, signs)
    return lambda rng, shape: f64(rng, shape, signs, scale_log2).astype(dtype)


def assert_summable(counts, dtype=np.float64):
    """no bin of the case holds more samples than the exactness of the weights' sums allows (`counts`: the oracle's counts, or
    an upper bound such as the samples per row)"""
    limit = F32_LIMIT if np.dtype(dtype) == np.float32 else F64_LIMIT
    top = int(np.max(counts)) if np.size(counts) else 0
    assert top < limit, "a bin of %d samples: sums of exact weights are exact below %d" % (top, limit)


def assert_bits_equal(got, want, what=""):
    """identical float64 bits wherever `want` is not NaN (the sign of zero included), NaN exactly where `want` has NaN"""
    got = np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape, what)
    assert got.dtype == want.dtype == np.float64, (got.dtype, want.dtype, what)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "NaN in %d bins, expected in %d (%s)" % (gn.sum(), wn.sum(), what)
    bad = (got.view(np.int64) != want.view(np.int64)) & ~wn
    if bad.any():
        i = np.flatnonzero(bad.reshape(-1))
        g, w = got.reshape(-1)[i], want.reshape(-1)[i]
        rel = np.abs(g - w) / np.maximum(np.abs(w), np.finfo(np.float64).tiny)
        raise AssertionError("%d of %d bins differ in their bits (%s); first at flat %d: %r != %r; largest relative difference %.3g"
                             % (i.size, want.size, what, i[0], g[0], w[0], rel.max()))


def gamma(n):
    """Higham's gamma_n for float64 (u = 2^-53): the relative error bound of a sum of n terms in any order"""
    nu = np.asarray(n, dtype=np.float64) * 2.0 ** -53
    return nu / (1.0 - nu)


def assert_within_f64_bound(got, want, abs_sum, n_per_bin, rounding=0.0, what=""):
    """for weights with full mantissas: |got - want| <= 2 gamma(n_b) A_b + rounding A_b per bin, where A_b is the oracle's
    histogram of |w| and n_b its counts (both results are float64 sums of the same terms in some order).  `rounding` is 2^-37
    where the call's description shows packed records (every weight rounded to 36 mantissa bits), 0 elsewhere.  Bins whose
    expected value is not finite must match exactly."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    a = np.asarray(abs_sum, dtype=np.float64)
    n = np.asarray(n_per_bin)
    assert got.shape == want.shape == a.shape == n.shape, (got.shape, want.shape, a.shape, n.shape, what)
    fin = np.isfinite(want)
    nf_got, nf_want = got[~fin], want[~fin]
    assert np.array_equal(np.isnan(nf_got), np.isnan(nf_want)) and np.array_equal(nf_got[~np.isnan(nf_got)], nf_want[~np.isnan(nf_want)]), \
        "non-finite bins differ (%s)" % what
    assert np.isfinite(got[fin]).all(), "a finite bin came back non-finite (%s)" % what
    bound = 2.0 * gamma(n[fin]) * a[fin] + rounding * a[fin]
    err = np.abs(got[fin] - want[fin])
    bad = err > bound
    if bad.any():
        i = int(np.argmax(np.where(bad, err / np.maximum(bound, np.finfo(np.float64).tiny), 0.0)))
        raise AssertionError("%d of %d bins beyond the float64 bound (%s); worst: |%r - %r| = %.3g > %.3g (n=%d, A=%r)"
                             % (bad.sum(), bad.size, what, got[fin][i], want[fin][i], err[i], bound[i], n[fin][i], a[fin][i]))


def records_rounding(desc):
    """2^-37 where the call's description shows packed weight records (routing: records=packed48, exchange: packed8), else 0"""
    return 2.0 ** -37 if ("records=packed48" in desc or "exchange_records=packed8" in desc) else 0.0
