"""Host statement of histogram_mean_var's weighted contract (no GPU, no package code): which samples count comes from
meanvar_oracle (numpy.histogram's edge rule, NaN values dropped), and each counted sample contributes its pair (w, v):

    W = sum(w),  mean = sum(w v) / W,  d = v - mean,  M2 = max(0, sum(w d^2) - sum(w d)^2 / W),  var = M2 / (W - ddof)

mean and M2 are NaN where W == 0, var where W <= ddof.

Two modes:
  exact=False  exactly rounded sums (math.fsum) of W, of w*v and of w*(v - mean)^2 — the reference of the random-data tests;
  exact=True   plain float64 np.add.at with the kernels' formula (the terms w*v, w*d and (w*d)*d as the kernels form them) —
               bit for bit what the GPU gives when every sum is exact in any order.

When the sums are exact (`exact=True` is then the answer bit for bit).  Values on values_exact.grid (k 2^-10, |k| < 2^12) and
integer weights m in 0..7: every w*v is a multiple of 2^-10 below 2^15, so S and W are exact for fewer than 2^31 samples per
bin, and mean = fl(S / W) bit for bit for any W.  When W = 2^j the mean is exact as well: d = v - mean is a multiple of
2^-(10 + j) below 2^13 (13 + j significant bits at most, as in values_exact), w*d holds 16 + j bits, (w*d)*d at most
29 + 2j, and a sum of at most W such terms at most 29 + 3j bits: exact in any order while 29 + 3j <= 53, i.e. j <= 8, W <= 2^8
(POW2_EXACT).  Other W: `m2_bound` bounds the distance of the kernel's M2 from the exact M2 of the terms it adds."""
import math

import numpy as np

from meanvar_oracle import _flat_bins, _rows_cols
from oracle.oracle_np import normalise_axis

U = 2.0 ** -53
POW2_EXACT = 1 << 8  # the largest power-of-two W whose M2 is exact (integer weights <= 7, values on the grid)


def gamma(n):
    nu = float(n) * U
    return nu / (1.0 - nu)


def _terms(samples, edges, values, weights):
    """(row-flat bin of every counted sample with a value, v, w, output size, bins shape)"""
    m = samples[0].shape[0]
    ok, flat, nbs = _flat_bins(samples, edges)
    n_bins = int(np.prod(nbs, dtype=np.int64))
    v = np.asarray(values, np.float64)
    w = np.asarray(weights, np.float64)
    ok &= ~np.isnan(v)
    flat = (flat + (np.arange(m, dtype=np.int64) * n_bins)[:, None])[ok]
    return flat, v[ok], w[ok], m * n_bins, (m,) + tuple(nbs)


def mean_var_w_rows(samples, edges, values, weights, exact=False):
    """[M, C] samples (D arrays), D edge arrays, [M, C] values and weights -> (W, mean, M2), each [M, nb_0, ..., nb_{D-1}]"""
    flat, v, w, size, shape = _terms(samples, edges, values, weights)
    wsum = np.zeros(size)
    mean = np.full(size, np.nan)
    m2 = np.full(size, np.nan)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if exact:
            np.add.at(wsum, flat, w)
            s = np.zeros(size)
            np.add.at(s, flat, w * v)
            mean = np.where(wsum != 0, s / np.where(wsum != 0, wsum, 1), np.nan)
            d = v - mean[flat]
            wd = w * d
            sd = np.zeros(size)
            s2 = np.zeros(size)
            np.add.at(sd, flat, wd)
            np.add.at(s2, flat, wd * d)
            r = s2 - sd * sd / np.where(wsum != 0, wsum, 1)
            m2 = np.where(wsum != 0, np.where(r <= 0, 0.0, r), np.nan)
        else:
            order = np.argsort(flat, kind="stable")
            fs, vs, ws = flat[order], v[order], w[order]
            starts = np.flatnonzero(np.r_[True, fs[1:] != fs[:-1]]) if len(fs) else np.zeros(0, np.int64)
            ends = np.r_[starts[1:], len(fs)]
            for a, b in zip(starts, ends):
                k, vals, wts = fs[a], vs[a:b], ws[a:b]
                if not (np.isfinite(vals).all() and np.isfinite(wts).all()):  # (fsum refuses infinities; NaN spreads)
                    wsum[k] = np.sum(wts)
                    mean[k] = np.sum(wts * vals) / wsum[k] if wsum[k] != 0 else np.nan
                    m2[k] = np.nan
                    continue
                W = math.fsum(wts)
                wsum[k] = W
                if W == 0:
                    continue
                mu = math.fsum(wts * vals) / W
                mean[k] = mu
                m2[k] = max(0.0, math.fsum(wts * (vals - mu) ** 2))
    return wsum.reshape(shape), mean.reshape(shape), m2.reshape(shape)


def m2_bound(samples, edges, values, weights, mean):
    """per bin, how far a float64 M2 of the kernels' terms may be from the exact M2 of those terms (given the kernel's `mean`):
    with n terms, Q = sum((w d) d), A = sum(|w d|), W = sum(w) — |M2 - M2*| <= g(n + 3) (Q + A^2 / |W|) + g(n + 3) A, where the
    first term covers the sums of n rounded products (Higham 4.2) and the correction's division, the second the rounding of
    d and w*d.  Widened by 4x for the host's own arithmetic."""
    flat, v, w, size, shape = _terms(samples, edges, values, weights)
    mu = np.asarray(mean, np.float64).reshape(-1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = v - mu[flat]
        wd = np.abs(w * d)
        q = np.zeros(size)
        a = np.zeros(size)
        n = np.zeros(size)
        wsum = np.zeros(size)
        np.add.at(q, flat, np.abs(wd * d))
        np.add.at(a, flat, wd)
        np.add.at(n, flat, 1.0)
        np.add.at(wsum, flat, w)
        g = (n + 3) * U / (1 - (n + 3) * U)
        b = 4 * g * (q + a * a / np.where(wsum != 0, np.abs(wsum), 1) + a)
    return b.reshape(shape)


def histogram_mean_var_w(*args, values, weights, bins, axis=None, ddof=0, exact=False):
    """the N-D contract on numpy inputs with explicit edge arrays: (W, mean, var), kept axes then bin axes"""
    arrays = np.broadcast_arrays(*[np.asarray(a) for a in args], np.asarray(values), np.asarray(weights))
    samples, vals, wts = arrays[:-2], arrays[-2], arrays[-1]
    a0 = samples[0]
    axis = normalise_axis(axis, a0.ndim)
    full = axis is None or set(axis) == set(range(a0.ndim))
    kept = () if full else tuple(a0.shape[i] for i in range(a0.ndim) if i not in axis)
    rows = [_rows_cols(s, axis) for s in samples]
    wsum, mean, m2 = mean_var_w_rows(rows, [np.asarray(b) for b in bins], _rows_cols(vals.astype(np.float64), axis),
                                     _rows_cols(wts.astype(np.float64), axis), exact=exact)
    out = kept + wsum.shape[1:]
    return wsum.reshape(out), mean.reshape(out), var_of(wsum, m2, ddof).reshape(out)


def var_of(wsum, m2, ddof):
    """M2 / (W - ddof), NaN where W <= ddof"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(wsum > ddof, m2 / (wsum - ddof), np.nan)


def var_bound(wsum, m2, b, ddof):
    """(var, its bound, exact) from the exact mode's W and M2 and m2_bound's b: var = M2 / (W - ddof) is bit for bit (`exact`)
    where W is a power of two up to POW2_EXACT and above ddof; elsewhere the kernels' lies within b / (W - ddof) plus the
    division's and the host's roundings, 4 U |var|"""
    var = var_of(wsum, m2, ddof)
    lg = np.log2(np.where(wsum > 0, wsum, 1))
    pow2 = (wsum > ddof) & (wsum <= POW2_EXACT) & (lg == np.round(lg))
    with np.errstate(invalid="ignore", divide="ignore"):
        lim = b / np.where(wsum > ddof, wsum - ddof, 1) + 4 * U * np.abs(var)
    return var, lim, pow2
