"""Host statement of histogram_weighted_quantile's contract (no GPU, no package code): which samples count comes from the
oracle's digitize (oracle_np.digitize_inclusive, numpy.histogram's edge rule, as in tests/quantile_oracle.py), and each bin's
quantiles are np.nanquantile(values, q, weights=weights, method="inverted_cdf") of its values and weights as float64.  NaN for a
bin that is empty (no value that is not NaN), whose sum of weights W is not finite and positive, or that holds a NaN or negative
weight: there numpy raises or returns garbage, and the library answers NaN."""
import warnings

import numpy as np

from extrema_oracle import _rows_cols
from oracle.oracle_np import digitize_inclusive, normalise_axis


def bin_quantiles(v, w, q):
    """one bin: float64 values v and weights w of its counted samples, 1-D q -> len(q) quantiles"""
    q = np.asarray(q, np.float64).ravel()
    keep = ~np.isnan(v)  # (a NaN value contributes nothing, whatever its weight)
    v, w = v[keep], w[keep]
    nan = np.full(len(q), np.nan)
    if v.size == 0 or not np.all(w >= 0):  # (NaN fails w >= 0)
        return nan
    with np.errstate(over="ignore"):
        total = np.cumsum(w)[-1]  # (numpy's own W: cdf[-1] of the weights in sorted order; exact weights sum alike in any order)
    if not (total > 0 and np.isfinite(total)):
        return nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.asarray(np.nanquantile(v, q, weights=w, method="inverted_cdf"), np.float64)


def weighted_quantile_rows(samples, edges, values, weights, q):
    """[M, C] samples (D arrays), D edge arrays, [M, C] values and weights, 1-D q -> ([len(q), M, nb_0, ..., nb_{D-1}]
    quantiles, [M, nb_0, ...] counts of the values that are not NaN)"""
    q = np.asarray(q, np.float64).ravel()
    m = samples[0].shape[0]
    nbs = [len(e) - 1 for e in edges]
    n_bins = int(np.prod(nbs, dtype=np.int64))
    ok = np.ones(samples[0].shape, bool)
    flat = np.zeros(samples[0].shape, np.int64)
    for s, e, nb in zip(samples, edges, nbs):
        code = digitize_inclusive(s, e)  # 1 .. E-1: real bins
        ok &= (code >= 1) & (code <= nb)
        flat = flat * nb + np.clip(code - 1, 0, max(nb - 1, 0))
    v = np.asarray(values, np.float64)
    w = np.asarray(weights, np.float64)
    flat = flat + (np.arange(m, dtype=np.int64) * n_bins)[:, None]
    out = np.full((len(q), m * n_bins), np.nan)
    counts = np.zeros(m * n_bins, np.int64)
    f, vv, ww = flat[ok], v[ok], w[ok]
    order = np.argsort(f, kind="stable")
    f, vv, ww = f[order], vv[order], ww[order]
    ids, starts = np.unique(f, return_index=True)
    ends = np.r_[starts[1:], len(f)]
    for b, s0, s1 in zip(ids, starts, ends):
        out[:, b] = bin_quantiles(vv[s0:s1], ww[s0:s1], q)
        counts[b] = np.count_nonzero(~np.isnan(vv[s0:s1]))
    return out.reshape((len(q), m) + tuple(nbs)), counts.reshape((m,) + tuple(nbs))


def histogram_weighted_quantile(*args, values, weights, q, bins, axis=None, return_counts=False):
    """the N-D contract on numpy inputs with explicit edge arrays (one per argument): [len(q)] (when q is 1-D), kept axes, then
    bin axes; with return_counts also the values per bin (for exact_weights.assert_summable)"""
    arrays = np.broadcast_arrays(*[np.asarray(a) for a in args], np.asarray(values), np.asarray(weights))
    samples, vals, wts = arrays[:-2], arrays[-2], arrays[-1]
    a0 = samples[0]
    axis = normalise_axis(axis, a0.ndim)
    full = axis is None or set(axis) == set(range(a0.ndim))
    kept = () if full else tuple(a0.shape[i] for i in range(a0.ndim) if i not in axis)
    rows = [_rows_cols(s, axis) for s in samples]
    res, counts = weighted_quantile_rows(rows, [np.asarray(b) for b in bins], _rows_cols(vals.astype(np.float64), axis),
                                         _rows_cols(wts.astype(np.float64), axis), np.atleast_1d(q))
    res = res.reshape((res.shape[0],) + kept + res.shape[2:])
    res = res[0] if np.ndim(q) == 0 else res
    return (res, counts.reshape(kept + counts.shape[1:])) if return_counts else res
