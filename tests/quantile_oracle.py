"""Host statement of histogram_quantile's contract (no GPU, no package code): which samples count comes from the oracle's
digitize (oracle_np.digitize_inclusive, numpy.histogram's edge rule, as in tests/extrema_oracle.py), and each bin's quantiles are
np.nanquantile of its values as float64, NaN for a bin without a value."""
import warnings

import numpy as np

from extrema_oracle import _rows_cols
from oracle.oracle_np import digitize_inclusive, normalise_axis


def quantile_rows(samples, edges, values, q, method="linear"):
    """[M, C] samples (D arrays), D edge arrays, [M, C] values, 1-D q -> [len(q), M, nb_0, ..., nb_{D-1}]"""
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
    flat = flat + (np.arange(m, dtype=np.int64) * n_bins)[:, None]
    out = np.full((len(q), m * n_bins), np.nan)
    f, vv = flat[ok], v[ok]
    order = np.argsort(f, kind="stable")
    f, vv = f[order], vv[order]
    ids, starts = np.unique(f, return_index=True)
    ends = np.r_[starts[1:], len(f)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (all-NaN bins)
        for b, s0, s1 in zip(ids, starts, ends):
            out[:, b] = np.nanquantile(vv[s0:s1], q, method=method)
    return out.reshape((len(q), m) + tuple(nbs))


def histogram_quantile(*args, values, q, bins, axis=None, method="linear"):
    """the N-D contract on numpy inputs with explicit edge arrays (one per argument): [len(q)] (when q is 1-D), kept axes, then
    bin axes"""
    arrays = np.broadcast_arrays(*[np.asarray(a) for a in args], np.asarray(values))
    samples, vals = arrays[:-1], arrays[-1]
    a0 = samples[0]
    axis = normalise_axis(axis, a0.ndim)
    full = axis is None or set(axis) == set(range(a0.ndim))
    kept = () if full else tuple(a0.shape[i] for i in range(a0.ndim) if i not in axis)
    rows = [_rows_cols(s, axis) for s in samples]
    res = quantile_rows(rows, [np.asarray(b) for b in bins], _rows_cols(vals.astype(np.float64), axis), np.atleast_1d(q), method)
    res = res.reshape((res.shape[0],) + kept + res.shape[2:])
    return res[0] if np.ndim(q) == 0 else res
