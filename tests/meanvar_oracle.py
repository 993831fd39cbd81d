"""Host statement of histogram_mean_var's contract (no GPU, no package code): which samples count comes from the oracle's
digitize (oracle_np.digitize_inclusive — numpy.histogram's edge rule), NaN values are dropped, and each bin's count, mean and
M2 (sum of squared deviations) follow.

Two modes:
  exact=False  exactly rounded sums: math.fsum over each bin's values for the mean, then over (v - mean)^2 for M2 — the
               reference of the random-data tests;
  exact=True   plain float64 np.add.at with the kernels' formula (mean = S / n, d = v - mean, M2 = max(0, sum(d^2) -
               sum(d)^2 / n)) — bit for bit what the GPU gives when every sum is exact in any order."""
import math

import numpy as np

from oracle.oracle_np import digitize_inclusive, normalise_axis, to_rows_cols


def _flat_bins(samples, edges):
    """(counted mask, flat bin index) of [M, C] samples"""
    nbs = [len(e) - 1 for e in edges]
    ok = np.ones(samples[0].shape, bool)
    flat = np.zeros(samples[0].shape, np.int64)
    for s, e, nb in zip(samples, edges, nbs):
        code = digitize_inclusive(s, e)  # 1 .. E-1: real bins
        ok &= (code >= 1) & (code <= nb)
        flat = flat * nb + np.clip(code - 1, 0, max(nb - 1, 0))
    return ok, flat, nbs


def mean_var_rows(samples, edges, values, exact=False):
    """[M, C] samples (D arrays), D edge arrays, [M, C] values -> (count int64, mean, M2) of shape [M, nb_0, ..., nb_{D-1}];
    mean and M2 are NaN where the count is 0"""
    m = samples[0].shape[0]
    ok, flat, nbs = _flat_bins(samples, edges)
    n_bins = int(np.prod(nbs, dtype=np.int64))
    v = np.asarray(values, np.float64)
    ok &= ~np.isnan(v)
    flat = (flat + (np.arange(m, dtype=np.int64) * n_bins)[:, None])[ok]
    v = v[ok]
    size = m * n_bins
    cnt = np.bincount(flat, minlength=size).astype(np.int64)
    mean = np.full(size, np.nan)
    m2 = np.full(size, np.nan)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if exact:
            s = np.zeros(size)
            np.add.at(s, flat, v)
            mean = np.where(cnt > 0, s / np.maximum(cnt, 1), np.nan)
            d = v - mean[flat]
            sd = np.zeros(size)
            s2 = np.zeros(size)
            np.add.at(sd, flat, d)
            np.add.at(s2, flat, d * d)
            r = s2 - sd * sd / np.maximum(cnt, 1)
            m2 = np.where(cnt > 0, np.where(r <= 0, 0.0, r), np.nan)
        else:
            order = np.argsort(flat, kind="stable")
            fs, vs = flat[order], v[order]
            starts = np.flatnonzero(np.r_[True, fs[1:] != fs[:-1]]) if len(fs) else np.zeros(0, np.int64)
            ends = np.r_[starts[1:], len(fs)]
            for a, b in zip(starts, ends):
                k, vals = fs[a], vs[a:b]
                if not np.isfinite(vals).all():  # what np.nanmean / np.nanvar give with infinities: fsum refuses them
                    mean[k] = np.mean(vals)
                    m2[k] = np.nan
                    continue
                mu = math.fsum(vals) / len(vals)
                mean[k] = mu
                m2[k] = math.fsum((vals - mu) ** 2)
    shape = (m,) + tuple(nbs)
    return cnt.reshape(shape), mean.reshape(shape), m2.reshape(shape)


def var_of(cnt, m2, ddof):
    """M2 / (n - ddof), NaN where n <= ddof"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(cnt > ddof, m2 / (cnt - ddof), np.nan)


def _rows_cols(a, axis):
    """to_rows_cols, also for arrays without elements"""
    if a.size:
        return to_rows_cols(a, axis)
    full = axis is None or set(axis) == set(range(a.ndim))
    m = 1 if full else int(np.prod([a.shape[i] for i in range(a.ndim) if i not in axis], dtype=np.int64))
    c = 0 if m else int(np.prod([a.shape[i] for i in range(a.ndim) if full or i in axis], dtype=np.int64))
    return a.reshape(m, c)


def histogram_mean_var(*args, values, bins, axis=None, ddof=0, exact=False):
    """the N-D contract on numpy inputs with explicit edge arrays (one per argument): (count, mean, var), kept axes then bin
    axes"""
    arrays = np.broadcast_arrays(*[np.asarray(a) for a in args], np.asarray(values))
    samples, vals = arrays[:-1], arrays[-1]
    a0 = samples[0]
    axis = normalise_axis(axis, a0.ndim)
    full = axis is None or set(axis) == set(range(a0.ndim))
    kept = () if full else tuple(a0.shape[i] for i in range(a0.ndim) if i not in axis)
    rows = [_rows_cols(s, axis) for s in samples]
    cnt, mean, m2 = mean_var_rows(rows, [np.asarray(b) for b in bins], _rows_cols(vals.astype(np.float64), axis), exact=exact)
    out = kept + cnt.shape[1:]
    return cnt.reshape(out), mean.reshape(out), var_of(cnt, m2, ddof).reshape(out)
