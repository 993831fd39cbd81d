"""Host statement of histogram_cov's contract (no GPU, no package code): which samples count comes from the oracle's digitize
(meanvar_oracle._flat_bins — numpy.histogram's edge rule), a counted sample contributes its pair (a, b) only if neither value
is NaN (pairwise-complete), and each bin's count, means, M2_a, M2_b (sums of squared deviations) and co-moment C_ab follow.

Two modes, as meanvar_oracle:
  exact=False  exactly rounded sums: math.fsum over each bin's values for the means, then over da^2, db^2 and da*db;
  exact=True   plain float64 np.add.at with the kernels' formula (mean = S / n, d = v - mean, M2 = max(0, sum(d^2) -
               sum(d)^2 / n), C = sum(da db) - sum(da) sum(db) / n) — bit for bit what the GPU gives when every sum is exact
               in any order."""
import math

import numpy as np

from meanvar_oracle import _flat_bins, _rows_cols, var_of  # noqa: F401  (var_of: for the callers)
from oracle.oracle_np import normalise_axis


def cov_rows(samples, edges, a, b, exact=False):
    """[M, C] samples (D arrays), D edge arrays, [M, C] values a and b -> (count int64, mean_a, mean_b, M2_a, M2_b, C_ab) of
    shape [M, nb_0, ..., nb_{D-1}]; everything but the count is NaN where the count is 0"""
    m = samples[0].shape[0]
    ok, flat, nbs = _flat_bins(samples, edges)
    n_bins = int(np.prod(nbs, dtype=np.int64))
    a = np.broadcast_to(np.asarray(a, np.float64), ok.shape)
    b = np.broadcast_to(np.asarray(b, np.float64), ok.shape)
    ok = ok & ~np.isnan(a) & ~np.isnan(b)
    flat = (flat + (np.arange(m, dtype=np.int64) * n_bins)[:, None])[ok]
    a, b = a[ok], b[ok]
    size = m * n_bins
    cnt = np.bincount(flat, minlength=size).astype(np.int64)
    out = [np.full(size, np.nan) for _ in range(5)]  # mean_a, mean_b, M2_a, M2_b, C_ab
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if exact:
            den = np.maximum(cnt, 1)
            sums = []
            for v in (a, b):
                s = np.zeros(size)
                np.add.at(s, flat, v)
                sums.append(np.where(cnt > 0, s / den, np.nan))
            da, db = a - sums[0][flat], b - sums[1][flat]
            acc = []
            for t in (da, db, da * da, db * db, da * db):
                s = np.zeros(size)
                np.add.at(s, flat, t)
                acc.append(s)
            sda, sdb, saa, sbb, sab = acc
            ra = saa - sda * sda / den
            rb = sbb - sdb * sdb / den
            out = [sums[0], sums[1], np.where(cnt > 0, np.where(ra <= 0, 0.0, ra), np.nan),
                   np.where(cnt > 0, np.where(rb <= 0, 0.0, rb), np.nan), np.where(cnt > 0, sab - sda * sdb / den, np.nan)]
        else:
            order = np.argsort(flat, kind="stable")
            fs, as_, bs = flat[order], a[order], b[order]
            starts = np.flatnonzero(np.r_[True, fs[1:] != fs[:-1]]) if len(fs) else np.zeros(0, np.int64)
            ends = np.r_[starts[1:], len(fs)]
            for lo, hi in zip(starts, ends):
                k, va, vb = fs[lo], as_[lo:hi], bs[lo:hi]
                if not (np.isfinite(va).all() and np.isfinite(vb).all()):  # infinities: the means numpy gives, NaN moments
                    out[0][k], out[1][k] = np.mean(va), np.mean(vb)
                    continue
                ma, mb = math.fsum(va) / len(va), math.fsum(vb) / len(vb)
                out[0][k], out[1][k] = ma, mb
                out[2][k] = math.fsum((va - ma) ** 2)
                out[3][k] = math.fsum((vb - mb) ** 2)
                out[4][k] = math.fsum((va - ma) * (vb - mb))
    shape = (m,) + tuple(nbs)
    return (cnt.reshape(shape),) + tuple(o.reshape(shape) for o in out)


def histogram_cov(*args, values, bins, axis=None, ddof=0, exact=False):
    """the N-D contract on numpy inputs with explicit edge arrays (one per argument): (count, mean_a, mean_b, var_a, var_b,
    cov_ab), kept axes then bin axes"""
    va, vb = values
    arrays = np.broadcast_arrays(*[np.asarray(x) for x in args], np.asarray(va), np.asarray(vb))
    samples, a, b = arrays[:-2], arrays[-2], arrays[-1]
    a0 = samples[0]
    axis = normalise_axis(axis, a0.ndim)
    full = axis is None or set(axis) == set(range(a0.ndim))
    kept = () if full else tuple(a0.shape[i] for i in range(a0.ndim) if i not in axis)
    rows = [_rows_cols(s, axis) for s in samples]
    cnt, ma, mb, qa, qb, cc = cov_rows(rows, [np.asarray(e) for e in bins], _rows_cols(a.astype(np.float64), axis),
                                       _rows_cols(b.astype(np.float64), axis), exact=exact)
    out = kept + cnt.shape[1:]
    return (cnt.reshape(out), ma.reshape(out), mb.reshape(out), var_of(cnt, qa, ddof).reshape(out), var_of(cnt, qb, ddof).reshape(out),
            var_of(cnt, cc, ddof).reshape(out))
