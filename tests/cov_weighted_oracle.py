"""Host statement of histogram_weighted_cov's contract (no GPU, no package code): which samples count comes from the oracle's
digitize (meanvar_oracle._flat_bins — numpy.histogram's edge rule), and a counted sample contributes its triple (w, a, b) only
if neither a nor b is NaN, whatever its weight (pairwise-complete; frequency weights):

    W = sum(w),  mean_a = sum(w a) / W,  mean_b = sum(w b) / W,  da = a - mean_a,  db = b - mean_b,
    M2_a = max(0, sum(w da^2) - sum(w da)^2 / W),  M2_b likewise,  C_ab = sum(w da db) - sum(w da) sum(w db) / W  (not clamped),
    var = M2 / (W - ddof),  cov_ab = C_ab / (W - ddof).

Means and moments are NaN where W == 0, variances and covariance where W <= ddof.

Two modes, as cov_oracle and meanvar_weighted_oracle:
  exact=False  exactly rounded sums (math.fsum) of W, of w*a and w*b, then of w*da^2, w*db^2 and w*da*db;
  exact=True   plain float64 np.add.at with the kernels' formula and the kernels' terms, formed in their order: w*a, w*b, then
               wda = w*da, wdb = w*db and wda*da, wda*db, wdb*db — bit for bit what the GPU gives when every sum is exact in
               any order (tests/cov_weighted_exact.py says when)."""
import math

import numpy as np

from meanvar_oracle import _flat_bins, _rows_cols
from meanvar_weighted_oracle import var_of  # noqa: F401  (for the callers too)
from oracle.oracle_np import normalise_axis


def _terms(samples, edges, a, b, w):
    """(row-flat bin of every counted sample with a complete pair, a, b, w, output size, output shape)"""
    m = samples[0].shape[0]
    ok, flat, nbs = _flat_bins(samples, edges)
    n_bins = int(np.prod(nbs, dtype=np.int64))
    a = np.broadcast_to(np.asarray(a, np.float64), ok.shape)
    b = np.broadcast_to(np.asarray(b, np.float64), ok.shape)
    w = np.broadcast_to(np.asarray(w, np.float64), ok.shape)
    ok = ok & ~np.isnan(a) & ~np.isnan(b)
    flat = (flat + (np.arange(m, dtype=np.int64) * n_bins)[:, None])[ok]
    return flat, a[ok], b[ok], w[ok], m * n_bins, (m,) + tuple(nbs)


def cov_w_rows(samples, edges, a, b, w, exact=False):
    """[M, C] samples (D arrays), D edge arrays, [M, C] values a, b and weights w -> (W, mean_a, mean_b, M2_a, M2_b, C_ab) of
    shape [M, nb_0, ..., nb_{D-1}]; everything but W is NaN where W == 0"""
    flat, a, b, w, size, shape = _terms(samples, edges, a, b, w)
    wsum = np.zeros(size)
    out = [np.full(size, np.nan) for _ in range(5)]  # mean_a, mean_b, M2_a, M2_b, C_ab
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if exact:
            np.add.at(wsum, flat, w)
            has = wsum != 0
            den = np.where(has, wsum, 1)
            means = []
            for v in (a, b):
                s = np.zeros(size)
                np.add.at(s, flat, w * v)
                means.append(np.where(has, s / den, np.nan))
            da, db = a - means[0][flat], b - means[1][flat]
            wda, wdb = w * da, w * db
            acc = []
            for t in (wda, wdb, wda * da, wda * db, wdb * db):
                s = np.zeros(size)
                np.add.at(s, flat, t)
                acc.append(s)
            sda, sdb, saa, sab, sbb = acc
            ra = saa - sda * sda / den
            rb = sbb - sdb * sdb / den
            out = [means[0], means[1], np.where(has, np.where(ra <= 0, 0.0, ra), np.nan),
                   np.where(has, np.where(rb <= 0, 0.0, rb), np.nan), np.where(has, sab - sda * sdb / den, np.nan)]
        else:
            order = np.argsort(flat, kind="stable")
            fs, as_, bs, ws = flat[order], a[order], b[order], w[order]
            starts = np.flatnonzero(np.r_[True, fs[1:] != fs[:-1]]) if len(fs) else np.zeros(0, np.int64)
            ends = np.r_[starts[1:], len(fs)]
            for lo, hi in zip(starts, ends):
                k, va, vb, wt = fs[lo], as_[lo:hi], bs[lo:hi], ws[lo:hi]
                if not (np.isfinite(va).all() and np.isfinite(vb).all() and np.isfinite(wt).all()):  # (fsum refuses infinities)
                    wsum[k] = np.sum(wt)
                    if wsum[k] != 0:
                        out[0][k], out[1][k] = np.sum(wt * va) / wsum[k], np.sum(wt * vb) / wsum[k]
                    continue
                W = math.fsum(wt)
                wsum[k] = W
                if W == 0:
                    continue
                ma, mb = math.fsum(wt * va) / W, math.fsum(wt * vb) / W
                out[0][k], out[1][k] = ma, mb
                out[2][k] = max(0.0, math.fsum(wt * (va - ma) ** 2))
                out[3][k] = max(0.0, math.fsum(wt * (vb - mb) ** 2))
                out[4][k] = math.fsum(wt * (va - ma) * (vb - mb))
    return (wsum.reshape(shape),) + tuple(o.reshape(shape) for o in out)


def histogram_weighted_cov(*args, values, weights, bins, axis=None, ddof=0, exact=False):
    """the N-D contract on numpy inputs with explicit edge arrays (one per argument): (W, mean_a, mean_b, var_a, var_b,
    cov_ab), kept axes then bin axes"""
    va, vb = values
    arrays = np.broadcast_arrays(*[np.asarray(x) for x in args], np.asarray(va), np.asarray(vb), np.asarray(weights))
    samples, a, b, w = arrays[:-3], arrays[-3], arrays[-2], arrays[-1]
    a0 = samples[0]
    axis = normalise_axis(axis, a0.ndim)
    full = axis is None or set(axis) == set(range(a0.ndim))
    kept = () if full else tuple(a0.shape[i] for i in range(a0.ndim) if i not in axis)
    rows = [_rows_cols(s, axis) for s in samples]
    W, ma, mb, qa, qb, cc = cov_w_rows(rows, [np.asarray(e) for e in bins], _rows_cols(a.astype(np.float64), axis),
                                       _rows_cols(b.astype(np.float64), axis), _rows_cols(w.astype(np.float64), axis), exact=exact)
    out = kept + W.shape[1:]
    return (W.reshape(out), ma.reshape(out), mb.reshape(out), var_of(W, qa, ddof).reshape(out), var_of(W, qb, ddof).reshape(out),
            var_of(W, cc, ddof).reshape(out))
