"""Host statement of histogram_extrema's contract (no GPU, no package code): which samples count comes from the oracle's
digitize (oracle_np.digitize_inclusive — numpy.histogram's edge rule), the per-bin extremes from np.minimum.at /
np.maximum.at on order-preserving integer keys of the float64 values, NaN values skipped, empty bins NaN."""
import numpy as np

from oracle.oracle_np import digitize_inclusive, normalise_axis, to_rows_cols

_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
_TOP = np.uint64(1 << 63)


def key(v):
    """uint64 key of float64 values whose unsigned order is the total order with -0.0 < +0.0"""
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return np.where(b >= _TOP, ~b, b | _TOP)


def unkey(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where(k >= _TOP, k & ~_TOP, ~k).view(np.float64)


def extrema_rows(samples, edges, values):
    """[M, C] samples (D arrays), D edge arrays, [M, C] values -> (vmin, vmax) of shape [M, nb_0, ..., nb_{D-1}]"""
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
    ok &= ~np.isnan(v)
    flat = flat + (np.arange(m, dtype=np.int64) * n_bins)[:, None]
    k = key(v)
    kmin = np.full(m * n_bins, _ONES)
    kmax = np.zeros(m * n_bins, np.uint64)
    np.minimum.at(kmin, flat[ok], k[ok])
    np.maximum.at(kmax, flat[ok], k[ok])
    lo = np.where(kmin == _ONES, np.nan, unkey(kmin))
    hi = np.where(kmax == 0, np.nan, unkey(kmax))
    shape = (m,) + tuple(nbs)
    return lo.reshape(shape), hi.reshape(shape)


def _rows_cols(a, axis):
    """to_rows_cols, also for arrays without elements"""
    if a.size:
        return to_rows_cols(a, axis)
    full = axis is None or set(axis) == set(range(a.ndim))
    m = 1 if full else int(np.prod([a.shape[i] for i in range(a.ndim) if i not in axis], dtype=np.int64))
    c = 0 if m else int(np.prod([a.shape[i] for i in range(a.ndim) if full or i in axis], dtype=np.int64))
    return a.reshape(m, c)


def histogram_extrema(*args, values, bins, axis=None):
    """the N-D contract on numpy inputs with explicit edge arrays (one per argument): kept axes, then bin axes"""
    arrays = np.broadcast_arrays(*[np.asarray(a) for a in args], np.asarray(values))
    samples, vals = arrays[:-1], arrays[-1]
    a0 = samples[0]
    axis = normalise_axis(axis, a0.ndim)
    full = axis is None or set(axis) == set(range(a0.ndim))
    kept = () if full else tuple(a0.shape[i] for i in range(a0.ndim) if i not in axis)
    rows = [_rows_cols(s, axis) for s in samples]
    vmin, vmax = extrema_rows(rows, [np.asarray(b) for b in bins], _rows_cols(vals.astype(np.float64), axis))
    out = kept + vmin.shape[1:]
    return vmin.reshape(out), vmax.reshape(out)


def definitional(samples, edges, values):
    """loop-and-compare statement for tiny 1-row inputs: the sorted keys of the values of each bin, first and last"""
    nbs = [len(e) - 1 for e in edges]
    lo = np.full(nbs, np.nan)
    hi = np.full(nbs, np.nan)
    for i in range(len(values)):
        v = float(values[i])
        if v != v:
            continue
        idx = []
        for s, e in zip(samples, edges):
            x = s[i]
            if not (x >= e[0] and x <= e[-1]):
                idx = None
                break
            b = next(k for k in range(len(e) - 1) if e[k] <= x and (x < e[k + 1] or k == len(e) - 2))
            idx.append(b)
        if idx is None:
            continue
        idx = tuple(idx)
        cur = [c for c in (lo[idx], hi[idx], v) if c == c]
        cur.sort(key=lambda t: int(key(np.array([t]))[0]))
        lo[idx], hi[idx] = cur[0], cur[-1]
    return lo, hi
