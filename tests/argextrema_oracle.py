"""Host statement of histogram_argextrema's contract (no GPU, no package code): which samples count comes from the oracle's
digitize (oracle_np.digitize_inclusive — numpy.histogram's edge rule), the order of the values from extrema_oracle.key
(-0.0 < +0.0), NaN values skipped.  A bin's argmin is the first row of a stable sort by (bin, key, position), its argmax the
first row of the sort by (bin, descending key, position); empty bins hold -1 / NaN.  A position is the column of the [M, C]
arrangement whose columns are the reduced axes in ASCENDING axis number, C order, whatever order `axis` lists them in."""
import numpy as np

from extrema_oracle import key, unkey
from oracle.oracle_np import digitize_inclusive, normalise_axis

_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def counted_bins(samples, edges, values):
    """(ok, flat bin inside the row, bins per input) of [M, C] samples and values"""
    nbs = [len(e) - 1 for e in edges]
    ok = np.ones(samples[0].shape, bool)
    flat = np.zeros(samples[0].shape, np.int64)
    for s, e, nb in zip(samples, edges, nbs):
        code = digitize_inclusive(s, e)  # 1 .. E-1: real bins
        ok &= (code >= 1) & (code <= nb)
        flat = flat * nb + np.clip(code - 1, 0, max(nb - 1, 0))
    ok &= ~np.isnan(np.asarray(values, np.float64))
    return ok, flat, nbs


def _first_per_bin(bins, keys, pos, n_out):
    """per bin: (position, key) of the row with the smallest (key, position); -1 / no key where the bin has no row"""
    order = np.lexsort((pos, keys, bins))  # stable; the last key is the primary one
    b = bins[order]
    first = np.ones(b.size, bool)
    first[1:] = b[1:] != b[:-1]
    at = np.full(n_out, -1, np.int64)
    k = np.zeros(n_out, np.uint64)
    at[b[first]] = pos[order][first]
    k[b[first]] = keys[order][first]
    return at, k


def argextrema_rows(samples, edges, values):
    """[M, C] samples (D arrays), D edge arrays, [M, C] values -> (argmin, argmax, vmin, vmax) of shape [M, nb_0, ..., nb_{D-1}]"""
    m, c = samples[0].shape
    ok, flat, nbs = counted_bins(samples, edges, values)
    n_bins = int(np.prod(nbs, dtype=np.int64))
    flat = (flat + (np.arange(m, dtype=np.int64) * n_bins)[:, None])[ok]
    pos = np.broadcast_to(np.arange(c, dtype=np.int64), (m, c))[ok]
    k = key(np.broadcast_to(np.asarray(values, np.float64), (m, c)))[ok]
    amin, kmin = _first_per_bin(flat, k, pos, m * n_bins)
    amax, kmax = _first_per_bin(flat, ~k, pos, m * n_bins)
    lo = np.where(amin < 0, np.nan, unkey(kmin))
    hi = np.where(amax < 0, np.nan, unkey(~kmax))
    shape = (m,) + tuple(nbs)
    return amin.reshape(shape), amax.reshape(shape), lo.reshape(shape), hi.reshape(shape)


def rows_cols_sorted(a, axis):
    """[M, C]: kept axes -> rows, the reduced axes in ascending axis number -> columns (also for arrays without elements)"""
    a = np.asarray(a)
    full = axis is None or set(axis) == set(range(a.ndim))
    red = list(range(a.ndim)) if full else sorted(axis)
    kept = [i for i in range(a.ndim) if i not in red]
    m = int(np.prod([a.shape[i] for i in kept], dtype=np.int64))
    c = int(np.prod([a.shape[i] for i in red], dtype=np.int64))
    return np.transpose(a, kept + red).reshape(m, c)


def histogram_argextrema(*args, values, bins, axis=None):
    """the N-D contract on numpy inputs with explicit edge arrays (one per argument): (argmin, argmax, vmin, vmax), kept axes,
    then bin axes"""
    arrays = np.broadcast_arrays(*[np.asarray(a) for a in args], np.asarray(values))
    samples, vals = arrays[:-1], arrays[-1]
    a0 = samples[0]
    axis = normalise_axis(axis, a0.ndim)
    full = axis is None or set(axis) == set(range(a0.ndim))
    kept = () if full else tuple(a0.shape[i] for i in range(a0.ndim) if i not in axis)
    rows = [rows_cols_sorted(s, axis) for s in samples]
    outs = argextrema_rows(rows, [np.asarray(b) for b in bins], rows_cols_sorted(vals.astype(np.float64), axis))
    shape = kept + outs[0].shape[1:]
    return tuple(o.reshape(shape) for o in outs)


def definitional(samples, edges, values):
    """loop-and-compare statement for tiny 1-row inputs: a later sample replaces a bin's extreme only where its key is strictly
    beyond it, so the first holder stays"""
    nbs = [len(e) - 1 for e in edges]
    amin = np.full(nbs, -1, np.int64)
    amax = np.full(nbs, -1, np.int64)
    lo = np.full(nbs, np.nan)
    hi = np.full(nbs, np.nan)
    k_of = lambda t: int(key(np.array([t]))[0])  # noqa: E731
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
            idx.append(next(k for k in range(len(e) - 1) if e[k] <= x and (x < e[k + 1] or k == len(e) - 2)))
        if idx is None:
            continue
        idx = tuple(idx)
        if amin[idx] < 0 or k_of(v) < k_of(lo[idx]):
            amin[idx], lo[idx] = i, v
        if amax[idx] < 0 or k_of(v) > k_of(hi[idx]):
            amax[idx], hi[idx] = i, v
    return amin, amax, lo, hi
