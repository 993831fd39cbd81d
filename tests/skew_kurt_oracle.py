"""Host statement of histogram_skew_kurt's contract (no GPU, no package code), from the definition and from the raw values.

Which samples count comes from the oracle's digitize (meanvar_oracle._flat_bins: numpy.histogram's edge rule), NaN values are
dropped, and each bin's x (the count, or the sum of weights W), mean and central moments follow in exact rational arithmetic:
every finite float64 is an integer times a power of two, so with values v_i = k_i 2^s and weights w_i = u_i 2^t (Python ints)

    U = sum(u_i),  S = sum(u_i k_i),  mean = S / U 2^s,  M_j = sum(u_i (k_i U - S)^j) / U^j 2^(s j + t)      (j = 2, 3, 4)

are ratios of integers, rounded to float64 once (Fraction -> float is correctly rounded).  Nothing here forms the kernels' terms
d, t1 .. t4 or their corrections; that is tests/skew_kurt_exact.py's business.

The outputs restate the public formulas, in the order the issue gives them:
    var  = M2 / (x - ddof), NaN where x <= ddof
    m2 = M2 / x,  g1 = (M3 / x) / (m2 sqrt(m2)),  g2 = (M4 / x) / (m2 m2),  both NaN where x == 0 or M2 == 0
    bias=False:  G1 = sqrt(x (x - 1)) / (x - 2) g1, NaN where x <= 2
                 G2 = (x - 1) / ((x - 2) (x - 3)) ((x + 1) g2 - 3 (x - 1)) + 3, NaN where x <= 3
    skew = g1 (G1),  kurt = g2 (G2), minus 3 under fisher
A bin that holds a NaN weight is NaN in every output; infinite values are not handled here (the tests that use this module
have none)."""
from fractions import Fraction

import numpy as np

from meanvar_oracle import _flat_bins, _rows_cols
from oracle.oracle_np import normalise_axis


def _ints(a):
    """(Python ints k as an object array, s) with a == k * 2^s exactly, for finite float64 values"""
    a = np.asarray(a, np.float64)
    if a.size == 0:
        return np.zeros(0, object), 0
    m, e = np.frexp(a)  # a = m 2^e, 0.5 <= |m| < 1: m 2^53 is an integer
    nz = a != 0
    s = int(np.min(e[nz])) - 53 if nz.any() else 0
    k = np.array([int(x) for x in np.ldexp(m, 53)], object)
    sh = np.array([int(x) for x in np.where(nz, e - 53 - s, 0)], object)
    return k * (2 ** sh), s


def bin_moments(vals, weights=None):
    """(x, mean, M2, M3, M4) of one bin's values (no NaN among them), correctly rounded; weights None: x = the count"""
    n = len(vals)
    if n == 0:
        return 0.0, np.nan, np.nan, np.nan, np.nan
    if weights is not None and np.isnan(weights).any():
        return (np.nan,) * 5
    k, s = _ints(vals)
    if weights is None:
        u, t = np.array([1] * n, object), 0
    else:
        u, t = _ints(weights)
    U = int(np.sum(u))
    x = float(Fraction(U) * Fraction(2) ** t)
    if U == 0:
        return x, np.nan, np.nan, np.nan, np.nan
    S = int(np.sum(u * k))
    c = k * U - S
    two = Fraction(2)
    out = [x, float(Fraction(S, U) * two ** s)]
    for j in (2, 3, 4):
        out.append(float(Fraction(int(np.sum(u * c ** j)), U ** j) * two ** (s * j + t)))
    return tuple(out)


def moments_rows(samples, edges, values, weights=None):
    """[M, C] samples (D arrays), D edge arrays, [M, C] values (and weights) -> (x, mean, M2, M3, M4), each float64 of shape
    [M, nb_0, ..., nb_{D-1}]; x is the count as float64, or W"""
    m = samples[0].shape[0]
    ok, flat, nbs = _flat_bins(samples, edges)
    n_bins = int(np.prod(nbs, dtype=np.int64))
    v = np.broadcast_to(np.asarray(values, np.float64), ok.shape)
    ok = ok & ~np.isnan(v)
    flat = (flat + (np.arange(m, dtype=np.int64) * n_bins)[:, None])[ok]
    v = v[ok]
    w = None if weights is None else np.broadcast_to(np.asarray(weights, np.float64), ok.shape)[ok]
    size = m * n_bins
    out = np.full((5, size), np.nan)
    out[0] = 0.0
    order = np.argsort(flat, kind="stable")
    fs = flat[order]
    starts = np.flatnonzero(np.r_[True, fs[1:] != fs[:-1]]) if len(fs) else np.zeros(0, np.int64)
    ends = np.r_[starts[1:], len(fs)]
    for a, b in zip(starts, ends):
        sel = order[a:b]
        out[:, fs[a]] = bin_moments(v[sel], None if w is None else w[sel])
    shape = (m,) + tuple(nbs)
    return tuple(o.reshape(shape) for o in out)


def outputs(x, m2, m3, m4, ddof=0, bias=True, fisher=True):
    """(var, skew, kurt) from x and the central moments' sums, by the public formulas (module docstring)"""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        var = np.where(x > ddof, m2 / (x - ddof), np.nan)
        v = m2 / x
        ok = (x != 0) & (m2 != 0)
        g1 = np.where(ok, (m3 / x) / (v * np.sqrt(v)), np.nan)
        g2 = np.where(ok, (m4 / x) / (v * v), np.nan)
        if not bias:
            g1 = np.where(x <= 2, np.nan, np.sqrt(x * (x - 1.0)) / (x - 2.0) * g1)
            g2 = np.where(x <= 3, np.nan, (x - 1.0) / ((x - 2.0) * (x - 3.0)) * ((x + 1.0) * g2 - 3.0 * (x - 1.0)) + 3.0)
        if fisher:
            g2 = g2 - 3.0
    return var, g1, g2


def histogram_skew_kurt(*args, values, bins, axis=None, weights=None, ddof=0, bias=True, fisher=True):
    """the N-D contract on numpy inputs with explicit edge arrays (one per argument): (count int64 | W, mean, var, skew, kurt),
    kept axes then bin axes"""
    extra = [] if weights is None else [np.asarray(weights)]
    arrays = np.broadcast_arrays(*[np.asarray(a) for a in args], np.asarray(values), *extra)
    samples, vals = arrays[:len(args)], arrays[len(args)]
    a0 = samples[0]
    axis = normalise_axis(axis, a0.ndim)
    full = axis is None or set(axis) == set(range(a0.ndim))
    kept = () if full else tuple(a0.shape[i] for i in range(a0.ndim) if i not in axis)
    rows = [_rows_cols(s, axis) for s in samples]
    w = None if weights is None else _rows_cols(arrays[-1].astype(np.float64), axis)
    x, mean, m2, m3, m4 = moments_rows(rows, [np.asarray(b) for b in bins], _rows_cols(vals.astype(np.float64), axis), w)
    var, skew, kurt = outputs(x, m2, m3, m4, ddof, bias, fisher)
    out = kept + x.shape[1:]
    first = x.astype(np.int64) if weights is None else x
    return tuple(a.reshape(out) for a in (first, mean, var, skew, kurt))
