"""Host statement of histogram_sum's contract in Python integers (no GPU, no package code): which samples count comes from
the oracle's digitize (oracle_np.digitize_inclusive — numpy.histogram's edge rule), NaN values are dropped, and each bin's
total follows the definition, per (row, bin):

  1. A = the largest |v| of the bin.  Empty bin or A == 0: total = +0.0.  A == inf: step 6.
  2. E = frexp(A)'s exponent (|v| < 2^E), U = max(E - 96, -1074): the unit is 2^U.
  3. v = s * m * 2^e (m the 53-bit integer significand, e = -1074 for subnormals) becomes q = m << (e - U), or m >> (U - e)
     truncated towards zero (0 once the shift reaches 64); q < 2^96, three unsigned 32-bit limbs, s * limb_j added into L0, L1, L2.
  4. S = L0 + L1 * 2^32 + L2 * 2^64.
  5. total = RN_even(S * 2^U): one rounding, overflow to +-inf, a zero result +0.0.
  6. A == inf: NaN if the bin holds both infinities, else the one it holds.

Python integers are unbounded, so nothing here can wrap: the limbs are kept only to state the definition as it is written."""
import math

import numpy as np

from meanvar_oracle import _flat_bins, _rows_cols
from oracle.oracle_np import normalise_axis

UNIT_MIN = -1074


def decompose(v):
    """a finite float64 -> (negative, m, e) with |v| = m * 2^e, m the integer significand (below 2^53), e = -1074 for subnormals"""
    bits = int(np.float64(v).view(np.uint64))
    be = (bits >> 52) & 0x7FF
    frac = bits & ((1 << 52) - 1)
    assert be != 0x7FF, "finite values only"
    return bool(bits >> 63), (frac | (1 << 52)) if be else frac, (be - 1075) if be else -1074


def unit_exponent(a):
    """U of a bin whose largest magnitude is the finite a > 0"""
    return max(math.frexp(a)[1] - 96, UNIT_MIN)


def quantum(v, u):
    """(negative, q): |v| in units of 2^u, truncated towards zero"""
    neg, m, e = decompose(v)
    if e >= u:
        return neg, m << (e - u)
    return neg, (m >> (u - e)) if u - e < 64 else 0


def round_scaled(s, u):
    """RN_even(s * 2^u) as a float64, for an integer s and u >= -1074: +-inf on overflow, +0.0 for zero"""
    if s == 0:
        return 0.0
    neg, mag = s < 0, abs(s)
    nbits = mag.bit_length()
    e_top = u + nbits - 1  # mag * 2^u lies in [2^e_top, 2^(e_top + 1))
    if e_top < -1022:  # subnormal: a whole number of units 2^-1074
        bits = mag << (u + 1074)
        assert bits < (1 << 52)
    else:
        if nbits <= 53:
            mant = mag << (53 - nbits)
        else:
            drop = nbits - 53
            mant, rem, half = mag >> drop, mag & ((1 << drop) - 1), 1 << (drop - 1)
            if rem > half or (rem == half and (mant & 1)):
                mant += 1
            if mant >> 53:
                mant >>= 1
                e_top += 1
        bits = (0x7FF << 52) if e_top > 1023 else ((e_top + 1023) << 52) | (mant & ((1 << 52) - 1))
    return float(np.uint64(bits | ((1 << 63) if neg else 0)).view(np.float64))


def bin_sum(values):
    """(count, total) of one bin's values (NaN ignored), by the definition"""
    v = np.asarray(values, np.float64).reshape(-1)
    v = v[~np.isnan(v)]
    if v.size == 0:
        return 0, 0.0
    a = float(np.max(np.abs(v)))
    if a == 0.0:
        return int(v.size), 0.0
    if math.isinf(a):
        pos, neg = bool(np.any(v == np.inf)), bool(np.any(v == -np.inf))
        return int(v.size), (math.nan if pos and neg else math.inf if pos else -math.inf)
    u = unit_exponent(a)
    acc = [0, 0, 0]
    for x in v.tolist():
        neg, q = quantum(x, u)
        assert q < (1 << 96)
        for j in range(3):
            limb = (q >> (32 * j)) & 0xFFFFFFFF
            acc[j] += -limb if neg else limb
    assert all(abs(a_) < (1 << 63) for a_ in acc)
    return int(v.size), round_scaled(acc[0] + (acc[1] << 32) + (acc[2] << 64), u)


def bound(values):
    """the bound on |total - exact sum| of one bin: n * 2^(E - 96), without the half ulp of the one rounding (0 where the
    unit is the subnormals' or the bin has no finite largest magnitude)"""
    v = np.asarray(values, np.float64).reshape(-1)
    v = v[~np.isnan(v)]
    if v.size == 0 or not np.isfinite(v).all() or not np.any(v):
        return 0.0
    e = math.frexp(float(np.max(np.abs(v))))[1]
    return 0.0 if e - 96 <= UNIT_MIN else v.size * math.ldexp(1.0, e - 96)


def sum_rows(samples, edges, values):
    """[M, C] samples (D arrays), D edge arrays, [M, C] values -> (count int64, total float64) of shape [M, nb_0, ..., nb_{D-1}]"""
    m = samples[0].shape[0]
    ok, flat, nbs = _flat_bins(samples, edges)
    n_bins = int(np.prod(nbs, dtype=np.int64))
    v = np.asarray(values, np.float64)
    ok = ok & ~np.isnan(v)
    flat = (flat + (np.arange(m, dtype=np.int64) * n_bins)[:, None])[ok]
    v = v[ok]
    size = m * n_bins
    cnt = np.bincount(flat, minlength=size).astype(np.int64)
    total = np.zeros(size)
    order = np.argsort(flat, kind="stable")
    fs, vs = flat[order], v[order]
    starts = np.flatnonzero(np.r_[True, fs[1:] != fs[:-1]]) if len(fs) else np.zeros(0, np.int64)
    ends = np.r_[starts[1:], len(fs)]
    for a, b in zip(starts, ends):
        total[fs[a]] = bin_sum(vs[a:b])[1]
    shape = (m,) + tuple(nbs)
    return cnt.reshape(shape), total.reshape(shape)


def histogram_sum(*args, values, bins, axis=None):
    """the N-D contract on numpy inputs with explicit edge arrays (one per argument): (count, total), kept axes then bin axes"""
    arrays = np.broadcast_arrays(*[np.asarray(a) for a in args], np.asarray(values))
    samples, vals = arrays[:-1], arrays[-1]
    a0 = samples[0]
    axis = normalise_axis(axis, a0.ndim)
    full = axis is None or set(axis) == set(range(a0.ndim))
    kept = () if full else tuple(a0.shape[i] for i in range(a0.ndim) if i not in axis)
    rows = [_rows_cols(s, axis) for s in samples]
    cnt, total = sum_rows(rows, [np.asarray(b) for b in bins], _rows_cols(vals.astype(np.float64), axis))
    out = kept + cnt.shape[1:]
    return cnt.reshape(out), total.reshape(out)
