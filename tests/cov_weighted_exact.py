"""What histogram_weighted_cov must give for ANY sum of weights per bin on exactly summable data: both value arrays on the grid
of tests/values_exact.py (k * 2^-10, |k| < 2^12), the weights integers 0..7.  The analysis of tests/cov_exact.py and of
tests/meanvar_weighted_oracle.py, put together.

A triple counts only if neither value is NaN.  Every w, w*a and w*b is a multiple of 2^-10 below 2^15, so every partial sum of
fewer than 2^31 of them fits 53 bits: W, Swa and Swb are exact in any order, hence

    W,  mean_a = fl(Swa / W),  mean_b = fl(Swb / W)         bit for bit, for every bin.

With W = 2^j <= 2^8 (meanvar_weighted_oracle.POW2_EXACT) both means are exact, and so are da = a - mean_a and db = b - mean_b:
multiples of 2^-(10 + j) below 2^3 in magnitude, 13 + j significant bits at most.  wda = w*da holds 16 + j bits, (wda)*db and
(wda)*da at most 29 + 2j, multiples of 2^-(20 + 2j); a partial sum of the terms of a bin is below sum(w) * 2^6 = 2^(6 + j) in
magnitude, so it holds at most 26 + 3j bits <= 29 + 3j <= 53: exact in any order.  sum(wda) = Swa - W mean_a = 0 and
sum(wdb) = 0 exactly, so M2_a, M2_b and C_ab are bit for bit (cov_weighted_oracle's exact mode).

Other W: with n the number of triples of the bin, W its exact sum of weights, and for a pair of deviation arrays (dx, dy) among
(da, da), (da, db), (db, db) the very terms the kernel adds, wdx = fl(w dx), wdy = fl(w dy), p = fl(wdx dy) — C = sum(p),
P = sum |p|, Dx = sum(wdx), Dy = sum(wdy), Ax = sum |wdx|, Ay = sum |wdy| (exact sums; u = 2^-53, g(k) = k u / (1 - k u)):

  C^  = C + t,                 |t| <= g(n) P                (a float64 sum of n terms of either sign in any order; Higham 4.2)
  Dx^ = Dx + ex, Dy^ = Dy + ey,  |ex| <= Ex = g(n) Ax, |ey| <= Ey = g(n) Ay
  T^  = fl(fl(Dx^ Dy^) / W),   |T^ - Dx Dy / W| <= (|Dx| Ey + |Dy| Ex + Ex Ey + g(2) (|Dx| + Ex) (|Dy| + Ey)) / W
  R^  = fl(C^ - T^),           |R^ - (C^ - T^)| <= u (|C^| + |T^|) <= u ((1 + g(n)) P + (1 + g(2)) (|Dx| + Ex) (|Dy| + Ey) / W)

This is cov_exact's derivation with the weighted sums of |wdx| and |wdy| in the place of the sums of |da| and |db| and W in the
place of n in the correction term (W is exact on this data, and W > 0 where anything is checked).  With C* = C - Dx Dy / W

  |R^ - C*| <= g(n) P + (|Dx| Ey + |Dy| Ex + Ex Ey + g(2) DEx DEy) / W + u ((1 + g(n)) P + (1 + g(2)) DEx DEy / W) =: B,

DEx = |Dx| + Ex, DEy = |Dy| + Ey.  C_ab is R^ itself.  The M2 are max(0, R^) of the pairs (da, da) and (db, db); max(0, .) moves
two numbers no further apart, so |M2 - max(0, C*)| <= B as well.  The host evaluates the six sums with math.fsum and C* in three
more operations; as in cov_exact, B is widened by g(6) (P + |Dx Dy| / W) for that and by g(4) B for its own arithmetic.
var = M2 / (W - ddof) and cov = C_ab / (W - ddof) then carry B / (W - ddof) plus one more rounding (values_exact.var_bound).

No tolerance is picked by hand.  Adding p in float32 breaks B by orders of magnitude: tests/test_cov_weighted_cpu.py shows it."""
import math

import numpy as np

import values_exact as vx
from meanvar_weighted_oracle import POW2_EXACT
from values_exact import U, gamma

W_MAX = 7  # the integer weights are 0..7


def kernel_terms(x, y, w, mean_x, mean_y):
    """wdx = fl(w * fl(x - mean_x)), wdy likewise, and p = fl(wdx * dy), the terms the kernels add for one bin"""
    dx = np.asarray(x, np.float64) - mean_x
    dy = np.asarray(y, np.float64) - mean_y
    w = np.asarray(w, np.float64)
    wdx, wdy = w * dx, w * dy
    return wdx, wdy, wdx * dy


def c_star_and_bound(x, y, w, mean_x, mean_y, W):
    """(C*, B) of the module docstring for the triples of one bin (float64), its means fl(S / W) and its sum of weights W > 0"""
    n = len(x)
    wdx, wdy, p = kernel_terms(x, y, w, mean_x, mean_y)
    C, P = math.fsum(p), math.fsum(np.abs(p))
    Dx, Dy, Ax, Ay = math.fsum(wdx), math.fsum(wdy), math.fsum(np.abs(wdx)), math.fsum(np.abs(wdy))
    g = gamma(n)
    Ex, Ey = g * Ax, g * Ay
    DEx, DEy = abs(Dx) + Ex, abs(Dy) + Ey
    b = g * P + (abs(Dx) * Ey + abs(Dy) * Ex + Ex * Ey + gamma(2) * DEx * DEy) / W + U * ((1.0 + g) * P + (1.0 + gamma(2)) * DEx * DEy / W)
    b += gamma(6) * (P + abs(Dx * Dy) / W)  # the host's fsums and its evaluation of C*
    b *= 1.0 + gamma(4)
    return C - Dx * Dy / W, b


def w_exact(W):
    """the sums of weights whose moments are exact on this data: powers of two up to 2^8"""
    W = np.asarray(W, np.float64)
    Wi = W.astype(np.int64)
    return (W == Wi) & vx.is_pow2(Wi) & (Wi <= POW2_EXACT)


def expected(flat, a, b, w, size):
    """flat bin indices (int64, one per counted sample), the samples' two values (any dtype; triples with a NaN value are
    dropped here) and their weights over `size` bins -> (W float64 exact, (mean_a, mean_b) bit-exact, (M2_a*, C_ab*, M2_b*),
    (B_a, B_c, B_b), exact bool).  `exact`: W is a power of two up to 2^8, so the three moments are the kernels' bit for bit
    (their bounds are 0).  Bins with W == 0: NaN everywhere but W."""
    a = np.asarray(a).astype(np.float64)
    b = np.asarray(b).astype(np.float64)
    w = np.asarray(w).astype(np.float64)
    flat = np.asarray(flat, np.int64)
    keep = ~np.isnan(a) & ~np.isnan(b)
    flat, a, b, w = flat[keep], a[keep], b[keep], w[keep]
    assert vx.on_grid(a) and vx.on_grid(b), "values off the grid: their sums are not exact"
    assert np.all(w == np.round(w)) and w.min(initial=0) >= 0 and w.max(initial=0) <= W_MAX, "weights must be integers 0..7"
    assert np.bincount(flat, minlength=size).max(initial=0) < vx.COUNT_LIMIT
    sums = []
    for t in (w, w * a, w * b):  # exact in any order
        s = np.zeros(size)
        np.add.at(s, flat, t)
        sums.append(s)
    W = sums[0]
    has = W != 0
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_a = np.where(has, sums[1] / np.where(has, W, 1), np.nan)
        mean_b = np.where(has, sums[2] / np.where(has, W, 1), np.nan)
    star = [np.full(size, np.nan) for _ in range(3)]
    bound = [np.full(size, np.nan) for _ in range(3)]
    order = np.argsort(flat, kind="stable")
    fs = flat[order]
    starts = np.flatnonzero(np.r_[True, fs[1:] != fs[:-1]]) if len(fs) else np.zeros(0, np.int64)
    ends = np.r_[starts[1:], len(fs)]
    for lo, hi in zip(starts, ends):
        k, idx = int(fs[lo]), order[lo:hi]
        if not has[k]:
            continue
        va, vb, vw = a[idx], b[idx], w[idx]
        for m, (x, y, mx, my) in enumerate(((va, va, mean_a[k], mean_a[k]), (va, vb, mean_a[k], mean_b[k]), (vb, vb, mean_b[k], mean_b[k]))):
            c, bd = c_star_and_bound(x, y, vw, mx, my, W[k])
            star[m][k], bound[m][k] = (c if m == 1 else max(0.0, c)), bd
    pow2 = has & w_exact(W)
    if pow2.any():  # these bins: the exact-mode formula, every term exact
        with np.errstate(invalid="ignore"):
            da, db = a - mean_a[flat], b - mean_b[flat]
        wda, wdb = w * da, w * db
        acc = []
        for t in (wda, wdb, wda * da, wda * db, wdb * db):
            s = np.zeros(size)
            np.add.at(s, flat, np.where(np.isnan(t), 0.0, t))  # (NaN only in bins with W == 0, which are not `pow2`)
            acc.append(s)
        sda, sdb, saa, sab, sbb = acc
        den = np.where(has, W, 1)
        ra, rb = saa - sda * sda / den, sbb - sdb * sdb / den
        exact_m = (np.where(ra <= 0, 0.0, ra), sab - sda * sdb / den, np.where(rb <= 0, 0.0, rb))
        star = [np.where(pow2, e, s) for e, s in zip(exact_m, star)]
        bound = [np.where(pow2, 0.0, bd) for bd in bound]
    return W, (mean_a, mean_b), tuple(star), tuple(bound), pow2


def assert_moments(got, want, bounds, exact, W=None, ddof=None, what=""):
    """the kernels' (M2_a, C_ab, M2_b) — or, with W and ddof, (var_a, cov_ab, var_b) — against `expected`'s: bit for bit where
    `exact`, within the bounds elsewhere, NaN exactly where expected"""
    for g, w, b, name in zip(got, want, bounds, ("a", "ab", "b")):
        if ddof is not None:
            w, b = vx.var_bound(W, w, b, ddof)
        vx.assert_m2(g, w, b, exact, "%s %s" % (name, what))
