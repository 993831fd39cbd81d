"""What histogram_cov must give for ANY count per bin on the exactly summable grid of tests/values_exact.py: that module's
analysis, extended to the co-moment.

Both value arrays are on the grid k * 2^-10, |k| < 2^12.  A pair counts only if neither value is NaN, so n, Sa and Sb are
those of the pairwise-complete samples; every partial sum is exact in any order (values_exact), hence

    mean_a = fl(Sa / n),  mean_b = fl(Sb / n)               bit for bit, for every count n.

With a power-of-two count n = 2^j <= 2^9 both means are exact, and so are da = a - mean_a and db = b - mean_b: multiples of
2^-(10 + j) below 2^3 in magnitude, 13 + j significant bits at most.  Then da * db is exact like da * da: a multiple of
2^-(20 + 2j) below 2^6, and every partial sum of n of them, of either sign, holds at most 26 + 3j <= 53 bits: exact in any
order.  sum(da) = Sa - n mean_a = 0 and sum(db) = 0 exactly, so M2_a, M2_b and C_ab = sum(da db) - sum(da) sum(db) / n are
bit for bit (cov_oracle's exact mode).

Other counts: M2_a and M2_b take values_exact.m2_star_and_bound as they are.  For the co-moment, with p = fl(da * db) the
very terms the kernel adds, C = sum(p), P = sum |p|, Da = sum(da), Db = sum(db), Aa = sum |da|, Ab = sum |db| (exact sums;
u = 2^-53, g(k) = k u / (1 - k u)):

  C^  = C + t,                 |t| <= g(n) P                (a float64 sum of n terms of either sign in any order; Higham 4.2)
  Da^ = Da + ea, Db^ = Db + eb,  |ea| <= Ea = g(n) Aa, |eb| <= Eb = g(n) Ab
  T^  = fl(fl(Da^ Db^) / n),   |T^ - Da Db / n| <= (|Da| Eb + |Db| Ea + Ea Eb + g(2) (|Da| + Ea) (|Db| + Eb)) / n
  R^  = fl(C^ - T^),           |R^ - (C^ - T^)| <= u (|C^| + |T^|) <= u ((1 + g(n)) P + (1 + g(2)) (|Da| + Ea) (|Db| + Eb) / n)

The cross term Da Db / n is signed and nothing is clamped, so with C* = C - Da Db / n

  |C_ab - C*| <= g(n) P + (|Da| Eb + |Db| Ea + Ea Eb + g(2) DEa DEb) / n + u ((1 + g(n)) P + (1 + g(2)) DEa DEb / n) =: B,

DEa = |Da| + Ea, DEb = |Db| + Eb.  The host evaluates the six sums with math.fsum (each within u of the exact sum: u P for C,
2 u |Da Db| / n for the cross term), C* as fl(C - fl(fl(Da Db) / n)) with at most g(3) (|C| + |Da Db| / n) more; together at
most g(6) (P + |Da Db| / n), by which B is widened, and by g(4) B for its own arithmetic.  cov = C_ab / (n - ddof) then carries
B / (n - ddof) plus one more rounding (values_exact.var_bound).

Adding p in float32 breaks B by orders of magnitude: tests/test_cov_cpu.py shows it."""
import math

import numpy as np

import values_exact as vx
from values_exact import U, gamma


def kernel_terms(avals, bvals, mean_a, mean_b):
    """the da = fl(a - mean_a), db = fl(b - mean_b) and p = fl(da * db) the kernels add, for one bin"""
    da = np.asarray(avals, np.float64) - mean_a
    db = np.asarray(bvals, np.float64) - mean_b
    return da, db, da * db


def c_star_and_bound(avals, bvals, mean_a, mean_b):
    """(C*, B) of the module docstring for the pairs of one bin (float64) and its means fl(S / n)"""
    n = len(avals)
    da, db, p = kernel_terms(avals, bvals, mean_a, mean_b)
    C, P = math.fsum(p), math.fsum(np.abs(p))
    Da, Db, Aa, Ab = math.fsum(da), math.fsum(db), math.fsum(np.abs(da)), math.fsum(np.abs(db))
    g = gamma(n)
    Ea, Eb = g * Aa, g * Ab
    DEa, DEb = abs(Da) + Ea, abs(Db) + Eb
    b = g * P + (abs(Da) * Eb + abs(Db) * Ea + Ea * Eb + gamma(2) * DEa * DEb) / n + U * ((1.0 + g) * P + (1.0 + gamma(2)) * DEa * DEb / n)
    b += gamma(6) * (P + abs(Da * Db) / n)  # the host's fsums and its evaluation of C*
    b *= 1.0 + gamma(4)
    return C - Da * Db / n, b


def expected(flat, a, b, size):
    """flat bin indices (int64, one per counted sample) and the samples' two values (any dtype; pairs with a NaN are dropped
    here) over `size` bins -> (count int64, (mean_a, mean_b) bit-exact, (M2_a*, C_ab*, M2_b*), (B_a, B_c, B_b), exact bool).
    `exact`: the count is a power of two up to 2^9, so the three moments are the kernels' bit for bit (their bounds are 0).
    Empty bins: count 0, NaN everywhere."""
    a = np.asarray(a).astype(np.float64)
    b = np.asarray(b).astype(np.float64)
    flat = np.asarray(flat, np.int64)
    keep = ~np.isnan(a) & ~np.isnan(b)
    flat, a, b = flat[keep], a[keep], b[keep]
    cnt, mean_a, m2a, ba, pow2 = vx.expected(flat, a, size)
    cnt_b, mean_b, m2b, bb, _ = vx.expected(flat, b, size)
    assert np.array_equal(cnt, cnt_b)
    c = np.full(size, np.nan)
    bc = np.full(size, np.nan)
    groups_a = dict(vx._groups(flat, a, size))
    for k, bvals in vx._groups(flat, b, size):  # (the same stable order: the pairs stay together)
        c[k], bc[k] = c_star_and_bound(groups_a[k], bvals, mean_a[k], mean_b[k])
    if pow2.any():  # these bins: the exact-mode formula, every term exact
        da, db = a - mean_a[flat], b - mean_b[flat]
        sda, sdb, sab = np.zeros(size), np.zeros(size), np.zeros(size)
        np.add.at(sda, flat, da)
        np.add.at(sdb, flat, db)
        np.add.at(sab, flat, da * db)
        c = np.where(pow2, sab - sda * sdb / np.maximum(cnt, 1), c)
        bc = np.where(pow2, 0.0, bc)
    return cnt, (mean_a, mean_b), (m2a, c, m2b), (ba, bc, bb), pow2


def assert_moments(got, want, bounds, exact, cnt=None, ddof=None, what=""):
    """the kernels' (M2_a, C_ab, M2_b) — or, with cnt and ddof, (var_a, cov_ab, var_b) — against `expected`'s: bit for bit where
    `exact`, within the bounds elsewhere, NaN exactly where expected"""
    for g, w, b, name in zip(got, want, bounds, ("a", "ab", "b")):
        if ddof is not None:
            w, b = vx.var_bound(cnt, w, b, ddof)
        vx.assert_m2(g, w, b, exact, "%s %s" % (name, what))
