"""Values whose per-bin sums are exact, and what histogram_mean_var must then give for ANY count per bin.

The grid.  A value is k * 2^-10 with |k| < 2^12 (float64 or float32: 22 significant bits at most), or a small integer (int32).
Every partial sum of fewer than 2^31 such values is a multiple of 2^-10 below 2^43 in magnitude: it fits 53 bits, so any order
of float64 additions (LDS atomics, lane copies, workgroup flushes, global atomics) gives the exact sum S of a bin.  Hence

    mean = fl(S / n)                                        bit for bit, for every count n.

With a power-of-two count n = 2^j <= 2^9 the mean is exact too, and so is every d = v - mean: a multiple of 2^-(10 + j) below
2^3 in magnitude (of 2^-j below 2^13 for the integers), 13 + j significant bits at most.  Then d * d is exact, a multiple of
2^-(20 + 2j) below 2^6 (2^-2j below 2^26), and every partial sum of n of them holds at most 26 + 3j <= 53 bits: exact in any
order.  sum(d) = S - n mean = 0 exactly, and M2 = max(0, sum(d^2) - sum(d)^2 / n) is bit for bit as well (meanvar_oracle's exact
mode).  From 2^10 values on the sums of d^2 round: those counts take the bound below.

Other counts: the mean is rounded, d = fl(v - mean) and q = fl(d * d) carry full mantissas, and the kernel adds them in an order
of its own.  `m2_bound` states how far its M2 may then be from M2* = Q - D^2 / n, where Q = sum(q) and D = sum(d) are the exact
sums of the very terms the kernel adds (d and q are computed as the kernel computes them; u = 2^-53, g(k) = k u / (1 - k u)):

  Q^ = Q (1 + t),          |t| <= g(n)                 (a float64 sum of n terms >= 0 in any order; Higham 4.2)
  D^ = D + e,              |e| <= g(n) A               (A = sum |d|)
  T^ = fl(fl(D^ D^) / n),  |T^ - D^2 / n| <= |D^^2 - D^2| / n + g(2) D^^2 / n <= (E (2|D| + E) + g(2) (|D| + E)^2) / n,  E = g(n) A
  R^ = fl(Q^ - T^),        |R^ - (Q^ - T^)| <= u (Q^ + T^)
  M2 = max(0, R^):         max(0, .) moves nothing closer than 0 and M2* >= 0 (Cauchy-Schwarz), so |M2 - M2*| <= |R^ - M2*|.

So |M2 - M2*| <= g(n) Q + (E (2|D| + E) + g(2) (|D| + E)^2) / n + u ((1 + g(n)) Q + (1 + g(2)) (|D| + E)^2 / n) =: B.
The host evaluates Q, D and A with math.fsum (each correctly rounded: within u of the exact sum), M2* as fl(Q - fl(D^2) / n) with
at most g(3) (Q + D^2 / n) more error, and widens B by those terms and by g(4) B for its own arithmetic.  var = M2 / (n - ddof)
then carries B / (n - ddof) plus one more rounding, u |var|.

Adding q in float32 (or any accumulator of fewer bits) breaks B by orders of magnitude: tests/test_values_exact_cpu.py shows it."""
import math

import numpy as np

U = 2.0 ** -53
K_MAX = 1 << 12  # |k| < 2^12
SCALE = 2.0 ** -10
COUNT_LIMIT = 1 << 31  # values per bin below which the sums of the grid stay exact
POW2_EXACT = 1 << 9  # the largest power-of-two count whose M2 is exact


def gamma(n):
    nu = float(n) * U
    return nu / (1.0 - nu)


def grid(rng, shape, dtype=np.float64):
    """values k * 2^-10, |k| < 2^12, as `dtype` (float64 / float32); integer dtypes: the integers k themselves"""
    k = rng.integers(-(K_MAX - 1), K_MAX, shape)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return (k * SCALE).astype(dt)
    return k.astype(dt)


def on_grid(values):
    """every finite value is a multiple of 2^-10 below 2^12 in magnitude (the grid k * 2^-10, and the integers |k| < 2^12)"""
    v = np.asarray(values, np.float64)
    v = v[np.isfinite(v)]
    k = v / SCALE
    return bool(np.all(k == np.round(k)) and np.all(np.abs(v) < K_MAX))


def is_pow2(n):
    n = np.asarray(n, np.int64)
    return (n > 0) & ((n & (n - 1)) == 0)


def m2_exact(n):
    """the counts whose M2 is exact on the grid: powers of two up to 2^9"""
    return is_pow2(n) & (np.asarray(n) <= POW2_EXACT)


def _groups(flat, v, size):
    """(bin, values of that bin) for every bin a value reached, in the order of `flat`'s sort"""
    order = np.argsort(flat, kind="stable")
    fs, vs = flat[order], v[order]
    if not len(fs):
        return
    starts = np.flatnonzero(np.r_[True, fs[1:] != fs[:-1]])
    ends = np.r_[starts[1:], len(fs)]
    for a, b in zip(starts, ends):
        yield int(fs[a]), vs[a:b]


def kernel_terms(vals, mean):
    """the d = fl(v - mean) and q = fl(d * d) the kernels add, for one bin"""
    d = np.asarray(vals, np.float64) - mean
    return d, d * d


def m2_star_and_bound(vals, mean):
    """(M2*, B) of the module docstring for the values of one bin (float64) and its mean fl(S / n)"""
    n = len(vals)
    d, q = kernel_terms(vals, mean)
    Q, D, A = math.fsum(q), math.fsum(d), math.fsum(np.abs(d))
    g = gamma(n)
    E = g * A
    DE = abs(D) + E
    b = g * Q + (E * (2.0 * abs(D) + E) + gamma(2) * DE * DE) / n + U * ((1.0 + g) * Q + (1.0 + gamma(2)) * DE * DE / n)
    b += 3.0 * U * (Q + abs(D)) + gamma(3) * (Q + D * D / n)  # the host's fsums and its evaluation of M2*
    b *= 1.0 + gamma(4)
    m2 = Q - D * D / n
    return max(0.0, m2), b


def expected(flat, values, size):
    """flat bin indices (int64, one per counted sample: digitized inside the edges) and their values (any dtype; NaN values are
    dropped here) over `size` bins -> (count int64, mean float64 bit-exact, M2* float64, B float64, exact bool).  `exact`: the
    count is a power of two up to 2^9, so M2* is the kernels' M2 bit for bit.  Empty bins: count 0, NaN everywhere."""
    v = np.asarray(values).astype(np.float64)
    flat = np.asarray(flat, np.int64)
    keep = ~np.isnan(v)
    flat, v = flat[keep], v[keep]
    assert on_grid(v), "values off the grid: their sums are not exact"
    cnt = np.bincount(flat, minlength=size).astype(np.int64)
    assert cnt.max(initial=0) < COUNT_LIMIT
    s = np.zeros(size)
    np.add.at(s, flat, v)  # exact in any order
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(cnt > 0, s / np.maximum(cnt, 1), np.nan)
    m2 = np.full(size, np.nan)
    bound = np.full(size, np.nan)
    for b, vals in _groups(flat, v, size):
        m2[b], bound[b] = m2_star_and_bound(vals, mean[b])
    pow2 = m2_exact(cnt)
    if pow2.any():  # these bins: the exact-mode formula, every term exact
        d = v - mean[flat]
        sd = np.zeros(size)
        s2 = np.zeros(size)
        np.add.at(sd, flat, d)
        np.add.at(s2, flat, d * d)
        r = s2 - sd * sd / np.maximum(cnt, 1)
        m2 = np.where(pow2, np.where(r <= 0, 0.0, r), m2)
        bound = np.where(pow2, 0.0, bound)
    return cnt, mean, m2, bound, pow2


def var_bound(cnt, m2_star, bound, ddof):
    """(var*, bound of var) from M2* and its bound B: var = fl(M2 / (n - ddof)), NaN where n <= ddof"""
    cnt = np.asarray(cnt)
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.where(cnt > ddof, cnt - ddof, 1).astype(np.float64)
        var = np.where(cnt > ddof, m2_star / den, np.nan)
        b = np.where(cnt > ddof, bound / den + 2.0 * U * np.abs(var), np.nan)
    return var, b


def assert_m2(got, want, bound, exact, what=""):
    """the kernels' M2 (or var) against M2* (var*): bit for bit where `exact`, within `bound` elsewhere; NaN exactly where
    `want` is NaN"""
    got = np.asarray(got, np.float64).reshape(-1)
    want = np.asarray(want, np.float64).reshape(-1)
    bound = np.asarray(bound, np.float64).reshape(-1)
    exact = np.asarray(exact, bool).reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape, what)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "NaN in %d bins, expected in %d (%s)" % (gn.sum(), wn.sum(), what)
    ok = ~wn
    bits = ok & exact
    bad = bits & (got.view(np.int64) != want.view(np.int64))
    if bad.any():
        i = np.flatnonzero(bad)[0]
        raise AssertionError("%d power-of-two-count bins differ in their bits (%s); first at %d: %r != %r" % (bad.sum(), what, i, got[i], want[i]))
    rest = ok & ~exact
    err = np.abs(got - want)
    bad = rest & ~(err <= bound)
    if bad.any():
        i = np.flatnonzero(bad)[0]
        raise AssertionError("%d bins beyond the float64 bound (%s); first at %d: |%r - %r| = %.3g > %.3g"
                             % (bad.sum(), what, i, got[i], want[i], err[i], bound[i]))
