"""What histogram_skew_kurt must give on exactly summable data: bit for bit where every term and sum is exact, and within
float64 bounds derived here for every other count.

1. The narrow grid.  A value is k * 2^-4 with |k| < 2^6 (float64 or float32; the integers k themselves for integer dtypes): a
subset of values_exact.grid, so pass 1 is exact for any count (values_exact's argument) and mean = fl(S / x) bit for bit.  With
a power-of-two count x = 2^j <= 2^5 the mean S / x is exact, a multiple of 2^-(4 + j) below 2^2, and so is every d = v - mean:
a multiple of 2^-(4 + j) below 2^3 in magnitude, 7 + j significant bits.  Then t2 = d * d (14 + 2j bits), t3 = t2 * d (21 + 3j)
and t4 = t3 * d (28 + 4j <= 48) are exact products, and every partial sum of at most x = 2^j of the t4 is a multiple of
2^-(16 + 4j) below 2^(12 + j): 28 + 5j <= 53 bits, exact in ANY order of addition (the sums of t2 and t3 need fewer bits).
D = sum(d) = S - x mean = 0 exactly, so delta = 0 and M2 = Q2, M3 = Q3, M4 = Q4 bit for bit.  With integer weights 0..7 (three
bits) and W = sum(w) = 2^j <= 2^5 the same holds: the mean sum(w v) / W is exact, t1 = w * d has 10 + j bits, t4 = w d^4 has
31 + 4j <= 51, and a partial sum of the t4 is a multiple of 2^-(16 + 4j) below W 2^12 = 2^(12 + j): 28 + 5j <= 53 bits again
(samples of weight 0 add exact zeros).  `exact_x` names those bins: x in {2, 4, 8, 16, 32}.

2. Every other count.  The mean is rounded, the terms d = fl(v - mean), t1 = d or fl(w d), t2 = fl(t1 d), t3 = fl(t2 d),
t4 = fl(t3 d) carry full mantissas (they are formed here exactly as the kernel forms them) and the kernel adds them in an
order of its own.  Let S_k be the exact sum of the very terms t_k and A_k = sum |t_k| (math.fsum: within u = 2^-53 relative).
A float64 sum of n terms in any order is within g(n) A_k of S_k (g(n) = n u / (1 - n u); Higham 4.2): Q3 is a signed sum, so
its term is g(n) sum |t3|, not g(n) |Q3|.  The finalize step is then followed operation by operation, in the kernel's order
    delta = D / x;  d2 = delta delta;  d3 = d2 delta;  d4 = d2 d2
    M2 = max(0, Q2 - (D D) / x)
    M3 = (Q3 - (3 delta) Q2) + (2 x) d3
    M4 = max(0, ((Q4 - (4 delta) Q3) + (6 d2) Q2) - (3 x) d4)
with a running error bound (class Err): a quantity is a pair (val, err), val what this host computes in float64 from the fsums
and err a bound on |the kernel's float64 value - val|.  For z = a op b the kernel's fl(a_k op b_k) and the host's
fl(a.val op b.val) differ by at most |a_k op b_k - a.val op b.val| plus one rounding of each, u times their magnitudes:
    a b    |a.val| e_b + |b.val| e_a + e_a e_b + 2u (|a.val| + e_a) (|b.val| + e_b)
    a +- b e_a + e_b + 2u (|a.val| + |b.val| + e_a + e_b)
    a / b  (e_a + |val| e_b) / lo + 2u (|a.val| + e_a) / lo,  lo = |b.val| - e_b > 0        (infinite where lo <= 0)
    sqrt a e_a / sqrt(a.val) + 2u sqrt(a.val + e_a)
(2u also covers an operation that is only faithfully rounded.)  This propagates the error of delta into each correction
product and counts the host's own roundings, since val is the host's.  max(0, .) is 1-Lipschitz, and the exact M2 and M4 of
non-negative weights are >= 0, so the clamp moves nothing further away.  The err arithmetic itself runs in float64, a chain of
fewer than a hundred operations each within u relative: every bound is widened by 1 + 2^-40 for it.  Without weights, M2's
value and bound are values_exact.m2_star_and_bound's, the existing ones.

3. The outputs.  var, skew and kurt are formed from (x, M2, M3, M4) by the public formulas; `outputs` follows them with the
same Err arithmetic, x exact, so their bounds are the moments' bounds propagated, plus the roundings of the formulas on both
sides.

Accumulating t3 / t4 in float32 breaks these bounds by orders of magnitude: tests/test_skew_kurt_cpu.py shows it."""
import math

import numpy as np

import values_exact as vx

U = vx.U
K_MAX = 1 << 6  # |k| < 2^6
SCALE = 2.0 ** -4
W_MAX = 7  # the integer weights are 0..7
X_EXACT = (2, 4, 8, 16, 32)
WIDEN = 1.0 + 2.0 ** -40


def narrow(rng, shape, dtype=np.float64):
    """values k * 2^-4, |k| < 2^6, as `dtype` (float64 / float32); integer dtypes: the integers k themselves"""
    k = rng.integers(-(K_MAX - 1), K_MAX, shape)
    dt = np.dtype(dtype)
    return (k * SCALE).astype(dt) if dt.kind == "f" else k.astype(dt)


def narrow_nan(rng, shape, dtype=np.float64):
    """narrow-grid values with NaNs of their own (float dtypes)"""
    v = narrow(rng, shape, dtype)
    if np.dtype(dtype).kind == "f":
        v.reshape(-1)[rng.permutation(v.size)[: max(1, v.size // 100)]] = np.nan
    return v


def on_narrow(values):
    """every finite value is k * 2^-4 with |k| < 2^6, or every one is an integer k with |k| < 2^6 (the same bits, 2^4 times
    the size: the argument of the module docstring holds for both, not for a mixture)"""
    v = np.asarray(values, np.float64)
    v = v[np.isfinite(v)]
    k = v / SCALE
    return bool((np.all(k == np.round(k)) and np.all(np.abs(k) < K_MAX)) or (np.all(v == np.round(v)) and np.all(np.abs(v) < K_MAX)))


def exact_x(x):
    """the bins of the bit-for-bit path: x (count or integer W) in {2, 4, 8, 16, 32}"""
    return np.isin(np.asarray(x, np.float64), X_EXACT)


class Err:
    """(val, err) with the running error bounds of the module docstring; numpy arrays or scalars"""

    def __init__(self, val, err=0.0):
        self.val = np.asarray(val, np.float64)
        self.err = np.broadcast_to(np.asarray(err, np.float64), self.val.shape) if np.ndim(val) else np.float64(err)

    @staticmethod
    def of(a):
        return a if isinstance(a, Err) else Err(a)

    def __mul__(self, b):
        b = Err.of(b)
        av, bv = np.abs(self.val), np.abs(b.val)
        return Err(self.val * b.val, av * b.err + bv * self.err + self.err * b.err + 2 * U * (av + self.err) * (bv + b.err))

    __rmul__ = __mul__

    def _addsub(self, b, sign):
        b = Err.of(b)
        return Err(self.val + sign * b.val, self.err + b.err + 2 * U * (np.abs(self.val) + np.abs(b.val) + self.err + b.err))

    def __add__(self, b):
        return self._addsub(b, 1.0)

    def __sub__(self, b):
        return self._addsub(b, -1.0)

    def __truediv__(self, b):
        b = Err.of(b)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            val = self.val / b.val
            lo = np.abs(b.val) - b.err
            err = np.where(lo > 0, ((self.err + np.abs(val) * b.err) + 2 * U * (np.abs(self.val) + self.err)) / lo, np.inf)
        return Err(val, err)

    def sqrt(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            val = np.sqrt(self.val)
            err = np.where(self.val > 0, self.err / val, np.inf) + 2 * U * np.sqrt(np.abs(self.val) + self.err)
        return Err(val, np.where(self.err == 0, 2 * U * val, err))

    def clamp0(self):
        return Err(np.where(self.val <= 0, 0.0, self.val), self.err)


def kernel_terms(vals, mean, w=None):
    """the terms t1 .. t4 the kernels add for one bin, formed in their order of products"""
    d = np.asarray(vals, np.float64) - mean
    t1 = d if w is None else np.asarray(w, np.float64) * d
    t2 = t1 * d
    t3 = t2 * d
    t4 = t3 * d
    return t1, t2, t3, t4


def kernel_sums(vals, mean, w=None, acc=None):
    """four Err: the exact sums of the bin's terms (fsum) with the kernel's summation error g(n) sum |t_k| + the fsum's own u.
    acc: a dtype to accumulate in instead (test_skew_kurt_cpu's float32 accumulator), err 0."""
    n = len(vals)
    g = vx.gamma(max(n, 1))
    out = []
    for t in kernel_terms(vals, mean, w):
        if acc is not None:
            s = np.zeros((), acc)
            for x in t:
                s = (s + np.asarray(x, acc)).astype(acc)
            out.append(Err(float(s), 0.0))
            continue
        s = math.fsum(t)
        out.append(Err(s, g * math.fsum(np.abs(t)) + U * abs(s)))
    return out


def finalize(x, D, Q2, Q3, Q4):
    """the finalize step on Err sums, in the kernel's order of evaluation: (M2, M3, M4)"""
    x = Err.of(x)
    delta = D / x
    d2 = delta * delta
    d3 = d2 * delta
    d4 = d2 * d2
    m2 = (Q2 - (D * D) / x).clamp0()
    m3 = (Q3 - (3.0 * delta) * Q2) + (2.0 * x) * d3
    m4 = (((Q4 - (4.0 * delta) * Q3) + (6.0 * d2) * Q2) - (3.0 * x) * d4).clamp0()
    return m2, m3, m4


def moments_star_and_bound(vals, mean, x, w=None):
    """((M2*, M3*, M4*), (B2, B3, B4)) of one bin: its values (float64, no NaN), the kernel's mean and x, its weights"""
    D, Q2, Q3, Q4 = kernel_sums(vals, mean, w)
    m2, m3, m4 = finalize(x, D, Q2, Q3, Q4)
    if w is None:
        m2 = Err(*vx.m2_star_and_bound(vals, mean))  # the existing value and bound
    return tuple(float(m.val) for m in (m2, m3, m4)), tuple(float(m.err) * WIDEN for m in (m2, m3, m4))


def expected(flat, values, size, weights=None):
    """flat bin indices (int64, one per counted sample) and their values (any dtype; NaN values are dropped here), optionally
    their integer weights 0..7, over `size` bins -> (x, mean, moments [3, size], bounds [3, size], exact): x the count (int64) or
    W (float64), the mean bit-exact, M2*, M3*, M4* and their bounds (0 where `exact`, the bins of the bit-for-bit path).  Empty
    bins and bins of W == 0: NaN mean and moments."""
    v = np.asarray(values).astype(np.float64)
    flat = np.asarray(flat, np.int64)
    keep = ~np.isnan(v)
    flat, v = flat[keep], v[keep]
    assert on_narrow(v), "values off the narrow grid"
    if weights is None:
        w = None
        x = np.bincount(flat, minlength=size).astype(np.int64)
        s = np.zeros(size)
        np.add.at(s, flat, v)  # exact in any order
    else:
        w = np.asarray(weights).astype(np.float64)[keep]
        assert np.all((w == np.round(w)) & (w >= 0) & (w <= W_MAX)), "weights must be integers 0..7"
        x = np.zeros(size)
        np.add.at(x, flat, w)
        s = np.zeros(size)
        np.add.at(s, flat, w * v)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(x != 0, s / np.where(x != 0, x, 1), np.nan)
    moments = np.full((3, size), np.nan)
    bounds = np.full((3, size), np.nan)
    order = np.argsort(flat, kind="stable")
    fs = flat[order]
    starts = np.flatnonzero(np.r_[True, fs[1:] != fs[:-1]]) if len(fs) else np.zeros(0, np.int64)
    ends = np.r_[starts[1:], len(fs)]
    for a, b in zip(starts, ends):
        k, sel = int(fs[a]), order[a:b]
        if x[k] == 0:
            continue
        moments[:, k], bounds[:, k] = moments_star_and_bound(v[sel], mean[k], float(x[k]), None if w is None else w[sel])
    exact = exact_x(x)
    bounds[:, exact] = 0.0
    return x, mean, moments, bounds, exact


def outputs(x, m2, m3, m4, ddof=0, bias=True, fisher=True):
    """(var, skew, kurt) as Err from x (exact) and the moments as Err, by the public formulas; NaN val where the public
    function gives NaN"""
    x = Err(np.asarray(x, np.float64))
    nan = np.nan
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        var = m2 / (x - Err(float(ddof)))
        var = Err(np.where(x.val > ddof, var.val, nan), var.err)
        v = m2 / x
        ok = (x.val != 0) & (m2.val != 0)
        g1 = (m3 / x) / (v * v.sqrt())
        g2 = (m4 / x) / (v * v)
        g1 = Err(np.where(ok, g1.val, nan), g1.err)
        g2 = Err(np.where(ok, g2.val, nan), g2.err)
        if not bias:
            g1 = (x * (x - 1.0)).sqrt() / (x - 2.0) * g1
            g1 = Err(np.where(x.val <= 2, nan, g1.val), g1.err)
            g2 = (x - 1.0) / ((x - 2.0) * (x - 3.0)) * ((x + 1.0) * g2 - 3.0 * (x - 1.0)) + 3.0
            g2 = Err(np.where(x.val <= 3, nan, g2.val), g2.err)
        if fisher:
            g2 = g2 - 3.0
    return tuple(Err(o.val, o.err * WIDEN) for o in (var, g1, g2))


def expected_outputs(x, moments, bounds, ddof=0, bias=True, fisher=True):
    """((var, skew, kurt) values, their bounds) from `expected`'s moments and bounds"""
    outs = outputs(x, *[Err(m, b) for m, b in zip(moments, bounds)], ddof=ddof, bias=bias, fisher=fisher)
    return [o.val for o in outs], [o.err for o in outs]


def assert_within(got, want, bound, exact=None, what=""):
    """got against want: NaN exactly where want is NaN, bit for bit where `exact`, within `bound` elsewhere"""
    got = np.asarray(got, np.float64).reshape(-1)
    want = np.asarray(want, np.float64).reshape(-1)
    bound = np.broadcast_to(np.asarray(bound, np.float64).reshape(-1), want.shape)
    exact = np.zeros(want.shape, bool) if exact is None else np.asarray(exact, bool).reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape, what)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "NaN in %d bins, expected in %d (%s)" % (gn.sum(), wn.sum(), what)
    ok = ~wn
    bad = ok & exact & (got.view(np.int64) != want.view(np.int64)) & ~((got == 0) & (want == 0))
    if bad.any():
        i = np.flatnonzero(bad)[0]
        raise AssertionError("%d bins of the bit-for-bit path differ (%s); first at %d: %r != %r" % (bad.sum(), what, i, got[i], want[i]))
    rest = ok & ~exact
    err = np.abs(got - want)
    bad = rest & ~(err <= bound)
    if bad.any():
        i = np.flatnonzero(bad)[0]
        raise AssertionError("%d bins beyond the float64 bound (%s); first at %d: |%r - %r| = %.3g > %.3g"
                             % (bad.sum(), what, i, got[i], want[i], err[i], bound[i]))
    return err, bound
