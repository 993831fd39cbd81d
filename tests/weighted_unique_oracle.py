"""bin_weighted_unique and histogram_weighted_mode on the CPU, built on tests/bin_unique_oracle.py: the runs of the sorted domain
(tests/bin_rank_oracle.sorted_domain) are bin_unique's entries, and an entry's weight sum is math.fsum over the float64 weights
of its run, in run order.  math.fsum is the correctly rounded sum, so on exactly summable weights (tests/exact_weights.py) it is
the one float64 any order of additions gives, and the comparison is bit for bit; on other weights it is the centre of
exact_weights.assert_within_f64_bound.  The one place a float64 sum is not math.fsum's is the sign of a zero: a sum of nothing but
-0.0 is -0.0 in IEEE arithmetic, and so it is here.

The weighted mode comes from the entries: per bin the largest sum (IEEE compare; NaN if any sum of the bin is NaN), the first entry
that holds it, and that entry's value and sum by their bits."""
import math
import re

import numpy as np

import bin_rank_oracle as ro
import bin_sort_oracle as so
import bin_unique_oracle as uo
import exact_weights as xw

WORD = ro.WORD
TILE_WORDS = 1024  # words of one tile (kRankTile of xhist_rank.hip.h)
TILE = TILE_WORDS * WORD
NAN_BITS = uo.NAN_BITS
PAD = uo.PAD


def run_sum(ws):
    """the float64 sum of one run's weights: math.fsum, NaN as IEEE addition gives it, -0.0 for a run of only -0.0"""
    ws = [float(x) for x in ws]
    if any(x != x for x in ws) or (math.inf in ws and -math.inf in ws):
        return math.nan
    s = math.fsum(ws)
    if s == 0 and all(x == 0 and math.copysign(1.0, x) < 0 for x in ws):
        return -0.0
    return s


def runs_row(index, values, weights, n_bins):
    """one row's entries before any cut: (bin [U], value [U], count [U], weight sum [U], sum of |w| [U], inverse [c])"""
    order, ks, vs, head = ro.sorted_domain(index, values, n_bins)
    b, vals, cnt, inverse = uo.runs_row(index, values, n_bins)
    w = np.asarray(np.broadcast_to(weights, np.shape(index))).astype(np.float64)[order]
    sums, mags = np.zeros(len(b)), np.zeros(len(b))
    if len(b):
        valid = (ks < n_bins) & ~np.isnan(vs)
        s = np.flatnonzero(head)
        e = np.concatenate([s[1:], [len(ks)]])
        keep = valid[s]
        for u, (s0, e0) in enumerate(zip(s[keep], e[keep])):
            sums[u] = run_sum(w[s0:e0])
            mags[u] = math.fsum(abs(x) for x in w[s0:e0] if x == x and abs(x) != math.inf)
    return b, vals, cnt, sums, mags, inverse


def wunique_row(index, values, weights, n_bins, size=None):
    """(uniques [W], counts [W], weight_sums [W], offsets [B + 1], inverse [c]) of one row; W = c where size is None"""
    b, vals, cnt, sums, _, inverse = runs_row(index, values, weights, n_bins)
    width = len(np.asarray(index)) if size is None else int(size)
    uniques, counts, offsets = uo.cut(b, vals, cnt, n_bins, width)
    wsums = np.zeros(width)
    k = min(len(b), width)
    wsums[:k] = sums[:k]
    return uniques, counts, wsums, offsets, inverse


def _rows(fn, idx, v, w, widths, dtypes, fills):
    idx = np.asarray(idx)
    v, w = np.broadcast_to(v, idx.shape), np.broadcast_to(w, idx.shape)
    c = idx.shape[-1] if idx.ndim else 1
    lead = idx.shape[:-1] if idx.ndim else ()
    n = int(np.prod(lead, dtype=np.int64))
    out = [np.full((n, wd if wd is not None else c), f, dt) for wd, dt, f in zip(widths, dtypes, fills)]
    fi, fv, fw = idx.reshape(n, c), np.asarray(v).reshape(n, c), np.asarray(w).reshape(n, c)
    for r in range(n):
        for o, x in zip(out, fn(fi[r], fv[r], fw[r])):
            o[r] = x
    return [o.reshape(lead + o.shape[1:]) for o in out]


def wunique_rows(idx, v, w, n_bins, size=None):
    """the same along the last axis of idx"""
    idx = np.asarray(idx)
    c = idx.shape[-1] if idx.ndim else 1
    wd = c if size is None else int(size)
    out = _rows(lambda i, x, y: wunique_row(i, x, y, n_bins, size), idx, v, w, (wd, wd, wd, n_bins + 1, None),
                (np.float64, np.int64, np.float64, np.int64, np.int64), (PAD, 0, 0.0, 0, -1))
    out[4] = out[4].reshape(idx.shape)
    return tuple(out)


def wmode_row(index, values, weights, n_bins):
    """(count [B], nunique [B], mode [B], mode_weight [B]) of one row, from its entries"""
    b, vals, cnt, sums, _, _ = runs_row(index, values, weights, n_bins)
    count, nunique = np.zeros(n_bins, np.int64), np.zeros(n_bins, np.int64)
    mode, mode_weight = np.full(n_bins, PAD), np.zeros(n_bins)
    for bin_ in range(n_bins):
        sel = np.flatnonzero(b == bin_)
        if not len(sel):
            continue
        count[bin_], nunique[bin_] = cnt[sel].sum(), len(sel)
        if np.isnan(sums[sel]).any():
            mode[bin_] = mode_weight[bin_] = PAD
        else:
            first = sel[int(np.argmax(sums[sel]))]  # (np.argmax: the first of equal ones; -0.0 == +0.0)
            mode[bin_], mode_weight[bin_] = vals[first], sums[first]
    return count, nunique, mode, mode_weight


def wmode_rows(idx, v, w, n_bins):
    return tuple(_rows(lambda i, x, y: wmode_row(i, x, y, n_bins), idx, v, w, (n_bins,) * 4,
                       (np.int64, np.int64, np.float64, np.float64), (0, 0, PAD, 0.0)))


def brute_force(index, values, weights, n_bins):
    """one row from the definition, a loop per bin with np.unique: (uniques, counts, weight sums, offsets) uncut, the sums with
    math.fsum over the members in position order"""
    index = np.asarray(index)
    v = np.asarray(values).astype(np.float64)
    w = np.asarray(np.broadcast_to(weights, index.shape)).astype(np.float64)
    uniques, counts, sums, offsets = [], [], [], [0]
    for b in range(n_bins):
        sel = (index == b) & ~np.isnan(v)
        vals, cnt = np.unique(v[sel], return_counts=True)  # (np.unique: -0.0 and +0.0 are one value)
        for x, n in zip(vals, cnt):
            uniques.append(x)
            counts.append(n)
            sums.append(run_sum(w[sel & (v == x)]))
        offsets.append(len(uniques))
    return np.array(uniques, np.float64), np.array(counts, np.int64), np.array(sums, np.float64), np.array(offsets, np.int64)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_sums(got, want, what=""):
    """float64 by bits, the sign of zero included; NaN where `want` has NaN (any NaN)"""
    xw.assert_bits_equal(np.ascontiguousarray(got), np.ascontiguousarray(want, np.float64), what)


def assert_same(got, want, what=""):
    """(uniques, counts, weight_sums, offsets[, inverse]): bin_unique's outputs by uo.assert_same, the sums by their bits"""
    assert len(got) == len(want) and len(got) in (4, 5), "%s: %d outputs, want %d" % (what, len(got), len(want))
    uo.assert_same(tuple(got[:2]) + tuple(got[3:]), tuple(want[:2]) + tuple(want[3:]), what)
    assert_sums(got[2], want[2], what + " weight_sums")


def assert_mode_same(got, want, what=""):
    """(count, nunique, mode, mode_weight): int64 by value; mode and mode_weight by bits, their NaN 0x7ff8000000000000"""
    for name, g, w in zip(("count", "nunique"), got[:2], want[:2]):
        g = np.asarray(g)
        assert g.dtype == np.int64 and g.shape == np.shape(w), "%s %s: %s %s" % (what, name, g.dtype, g.shape)
        np.testing.assert_array_equal(g, w, err_msg="%s %s" % (what, name))
    for name, g, w in zip(("mode", "mode_weight"), got[2:], want[2:]):
        g = np.asarray(g)
        assert g.dtype == np.float64 and g.shape == np.shape(w), "%s %s: %s %s" % (what, name, g.dtype, g.shape)
        gb, wb = bits(g), np.where(np.isnan(w), np.uint64(NAN_BITS), bits(w))
        bad = np.flatnonzero((gb != wb).reshape(-1))
        assert bad.size == 0, "%s %s: %d of %d differ, first at %d: got %r want %r" % (
            what, name, bad.size, gb.size, bad[0], g.reshape(-1)[bad[0]], np.asarray(w).reshape(-1)[bad[0]])


def assert_within_bound(got_sums, idx, v, w, n_bins, what=""):
    """every stored sum of the rows within exact_weights' 2 gamma(n) sum|w| of math.fsum over its run"""
    idx = np.asarray(idx)
    for r in range(idx.shape[0]):
        _, _, cnt, sums, mags, _ = runs_row(idx[r], v[r], w[r], n_bins)
        k = min(len(sums), got_sums.shape[-1])
        xw.assert_within_f64_bound(got_sums[r, :k], sums[:k], mags[:k], cnt[:k], what="%s row %d" % (what, r))


# ---------------------------------------------------------------------------------------------------------------------
# the describe() lines, restated (xhist_rank.hip)
# ---------------------------------------------------------------------------------------------------------------------
def predict_unique(*args, **kw):
    return uo.predict(*args, **kw)


def predict_mode(cus, edges, cmp, sdt, vdt, n_rows, n_cols, layout_fast=True):
    if n_cols == 0:
        return dict(words=0, rows_per_launch=0, sort=None)
    sort = so.predict(cus, edges, cmp, sdt, vdt, n_rows, n_cols, layout_fast=layout_fast)
    return dict(words=-(-n_cols // WORD), rows_per_launch=sort["rows_per_launch"], sort=sort)


def parse(desc, name):
    assert desc.startswith(name + " ") and " | " in desc, desc
    mine, sort = desc.split(" | ", 1)
    out = {k: int(x) for k, x in re.findall(r"(\w+)=(\S+)", mine)}
    out["sort"] = None if sort == "none" else so.parse(sort)
    return out


def assert_variant(desc, name, want):
    got = parse(desc, name)
    assert got == want, "landed elsewhere:\n  got  %s\n  want %s\n  (%s)" % (got, want, desc)
    return got
