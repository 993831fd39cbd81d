"""bin_unique on the CPU: what (uniques, counts, offsets, inverse) must be for bin indices and values, stated on
tests/bin_rank_oracle.sorted_domain (np.lexsort over the bin indices and core.extrema_keys, tie runs by == inside each bin): a
bin's distinct values are its runs of non-NaN values, in the order the sort leaves them, an entry's count the length of its run,
and the entry of a sample the number of such runs that start at or before its sorted position, less one; the cut at `size` and
the padding behind min(U, W); a brute-force restatement with Python lists and == to hold it to; and the describe() line of the
call, restated.

Everything here is an integer or the bits of one of the input values: every comparison made with this is bit for bit (int64 by
value, `uniques` by its bit pattern)."""
import re

import numpy as np

import bin_rank_oracle as ro
import bin_sort_oracle as so

WORD = ro.WORD
SCAN_TILE = 1024  # offsets one workgroup scans at a time (kUniqueTile of xhist_unique.hip.h)
NAN_BITS = 0x7FF8000000000000
PAD = np.array([NAN_BITS], np.uint64).view(np.float64)[0]


# ---------------------------------------------------------------------------------------------------------------------
# results
# ---------------------------------------------------------------------------------------------------------------------
def runs_row(index, values, n_bins):
    """one row's entries before any cut: (bin int64 [U], value float64 [U], count int64 [U], inverse int64 [c]).  A run never
    mixes a NaN with a value, nor two bins, so the kept runs are the heads that are counted and not NaN."""
    order, ks, vs, head = ro.sorted_domain(index, values, n_bins)
    c = len(ks)
    inverse = np.full(c, -1, np.int64)
    if c == 0 or n_bins == 0:
        return np.zeros(0, np.int64), np.zeros(0), np.zeros(0, np.int64), inverse
    valid = (ks < n_bins) & ~np.isnan(vs)
    s = np.flatnonzero(head)
    e = np.concatenate([s[1:], [c]])
    keep = valid[s]
    s, e = s[keep], e[keep]
    entry = np.cumsum(head & valid) - 1  # of a valid position: the kept heads at or before it, less one
    inverse[order[valid]] = entry[valid]
    return ks[s].astype(np.int64), vs[s], (e - s).astype(np.int64), inverse


def cut(b, vals, cnt, n_bins, width):
    """(uniques float64 [width], counts int64 [width], offsets int64 [B + 1]) of one row's entries: the first min(U, width) of
    them, padding behind; the offsets count every entry, cut or not"""
    uniques = np.full(width, PAD)
    counts = np.zeros(width, np.int64)
    offsets = np.zeros(n_bins + 1, np.int64)
    if n_bins > 0:
        offsets[1:] = np.cumsum(np.bincount(b, minlength=n_bins))
    k = min(len(b), width)
    uniques[:k] = vals[:k]
    counts[:k] = cnt[:k]
    return uniques, counts, offsets


def unique_row(index, values, n_bins, size=None):
    """(uniques [W], counts [W], offsets [B + 1], inverse [c]) of one row; W = c where size is None"""
    b, vals, cnt, inverse = runs_row(index, values, n_bins)
    return cut(b, vals, cnt, n_bins, len(np.asarray(index)) if size is None else int(size)) + (inverse,)


def unique_rows(idx, v, n_bins, size=None):
    """the same along the last axis of idx: uniques and counts in idx.shape[:-1] + (W,), offsets + (B + 1,), inverse idx.shape"""
    idx = np.asarray(idx)
    v = np.broadcast_to(v, idx.shape)
    c = idx.shape[-1] if idx.ndim else 1
    lead = idx.shape[:-1] if idx.ndim else ()
    n = int(np.prod(lead, dtype=np.int64))
    w = c if size is None else int(size)
    out = (np.full((n, w), PAD), np.zeros((n, w), np.int64), np.zeros((n, n_bins + 1), np.int64), np.full((n, c), -1, np.int64))
    flat_i, flat_v = idx.reshape(n, c), np.asarray(v).reshape(n, c)
    for r in range(n):
        for o, x in zip(out, unique_row(flat_i[r], flat_v[r], n_bins, size)):
            o[r] = x
    return out[0].reshape(lead + (w,)), out[1].reshape(lead + (w,)), out[2].reshape(lead + (n_bins + 1,)), out[3].reshape(idx.shape)


def brute_force(index, values, n_bins, size=None):
    """the same for one row from the definition: per bin a Python list of the non-NaN values, the distinct ones found with ==,
    sorted, each counted with ==; a zero reads -0.0 where the bin holds a -0.0; a sample's entry is found with == in its bin's
    list"""
    index = np.asarray(index).tolist()
    v = [float(x) for x in np.asarray(values).astype(np.float64)]
    width = len(v) if size is None else int(size)
    vals, cnt, offsets, first = [], [], [0], {}
    for b in range(n_bins):
        members = [x for i, x in zip(index, v) if i == b and x == x]
        distinct = []
        for x in members:
            if not any(x == y for y in distinct):
                distinct.append(x)
        distinct.sort()
        first[b] = len(vals)
        for x in distinct:
            if x == 0:
                x = -0.0 if any(y == 0 and np.signbit(y) for y in members) else 0.0
            vals.append(x)
            cnt.append(sum(1 for y in members if y == x))
        offsets.append(len(vals))
    inverse = np.full(len(v), -1, np.int64)
    for p, (b, x) in enumerate(zip(index, v)):
        if 0 <= b < n_bins and x == x:
            inverse[p] = next(u for u in range(first[b], offsets[b + 1]) if vals[u] == x)
    uniques, counts = np.full(width, PAD), np.zeros(width, np.int64)
    k = min(len(vals), width)
    uniques[:k] = vals[:k]
    counts[:k] = cnt[:k]
    return uniques, counts, np.array(offsets, np.int64), inverse


def assert_same(got, want, what=""):
    """(uniques, counts, offsets) or (uniques, counts, offsets, inverse): int64 by value, uniques by its bits (the padding is
    0x7ff8000000000000)"""
    names = ("uniques", "counts", "offsets", "inverse")
    assert len(got) == len(want) and len(got) in (3, 4), "%s: %d outputs, want %d" % (what, len(got), len(want))
    for name, g, w in zip(names, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, "%s %s: shape %s, want %s" % (what, name, g.shape, w.shape)
        if name == "uniques":
            assert g.dtype == np.float64, "%s uniques: dtype %s" % (what, g.dtype)
            gb, wb = np.ascontiguousarray(g).view(np.uint64), np.ascontiguousarray(w, np.float64).view(np.uint64)
        else:
            assert g.dtype == np.int64, "%s %s: dtype %s" % (what, name, g.dtype)
            gb, wb = g, w.astype(np.int64)
        bad = np.flatnonzero((gb != wb).reshape(-1))
        assert bad.size == 0, "%s %s: %d of %d differ, first at %d: got %r want %r" % (
            what, name, bad.size, gb.size, bad[0], g.reshape(-1)[bad[0]], w.reshape(-1)[bad[0]])


# ---------------------------------------------------------------------------------------------------------------------
# the describe() line, restated (xhist_rank.hip)
# ---------------------------------------------------------------------------------------------------------------------
def predict(cus, edges, cmp, sdt, vdt, n_rows, n_cols, size, inverse, layout_fast=True):
    """the fields of a bin_unique call with bins: its own, and under "sort" those of the bin_sort call inside it"""
    head = dict(size=int(size), inverse=int(bool(inverse)))
    if n_cols == 0:
        return dict(head, words=0, rows_per_launch=0, sort=None)
    sort = so.predict(cus, edges, cmp, sdt, vdt, n_rows, n_cols, layout_fast=layout_fast)
    return dict(head, words=-(-n_cols // WORD), rows_per_launch=sort["rows_per_launch"], sort=sort)


def parse(desc):
    assert desc.startswith("unique ") and " | " in desc, desc
    mine, sort = desc.split(" | ", 1)
    out = {k: int(v) for k, v in re.findall(r"(\w+)=(\S+)", mine)}
    out["sort"] = None if sort == "none" else so.parse(sort)
    return out


def assert_variant(desc, want):
    got = parse(desc)
    assert got == want, "landed elsewhere:\n  got  %s\n  want %s\n  (%s)" % (got, want, desc)
    return got
