"""histogram_mode on the CPU: what (count, nunique, mode, mode_count) must be for bin indices and values, stated on
tests/bin_rank_oracle.sorted_domain (np.lexsort over the bin indices and core.extrema_keys, tie runs by == inside each bin): a
bin's distinct values are its runs of non-NaN values, its mode the first of its longest runs; a brute-force count with Python's
== to hold it to; and the describe() line of the call, restated.

Everything here is an integer or the bits of one of the input values: every comparison made with this is bit for bit (int64 by
value, `mode` by its bit pattern, as tests/map_oracle.assert_bits holds it)."""
import re

import numpy as np

import bin_rank_oracle as ro
import bin_sort_oracle as so

WORD = ro.WORD
NAN_BITS = 0x7FF8000000000000


# ---------------------------------------------------------------------------------------------------------------------
# results
# ---------------------------------------------------------------------------------------------------------------------
def mode_row(index, values, n_bins):
    """(count int64 [B], nunique int64 [B], mode float64 [B], mode_count int64 [B]) of one row"""
    _, ks, vs, head = ro.sorted_domain(index, values, n_bins)
    count = np.zeros(n_bins, np.int64)
    nunique = np.zeros(n_bins, np.int64)
    mode = np.full(n_bins, np.nan)
    mode_count = np.zeros(n_bins, np.int64)
    if len(ks) == 0 or n_bins == 0:
        return count, nunique, mode, mode_count
    valid = (ks < n_bins) & ~np.isnan(vs)
    count += np.bincount(ks[valid], minlength=n_bins + 1)[:n_bins]
    s = np.flatnonzero(head)
    e = np.concatenate([s[1:], [len(ks)]])
    keep = valid[s]  # (a run never mixes a NaN with a value, nor two bins)
    s, e = s[keep], e[keep]
    b = ks[s].astype(np.int64)
    nunique += np.bincount(b, minlength=n_bins)
    first = np.lexsort((s, -(e - s), b))  # by bin, the longest run first, of equally long ones the one that starts first
    first = first[np.concatenate([[True], b[first][1:] != b[first][:-1]])] if len(first) else first
    mode[b[first]] = vs[s[first]]
    mode_count[b[first]] = (e - s)[first]
    return count, nunique, mode, mode_count


def mode_rows(idx, v, n_bins):
    """the same along the last axis of idx: four arrays in the shape idx.shape[:-1] + (B,)"""
    idx = np.asarray(idx)
    v = np.broadcast_to(v, idx.shape)
    c = idx.shape[-1] if idx.ndim else 1
    lead = idx.shape[:-1] if idx.ndim else ()
    n = int(np.prod(lead, dtype=np.int64))
    out = (np.zeros((n, n_bins), np.int64), np.zeros((n, n_bins), np.int64), np.full((n, n_bins), np.nan), np.zeros((n, n_bins), np.int64))
    flat_i, flat_v = idx.reshape(n, c), np.asarray(v).reshape(n, c)
    for r in range(n):
        for o, x in zip(out, mode_row(flat_i[r], flat_v[r], n_bins)):
            o[r] = x
    return tuple(o.reshape(lead + (n_bins,)) for o in out)


def brute_force(index, values, n_bins):
    """the same for one row from the definition: per bin a Python list of the non-NaN values, the distinct ones found with ==,
    each counted with ==; the most frequent, then the smallest; -0.0 where the winner is a zero and the bin holds a -0.0"""
    index = np.asarray(index).tolist()
    v = [float(x) for x in np.asarray(values).astype(np.float64)]
    count, nunique, mode, mode_count = np.zeros(n_bins, np.int64), np.zeros(n_bins, np.int64), np.full(n_bins, np.nan), np.zeros(n_bins, np.int64)
    for b in range(n_bins):
        members = [x for i, x in zip(index, v) if i == b and x == x]
        distinct = []
        for x in members:
            if not any(x == y for y in distinct):
                distinct.append(x)
        count[b], nunique[b] = len(members), len(distinct)
        if members:
            best = max(sum(1 for y in members if y == x) for x in distinct)
            win = min(x for x in distinct if sum(1 for y in members if y == x) == best)
            if win == 0:
                win = -0.0 if any(y == 0 and np.signbit(y) for y in members) else 0.0
            mode[b], mode_count[b] = win, best
    return count, nunique, mode, mode_count


def assert_same(got, want, what=""):
    """the four outputs: int64 by value, mode by its bits (the NaN of an empty bin is 0x7ff8000000000000)"""
    names = ("count", "nunique", "mode", "mode_count")
    for name, g, w in zip(names, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, "%s %s: shape %s, want %s" % (what, name, g.shape, w.shape)
        if name == "mode":
            assert g.dtype == np.float64, "%s mode: dtype %s" % (what, g.dtype)
            gb, wb = np.ascontiguousarray(g).view(np.uint64), np.ascontiguousarray(w, np.float64).view(np.uint64)
            wb = np.where(np.isnan(w), np.uint64(NAN_BITS), wb)
        else:
            assert g.dtype == np.int64, "%s %s: dtype %s" % (what, name, g.dtype)
            gb, wb = g, w.astype(np.int64)
        bad = np.flatnonzero((gb != wb).reshape(-1))
        assert bad.size == 0, "%s %s: %d of %d differ, first at %d: got %r want %r" % (
            what, name, bad.size, gb.size, bad[0], g.reshape(-1)[bad[0]], w.reshape(-1)[bad[0]])


# ---------------------------------------------------------------------------------------------------------------------
# the describe() line, restated (xhist_rank.hip)
# ---------------------------------------------------------------------------------------------------------------------
def predict(cus, edges, cmp, sdt, vdt, n_rows, n_cols, layout_fast=True):
    """the fields of a histogram_mode call with bins: its own, and under "sort" those of the bin_sort call inside it"""
    if n_cols == 0:
        return dict(words=0, rows_per_launch=0, sort=None)
    sort = so.predict(cus, edges, cmp, sdt, vdt, n_rows, n_cols, layout_fast=layout_fast)
    return dict(words=-(-n_cols // WORD), rows_per_launch=sort["rows_per_launch"], sort=sort)


def parse(desc):
    assert desc.startswith("mode ") and " | " in desc, desc
    mine, sort = desc.split(" | ", 1)
    out = {k: int(v) for k, v in re.findall(r"(\w+)=(\S+)", mine)}
    out["sort"] = None if sort == "none" else so.parse(sort)
    return out


def assert_variant(desc, want):
    got = parse(desc)
    assert got == want, "landed elsewhere:\n  got  %s\n  want %s\n  (%s)" % (got, want, desc)
    return got
