"""bin_rank on the CPU: what `rank` must be for bin indices and values, stated with np.lexsort over the bin indices and
core.extrema_keys as tests/bin_sort_oracle.py states bin_sort, with tie runs by == inside each bin; a brute-force count of lt,
eq, d and D per sample to hold it to; and the describe() line of the call, restated.

Every rank is an integer or a half-integer below 2^31 and pct is one IEEE float64 division: every comparison made with this is
bit for bit (a NaN is held to its place, as tests/map_oracle.assert_bits holds it)."""
import re

import numpy as np

import bin_order_oracle as bo
import bin_sort_oracle as so

METHODS = ("average", "min", "max", "dense", "ordinal")
WORD = 64  # sorted positions of one word of head bits


# ---------------------------------------------------------------------------------------------------------------------
# results
# ---------------------------------------------------------------------------------------------------------------------
def sorted_domain(index, values, n_bins, descending=False):
    """one row in bin_sort's order: (order, the sorted bin keys, the sorted values as float64, head) with head[i] true where
    position i starts a tie run: i == 0, another bin than i - 1, or a value that is not == the one before (every NaN)"""
    key = bo.keys_of(np.asarray(index), n_bins)
    v = np.asarray(np.broadcast_to(values, key.shape)).astype(np.float64)
    order = np.lexsort((so.value_keys(v, descending), key))
    ks, vs = key[order], v[order]
    head = np.ones(len(ks), bool)
    head[1:] = (ks[1:] != ks[:-1]) | ~(vs[1:] == vs[:-1])
    return order, ks, vs, head


def rank_row(index, values, n_bins, method="average", descending=False, pct=False):
    """float64 [c]: the ranks of one row"""
    assert method in METHODS, method
    order, ks, vs, head = sorted_domain(index, values, n_bins, descending)
    c = len(ks)
    out = np.full(c, np.nan)
    if c == 0:
        return out
    i = np.arange(c)
    valid = (ks < n_bins) & ~np.isnan(vs)
    s = np.maximum.accumulate(np.where(head, i, 0))  # the last head at or before i
    nxt = np.minimum.accumulate(np.where(head, i, c)[::-1])[::-1]  # the first head at or after i
    e = np.concatenate([nxt[1:], [c]])  # the first head after i
    o = np.searchsorted(ks, ks, side="left")  # where the bin of i starts
    heads = np.cumsum(head)
    if method == "average":
        r = (s + e - 2 * o + 1) / 2.0
    elif method == "min":
        r = (s - o + 1).astype(np.float64)
    elif method == "max":
        r = (e - o).astype(np.float64)
    elif method == "dense":
        r = (heads - heads[o] + 1).astype(np.float64)
    else:
        r = (i - o + 1).astype(np.float64)
    if pct:
        per_bin = np.bincount(ks[valid & head] if method == "dense" else ks[valid], minlength=n_bins + 1)
        with np.errstate(invalid="ignore", divide="ignore"):
            r = r / per_bin[ks].astype(np.float64)
    out[order] = np.where(valid, r, np.nan)
    return out


def rank_rows(idx, v, n_bins, method="average", descending=False, pct=False):
    """float64 in the shape of idx: the ranks along the last axis"""
    idx = np.asarray(idx)
    v = np.broadcast_to(v, idx.shape)
    c = idx.shape[-1] if idx.ndim else 1
    if idx.size == 0:
        return np.empty(idx.shape, np.float64)
    flat_i, flat_v = idx.reshape(-1, c), np.asarray(v).reshape(-1, c)
    out = np.empty(flat_i.shape, np.float64)
    for r in range(flat_i.shape[0]):
        out[r] = rank_row(flat_i[r], flat_v[r], n_bins, method, descending, pct)
    return out.reshape(idx.shape)


def brute_force(index, values, n_bins, method="average", descending=False, pct=False):
    """the same for one row from the definition: lt, eq, d and D counted per sample over the values of its bin with Python's
    comparisons, and ordinal from sorted() on (value key, position) tuples"""
    index = np.asarray(index).tolist()
    v = [float(x) for x in np.asarray(values).astype(np.float64)]
    vk = [int(x) for x in so.value_keys(np.asarray(values), descending)]
    out = np.full(len(v), np.nan)
    for p, (b, x) in enumerate(zip(index, v)):
        if not 0 <= b < n_bins or x != x:
            continue
        members = [q for q in range(len(v)) if index[q] == b and v[q] == v[q]]
        before = (lambda y: y > x) if descending else (lambda y: y < x)
        lt = sum(1 for q in members if before(v[q]))
        eq = sum(1 for q in members if v[q] == x)
        d = len({v[q] for q in members if before(v[q])}) + 1  # (-0.0 and 0.0 are one element of a set)
        n, D = len(members), len({v[q] for q in members})
        if method == "average":
            r = (2 * lt + eq + 1) / 2
        elif method == "min":
            r = lt + 1
        elif method == "max":
            r = lt + eq
        elif method == "dense":
            r = d
        else:
            r = sorted((vk[q], q) for q in members).index((vk[p], p)) + 1
        out[p] = np.float64(r) / np.float64(D if method == "dense" else n) if pct else r
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the describe() line, restated (xhist_rank.hip)
# ---------------------------------------------------------------------------------------------------------------------
def predict(cus, edges, cmp, sdt, vdt, n_rows, n_cols, method, descending, pct, layout_fast=True):
    """the fields of a bin_rank call with bins: its own, and under "sort" those of the bin_sort call inside it"""
    head = dict(method=method, pct=int(bool(pct)), descending=int(bool(descending)))
    if n_cols == 0:
        return dict(head, words=0, rows_per_launch=0, sort=None)
    sort = so.predict(cus, edges, cmp, sdt, vdt, n_rows, n_cols, layout_fast=layout_fast)
    return dict(head, words=-(-n_cols // WORD), rows_per_launch=sort["rows_per_launch"], sort=sort)


def parse(desc):
    assert desc.startswith("rank ") and " | " in desc, desc
    mine, sort = desc.split(" | ", 1)
    kv = dict(re.findall(r"(\w+)=(\S+)", mine))
    out = {k: (v if k == "method" else int(v)) for k, v in kv.items()}
    out["sort"] = None if sort == "none" else so.parse(sort)
    return out


def assert_variant(desc, want):
    got = parse(desc)
    assert got == want, "landed elsewhere:\n  got  %s\n  want %s\n  (%s)" % (got, want, desc)
    return got
