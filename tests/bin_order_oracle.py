"""bin_order on the CPU: what `order` and `offsets` must be for an array of bin indices, stated with numpy's own stable sort,
and the host's launch geometry (xhist_group.hip's group_geometry, over xhist_runs.hip.h's runs_geometry) with the describe() line
it leads to, restated.

Everything here is integer work: every comparison made with it is bit for bit."""
import re

import numpy as np

import map_oracle as mo

LDS_MAX = mo.LDS_MAX
STEP = 64  # positions of one step of a wave: a chunk is whole steps
SLICE = 64  # chunks of one slice of the scan
SLICE_GRID = 4096  # workgroups that walk the (row, tile of bins, slice) units of the slices' kernels
MAX_BINS = LDS_MAX // 4 - 1  # one 4-byte counter per bin and one more for the dropped samples, one wave per workgroup


# ---------------------------------------------------------------------------------------------------------------------
# results
# ---------------------------------------------------------------------------------------------------------------------
def keys_of(index, n_bins):
    """bin_index with -1 replaced by n_bins: the dropped samples sort behind every bin"""
    index = np.asarray(index)
    return np.where(index < 0, n_bins, index).astype(np.int64)


def order_offsets(index, n_bins):
    """(order, offsets) of bin indices [..., c] (-1: dropped) along the last axis: order = np.argsort(key, kind="stable"),
    offsets[b] = #{p : key[p] < b} for b = 0 .. n_bins, by np.searchsorted on the sorted keys"""
    key = keys_of(index, n_bins)
    order = np.argsort(key, axis=-1, kind="stable").astype(np.int64)
    lead = key.shape[:-1]
    c = key.shape[-1]
    k2 = np.take_along_axis(key, order, axis=-1).reshape(int(np.prod(lead, dtype=np.int64)), c)  # (numpy infers no extent next to 0)
    if k2.shape[0] > 1 << 16:  # (millions of short rows: the definition itself, counted at once)
        offsets = (k2[:, None, :] < np.arange(n_bins + 1)[None, :, None]).sum(-1, dtype=np.int64)
    else:
        offsets = np.empty((k2.shape[0], n_bins + 1), np.int64)
        for r in range(k2.shape[0]):
            offsets[r] = np.searchsorted(k2[r], np.arange(n_bins + 1), side="left")
    return order, offsets.reshape(lead + (n_bins + 1,))


def bucket_loop(index, n_bins):
    """the same for one row, by a pure-Python bucket loop: append every position to its key's list, in ascending position"""
    buckets = [[] for _ in range(n_bins + 1)]
    for p, b in enumerate(np.asarray(index).tolist()):
        buckets[n_bins if b < 0 else b].append(p)
    order = [p for bucket in buckets for p in bucket]
    offsets, run = [], 0
    for bucket in buckets:
        offsets.append(run)
        run += len(bucket)
    return np.array(order, np.int64).reshape(-1), np.array(offsets, np.int64)


def rows_of(index, axis):
    """bin indices in the sample shape -> [kept axes..., c]: the reduced axes in ascending number, C order, as the last axis"""
    index = np.asarray(index)
    ndim = index.ndim
    red = list(range(ndim)) if axis is None else sorted(int(a) % ndim for a in np.atleast_1d(axis))
    kept = [i for i in range(ndim) if i not in red]
    moved = np.transpose(index, kept + red)
    c = int(np.prod([index.shape[i] for i in red], dtype=np.int64))
    return moved.reshape(tuple(index.shape[i] for i in kept) + (c,))


# ---------------------------------------------------------------------------------------------------------------------
# the host's geometry, restated (xhist_group.hip)
# ---------------------------------------------------------------------------------------------------------------------
def geometry(cus, n_bins, n_rows, n_cols):
    """waves per workgroup, ballots of a step, how a row is cut, the LDS of a workgroup, rows per launch; n_cols > 0 and
    n_bins <= MAX_BINS"""
    nb1 = n_bins + 1
    wave_lds = nb1 * 4
    assert wave_lds <= LDS_MAX and n_cols > 0
    waves = 4 if 4 * wave_lds <= LDS_MAX else 2 if 2 * wave_lds <= LDS_MAX else 1
    bits = 0
    while (1 << bits) < nb1:
        bits += 1
    per_cu = max(1, min(32, 160 * 1024 // wave_lds))
    target = cus * per_cu
    steps = -(-n_cols // STEP)
    want = min(steps, -(-target // n_rows))
    want = max(1, min(want, n_cols // (2 * nb1)))  # (the counter table: at most a quarter of the key block's bytes)
    chunk = -(-(-(-n_cols // want)) // STEP) * STEP
    chunks = -(-n_cols // chunk)
    max_units = ((1 << 32) - 1) // (STEP * waves) * waves
    rows_per_launch = max(1, min(max_units // chunks, ((1 << 32) - 1) // 256))
    return dict(bits=bits, waves=waves, block=STEP * waves, chunks=chunks, chunk=chunk, lds_bytes=waves * wave_lds,
                rows_per_launch=rows_per_launch)


def slice_units(cus, n_bins, n_rows, n_cols):
    """(slices of a row, units of the slices' kernels over all rows of one launch; 0 where a row is one chunk and they are not
    launched)"""
    g = geometry(cus, n_bins, n_rows, n_cols)
    if g["chunks"] == 1:
        return 1, 0
    slices = -(-g["chunks"] // SLICE)
    block = 64 if n_bins + 1 <= 64 else 256
    return slices, min(n_rows, g["rows_per_launch"]) * -(-(n_bins + 1) // block) * slices


def table_bytes(cus, n_bins, n_rows, n_cols):
    g = geometry(cus, n_bins, n_rows, n_cols)
    return n_rows * g["chunks"] * (n_bins + 1) * 4


def predict(cus, edges, cmp, sdt, n_rows, n_cols, layout_fast=True):
    """the describe() fields of a bin_order call; `keys` is the family of bin_index's kernels (map_oracle.predict; np.linspace
    edges, whose fine table or arithmetic form the fast family always takes)"""
    D = len(edges)
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    if n_cols == 0:
        return dict(keys="none", bits=0, waves=0, block=0, chunks=0, chunk=0, lds_bytes=0, rows_per_launch=0, D=D, cmp=cmp)
    keys = mo.predict("index", cus, edges, cmp, sdt, None, n_rows, n_cols, fine=1, arith=True, layout_fast=layout_fast)["family"]
    return dict(geometry(cus, n_bins, n_rows, n_cols), keys=keys, D=D, cmp=cmp)


def parse(desc):
    assert desc.startswith("group "), desc
    kv = dict(re.findall(r"(\w+)=(\S+)", desc))
    return {k: (v if k == "keys" else int(v)) for k, v in kv.items()}


def assert_variant(desc, want):
    got = parse(desc)
    assert got == want, "landed elsewhere:\n  got  %s\n  want %s\n  (%s)" % (got, want, desc)
    return got


# ---------------------------------------------------------------------------------------------------------------------
# the identities a result must satisfy whatever produced it
# ---------------------------------------------------------------------------------------------------------------------
def assert_grouped(order, offsets, index, n_bins, what=""):
    """one row: a permutation, keys non-decreasing along it, positions ascending inside every segment, offsets the prefix of
    the counts"""
    order, offsets, key = np.asarray(order), np.asarray(offsets), keys_of(index, n_bins)
    c = key.shape[0]
    assert order.shape == (c,) and offsets.shape == (n_bins + 1,), (what, order.shape, offsets.shape)
    assert np.array_equal(np.sort(order), np.arange(c)), "%s: not a permutation" % what
    ks = key[order]
    assert (np.diff(ks) >= 0).all(), "%s: keys descend along the order" % what
    same = np.diff(ks) == 0
    assert (np.diff(order)[same] > 0).all(), "%s: positions of one key are not ascending" % what
    counts = np.bincount(key, minlength=n_bins + 1)
    assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(counts)[:-1]])), "%s: offsets are not the prefix of the counts" % what
