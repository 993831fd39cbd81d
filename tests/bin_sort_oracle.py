"""bin_sort on the CPU: what `order` and `offsets` must be for bin indices and values, stated with np.lexsort over
core.extrema_keys, and the host's launch geometry (xhist_runs.hip.h's runs_geometry with the constants xhist_sort.hip hands it),
pass table (xhist_sort.hip's sort_value_shift) and describe() line, restated.

Everything here is integer work: every comparison made with it is bit for bit."""
import re

import numpy as np

import bin_order_oracle as bo
import map_oracle as mo

STEP = 64  # records of one step of a wave: a chunk is whole steps
SLICE = 64  # chunks of one slice of the scan
WAVES = 4  # waves of a workgroup
MIN_CHUNK = 512  # positions of a chunk, unless the row is shorter
COUNTER_BYTES = 256 << 20  # counters of one launch's rows, 1 KiB per (row, chunk)
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)

# the low bits of a value key that are constant up to the sign, per dtype of the values (their name in describe())
VALUE_SHIFT = {"f64": 0, "f32": 29, "f16": 42, "i64": 0, "i32": 21, "i16": 37, "i8": 45, "u64": 0, "u32": 21, "u16": 37, "u8": 45,
               "bool": 52}
DTYPE_NAME = {np.dtype(np.float64): "f64", np.dtype(np.float32): "f32", np.dtype(np.float16): "f16", np.dtype(np.int64): "i64",
              np.dtype(np.int32): "i32", np.dtype(np.int16): "i16", np.dtype(np.int8): "i8", np.dtype(np.uint64): "u64",
              np.dtype(np.uint32): "u32", np.dtype(np.uint16): "u16", np.dtype(np.uint8): "u8", np.dtype(np.bool_): "bool"}


# ---------------------------------------------------------------------------------------------------------------------
# results
# ---------------------------------------------------------------------------------------------------------------------
def value_keys(values, descending=False):
    """uint64: core.extrema_keys of the values taken as float64, complemented when descending, 2^64 - 1 for NaN either way"""
    from xhistogram_amd import core

    v = np.asarray(values).astype(np.float64)
    k = core.extrema_keys(v).reshape(v.shape)
    if descending:
        k = ~k
    return np.where(np.isnan(v), ALL_ONES, k)


def order_offsets(index, values, n_bins, descending=False):
    """(order, offsets) of bin indices and values [..., c] along the last axis: order = np.lexsort((vk, key)), offsets[b] =
    #{p : key[p] < b} for b = 0 .. n_bins"""
    key = bo.keys_of(index, n_bins)
    vk = value_keys(np.broadcast_to(values, key.shape), descending)
    order = np.lexsort((vk, key), axis=-1).astype(np.int64)
    lead, c = key.shape[:-1], key.shape[-1]
    k2 = np.take_along_axis(key, order, axis=-1).reshape(int(np.prod(lead, dtype=np.int64)), c)
    offsets = np.empty((k2.shape[0], n_bins + 1), np.int64)
    for r in range(k2.shape[0]):
        offsets[r] = np.searchsorted(k2[r], np.arange(n_bins + 1), side="left")
    return order, offsets.reshape(lead + (n_bins + 1,))


def brute_force(index, values, n_bins, descending=False):
    """the same for one row by Python's sorted on (bin key, value key, position) tuples of Python integers"""
    key = bo.keys_of(index, n_bins).tolist()
    vk = [int(x) for x in value_keys(values, descending)]
    rows = sorted((key[p], vk[p], p) for p in range(len(key)))
    order = np.array([p for _, _, p in rows], np.int64).reshape(-1)
    offsets = np.array([sum(1 for k in key if k < b) for b in range(n_bins + 1)], np.int64)
    return order, offsets


# ---------------------------------------------------------------------------------------------------------------------
# the host's geometry and pass table, restated (xhist_sort.hip)
# ---------------------------------------------------------------------------------------------------------------------
def value_passes(vdtype):
    return 8 - VALUE_SHIFT[vdtype] // 8


def bin_passes(n_bins):
    bits = 0
    while (1 << bits) < n_bins + 1:
        bits += 1
    return -(-bits // 8)


def geometry(cus, n_rows, n_cols):
    """how a row is cut and the rows of a launch; n_cols > 0"""
    assert n_cols > 0 and n_rows > 0
    target = cus * 32
    steps = -(-n_cols // STEP)
    want = min(steps, -(-target // n_rows))
    want = max(1, min(want, n_cols // MIN_CHUNK))
    chunk = -(-(-(-n_cols // want)) // STEP) * STEP
    chunks = -(-n_cols // chunk)
    slices = 1 if chunks == 1 else -(-chunks // SLICE)
    max_units = ((1 << 32) - 1) // (STEP * WAVES) * WAVES
    rows = min(max_units // chunks, ((1 << 32) - 1) // 256)
    rows = max(1, min(rows, COUNTER_BYTES // (chunks * 1024)))
    return dict(waves=WAVES, block=STEP * WAVES, chunks=chunks, chunk=chunk, slices=slices, rows_per_launch=rows)


def predict(cus, edges, cmp, sdt, vdt, n_rows, n_cols, layout_fast=True):
    """the describe() fields of a bin_sort call; `keys` is the family of bin_index's kernels, "none" where none ran"""
    D = len(edges)
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    name = DTYPE_NAME[np.dtype(vdt)]
    if n_cols == 0:
        return dict(keys="none", value_passes=0, bin_passes=0, waves=0, block=0, chunks=0, chunk=0, slices=0, rows_per_launch=0, D=D,
                    cmp=cmp, vdtype=name)
    keys = "none"
    if n_bins > 0:
        keys = mo.predict("index", cus, edges, cmp, sdt, None, n_rows, n_cols, fine=1, arith=True, layout_fast=layout_fast)["family"]
    return dict(geometry(cus, n_rows, n_cols), keys=keys, value_passes=value_passes(name), bin_passes=bin_passes(n_bins), D=D, cmp=cmp,
                vdtype=name)


def parse(desc):
    assert desc.startswith("sort "), desc
    kv = dict(re.findall(r"(\w+)=(\S+)", desc))
    return {k: (v if k in ("keys", "vdtype") else int(v)) for k, v in kv.items()}


def assert_variant(desc, want):
    got = parse(desc)
    assert got == want, "landed elsewhere:\n  got  %s\n  want %s\n  (%s)" % (got, want, desc)
    return got


# ---------------------------------------------------------------------------------------------------------------------
# the identities a result must satisfy whatever produced it
# ---------------------------------------------------------------------------------------------------------------------
def assert_sorted(order, offsets, index, values, n_bins, descending=False, what=""):
    """one row: a permutation, (bin key, value key, position) strictly ascending along it, offsets the prefix of the counts"""
    order, offsets, key = np.asarray(order), np.asarray(offsets), bo.keys_of(index, n_bins)
    c = key.shape[0]
    assert order.shape == (c,) and offsets.shape == (n_bins + 1,), (what, order.shape, offsets.shape)
    assert np.array_equal(np.sort(order), np.arange(c)), "%s: not a permutation" % what
    ks, vs = key[order], value_keys(values, descending)[order]
    dk = np.diff(ks)
    assert (dk >= 0).all(), "%s: bin keys descend along the order" % what
    same = dk == 0
    assert (vs[1:][same] >= vs[:-1][same]).all(), "%s: value keys descend inside a bin" % what
    tie = same & (vs[1:] == vs[:-1])
    assert (np.diff(order)[tie] > 0).all(), "%s: positions of one (bin, value) are not ascending" % what
    counts = np.bincount(key, minlength=n_bins + 1)
    assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(counts)[:-1]])), "%s: offsets are not the prefix of the counts" % what
