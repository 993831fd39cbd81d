"""The helper kernels the library launches directly — strided copies, min / max, moments, buffer adds, the staging kernels of
Plan.execute — each held to an exact oracle, and each launch variant predicted from a restatement of the host's choice.

Memory comes from `_native.DeviceBuffer`; pointers and strides go to `_native.copy_nd`, `_native.minmax`, `_native.moments` and
`DeviceBuffer.add` directly, so that every case chooses alignment, strides and slack itself:

 * copies and adds write into allocations larger than their footprint, pre-filled with a byte pattern: every byte outside the
   footprint (computed on the host from shape and strides) must be unchanged, every byte inside must equal numpy's;
 * `predict_copy` / `predict_minmax` restate xhist_buffer_copy_nd's and xhist_minmax's host-side choice; every case asserts that
   the prediction is the variant the case was built for, and `test_helper_variants_as_launched` runs the cases once more in a
   fresh process whose kernel log records every launch (XHIST_AMD_KERNEL_LOG_ALL) and holds the kernels the library really
   launched against the predictions;
 * moments use the exactly summable grid of tests/values_exact.py: count, min, max and mean bit for bit, M2 within the float64
   bound of that module widened by the one term xhist_moments leaves out (derived at `_moments_m2_extra`);
 * the closing test holds the set of predicted instantiations against the helper instantiations the shared object carries and
   against the kernel log of the session."""
import ctypes as C
import itertools
import json
import math
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import values_exact as vx
from oracle import oracle_np as onp
from xhistogram_amd import _native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 1024  # bytes of slack on each side of a footprint
PATTERN = 0xA5

TAG_DTYPE = {
    _native.F64: np.float64, _native.F32: np.float32, _native.F16: np.float16, _native.I64: np.int64, _native.I32: np.int32,
    _native.I16: np.int16, _native.I8: np.int8, _native.U64: np.uint64, _native.U32: np.uint32, _native.U16: np.uint16,
    _native.U8: np.uint8, _native.BOOL: np.bool_,
}
ALL_DTYPES = [np.dtype(t) for t in TAG_DTYPE.values()]
C_UNSIGNED = {1: "unsigned char", 2: "unsigned short", 4: "unsigned int", 8: "unsigned long"}

# every helper instantiation some case of this module predicted (and then compared with its oracle)
PREDICTED = set()
RAN = set()


def _kernel_census():
    if os.path.join(ROOT, "tools") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_census

    return kernel_census


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _native.load()
    assert _native.device_count() >= 1, "no MI355X visible: GPU tests must not pass on a fallback"
    assert "gfx950" in _native.device_info(0)["name"]


@pytest.fixture(autouse=True)
def _note_ran(request):
    RAN.add(request.node.originalname or request.node.name)


# ---------------------------------------------------------------------------------------------------------------------
# device bytes behind a 256-byte aligned origin
# ---------------------------------------------------------------------------------------------------------------------
class DevBytes:
    def __init__(self, host):
        """a copy of the uint8 array `host` on GPU 0; `origin` (the address of host[0]) is 256-byte aligned"""
        host = np.ascontiguousarray(host, np.uint8)
        self.nbytes = host.nbytes
        self.buf = _native.DeviceBuffer(0, self.nbytes + 256)
        self.origin = (self.buf.ptr + 255) & ~255
        self.write(0, host)

    def write(self, offset, host):
        host = np.ascontiguousarray(host)
        assert 0 <= offset and offset + host.nbytes <= self.nbytes
        if host.nbytes:
            _native.check(_native.load().xhist_buffer_copy(0, C.c_void_p(self.origin + offset), C.c_void_p(host.ctypes.data), host.nbytes, 0, None))

    def read(self):
        out = np.empty(self.nbytes, np.uint8)
        if self.nbytes:
            _native.check(_native.load().xhist_buffer_copy(0, C.c_void_p(out.ctypes.data), C.c_void_p(self.origin), self.nbytes, 1, None))
        return out

    def close(self):
        self.buf.close()


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _reach(shape, strides, item):
    """lowest byte offset and one past the highest, relative to element [0, ..., 0]; (0, 0) for an empty array"""
    if any(n == 0 for n in shape):
        return 0, 0
    lo = sum(min(0, (n - 1) * s) for n, s in zip(shape, strides))
    hi = sum(max(0, (n - 1) * s) for n, s in zip(shape, strides)) + item
    return lo, hi


def _place(shape, strides, item, mis):
    """(offset of element [0, ..., 0] from the aligned origin, bytes to allocate): the offset is `mis` modulo 256 and leaves
    GUARD bytes below the footprint, the allocation GUARD bytes above it"""
    lo, hi = _reach(shape, strides, item)
    p = GUARD - lo
    p += (mis - p) % 256
    return p, p + hi + GUARD


def _view(buf, dtype, shape, strides, offset):
    """numpy's view of the strided array inside the host copy `buf` (its constructor checks the bounds)"""
    return np.ndarray(tuple(shape), dtype, buffer=buf, offset=offset, strides=tuple(strides))


def _footprint(nbytes, shape, strides, item, offset):
    mask = np.zeros(nbytes, np.uint8)
    if all(n > 0 for n in shape):
        _view(mask, "V%d" % item, shape, strides, offset)[...] = np.void(b"\x01" * item)
    return mask.astype(bool)


# ---------------------------------------------------------------------------------------------------------------------
# copy_nd: the host's choice, restated from xhist_buffer_copy_nd
# ---------------------------------------------------------------------------------------------------------------------
def predict_copy(shape, src_ptr, src_strides, dst_ptr, dst_strides, src_tag, dst_tag):
    """(kernel, ITEM or T, normalised ndim, wlog2, tiles) of a copy; None when nothing is launched (a zero extent).
    Strides in bytes.  ITEM 0: the converting kernel.  The transposing kernel has no wlog2 (None); its tiles are the 64 x 64
    tiles over all batches."""
    item = np.dtype(TAG_DTYPE[src_tag]).itemsize
    convert = dst_tag != src_tag
    n = 1
    for e in shape:
        n *= e
    if n == 0:
        return None
    dims = []  # [extent, source stride, destination stride]: extent-1 dimensions dropped, neighbours merged
    for e, s, d in zip(shape, src_strides, dst_strides):
        if e == 1:
            continue
        if dims and dims[-1][1] == s * e and dims[-1][2] == d * e:
            dims[-1] = [dims[-1][0] * e, s, d]
        else:
            dims.append([e, s, d])
    if not dims:
        dims = [[1, 0, 0]]
    eff = item
    if not convert and dims[-1][1] == item and dims[-1][2] == item:  # widen
        for wide in (16, 8, 4, 2):
            if wide <= item:
                break
            ok = (dims[-1][0] * item) % wide == 0 and src_ptr % wide == 0 and dst_ptr % wide == 0
            ok = ok and all(s % wide == 0 and d % wide == 0 for _, s, d in dims[:-1])
            if ok:
                dims[-1] = [dims[-1][0] * item // wide, wide, wide]
                n = n * item // wide
                eff = wide
                break
    nd = len(dims)
    if not convert and nd >= 2 and dims[-1][2] == item and dims[-1][1] != item and dims[-1][0] >= 16:  # the transposing test
        kd = -1
        for k in range(nd - 1):
            if dims[k][1] > 0 and dims[k][0] >= 16 and (kd < 0 or dims[k][1] < dims[kd][1]):
                kd = k
        if kd >= 0 and not (dims[kd][1] < abs(dims[-1][1]) and dims[kd][1] <= 8 * item):
            kd = -1
        if kd >= 0:
            tiles = ((dims[kd][0] + 63) // 64) * ((dims[-1][0] + 63) // 64)
            for k in range(nd - 1):
                if k != kd:
                    tiles *= dims[k][0]
            return ("copy_nd_transpose", C_UNSIGNED[item], nd, None, tiles)
    inner = dims[-1][0]
    rows = n // inner
    wlog2 = 0
    while wlog2 < 8 and (1 << wlog2) < inner:
        wlog2 += 1
    col_tiles = (inner + (16 << wlog2) - 1) // (16 << wlog2)
    rows_per_wg = 256 >> wlog2
    tiles = ((rows + rows_per_wg - 1) // rows_per_wg) * col_tiles
    return ("copy_nd_kernel", 0 if convert else eff, nd, wlog2, tiles)


def copy_instantiation(pred):
    return "%s<%s>" % (pred[0], pred[1])


def _cstrides(shape, item):
    """C-contiguous byte strides"""
    out, s = [], item
    for n in reversed(shape):
        out.append(s)
        s *= max(n, 1)
    return tuple(reversed(out))


class CopyCase:
    """one copy: dtype, shape, byte strides of both sides, the misalignment (modulo 256) of both pointers, and the variant it
    was built for — `want` = (kernel, ITEM or T, ndim, wlog2, tiles) with None for "whatever the restatement says"; `tiles` may
    be a (lowest, highest) pair.  values: the source's logical contents (conversion cases); random bytes otherwise."""

    def __init__(self, name, dtype, shape, ss, ds, want, smis=0, dmis=0, dst_dtype=None, values=None):
        self.name, self.dtype, self.shape, self.ss, self.ds = name, np.dtype(dtype), tuple(shape), tuple(ss), tuple(ds)
        self.want, self.smis, self.dmis, self.values = want, smis, dmis, values
        self.dst_dtype = np.dtype(dst_dtype) if dst_dtype is not None else self.dtype

    def __repr__(self):
        return self.name


def _special_values(dt):
    """the extremes of a dtype whose conversion to float64 a copy must get right"""
    dt = np.dtype(dt)
    if dt == np.bool_:
        return np.array([False, True, True, False], dt)
    if dt.kind == "f":
        fi = np.finfo(dt)
        v = [0.0, -0.0, fi.smallest_subnormal, -fi.smallest_subnormal, fi.tiny, fi.max, -fi.max, np.inf, -np.inf, np.nan, 1.0, -1.5]
        return np.array(v, dt)
    ii = np.iinfo(dt)
    v = [0, 1, ii.min, ii.max, ii.max - 1]
    if dt.kind == "i":
        v += [-1, ii.min + 1]
    if dt.itemsize == 8:
        v += [2 ** 53 + 1, 2 ** 53 - 1, 2 ** 53 + 3, 2 ** 62 + 1]
        v += [-(2 ** 53 + 1), -(2 ** 53 + 3)] if dt.kind == "i" else [2 ** 63, 2 ** 63 + 1025, 2 ** 64 - 1, 2 ** 64 - 1025]
    return np.array(v, dt)


def _convert_values(dt, shape):
    dt = np.dtype(dt)
    rng = _rng("convert-%s" % dt)
    n = int(np.prod(shape))
    raw = rng.integers(0, 256, n * dt.itemsize, dtype=np.uint8).view(dt) if dt != np.bool_ else rng.integers(0, 2, n).astype(dt)
    sp = _special_values(dt)
    assert len(sp) <= n
    raw = raw.copy()
    raw[rng.permutation(n)[: len(sp)]] = sp
    return raw.reshape(shape)


def _copy_cases():
    cases = []
    K, T = "copy_nd_kernel", "copy_nd_transpose"

    def add(*a, **k):
        cases.append(CopyCase(*a, **k))

    # ITEM 1, 2, 4, 8 from the dtype: 255 elements are no whole number of the next wider unit
    for dt in (np.uint8, np.uint16, np.float32, np.float64):
        it = np.dtype(dt).itemsize
        add("item%d-1d-255" % it, dt, (255,), (it,), (it,), (K, it, 1, 8, 1))
    # widening to 2, 4, 8, 16 from items of half the width, and the four near misses that keep the item
    for wide in (2, 4, 8, 16):
        it = wide // 2
        dt = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[it]
        shape, ss, ds = (5, 6), (4 * wide, it), (5 * wide, it)
        add("widen%d" % wide, dt, shape, ss, ds, (K, wide, 2, 2, 1))
        add("widen%d-src-ptr-off" % wide, dt, shape, ss, ds, (K, it, 2, 3, 1), smis=it)
        add("widen%d-dst-ptr-off" % wide, dt, shape, ss, ds, (K, it, 2, 3, 1), dmis=it)
        add("widen%d-src-stride-off" % wide, dt, shape, (4 * wide + it, it), ds, (K, it, 2, 3, 1))
        add("widen%d-dst-stride-off" % wide, dt, shape, ss, (5 * wide + it, it), (K, it, 2, 3, 1))
        add("widen%d-row-bytes-off" % wide, dt, (5, 7), ss, ds, (K, it, 2, 3, 1))
    add("widen16-from-bytes", np.uint8, (5, 48), (64, 1), (80, 1), (K, 16, 2, 2, 1))
    add("widen16-from-bytes-src-ptr-off-by-8", np.uint8, (5, 48), (64, 1), (80, 1), (K, 8, 2, 3, 1), smis=8)
    # wlog2 0 ... 8 by the inner extent, with row counts that are no multiple of 256 >> wlog2 (one stride odd: never widened)
    for inner, wlog2 in ((2, 1), (3, 2), (5, 3), (16, 4), (17, 5), (33, 6), (65, 7), (255, 8), (256, 8), (257, 8), (4097, 8)):
        rpw = 256 >> wlog2
        rows = 2 * rpw + 3 if inner < 4097 else 3
        col_tiles = -(-inner // (16 << wlog2))
        add("wlog2-%d-inner%d" % (wlog2, inner), np.uint8, (rows, inner), (inner + 1, 1), (inner + 2, 1),
            (K, 1, 2, wlog2, -(-rows // rpw) * col_tiles))
    # inner extent 1 exists after widening only (an extent-1 dimension is dropped): rows of two bytes moved as 2-byte items
    add("wlog2-0-inner1", np.uint8, (515, 2), (4, 1), (6, 1), (K, 2, 2, 0, 3))
    # more than 8192 tiles: the grid-stride loop of copy_nd_kernel runs twice (256 * 8192 + 3 rows of inner extent 1)
    add("grid-loop", np.uint8, (256 * 8192 + 3, 2), (4, 1), (2, 1), (K, 2, 2, 0, 8193))
    # ndim 0, and 8 dimensions that stay 8 (the source is a slice in every dimension; the destination alone would merge)
    add("scalar", np.uint32, (), (), (), (K, 4, 1, 0, 1))
    add("all-extents-1", np.uint16, (1, 1, 1), (64, 8, 2), (2, 2, 2), (K, 2, 1, 0, 1))
    s8 = (2, 3, 2, 3, 2, 3, 2, 5)
    add("ndim8", np.uint16, s8, _cstrides(tuple(n + 1 for n in s8), 2), _cstrides(s8, 2), (K, 2, 8, 3, None))
    # merges: both sides (to one dimension, then widened), one side only (nothing merges), the leading pair only
    add("merge-both", np.uint8, (4, 5, 6), (30, 6, 1), (30, 6, 1), (K, 8, 1, 4, 1))
    add("merge-leading-pair", np.uint8, (4, 5, 6), (30, 6, 1), (40, 8, 1), (K, 2, 2, 2, 1))  # (20 rows of 6 bytes, moved as 2-byte items)
    add("merge-src-only", np.uint8, (4, 5, 6), (30, 6, 1), (48, 8, 1), (K, 2, 3, 2, 1))
    add("merge-dst-only", np.uint8, (4, 5, 7), (64, 9, 1), (35, 7, 1), (K, 1, 3, 3, 1))
    add("merge-none", np.uint8, (4, 5, 7), (64, 9, 1), (50, 8, 1), (K, 1, 3, 3, 1))
    # a zero extent: nothing launched, destination untouched
    add("zero-extent", np.float32, (3, 0, 4), (16, 16, 4), (16, 16, 4), None)
    # broadcast sources: stride 0 in an outer and in the inner dimension
    add("broadcast-outer", np.uint16, (6, 40), (0, 2), (82, 2), (K, 2, 2, 6, 2))
    add("broadcast-inner", np.uint16, (6, 40), (2, 0), (82, 2), (K, 2, 2, 6, 2))
    add("broadcast-outer-widened", np.uint16, (6, 40), (0, 2), (80, 2), (K, 16, 2, 3, 1))
    # negative strides on either side, the pointer at the last element
    add("negative-src-1d", np.float32, (100,), (-4,), (4,), (K, 4, 1, 7, 1))
    add("negative-src-2d", np.uint8, (9, 21), (-32, -1), (21, 1), (K, 1, 2, 5, 2))
    add("negative-dst-2d", np.uint16, (9, 21), (64, 2), (-44, -2), (K, 2, 2, 5, 2))
    add("negative-outer-widened", np.uint8, (9, 32), (-32, 1), (-48, 1), (K, 16, 2, 1, 1))
    # strided (non-contiguous) destinations: what concatenate writes into
    add("strided-dst", np.uint16, (7, 33), (68, 2), (200, 4), (K, 2, 2, 6, 2))
    add("strided-dst-3d", np.float64, (3, 4, 5), (160, 40, 8), (800, 200, 16), (K, 8, 2, 3, 1))  # (the leading pair merges on both sides)
    # conversion to float64 from every dtype tag through a transposed source, the type's extremes among the values
    for dt in ALL_DTYPES:
        it = dt.itemsize
        shape = (19, 5)  # the transpose of a contiguous (5, 19) array
        want = (K, 0, 2, 3, 1) if dt != np.float64 else (K, 8, 2, 3, 1)
        add("to-f64-%s" % dt.name, dt, shape, (it, 19 * it), (40, 8), want, dst_dtype=np.float64, values=_convert_values(dt, shape))
    add("to-f64-int64-strided-dst", np.int64, (19, 5), (8, 19 * 8), (96, 16), (K, 0, 2, 3, 1), dst_dtype=np.float64,
        values=_convert_values(np.int64, (19, 5)))
    # the transposing kernel, items of 1, 2, 4, 8 bytes: the source of (k, l) is the transpose of a contiguous (l, k) array
    for dt in (np.uint8, np.uint16, np.uint32, np.uint64):
        it = np.dtype(dt).itemsize
        c = C_UNSIGNED[it]

        def tr(name, k, l, want, ss=None, ds=None, lead=(), lead_ss=()):
            shape = tuple(lead) + (k, l)
            ss_ = tuple(lead_ss) + (ss if ss is not None else (it, k * it))
            plane = k * (l + 3) * it  # destination: rows padded by three elements, planes of whole rows
            ds_ = tuple(plane * int(np.prod(lead[i + 1:], dtype=np.int64)) for i in range(len(lead))) + (ds if ds is not None else ((l + 3) * it, it))
            add("transpose-%d-%s" % (it, name), dt, shape, ss_, ds_, want)

        gen = lambda k, l: (K, it, 2, min(8, max(0, (l - 1).bit_length())), None)  # noqa: E731
        tr("last15", 20, 15, gen(20, 15))
        tr("last16", 20, 16, (T, c, 2, None, 1))
        tr("kd15", 15, 20, gen(15, 20))
        tr("kd16", 16, 20, (T, c, 2, None, 1))
        for s in (2, 8):
            tr("kd-stride%d" % s, 16, 20, (T, c, 2, None, 1), ss=(s * it, 16 * s * it))
        tr("kd-stride9", 16, 20, gen(16, 20), ss=(9 * it, 16 * 9 * it))
        tr("kd-stride-above-last", 16, 16, gen(16, 16), ss=(4 * it, 2 * it))
        tr("kd-stride-below-last", 16, 16, (T, c, 2, None, 1), ss=(2 * it, 4 * it))
        tr("kd-stride-equals-minus-last", 16, 16, gen(16, 16), ss=(it, -it))
        tr("ragged-65x127", 65, 127, (T, c, 2, None, 4))
        tr("ragged-129x65", 129, 65, (T, c, 2, None, 6))
        tr("ragged-127x129", 127, 129, (T, c, 2, None, 6))
        tr("negative-last", 70, 33, (T, c, 2, None, 2), ss=(it, -70 * it))
        tr("negative-kd-is-no-kd", 20, 33, gen(20, 33), ss=(-it, 20 * it))
        tr("batch-stride0", 20, 70, (T, c, 3, None, 6), lead=(3,), lead_ss=(0,))
        tr("batches", 17, 18, (T, c, 4, None, 6), lead=(2, 3), lead_ss=(4 * 17 * 18 * it, 17 * 18 * it))
    add("transpose-1-grid-loop", np.uint8, (4097, 16, 16), (256, 1, 16), (256, 16, 1), (T, "unsigned char", 3, None, 4097))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return cases


COPY_CASES = _copy_cases()


def _copy_layout(case):
    """offsets of both sides' first elements from their aligned origins, and the bytes of both allocations"""
    sp, sn = _place(case.shape, case.ss, case.dtype.itemsize, case.smis)
    dp, dn = _place(case.shape, case.ds, case.dst_dtype.itemsize, case.dmis)
    return sp, sn, dp, dn


def _check_want(case, pred):
    want = case.want
    if want is None:
        assert pred is None, (case, pred)
        return
    assert pred is not None, case
    for i, (w, p) in enumerate(zip(want, pred)):
        if w is None:
            continue
        if i == 4 and isinstance(w, tuple):
            assert w[0] <= p <= w[1], (case, want, pred)
        else:
            assert w == p, (case, want, pred)


def run_copy_case(case, check_data=True):
    """runs the copy on the GPU and compares it with numpy's; returns the prediction"""
    sp, sn, dp, dn = _copy_layout(case)
    rng = _rng(case.name)
    hsrc = rng.integers(0, 256, sn, dtype=np.uint8)
    sview = _view(hsrc, case.dtype, case.shape, case.ss, sp)
    if case.values is not None:
        sview[...] = case.values
    want = np.full(dn, PATTERN, np.uint8)
    convert = case.dst_dtype != case.dtype
    dview = _view(want, case.dst_dtype, case.shape, case.ds, dp)
    dview[...] = sview.astype(np.float64) if convert else sview  # numpy's copy of the same view
    inside = _footprint(dn, case.shape, case.ds, case.dst_dtype.itemsize, dp)
    src, dst = DevBytes(hsrc), DevBytes(np.full(dn, PATTERN, np.uint8))
    try:
        stag, dtag = _native.dtype_tag(case.dtype), _native.dtype_tag(case.dst_dtype)
        pred = predict_copy(case.shape, src.origin + sp, case.ss, dst.origin + dp, case.ds, stag, dtag)
        _check_want(case, pred)
        _native.copy_nd(0, case.shape, src.origin + sp, stag, case.ss, dst.origin + dp, dtag, case.ds)
        got = dst.read()
    finally:
        src.close()
        dst.close()
    if check_data:
        outside = got[~inside]
        assert np.all(outside == PATTERN), "%s: %d bytes outside the footprint were written" % (case, int(np.sum(outside != PATTERN)))
        if convert:  # float64 results: equal bit for bit, NaN by position
            g = _view(got, np.float64, case.shape, case.ds, dp)
            w = _view(want, np.float64, case.shape, case.ds, dp)
            assert np.array_equal(np.isnan(g), np.isnan(w)), case
            ok = ~np.isnan(w)
            assert np.array_equal(g[ok].view(np.uint64), w[ok].view(np.uint64)), case
        else:
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "%s: %d bytes differ from numpy's copy, first at %d" % (case, bad.size, bad[0])
    if pred is not None:
        PREDICTED.add(copy_instantiation(pred))
    return pred


@pytest.mark.parametrize("case", COPY_CASES, ids=repr)
def test_copy_nd(case):
    run_copy_case(case)


def test_copy_nd_cases_cover_every_variant():
    """the case table itself (no launch): every ITEM and T, every wlog2, both grid-stride loops, ndim 1 and 8"""
    base = 1 << 40
    seen, wlog2s, ndims = set(), set(), set()
    loops = {"copy_nd_kernel": False, "copy_nd_transpose": False}
    for case in COPY_CASES:
        sp, _, dp, _ = _copy_layout(case)
        pred = predict_copy(case.shape, base + sp, case.ss, base + dp, case.ds, _native.dtype_tag(case.dtype), _native.dtype_tag(case.dst_dtype))
        _check_want(case, pred)
        if pred is None:
            continue
        seen.add(copy_instantiation(pred))
        ndims.add(pred[2])
        if pred[0] == "copy_nd_kernel":
            wlog2s.add(pred[3])
            loops[pred[0]] |= pred[4] > 256 * 32
        else:
            loops[pred[0]] |= pred[4] > 256 * 16
    assert seen == {"copy_nd_kernel<%d>" % i for i in (0, 1, 2, 4, 8, 16)} | {"copy_nd_transpose<%s>" % c for c in C_UNSIGNED.values()}
    assert wlog2s == set(range(9)) and {1, 8} <= ndims and all(loops.values()), (wlog2s, ndims, loops)


# ---------------------------------------------------------------------------------------------------------------------
# min / max
# ---------------------------------------------------------------------------------------------------------------------
def predict_minmax(tag, ptr, n_rows, n_cols, row_stride, col_stride, inner_rows):
    """the kernel xhist_minmax launches on a device-resident view (strides in elements)"""
    item = np.dtype(TAG_DTYPE[tag]).itemsize
    flat = tag in (_native.F64, _native.F32) and inner_rows == 0 and (n_cols == 1 or col_stride == 1) and (
        n_rows == 1 or row_stride == n_cols) and ptr % item == 0
    if flat:
        return "xhist::minmax_flat<%s>" % ("double" if tag == _native.F64 else "float")
    return "xhist::minmax_kernel"


def _np_minmax(logical):
    """numpy's NaN-propagating min and max, as float64 values"""
    with np.errstate(invalid="ignore"):
        return float(np.float64(np.min(logical))), float(np.float64(np.max(logical)))


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _flat_sizes(dt):
    tile = 256 * (16 // np.dtype(dt).itemsize) * 4
    return tile, [("below-grid", 100), ("tile-1", tile - 1), ("tile", tile), ("tile+1", tile + 1), ("1024-tiles+tail", 1024 * tile + 777)]


FLAT_CASES = [(np.dtype(dt), name, n, mis) for dt in (np.float32, np.float64) for name, n in _flat_sizes(dt)[1] for mis in (0, 1)]
FLAT_CASES.append((np.dtype(np.float64), "1025-tiles+tail", 1025 * 2048 + 5, 1))  # the grid-stride loop over full tiles runs twice


def run_minmax_flat_case(dt, n, mis, check_data=True):
    """contiguous float data starting `mis` elements past a 256-byte boundary: the extreme, and separately a NaN and an
    infinity, in element 0, in the last full tile, and in the first and the last element of the ragged tail"""
    tile = _flat_sizes(dt)[0]
    it = dt.itemsize
    rng = _rng("flat-%s-%d-%d" % (dt, n, mis))
    x = vx.grid(rng, n, dt)
    dev = DevBytes(np.concatenate([np.zeros(mis * it, np.uint8), x.view(np.uint8)]))
    ptr = dev.origin + mis * it
    try:
        tag = _native.dtype_tag(dt)
        view = _native.make_view(ptr, tag, n, 1)
        kernel = predict_minmax(tag, ptr, 1, n, n, 1, 0)
        assert kernel == "xhist::minmax_flat<%s>" % ("double" if it == 8 else "float"), kernel
        assert (ptr % 16 != 0) == (mis == 1)
        got = _native.minmax(view, 1, n, _native.MEM_DEVICE)
        if check_data:
            assert got == _np_minmax(x), (got, _np_minmax(x))
            n_full = n // tile
            spots = {0, n - 1, n_full * tile - 1 if n_full else 0, (n_full - 1) * tile if n_full else 0, min(n_full * tile, n - 1)}
            for pos in sorted(spots):
                for v in (-1000.0, 1000.0, np.nan, np.inf, -np.inf):
                    y = x.copy()
                    y[pos] = v
                    dev.write((mis + pos) * it, y[pos:pos + 1])
                    got = _native.minmax(view, 1, n, _native.MEM_DEVICE)
                    want = _np_minmax(y)
                    assert _same(got[0], want[0]) and _same(got[1], want[1]), (pos, v, got, want)
                dev.write((mis + pos) * it, x[pos:pos + 1])
    finally:
        dev.close()
    PREDICTED.add(kernel)
    return kernel


@pytest.mark.parametrize("dt,name,n,mis", FLAT_CASES, ids=lambda v: str(v))
def test_minmax_flat(dt, name, n, mis):
    run_minmax_flat_case(dt, n, mis)


@pytest.mark.parametrize("dt", [np.dtype(np.float32), np.dtype(np.float64)], ids=str)
def test_minmax_flat_signed_zeros_and_infinities(dt):
    """-0.0 among +0.0 (and the reverse) is a zero either way; infinities alone are their own extremes; no NaN is invented"""
    n = _flat_sizes(dt)[0] + 77
    for fill, one in ((0.0, -0.0), (-0.0, 0.0), (np.inf, np.inf), (-np.inf, -np.inf), (np.inf, -np.inf)):
        x = np.full(n, fill, dt)
        x[[0, n - 1, n // 2]] = one
        dev = DevBytes(x.view(np.uint8))
        try:
            tag = _native.dtype_tag(dt)
            assert predict_minmax(tag, dev.origin, 1, n, n, 1, 0).startswith("xhist::minmax_flat")
            got = _native.minmax(_native.make_view(dev.origin, tag, n, 1), 1, n, _native.MEM_DEVICE)
        finally:
            dev.close()
        assert got == _np_minmax(x), (fill, one, got)


class ViewCase:
    """a [n_rows, n_cols] view of a 1-D element buffer: element (r, c) at row_offset(r) + c * col_stride (elements)"""

    def __init__(self, name, n_rows, n_cols, rs, cs, ir=0, os_=0, mis=0):
        self.name, self.n_rows, self.n_cols, self.rs, self.cs, self.ir, self.os, self.mis = name, n_rows, n_cols, rs, cs, ir, os_, mis

    def __repr__(self):
        return self.name

    def index(self):
        r = np.arange(self.n_rows)[:, None]
        c = np.arange(self.n_cols)[None, :]
        off = r * self.rs if self.ir == 0 else (r // self.ir) * self.os + (r % self.ir) * self.rs
        return off + c * self.cs

    def span(self):
        return int(self.index().max()) + 1


VIEW_CASES = [
    ViewCase("one-row", 1, 1500, 1500, 1),
    ViewCase("rows-flat", 3, 1500, 1500, 1),  # row_stride == n_cols: still the flat kernel for floats
    ViewCase("rows-padded", 3, 1500, 1501, 1),  # row_stride == n_cols + 1: the generic kernel
    ViewCase("one-element-in", 1, 1500, 1500, 1, mis=1),
    ViewCase("column-stride", 4, 301, 1000, 3),
    ViewCase("one-column-strided", 700, 1, 3, 5),
    ViewCase("grouped-rows", 6, 257, 300, 1, ir=2, os_=1000),
    ViewCase("grouped-rows-column-stride", 6, 129, 300, 2, ir=3, os_=777),
    ViewCase("stride0-rows", 5, 300, 0, 1),
    ViewCase("stride0-columns", 5, 300, 7, 0),
    ViewCase("many-blocks", 3, 100_001, 100_003, 1),  # more elements than the 1024 x 256 threads of the grid
]


def _values_for(dt, n, rng, extremes=True):
    """n values of a dtype: random, with the type's extremes (never NaN) among them"""
    dt = np.dtype(dt)
    if dt == np.bool_:
        return rng.integers(0, 2, n).astype(dt)
    if dt.kind == "f":
        x = (rng.standard_normal(n) * 8).astype(dt)
    else:
        ii = np.iinfo(dt)
        x = rng.integers(ii.min, ii.max, n, dtype=dt, endpoint=True)
        if dt.itemsize == 8:  # keep the bulk small, so that the extremes beyond 2^53 decide
            x = (x >> np.array(20, dt)).astype(dt)
    if extremes:
        sp = _special_values(dt)
        sp = sp[np.isfinite(sp)] if dt.kind == "f" else sp
        k = min(n, len(sp))
        x[rng.permutation(n)[:k]] = sp[:k]
    return x


def run_minmax_view_case(dt, vc, check_data=True):
    dt = np.dtype(dt)
    it = dt.itemsize
    rng = _rng("view-%s-%s" % (dt, vc.name))
    base = _values_for(dt, vc.span(), rng)
    logical = base[vc.index()]
    dev = DevBytes(np.concatenate([np.zeros(vc.mis * it, np.uint8), base.view(np.uint8)]))
    try:
        ptr = dev.origin + vc.mis * it
        tag = _native.dtype_tag(dt)
        kernel = predict_minmax(tag, ptr, vc.n_rows, vc.n_cols, vc.rs, vc.cs, vc.ir)
        got = _native.minmax(_native.make_view(ptr, tag, vc.rs, vc.cs, vc.ir, vc.os), vc.n_rows, vc.n_cols, _native.MEM_DEVICE)
    finally:
        dev.close()
    if check_data:
        assert got == _np_minmax(logical), (got, _np_minmax(logical))
    PREDICTED.add(kernel)
    return kernel


@pytest.mark.parametrize("vc", VIEW_CASES, ids=repr)
@pytest.mark.parametrize("dt", ALL_DTYPES, ids=str)
def test_minmax_views(dt, vc):
    """every dtype tag through every view shape: floats take the flat kernel exactly where the view is one dense run"""
    kernel = run_minmax_view_case(dt, vc)
    dense = vc.name in ("one-row", "rows-flat", "one-element-in")
    assert (kernel != "xhist::minmax_kernel") == (dense and dt in (np.float32, np.float64)), (kernel, dt, vc)


@pytest.mark.parametrize("dt", [np.dtype(np.float64), np.dtype(np.float32), np.dtype(np.float16)], ids=str)
def test_minmax_generic_nan(dt):
    """a NaN anywhere in a strided view makes both results NaN, as numpy's min and max do"""
    vc = ViewCase("nan", 3, 1000, 1001, 1)
    base = _values_for(dt, vc.span(), _rng("nan-%s" % dt))
    for pos in (0, 1001 * 2 + 999, 1500):
        y = base.copy()
        y[pos] = np.nan
        dev = DevBytes(y.view(np.uint8))
        try:
            got = _native.minmax(_native.make_view(dev.origin, _native.dtype_tag(dt), vc.rs, vc.cs), vc.n_rows, vc.n_cols, _native.MEM_DEVICE)
        finally:
            dev.close()
        assert math.isnan(got[0]) and math.isnan(got[1]), (pos, got)
    PREDICTED.add("xhist::minmax_kernel")


def test_minmax_host_staged():
    """MEM_HOST: a contiguous array and one with padded rows are staged densely (the flat kernel), rows that are the contiguous
    direction keep their layout (the generic kernel)"""
    rng = _rng("host")
    a = vx.grid(rng, (7, 1000), np.float64)
    a[3, 500], a[6, 999] = -77.0, 99.0
    for arr, rs, cs, nr, nc in ((a, 1000, 1, 7, 1000), (a[:, :900], 1000, 1, 7, 900), (a[:5].T, 1, 1000, 1000, 5), (a[0], 1000, 1, 1, 1000)):
        view = _native.make_view(arr.ctypes.data, _native.F64, rs, cs)
        got = _native.minmax(view, nr, nc, _native.MEM_HOST)
        assert got == _np_minmax(arr), (arr.shape, got)
    i = rng.integers(-2 ** 62, 2 ** 62, (5, 300)).astype(np.int64)
    i[2, 7], i[4, 299] = -(2 ** 63), 2 ** 63 - 1
    got = _native.minmax(_native.make_view(i.ctypes.data, _native.I64, 300, 1), 5, 300, _native.MEM_HOST)
    assert got == _np_minmax(i)
    b = a.copy()
    b[2, 2] = np.nan
    got = _native.minmax(_native.make_view(b.ctypes.data, _native.F64, 1000, 1), 7, 1000, _native.MEM_HOST)
    assert math.isnan(got[0]) and math.isnan(got[1])
    PREDICTED.update(("xhist::minmax_flat<double>", "xhist::minmax_kernel"))


# ---------------------------------------------------------------------------------------------------------------------
# moments
# ---------------------------------------------------------------------------------------------------------------------
def _grid_values(dt, n, rng):
    """values on the exactly summable grid of tests/values_exact.py that the dtype holds"""
    dt = np.dtype(dt)
    if dt == np.bool_:
        return rng.integers(0, 2, n).astype(dt)
    if dt == np.float16:  # 11 significant bits: k * 2^-10 with |k| < 2^10
        return (rng.integers(-1023, 1024, n) * vx.SCALE).astype(dt)
    if dt.kind == "f":
        return vx.grid(rng, n, dt)
    ii = np.iinfo(dt)
    return rng.integers(max(ii.min, -(vx.K_MAX - 1)), min(ii.max, vx.K_MAX - 1), n, endpoint=True).astype(dt)


def _moments_m2_extra(kept, mean):
    """What xhist_moments' M2 may differ by from values_exact's M2* = Q - D^2 / n beyond that module's bound B.

    xhist_moments returns Q^ = the float64 sum of q_i = fl(d_i^2), d_i = fl(v_i - mean), and leaves the correction D^2 / n out
    (D = sum d_i).  |Q^ - M2*| <= |Q^ - Q| + D^2 / n, and B covers |Q^ - Q| <= g(n) Q.  The size of D follows from the rounding of
    the mean alone: the sum S of the values is exact on the grid, mean = fl(S / n) = (S / n) (1 + e0) with |e0| <= u, so
    sum (v_i - mean) = S - n mean = -n (S / n) e0, at most n u |S / n| <= n u |mean| / (1 - u) in magnitude; and every
    d_i = (v_i - mean) (1 + e_i), |e_i| <= u, adds at most u |v_i - mean| <= u |d_i| / (1 - u).  Hence
        |D| <= (n |mean| + A) u / (1 - u),   A = sum |d_i|,
    and the term left out is at most ((n |mean| + A) u / (1 - u))^2 / n."""
    n = len(kept)
    a = math.fsum(np.abs(kept - mean))
    d_max = (n * abs(mean) + a) * vx.U / (1.0 - vx.U) * (1.0 + 4.0 * vx.U)  # (and the host's own roundings of this line)
    return d_max * d_max / n


def _expected_moments(logical, lo, hi):
    """(count, min, max, mean, kept values as float64) of the elements inside [lo, hi]; NaN counts only without a range"""
    v = np.asarray(logical).astype(np.float64).reshape(-1)
    if lo is not None:
        with np.errstate(invalid="ignore"):
            v = v[(v >= lo) & (v <= hi)]
    n = v.size
    if n == 0:
        return 0, np.inf, -np.inf, np.nan, v
    if np.isnan(v).any():
        return n, np.nan, np.nan, np.nan, v
    with np.errstate(invalid="ignore"):
        s = float(np.sum(v)) if not np.isfinite(v).all() else math.fsum(v)
        return n, float(v.min()), float(v.max()), s / n, v


def _bits(x):
    return np.float64(x).view(np.uint64)


def check_moments(dt, vc, base, lo=None, hi=None, want_m2=True):
    """xhist_moments of the view `vc` of `base` against the exact expectation: count, min, max and mean bit for bit, M2 as
    values_exact holds mean_var's with everything in one bin"""
    dt = np.dtype(dt)
    logical = base[vc.index()]
    dev = DevBytes(np.concatenate([np.zeros(vc.mis * dt.itemsize, np.uint8), base.view(np.uint8)]))
    try:
        view = _native.make_view(dev.origin + vc.mis * dt.itemsize, _native.dtype_tag(dt), vc.rs, vc.cs, vc.ir, vc.os)
        got = _native.moments(view, vc.n_rows, vc.n_cols, lo, hi, want_m2)
    finally:
        dev.close()
    n, mn, mx, mean, kept = _expected_moments(logical, lo, hi)
    assert got[0] == n, (got, n)
    for g, w, what in ((got[1], mn, "min"), (got[2], mx, "max"), (got[3], mean, "mean")):
        assert (math.isnan(g) and math.isnan(w)) or (g == w and _bits(g) == _bits(w) or (g == w == 0.0 and what != "mean")), (what, g, w)
    if not want_m2 or n == 0 or math.isnan(mean):
        assert math.isnan(got[4]), got
    elif np.isfinite(kept).all():
        cnt, mean_x, m2, bound, exact = vx.expected(np.zeros(n, np.int64), kept, 1)
        assert cnt[0] == n and _bits(mean_x[0]) == _bits(mean)
        vx.assert_m2([got[4]], m2, bound + _moments_m2_extra(kept, mean), exact, what="%s %s" % (dt, vc))
    PREDICTED.add("xhist::moments_kernel")
    return got


@pytest.mark.parametrize("n", [1, 255, 256, 512, 256 * 1024 - 1, 256 * 1024 + 1, 2_000_003])
def test_moments_sizes(n):
    """one value; fewer than a workgroup; power-of-two counts (M2 bit for bit); either side of one element per thread of the
    grid; eight elements per thread and a tail"""
    base = vx.grid(_rng("moments-%d" % n), n, np.float64)
    check_moments(np.float64, ViewCase("flat", 1, n, n, 1), base)


@pytest.mark.parametrize("dt", ALL_DTYPES, ids=str)
def test_moments_dtypes(dt):
    base = _grid_values(dt, 1000, _rng("moments-%s" % dt))
    check_moments(dt, ViewCase("flat", 1, 1000, 1000, 1), base)
    check_moments(dt, ViewCase("flat", 1, 512, 512, 1), base[:512])  # a power-of-two count: M2 bit for bit


@pytest.mark.parametrize("vc", VIEW_CASES, ids=repr)
@pytest.mark.parametrize("dt", [np.dtype(np.float64), np.dtype(np.float32), np.dtype(np.int16)], ids=str)
def test_moments_views(dt, vc):
    """column strides, grouped rows, n_rows > 1, stride-0 rows and columns, with and without a range"""
    base = _grid_values(dt, vc.span(), _rng("moments-view-%s-%s" % (dt, vc.name)))
    check_moments(dt, vc, base)
    check_moments(dt, vc, base, lo=-1.5, hi=2.25)


def test_moments_range_bounds_are_inclusive():
    """elements exactly on lo and on hi are kept, their nextafter neighbours are dropped"""
    lo, hi = -1.25, 2.5
    inside = vx.grid(_rng("range"), 5000, np.float64)
    inside = inside[(inside > lo) & (inside < hi)][:2000]
    edge = np.array([lo, hi, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf), np.nextafter(lo, np.inf), np.nextafter(hi, -np.inf)])
    for take in ([0], [1], [0, 1], [2], [3], [2, 3], [0, 1, 2, 3], [0, 0, 1, 1, 1]):
        base = np.concatenate([inside[:1000], edge[take], inside[1000:]])
        got = check_moments(np.float64, ViewCase("flat", 1, base.size, base.size, 1), base, lo=lo, hi=hi)
        assert got[0] == 2000 + sum(1 for t in take if t < 2)
    # the inner neighbours are kept (off the grid: count, min and max only)
    base = np.concatenate([inside, edge[[4, 5]]])
    dev = DevBytes(base.view(np.uint8))
    try:
        got = _native.moments(_native.make_view(dev.origin, _native.F64, base.size, 1), 1, base.size, lo, hi, False)
    finally:
        dev.close()
    assert got[:3] == (2002, edge[4], edge[5]), got


def test_moments_nan_and_infinities():
    x = vx.grid(_rng("nan"), 3000, np.float64)
    flat = lambda a: ViewCase("flat", 1, a.size, a.size, 1)  # noqa: E731
    y = x.copy()
    y[[0, 1500, 2999]] = np.nan
    got = check_moments(np.float64, flat(y), y, lo=-2.0, hi=2.0)  # dropped under a range
    assert got[0] == int(np.sum((np.delete(x, [0, 1500, 2999]) >= -2.0) & (np.delete(x, [0, 1500, 2999]) <= 2.0)))
    got = check_moments(np.float64, flat(y), y)  # flagged without one: min, max, mean and M2 are NaN, every element counts
    assert got[0] == 3000 and all(math.isnan(g) for g in got[1:])
    for inf in (np.inf, -np.inf):
        z = x.copy()
        z[[7, 2998]] = inf
        got = check_moments(np.float64, flat(z), z, want_m2=False)  # without a range: counted, the extreme and the mean
        assert got[0] == 3000 and got[3] == inf and (got[1] if inf < 0 else got[2]) == inf
        got = check_moments(np.float64, flat(z), z, lo=-4.0, hi=4.0)  # a finite range drops them
        assert got[0] == 2998
        got = check_moments(np.float64, flat(z), z, lo=-np.inf, hi=np.inf, want_m2=False)  # an infinite bound is inclusive too
        assert got[0] == 3000
    z = x.copy()
    z[3], z[4] = np.inf, -np.inf
    got = check_moments(np.float64, flat(z), z, want_m2=False)
    assert got[0] == 3000 and got[1] == -np.inf and got[2] == np.inf and math.isnan(got[3])
    got = check_moments(np.float64, flat(x), x, lo=100.0, hi=200.0)  # a range that keeps nothing
    assert got[0] == 0 and got[1] == np.inf and got[2] == -np.inf and math.isnan(got[3]) and math.isnan(got[4])
    got = check_moments(np.float64, flat(x), x, want_m2=False)  # want_m2 off
    assert math.isnan(got[4])


def test_moments_float32_against_bounds_rounded_to_float32():
    """float32 data meets the bounds as core._range_cut rounds them: float32(0.7) < 0.7 is kept by range=(0.7, 1.0), and
    dropped by a float64 bound"""
    from xhistogram_amd import core

    f7 = np.float32(0.7)
    assert float(f7) < 0.7
    x = np.array([f7, np.nextafter(f7, np.float32(0)), 0.75, 0.875, 1.0, np.nextafter(np.float32(1), np.float32(2)), 0.5], np.float32)
    lo, hi = core._range_cut((0.7, 1.0), np.dtype(np.float32))
    assert lo == float(f7) and hi == 1.0
    dev = DevBytes(x.view(np.uint8))
    try:
        view = _native.make_view(dev.origin, _native.F32, x.size, 1)
        got = _native.moments(view, 1, x.size, lo, hi, False)
        want = x[(x >= f7) & (x <= np.float32(1.0))].astype(np.float64)
        assert got[:3] == (4, float(f7), 1.0) and got[3] == math.fsum(want) / 4, got
        lo64, hi64 = core._range_cut((np.float64(0.7), 1.0), np.dtype(np.float32))
        assert lo64 == 0.7
        got = _native.moments(view, 1, x.size, lo64, hi64, False)
        assert got[:3] == (3, 0.75, 1.0), got
    finally:
        dev.close()
    PREDICTED.add("xhist::moments_kernel")


# ---------------------------------------------------------------------------------------------------------------------
# buffer_add
# ---------------------------------------------------------------------------------------------------------------------
class _At:
    """what DeviceBuffer.add needs of a buffer: a device and a pointer — here a pointer into the middle of an allocation"""

    def __init__(self, ptr):
        self.device, self.ptr = 0, ptr


@pytest.mark.parametrize("count", [0, 1, 255, 256, 257, 4096 * 256 + 5])
@pytest.mark.parametrize("tag", [_native.I64, _native.F64], ids=["int64", "float64"])
def test_buffer_add(tag, count):
    """dst[i] += src[i]: int64 wraps (np.add on uint64), float64 as np.add with NaN, infinities, -0.0 and subnormals among the
    values; guard bands on both sides of dst"""
    rng = _rng("add-%d-%d" % (tag, count))
    if tag == _native.I64:
        a = rng.integers(0, 2 ** 64, count, dtype=np.uint64, endpoint=False)
        b = rng.integers(0, 2 ** 64, count, dtype=np.uint64, endpoint=False)
        if count:
            a[0], b[0] = 2 ** 63 - 1, 1  # int64 max + 1 wraps to int64 min
            a[-1], b[-1] = 2 ** 63, 2 ** 63  # int64 min + int64 min wraps to 0
        want = np.add(a, b)
    else:
        sp = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, 1.0])
        a = rng.standard_normal(count)
        b = rng.standard_normal(count)
        k = min(count, 200)
        a[:k] = rng.choice(sp, k)
        b[:k] = rng.choice(sp, k)
        if count > 2:
            a[:3], b[:3] = (np.inf, -0.0, -0.0), (-np.inf, -0.0, 0.0)
        with np.errstate(invalid="ignore", over="ignore"):
            want = np.add(a, b)
    host = np.full(2 * GUARD + 8 * count, PATTERN, np.uint8)
    host[GUARD:GUARD + 8 * count] = a.view(np.uint8)
    dst, src = DevBytes(host), DevBytes(b.view(np.uint8) if count else np.zeros(8, np.uint8))
    try:
        _native.DeviceBuffer.add(_At(dst.origin + GUARD), _At(src.origin), count, tag)
        got = dst.read()
    finally:
        dst.close()
        src.close()
    assert np.all(got[:GUARD] == PATTERN) and np.all(got[GUARD + 8 * count:] == PATTERN), "bytes outside dst were written"
    body = got[GUARD:GUARD + 8 * count]
    if tag == _native.I64:
        assert np.array_equal(body.view(np.uint64), want)
    else:
        g = body.view(np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.array_equal(g[ok].view(np.uint64), want[ok].view(np.uint64))
    if count:
        PREDICTED.add("buffer_add_kernel")


# ---------------------------------------------------------------------------------------------------------------------
# the staging kernels reached only through Plan.execute
# ---------------------------------------------------------------------------------------------------------------------
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def xh():
    from xhistogram_amd import core

    return core


def _plan_of(core, samples, edges):
    dts = [core._np_dtype_of(s) for s in samples]
    cmp_domain, _, _ = core._compare_domain(dts, edges)
    return core._get_plan(edges, cmp_domain, 0)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["float32", "float64"])
def test_transpose_2d(xh, dt):
    """weighted rows of 63 | 64 | 65 columns, 63 | 64 | 65 of them, dense and as slices of wider rows: hist_lanes on scratch that
    transpose_2d filled (64 x 64 tiles), samples and weights alike"""
    rng = _rng("transpose-%s" % np.dtype(dt))
    edges = np.linspace(-4, 4, 41)
    for rows, cols, wide in itertools.product((63, 64, 65), (63, 64, 65), (False, True)):
        x = rng.standard_normal((rows, cols + (5 if wide else 0))).astype(dt)
        w = rng.integers(0, 8, x.shape).astype(dt)  # small integers: float sums exact in any order
        xt, wt = torch.as_tensor(x).cuda(), torch.as_tensor(w).cuda()
        if wide:
            x, w, xt, wt = x[:, :cols], w[:, :cols], xt[:, :cols], wt[:, :cols]
        plan = _plan_of(xh, [xt], [edges])
        plan.set_param("lanes", 1)
        plan.set_param("flat_rows", -1)
        try:
            got, _ = xh.histogram(xt, bins=edges, axis=1, weights=wt)
            desc = plan.describe()
        finally:
            plan.set_param("lanes", 0)
            plan.set_param("flat_rows", 0)
        assert "family=lanes" in desc and "transpose=1" in desc, desc
        want, _ = onp.histogram(x, bins=edges, axis=1, weights=w.astype(np.float64))
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=desc)
    PREDICTED.add("xhist::transpose_2d<%s>" % ("float" if dt == np.float32 else "double"))


def _gather_prediction(es, n_rows, col_stride, ptr, n_cols, n_bins):
    """the gather execute_table_columns launches for one (n, K) table column view, None where it declines"""
    if n_rows > 64 or n_cols < 4096 or not (col_stride >= n_rows and col_stride > 1) or ptr % es:
        return None
    if n_rows <= 4 and es == 8 and n_bins * 4 <= 96 * 1024:
        return None
    tile_lds = 256 * (n_rows + 1) * es
    if col_stride == n_rows and (n_rows * es) % 16 == 0 and ptr % 16 == 0 and es >= 4 and tile_lds <= 64 * 1024:
        return "xhist::gather_rows_tiled<%s>" % C_UNSIGNED[es]
    return "xhist::gather_rows<%s>" % C_UNSIGNED[es]


N_GATHER_BINS = 20_000  # more than the row-per-lane kernels hold in LDS: those take such views without a gather
GATHER_CASES = [
    # dtype, K of the table, first column, columns taken, n, elements between a 16-byte boundary and the table:
    # the view [n, k] of an (n, K) table histogrammed over axis 0
    ("u8-whole-16", np.uint8, 16, 0, 16, 4097, 0),
    ("u8-slice-3", np.uint8, 5, 1, 3, 4096, 0),
    ("i16-whole-8", np.int16, 8, 0, 8, 4097, 0),
    ("i16-slice-5", np.int16, 8, 2, 5, 4096, 0),
    ("f32-tiled-4", np.float32, 4, 0, 4, 4097, 0),
    ("f32-tiled-8", np.float32, 8, 0, 8, 4096, 0),
    ("f32-rows-not-16-bytes", np.float32, 6, 0, 6, 4097, 0),
    ("f32-pointer-off-16", np.float32, 8, 0, 8, 4097, 1),
    ("f32-slice-of-wider", np.float32, 8, 0, 4, 4096, 0),
    ("f32-below-4096", np.float32, 4, 0, 4, 4095, 0),
    ("f64-tiled-6", np.float64, 6, 0, 6, 4097, 0),
    ("f64-tiled-8", np.float64, 8, 0, 8, 4096, 0),
    ("f64-rows-not-16-bytes", np.float64, 5, 0, 5, 4097, 0),
    ("f64-pointer-off-16", np.float64, 6, 0, 6, 4096, 1),
    ("f64-slice-of-wider", np.float64, 8, 1, 6, 4096, 0),
    ("f64-below-4096", np.float64, 6, 0, 6, 4095, 0),
]


_GATHER_PLANS = {}


def _gather_plan(dt):
    """(plan, edges) for tables of a dtype: float64-domain edges over the values' range, one plan per range"""
    lo, hi = (-4, 4) if dt.kind == "f" else ((-160, 160) if dt != np.uint8 else (0, 255))
    if (lo, hi) not in _GATHER_PLANS:
        e = np.linspace(lo, hi, N_GATHER_BINS + 1)
        _GATHER_PLANS[(lo, hi)] = (_native.Plan([e], _native.CMP_F64, 0), e)
    return _GATHER_PLANS[(lo, hi)]


def run_gather_case(case, check_data=True):
    """Plan.execute on the view [k rows, n columns] of an (n, K) table (row stride 1, column stride K); returns the predicted
    gather kernel (None: no gather) and the plan's description of the call"""
    name, dt, K, c0, k, n, off = case
    dt = np.dtype(dt)
    it = dt.itemsize
    rng = _rng("gather-" + name)
    t = (rng.standard_normal((n, K)) * (1 if dt.kind == "f" else 40)).astype(dt) if dt != np.uint8 else rng.integers(0, 256, (n, K)).astype(dt)
    plan, e = _gather_plan(dt)
    dev = DevBytes(np.concatenate([np.zeros(off * it, np.uint8), t.reshape(-1).view(np.uint8)]))
    out = DevBytes(np.full(k * N_GATHER_BINS * 8, PATTERN, np.uint8))  # (not zeroed: the call has to)
    try:
        ptr = dev.origin + (off + c0) * it
        pred = _gather_prediction(it, k, K, ptr, n, N_GATHER_BINS)
        built_for = {"tiled": "gather_rows_tiled", "below": None}.get(name.split("-")[1], "gather_rows<")
        assert (pred is None) if built_for is None else (built_for in pred), (name, pred)
        plan.execute([_native.make_view(ptr, _native.dtype_tag(dt), 1, K)], None, k, n, out.origin, False, _native.MEM_DEVICE)
        got = out.read().view(np.int64).reshape(k, N_GATHER_BINS)
        desc = plan.describe()
    finally:
        dev.close()
        out.close()
    if check_data:
        want, _ = onp.histogram(np.ascontiguousarray(t[:, c0:c0 + k]), bins=e, axis=0)
        np.testing.assert_array_equal(got, want, err_msg=desc)
    if pred:
        PREDICTED.add(pred)
    return pred, desc


@pytest.mark.parametrize("case", GATHER_CASES, ids=[c[0] for c in GATHER_CASES])
def test_gather_rows(case):
    """the columns of an (n, K) table over its leading axis, 20000 bins: gathered into dense rows (tiled through LDS where the
    view is a whole table of 16-byte rows behind a 16-byte pointer), then histogrammed as dense rows.  describe() reports the
    histogram kernel's launch, which sees dense rows after a gather (test_helper_variants_as_launched holds the gather itself
    against the prediction)"""
    pred, desc = run_gather_case(case)
    # dense rows of floats stream through the vector kernels with the histogram in LDS; without the gather the strided view
    # is left to the generic family (integer tables go there either way)
    if np.dtype(case[1]).kind == "f":
        assert ("family=fast hist=lds" in desc) == (pred is not None), (pred, desc)
        assert ("family=generic" in desc) == (pred is None), (pred, desc)


def test_table_builders_zeroing_and_partition_prefix(xh):
    """what every plan and most executes launch besides their histogram kernel: the bucket-table builders of both float
    domains with 4-byte and 2-byte entries, of the int64 domain, the packed-entry builder, the output zeroing, and the prefix
    sums of the three-pass partitioned route — held to the oracle through the histograms that depend on them"""
    rng = _rng("builders")
    n = 40_013
    x = rng.standard_normal(n)
    # a fresh float64-domain plan; jittered steps: not arithmetic (the tables decide every bin), at most one edge per bucket of
    # the packed entries' grid (they are built only where three edges per bucket suffice)
    e = np.linspace(-4, 4, 301) + rng.uniform(-0.2, 0.2, 301) * (8 / 300)
    for a in (x, x.astype(np.float32)):
        at = torch.as_tensor(a).cuda()
        got, _ = xh.histogram(at, bins=e)
        np.testing.assert_array_equal(got.cpu().numpy(), onp.histogram(a, bins=e)[0])
        plan = _plan_of(xh, [at], [e])
        plan.set_param("pack", 1)  # the same through the packed entries (build_pack_tables: both sample widths)
        try:
            got, _ = xh.histogram(at, bins=e)
            desc = plan.describe()
        finally:
            plan.set_param("pack", 0)
        assert any("scan=%d " % k in desc for k in (6, 7, 8)), desc
        np.testing.assert_array_equal(got.cpu().numpy(), onp.histogram(a, bins=e)[0], err_msg=desc)
    i = rng.integers(-2 ** 62, 2 ** 62, n)
    ei = np.sort(rng.integers(-2 ** 62, 2 ** 62, 301))  # int64 edges beyond 2^53: the int64 compare domain
    it = torch.as_tensor(i).cuda()
    plan = _plan_of(xh, [it], [ei])
    assert plan.cmp == _native.CMP_I64
    got, _ = xh.histogram(it, bins=ei)
    np.testing.assert_array_equal(got.cpu().numpy(), onp.histogram(i, bins=ei)[0])
    # three passes over partitions of a histogram beyond LDS: part_count, part_prefix, part_scatter, part_accumulate
    y = rng.standard_normal(n)
    w = rng.integers(0, 8, n).astype(np.float64)
    e2 = [np.linspace(-4, 4, 1025)] * 2
    xt, yt, wt = (torch.as_tensor(a).cuda() for a in (x, y, w))
    plan = _plan_of(xh, [xt, yt], e2)
    plan.set_param("partition", 1)
    plan.set_param("fused", -1)
    try:
        got, _ = xh.histogram(xt, yt, bins=e2, weights=wt)
        desc = plan.describe()
    finally:
        plan.set_param("fused", 0)
        plan.set_param("partition", 0)
    assert "hist=partitioned" in desc and "route=fused" not in desc, desc
    np.testing.assert_array_equal(got.cpu().numpy(), onp.histogram(x, y, bins=e2, weights=w)[0], err_msg=desc)
    PREDICTED.update(["xhist::build_tables<%s>" % a for a in ("0, false", "0, true", "1, false", "2, false", "2, true")])
    PREDICTED.update(["xhist::build_pack_tables", "xhist::zero_words", "xhist::part_prefix"])


# ---------------------------------------------------------------------------------------------------------------------
# the variants as the library launched them, and the census of this module
# ---------------------------------------------------------------------------------------------------------------------
def _launched_since(log, pos):
    kc = _kernel_census()
    with open(log) as f:
        f.seek(pos)
        raw = [line.strip() for line in f if line.strip()]
        pos = f.tell()
    return [kc.norm(n) for n in kc.demangle(raw)], pos


def _child_variants(out_path):
    """(in a fresh process with XHIST_AMD_KERNEL_LOG_ALL=1) every copy, min / max and gather case once more, with the
    kernels the log shows for each"""
    log = os.environ["XHIST_AMD_KERNEL_LOG"]
    _native.load()
    pos = os.path.getsize(log) if os.path.exists(log) else 0
    out = {}
    for case in COPY_CASES:
        pred = run_copy_case(case, check_data=False)
        names, pos = _launched_since(log, pos)
        out["copy:" + case.name] = [copy_instantiation(pred) if pred else None, names]
    for dt, name, n, mis in FLAT_CASES:
        kernel = run_minmax_flat_case(dt, n, mis, check_data=False)
        names, pos = _launched_since(log, pos)
        out["flat:%s-%s-%d" % (dt, name, mis)] = [kernel, names]
    for dt in ALL_DTYPES:
        for vc in VIEW_CASES:
            kernel = run_minmax_view_case(dt, vc, check_data=False)
            names, pos = _launched_since(log, pos)
            out["view:%s-%s" % (dt, vc.name)] = [kernel, names]
    for case in GATHER_CASES:
        pred, _ = run_gather_case(case, check_data=False)
        names, pos = _launched_since(log, pos)
        out["gather:" + case[0]] = [pred, [n for n in names if "gather_rows" in n]]
    with open(out_path, "w") as f:
        json.dump(out, f)


def test_helper_variants_as_launched(tmp_path):
    """the library's own choice against the restatement: a fresh process logs every launch (the session's log names a kernel
    once), runs each copy, min / max and gather case, and must have launched exactly the predicted kernel for each"""
    env = dict(os.environ)
    env["XHIST_AMD_KERNEL_LOG"] = str(tmp_path / "launches.log")
    env["XHIST_AMD_KERNEL_LOG_ALL"] = "1"
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + [p for p in env.get("PYTHONPATH", "").split(os.pathsep) if p])
    out = tmp_path / "variants.json"
    code = "import test_gpu_helpers as t; t._child_variants(%r)" % str(out)
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.load(open(out))
    assert len(res) == len(COPY_CASES) + len(FLAT_CASES) + len(ALL_DTYPES) * len(VIEW_CASES) + len(GATHER_CASES)
    wrong = {k: v for k, (pred, names) in res.items() for v in [(pred, names)] if names != ([pred] if pred else [])}
    assert not wrong, "launched != predicted for %d cases: %s" % (len(wrong), dict(list(wrong.items())[:8]))


# the templates the library launches directly, without a dispatch table (debug_hold_kernel is test support and stays outside)
HELPER_TEMPLATES = ("zero_words", "build_tables", "build_pack_tables", "gather_rows", "gather_rows_tiled", "minmax_flat", "minmax_kernel",
                    "moments_kernel", "part_prefix", "transpose_2d", "buffer_add_kernel", "copy_nd_kernel", "copy_nd_transpose")


def test_zz_every_helper_instantiation_was_predicted_and_launched(request):
    """closing test: the instantiations the cases above predicted (and compared) are exactly the helper instantiations the
    shared object carries, and each is in the kernel log of this session"""
    log = os.environ.get("XHIST_AMD_KERNEL_LOG")
    if not log or not os.path.exists(log):
        pytest.skip("XHIST_AMD_KERNEL_LOG is not set for this run (tests/conftest.py sets it for `-m gpu` sessions)")
    mine = {n for n, f in globals().items() if n.startswith("test_") and callable(f)} - {request.node.name}
    if not mine <= RAN:
        pytest.skip("only part of this module ran: %s did not" % sorted(mine - RAN))
    kc = _kernel_census()
    have = kc.in_library(os.path.join(ROOT, "xhistogram_amd", "libxhist_amd.so"))
    helpers = {n for n in have if kc.template_of(n).split("::")[-1].split(" ")[0] in HELPER_TEMPLATES}
    assert PREDICTED == helpers, (sorted(PREDICTED - helpers), sorted(helpers - PREDICTED))
    raw = {line.strip() for line in open(log) if line.strip() and line.strip() != "?"}
    used = {kc.norm(n) for n in kc.demangle(sorted(raw))}
    assert helpers <= used, sorted(helpers - used)
