"""The Python front of the seven functions that return something per sample or per row (bin_index, histogram_lookup,
histogram_anomaly, bin_order, bin_sort, bin_rank, bin_unique with and without its inverse), held to what it must keep whatever
it is built of: the same bits from numpy, DeviceArray and torch inputs, for every way of naming the reduced axes; the bits of
the oracles the project already has (tests/map_oracle.py, bin_order_oracle.py, bin_sort_oracle.py, bin_rank_oracle.py,
bin_unique_oracle.py); what the docstrings promise where an extent is 0 or the plan has no bins; and the layout of the numpy
outputs.

The block is small on purpose, (3, 4, 5) samples in 4 bins: what is checked here is the front (which axes are rows, how the
outputs are allocated, carved and moved back), not the kernels, which the files of each function hold to their case tables.

A numpy output is writable and C-contiguous.  The one exception is what _sample_shape documents: a per-sample output over
reduced axes that are not the trailing ones is the C-contiguous [kept axes, reduced axes] block with its axes moved back where
the inputs have them, so it is that block, with the reduced axes moved last again, that is held to C-contiguity."""
import functools

import numpy as np
import pytest

import bin_order_oracle as bo
import bin_rank_oracle as ro
import bin_sort_oracle as so
import bin_unique_oracle as uo
import map_oracle as mo
from test_gpu_parity import xh  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SHAPE = (3, 4, 5)
EDGES = np.linspace(0.0, 1.0, 5)
N_BINS = 4
SIX = np.array([-2.0, -0.5, 0.0, 0.25, 1.0, 3.0])  # (on the exactly summable grid of tests/values_exact.py)
AXES = [None, 2, 0, (0, 2), (2, 0), (1,)]
FUNCS = ["bin_index", "histogram_lookup", "histogram_anomaly", "bin_order", "bin_sort", "bin_rank", "bin_unique", "bin_unique_inverse"]
PER_SAMPLE = {"bin_index": (0,), "histogram_lookup": (0,), "histogram_anomaly": (0,), "bin_rank": (0,), "bin_unique_inverse": (3,)}
BACKENDS = ("numpy", "device", "torch")


@functools.lru_cache(maxsize=None)
def _block():
    rng = np.random.default_rng(2026)
    x = rng.uniform(0.0, 1.0, SHAPE)
    x[0, 1, 2] = np.nan
    x[2, 3, 4] = 1.5  # (out of range)
    v = SIX[rng.integers(0, 6, SHAPE)]
    for a in (x, v):
        a.setflags(write=False)
    return x, v


def _put(backend):
    from xhistogram_amd.devicearray import DeviceArray

    return {"torch": lambda a: torch.as_tensor(np.array(a)).cuda(), "numpy": lambda a: a,
            "device": lambda a: DeviceArray.from_numpy(np.ascontiguousarray(a), 0)}[backend]


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else t


def _red(axis, ndim):
    return list(range(ndim)) if axis is None else sorted(int(a) % ndim for a in np.atleast_1d(axis))


def _table(shape, axis, n_bins=N_BINS):
    """a table in the shape histogram gives: kept axes, then the bins"""
    lead = tuple(s for i, s in enumerate(shape) if i not in _red(axis, len(shape)))
    n = int(np.prod(lead + (n_bins,), dtype=np.int64))
    return (np.arange(n, dtype=np.float64) * 0.5 - 3.0).reshape(lead + (n_bins,))


def _call(core, fn, backend, x, v, edges, axis, size=None):
    """the outputs of one public call (without the edges), as the call returns them"""
    put = _put(backend)
    xd = put(x)
    bins = [edges]
    if fn == "bin_index":
        return core.bin_index(xd, bins=bins)[:-1]
    if fn == "histogram_lookup":
        return core.histogram_lookup(xd, table=_table(x.shape, axis, len(edges) - 1), bins=bins, axis=axis)[:-1]
    if fn == "bin_order":
        return core.bin_order(xd, bins=bins, axis=axis)[:-1]
    vd = put(v)
    if fn == "histogram_anomaly":
        return core.histogram_anomaly(xd, values=vd, bins=bins, axis=axis)[:-1]
    if fn == "bin_sort":
        return core.bin_sort(xd, values=vd, bins=bins, axis=axis)[:-1]
    if fn == "bin_rank":
        return core.bin_rank(xd, values=vd, bins=bins, axis=axis)[:-1]
    return core.bin_unique(xd, values=vd, bins=bins, axis=axis, size=size, return_inverse=fn == "bin_unique_inverse")[:-1]


def _moved_back(flat, shape, axis):
    """[kept axes..., c] of the oracles' rows -> the sample shape"""
    ndim = len(shape)
    red = _red(axis, ndim)
    kept = [i for i in range(ndim) if i not in red]
    full = np.asarray(flat).reshape([shape[i] for i in kept] + [shape[i] for i in red])
    return np.moveaxis(full, range(len(kept), ndim), red) if kept else full


@functools.lru_cache(maxsize=None)
def _want(fn, axis, size=None):
    """the oracle's outputs for the block of _block(), computed once per (function, axis)"""
    x, v = _block()
    idx = mo.index([x], [EDGES])
    if fn == "bin_index":
        return (idx,)
    if fn == "histogram_lookup":
        return (mo.lookup([x], [EDGES], _table(SHAPE, axis), axis),)
    if fn == "histogram_anomaly":
        return (mo.anomaly([x], [EDGES], v, mo.exact_mean([x], [EDGES], v, axis), None, axis),)
    rows, v_rows = bo.rows_of(idx, axis), bo.rows_of(v, axis)
    if fn == "bin_order":
        return bo.order_offsets(rows, N_BINS)
    if fn == "bin_sort":
        return so.order_offsets(rows, v_rows, N_BINS)
    if fn == "bin_rank":
        return (_moved_back(ro.rank_rows(rows, v_rows, N_BINS), SHAPE, axis),)
    uniques, counts, offsets, inverse = uo.unique_rows(rows, v_rows, N_BINS, size)
    return (uniques, counts, offsets) + ((_moved_back(inverse, SHAPE, axis),) if fn == "bin_unique_inverse" else ())


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.float64, np.int64), a.dtype
    return a.view(np.int64)


def _assert_same_bits(got, ref, what):
    assert len(got) == len(ref), what
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape and g.dtype == r.dtype, (what, i, g.shape, r.shape, g.dtype, r.dtype)
        assert np.array_equal(_bits(g), _bits(r)), "%s: output %d differs" % (what, i)


def _assert_numpy_layout(fn, outs, axis, what):
    """every numpy output is writable and C-contiguous (a per-sample output: before its reduced axes were moved back)"""
    for i, o in enumerate(outs):
        assert isinstance(o, np.ndarray) and o.flags.writeable, (what, i)
        if i in PER_SAMPLE.get(fn, ()) and fn != "bin_index":
            red = _red(axis, o.ndim)
            o = np.moveaxis(o, red, range(o.ndim - len(red), o.ndim))
        assert o.flags.c_contiguous, "%s: output %d is not C-contiguous" % (what, i)


def _assert_oracle(fn, got, want, what):
    if fn.startswith("bin_unique"):
        uo.assert_same(got, want, what)
    else:
        assert len(got) == len(want), what
        for g, w in zip(got, want):
            mo.assert_bits(g, w, what)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the three backends and the six ways of naming the axes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", FUNCS)
def test_backends_agree_and_equal_the_oracle(xh, fn):
    x, v = _block()
    by_axis = {}
    for axis in AXES:
        what = "%s axis=%s" % (fn, axis)
        outs = {b: _call(xh, fn, b, x, v, EDGES, axis) for b in BACKENDS}
        assert all(isinstance(o, torch.Tensor) and o.is_cuda for o in outs["torch"]), what
        for b in ("numpy", "device"):
            _assert_numpy_layout(fn, outs[b], axis, "%s %s in" % (what, b))
        ref = [_np(o) for o in outs["numpy"]]
        for b in ("device", "torch"):
            _assert_same_bits([_np(o) for o in outs[b]], ref, "%s: %s in against numpy in" % (what, b))
        _assert_oracle(fn, ref, _want(fn, axis), what)  # (every axis: one trailing, the others not)
        by_axis[axis] = ref
    _assert_same_bits(by_axis[(2, 0)], by_axis[(0, 2)], "%s: axis=(2, 0) against axis=(0, 2)" % fn)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the empties
# ---------------------------------------------------------------------------------------------------------------------
def _each_backend(core, fn, x, v, edges, axis, size=None):
    """the numpy images of the call's outputs, per backend, equal across the backends"""
    outs = {b: _call(core, fn, b, x, v, edges, axis, size) for b in BACKENDS}
    for b in ("numpy", "device"):
        _assert_numpy_layout(fn, outs[b], axis, "%s %s in, shape %s" % (fn, b, x.shape))
    ref = [_np(o) for o in outs["numpy"]]
    for b in ("device", "torch"):
        _assert_same_bits([_np(o) for o in outs[b]], ref, "%s shape %s: %s in against numpy in" % (fn, x.shape, b))
    return ref


@pytest.mark.parametrize("fn", FUNCS)
def test_no_rows(xh, fn):
    """(0, 5) over axis 1: empty outputs, offsets of shape (0, B + 1)"""
    x = v = np.zeros((0, 5))
    got = _each_backend(xh, fn, x, v, EDGES, 1, size=2 if fn.startswith("bin_unique") else None)
    want = {"bin_order": [(0, 5), (0, 5)], "bin_sort": [(0, 5), (0, 5)], "bin_unique": [(0, 2), (0, 2), (0, 5)],
            "bin_unique_inverse": [(0, 2), (0, 2), (0, 5), (0, 5)]}.get(fn, [(0, 5)])
    assert [g.shape for g in got] == want
    want_dt = {"bin_index": [np.int64], "histogram_lookup": [np.float64], "histogram_anomaly": [np.float64], "bin_rank": [np.float64],
               "bin_unique": [np.float64] + [np.int64] * 2, "bin_unique_inverse": [np.float64] + [np.int64] * 3}.get(fn, [np.int64] * 2)
    assert [g.dtype for g in got] == want_dt


@pytest.mark.parametrize("fn", FUNCS)
def test_no_columns(xh, fn):
    """(3, 0) over axis 1: an empty order, offsets all 0, an empty rank; bin_unique(size=2) is all padding"""
    x = v = np.zeros((3, 0))
    got = _each_backend(xh, fn, x, v, EDGES, 1, size=2 if fn.startswith("bin_unique") else None)
    if fn in ("bin_order", "bin_sort"):
        order, offsets = got
        assert order.shape == (3, 0) and order.dtype == np.int64
        assert offsets.shape == (3, N_BINS + 1) and offsets.dtype == np.int64 and not offsets.any()
    elif fn.startswith("bin_unique"):
        uniques, counts, offsets = got[:3]
        assert uniques.shape == counts.shape == (3, 2) and offsets.shape == (3, N_BINS + 1)
        assert (uniques.view(np.uint64) == uo.NAN_BITS).all() and not counts.any() and not offsets.any()
        if fn == "bin_unique_inverse":
            assert got[3].shape == (3, 0) and got[3].dtype == np.int64
    else:
        assert got[0].shape == (3, 0) and got[0].dtype == (np.int64 if fn == "bin_index" else np.float64)


@pytest.mark.parametrize("fn", FUNCS)
def test_a_plan_without_bins(xh, fn):
    """one edge: offsets == [0], bin_order's order == arange(c), the index all -1; lookup, anomaly and rank all NaN"""
    x, v = _block()
    edges = np.array([0.25])
    got = _each_backend(xh, fn, x, v, edges, 2)
    if fn == "bin_index":
        assert got[0].shape == SHAPE and got[0].dtype == np.int64 and (got[0] == -1).all()
    elif fn in ("histogram_lookup", "histogram_anomaly", "bin_rank"):
        assert got[0].shape == SHAPE and got[0].dtype == np.float64 and np.isnan(got[0]).all()
    elif fn in ("bin_order", "bin_sort"):
        order, offsets = got
        assert offsets.shape == (3, 4, 1) and not offsets.any()
        if fn == "bin_order":
            assert np.array_equal(order, np.broadcast_to(np.arange(5), SHAPE))
        else:  # (the whole row sorted by value, ties in ascending position)
            assert np.array_equal(order, np.argsort(v, axis=-1, kind="stable"))
    else:
        uniques, counts, offsets = got[:3]
        assert offsets.shape == (3, 4, 1) and not offsets.any()
        assert uniques.shape == counts.shape == SHAPE and (uniques.view(np.uint64) == uo.NAN_BITS).all() and not counts.any()
        if fn == "bin_unique_inverse":
            assert got[3].shape == SHAPE and (got[3] == -1).all()


def test_unique_of_size_0_with_an_inverse(xh):
    """size=0: nothing is kept of uniques and counts, the offsets and the inverse still tell the truth"""
    x, v = _block()
    for axis in (2, 0):
        got = _each_backend(xh, "bin_unique_inverse", x, v, EDGES, axis, size=0)
        uo.assert_same(got, _want("bin_unique_inverse", axis, 0), "size=0 axis=%d" % axis)
        assert got[0].shape[-1] == 0 and got[1].shape[-1] == 0 and got[2][..., -1].min() > 0 and (got[3] >= 0).any()
