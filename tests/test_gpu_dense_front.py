"""The front that the per-sample and grouped entry points of the C ABI share (xhist_plan_execute_map, _group, _sort, _rank and
_unique), driven through the raw C ABI: the status and xhist_last_error() of every call are read as they are.

Their outputs are dense [n_rows, n_cols] blocks and CSR blocks, not [n_rows, n_bins] planes, so a plan without bins (one edge) and a
call without columns still have elements to write, and only a call without rows has none.  Every call writes into the middle of one
DeviceBuffer filled with a sentinel, lead | block | gap | block | ... | tail: the sentinel must be intact around the blocks and gone
from every element of them (0x5A5A... is neither 0, -1 nor a NaN), and intact everywhere after a refused call.  Expected values are
the oracles' (tests/map_oracle.py, bin_order_oracle.py, bin_sort_oracle.py, bin_rank_oracle.py, bin_unique_oracle.py), int64 by
value and float64 by value with NaN where the oracle has NaN; the fill of a plan without bins is the all-ones bit pattern.

Three rows of float64 throughout.  65 columns cross one word of 64 samples; 1515 cut a row into two chunks in the sort."""
import ctypes as C
import itertools

import numpy as np
import pytest

import bin_order_oracle as bo
import bin_rank_oracle as ro
import bin_sort_oracle as so
import bin_unique_oracle as uo
import map_oracle as mo
from test_gpu_parity import _plan_for, xh  # noqa: F401  (xh: the module fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROWS, WIDEST = 3, 1515
COLS = (0, 1, 65, WIDEST)
EDGES = {"no_bins": np.array([0.25]), "four_bins": np.linspace(-1.0, 1.0, 5)}
SENTINEL = 0x5A5A5A5A5A5A5A5A
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
GAP = 64
CASE_NO = itertools.count()

# entry point -> the prefix of the line its driver leaves in describe(), and what that line carries where nothing was binned
DESCRIBE = {
    "map_index": ("map ", "family=none"),
    "map_anomaly": ("map ", "family=none"),
    "group": ("group ", "keys=none"),
    "sort": ("sort ", "keys=none"),
    "rank": ("rank ", "| none"),
    "unique": ("unique ", "| none"),
}
ENTRIES = tuple(DESCRIBE)

# entry point -> output -> the message of a call with work to do (3 rows, 65 columns) that leaves this output NULL, as the entry
# points have always worded it.  (bin_unique's inverse may be NULL: a call without one.)
MISSING = {
    "map_index": {"out": "out is NULL"},
    "map_anomaly": {"out": "out is NULL"},
    "group": {"out_order": "out_order is NULL", "out_offsets": "out_offsets is NULL"},
    "sort": {"out_order": "out_order is NULL", "out_offsets": "out_offsets is NULL"},
    "rank": {"out": "out is NULL"},
    "unique": {"out_uniques": "out_uniques / out_counts is NULL", "out_counts": "out_uniques / out_counts is NULL",
               "out_offsets": "out_offsets is NULL"},
}

# what a case varies besides its shape: the rank's method, direction and pct, the sort's direction
RANK_OF = {0: ("average", 0, 0), 1: ("min", 0, 1), 65: ("dense", 0, 1), WIDEST: ("ordinal", 1, 0)}
DESCENDING_OF = {0: 0, 1: 1, 65: 1, WIDEST: 0}


@pytest.fixture(scope="module")
def data(xh):
    """the samples and values of every case (a case of fewer columns reads the head of every row), on the host and the device"""
    rng = np.random.default_rng(62)
    x = rng.uniform(-1.2, 1.2, (ROWS, WIDEST))
    x[rng.random(x.shape) < 0.05] = np.nan
    v = np.round(rng.standard_normal(x.shape) * 3, 0)  # (ties)
    v[rng.random(x.shape) < 0.05] = np.nan
    v[rng.random(x.shape) < 0.05] = -0.0
    centre = {key: np.arange(ROWS * (len(e) - 1), dtype=np.float64).reshape(ROWS, len(e) - 1) * 0.5 for key, e in EDGES.items()}
    dev = {"x": torch.as_tensor(x).cuda(), "v": torch.as_tensor(v).cuda()}
    dev.update({key: torch.as_tensor(np.append(c.reshape(-1), 0.0)).cuda() for key, c in centre.items()})  # (never without an element)
    torch.cuda.synchronize()
    return {"x": x, "v": v, "centre": centre, "dev": dev}


def sizes_of(name, n_rows, n_cols, nb, size=0, inverse=False):
    """the 8-byte elements of every output block of a call, in the order of the entry point's arguments"""
    if name in ("map_index", "map_anomaly", "rank"):
        return [n_rows * n_cols]
    if name in ("group", "sort"):
        return [n_rows * n_cols, n_rows * (nb + 1)]
    if name == "unique":
        return [n_rows * size, n_rows * size, n_rows * (nb + 1)] + ([n_rows * n_cols] if inverse else [])
    assert name == "mode"
    return [n_rows * nb] * 4


def invoke(native, name, plan, views, n_rows, n_cols, outs, mem=None, centre=0, method=0, descending=0, pct=0, size=0):
    """one call of the entry point through ctypes -> (status, xhist_last_error()); `outs` are device addresses, None / 0 for NULL"""
    lib = native.load()
    sv, vv = views
    head = (plan._h, (native.XhistArray * 1)(sv))
    p = [C.c_void_p(o or 0) for o in outs]
    tail = (native.MEM_DEVICE if mem is None else mem, C.c_void_p(0))
    if name == "map_index":
        rc = lib.xhist_plan_execute_map(*head, None, n_rows, n_cols, native.MAP_INDEX, C.c_void_p(0), C.c_void_p(0), p[0], *tail)
    elif name == "map_anomaly":
        rc = lib.xhist_plan_execute_map(*head, C.byref(vv), n_rows, n_cols, native.MAP_ANOMALY, C.c_void_p(centre), C.c_void_p(0), p[0], *tail)
    elif name == "group":
        rc = lib.xhist_plan_execute_group(*head, n_rows, n_cols, p[0], p[1], *tail)
    elif name == "sort":
        rc = lib.xhist_plan_execute_sort(*head, C.byref(vv), n_rows, n_cols, descending, p[0], p[1], *tail)
    elif name == "rank":
        rc = lib.xhist_plan_execute_rank(*head, C.byref(vv), n_rows, n_cols, method, descending, pct, p[0], *tail)
    elif name == "unique":
        rc = lib.xhist_plan_execute_unique(*head, C.byref(vv), n_rows, n_cols, size, p[0], p[1], p[2], p[3] if len(p) > 3 else C.c_void_p(0), *tail)
    else:
        assert name == "mode"
        rc = lib.xhist_plan_execute_mode(*head, C.byref(vv), n_rows, n_cols, p[0], p[1], p[2], p[3], *tail)
    return rc, lib.xhist_last_error().decode()


def guarded(native, sizes, call):
    """call(addresses of the blocks) with the blocks inside a DeviceBuffer of sentinels -> (what call returned, the blocks as int64,
    whether any element of the buffer changed); the sentinel around and between the blocks must be intact"""
    lead = 64 + next(CASE_NO) % 2  # (odd in every second case: the first block then starts 8 bytes off 16-byte alignment)
    starts, at = [], lead
    for n in sizes:
        starts.append(at)
        at += n + GAP
    host = np.full(at, SENTINEL, np.uint64).view(np.int64)
    guard = host[0]
    buf = native.DeviceBuffer(0, host.nbytes)
    buf.upload(host)
    torch.cuda.synchronize()
    result = call([buf.ptr + 8 * s for s in starts])
    torch.cuda.synchronize()
    buf.download(host)
    buf.close()
    inside = np.zeros(at, bool)
    for s, n in zip(starts, sizes):
        inside[s:s + n] = True
    assert (host[~inside] == guard).all(), "the guard bands were written"
    return result, [host[s:s + n].copy() for s, n in zip(starts, sizes)], bool((host != guard).any())


def views_of(native, data):
    dev = data["dev"]
    return (native.make_view(dev["x"].data_ptr(), native.F64, WIDEST, 1), native.make_view(dev["v"].data_ptr(), native.F64, WIDEST, 1))


def index_of(data, key, n_cols):
    x = data["x"][:, :n_cols]
    return mo.index([x], [EDGES[key]]) if len(EDGES[key]) > 1 else np.full(x.shape, -1, np.int64)


def assert_values(got, want, what):
    """float64 by value, NaN where the oracle has NaN"""
    np.testing.assert_array_equal(got.view(np.float64).reshape(want.shape), want, err_msg=what)


def run_case(native, xh, data, name, key, n_cols, size=0, inverse=False):
    """one call with work or without, the sentinel gone from every element of its blocks, against the oracle"""
    edges = EDGES[key]
    nb = len(edges) - 1
    plan = _plan_for(xh, [data["x"]], [edges])
    method, descending, pct = RANK_OF[n_cols] if name == "rank" else ("average", DESCENDING_OF[n_cols] if name == "sort" else 0, 0)
    what = "%s %s n_cols=%d size=%d inverse=%d" % (name, key, n_cols, size, inverse)
    (rc, err), blocks, _ = guarded(native, sizes_of(name, ROWS, n_cols, nb, size, inverse), lambda ptrs: invoke(
        native, name, plan, views_of(native, data), ROWS, n_cols, ptrs, centre=data["dev"][key].data_ptr(),
        method=native.RANK_METHODS[method], descending=descending, pct=pct, size=size))
    assert rc == native.OK, "%s: status %d, %s" % (what, rc, err)
    for b in blocks:
        assert not (b == SENTINEL).any(), "%s: %d elements were never written" % (what, (b == SENTINEL).sum())
    idx, v = index_of(data, key, n_cols), data["v"][:, :n_cols]
    if name == "map_index":
        np.testing.assert_array_equal(blocks[0].reshape(idx.shape), idx, err_msg=what)
    elif name == "map_anomaly":
        want = mo.anomaly([data["x"][:, :n_cols]], [edges], v, data["centre"][key], axis=1) if nb and n_cols else np.full(idx.shape, np.nan)
        assert_values(blocks[0], want, what)
    elif name in ("group", "sort"):
        order, offsets = so.order_offsets(idx, v, nb, bool(descending)) if name == "sort" and n_cols else bo.order_offsets(idx, nb)
        np.testing.assert_array_equal(blocks[0].reshape(idx.shape), order, err_msg=what)
        np.testing.assert_array_equal(blocks[1].reshape(ROWS, nb + 1), offsets, err_msg=what)
    elif name == "rank":
        assert_values(blocks[0], ro.rank_rows(idx, v, nb, method, bool(descending), bool(pct)), what)
    else:
        got = [blocks[0].view(np.float64).reshape(ROWS, size), blocks[1].reshape(ROWS, size), blocks[2].reshape(ROWS, nb + 1)]
        want = uo.unique_rows(idx, v, nb, size)
        uo.assert_same(got + ([blocks[3].reshape(idx.shape)] if inverse else []), want if inverse else want[:3], what)
    if nb == 0 and name in ("map_index", "map_anomaly", "rank"):
        assert (blocks[0].view(np.uint64) == ONES).all(), "%s: the fill of a plan without bins is bytes of all ones" % what
    return plan


# ---------------------------------------------------------------------------------------------------------------------
# 1. shapes: with and without columns, with and without bins
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(EDGES))
@pytest.mark.parametrize("n_cols", COLS)
@pytest.mark.parametrize("name", [n for n in ENTRIES if n != "unique"])
def test_shapes(xh, data, name, n_cols, key):
    from xhistogram_amd import _native as native

    run_case(native, xh, data, name, key, n_cols)


@pytest.mark.parametrize("key", list(EDGES))
@pytest.mark.parametrize("n_cols", COLS)
def test_shapes_of_unique(xh, data, n_cols, key):
    """size in {0, 7, n_cols}, with and without the inverse"""
    from xhistogram_amd import _native as native

    for size in sorted({0, 7, n_cols}):
        for inverse in (True, False):
            run_case(native, xh, data, "unique", key, n_cols, size, inverse)


# ---------------------------------------------------------------------------------------------------------------------
# 2. a call without rows has no output at all
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(EDGES))
@pytest.mark.parametrize("name", ENTRIES)
def test_no_rows_and_every_output_null(xh, data, name, key):
    from xhistogram_amd import _native as native

    plan = _plan_for(xh, [data["x"]], [EDGES[key]])
    before = plan.describe()
    for n_cols in (0, 65):
        rc, err = invoke(native, name, plan, views_of(native, data), 0, n_cols, [None] * 4, size=7)
        assert rc == native.OK, "%s %s n_cols=%d: status %d, %s" % (name, key, n_cols, rc, err)
    torch.cuda.synchronize()
    assert plan.describe() == before


# ---------------------------------------------------------------------------------------------------------------------
# 3. refusals: a missing output, and which of several refusals is reported
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(EDGES))
@pytest.mark.parametrize("name", ENTRIES)
def test_missing_outputs(xh, data, name, key):
    """each output NULL in turn, with work to do: XHIST_ERR_INVALID, the entry point's own message, nothing written"""
    from xhistogram_amd import _native as native

    nb = len(EDGES[key]) - 1
    plan = _plan_for(xh, [data["x"]], [EDGES[key]])
    before = plan.describe()
    for hole, (output, message) in enumerate(MISSING[name].items()):
        (rc, err), _, written = guarded(native, sizes_of(name, ROWS, 65, nb, 7, True), lambda ptrs: invoke(
            native, name, plan, views_of(native, data), ROWS, 65, [None if i == hole else p for i, p in enumerate(ptrs)],
            centre=data["dev"][key].data_ptr(), size=7))
        assert (rc, err) == (native.ERR_INVALID, message), "%s %s without %s: status %d, %s" % (name, key, output, rc, err)
        assert not written, "%s %s without %s wrote to the other outputs" % (name, key, output)
    assert plan.describe() == before


def test_a_missing_table_of_the_anomaly(xh, data):
    """the one input the maps' front speaks for: no centre table, with work to do"""
    from xhistogram_amd import _native as native

    plan = _plan_for(xh, [data["x"]], [EDGES["four_bins"]])
    (rc, err), _, written = guarded(native, [ROWS * 65], lambda ptrs: invoke(native, "map_anomaly", plan, views_of(native, data), ROWS, 65, ptrs))
    assert (rc, err) == (native.ERR_INVALID, "the table (centre) is NULL") and not written


@pytest.mark.parametrize("name", ["group", "sort", "rank", "unique", "mode"])
def test_the_limit_of_a_row_is_reported_first(xh, data, name):
    """host memory and a row of 2^31 columns (one element at stride 0) at once: the limit's message; with an unknown rank method
    on top, the method's"""
    from xhistogram_amd import _native as native

    nb = len(EDGES["four_bins"]) - 1
    plan = _plan_for(xh, [data["x"]], [EDGES["four_bins"]])
    before = plan.describe()
    wide = native.make_view(data["dev"]["x"].data_ptr(), native.F64, 0, 0)
    public = {"group": "bin_order", "sort": "bin_sort", "rank": "bin_rank", "unique": "bin_unique", "mode": "histogram_mode"}[name]
    (rc, err), _, written = guarded(native, sizes_of(name, 1, 8, nb, 7, True), lambda ptrs: invoke(
        native, name, plan, (wide, wide), 1, 1 << 31, ptrs, mem=native.MEM_HOST, size=7))
    assert rc == native.ERR_UNSUPPORTED and err.startswith(public + " takes fewer than 2^31 samples per output row") and not written, (rc, err)
    if name == "rank":
        (rc, err), _, written = guarded(native, [8], lambda ptrs: invoke(native, name, plan, (wide, wide), 1, 1 << 31, ptrs, mem=native.MEM_HOST,
                                                                         method=9))
        assert (rc, err) == (native.ERR_INVALID, "unknown rank method 9") and not written
    assert plan.describe() == before


# ---------------------------------------------------------------------------------------------------------------------
# 4. describe() after a call on a plan without bins: the driver's own line
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ENTRIES)
def test_describe_after_a_plan_without_bins(xh, data, name):
    from xhistogram_amd import _native as native

    other = "group" if name == "sort" else "sort"  # (whose line the plan holds before the call)
    for n_cols in (65, WIDEST):
        run_case(native, xh, data, other, "no_bins", n_cols)
        plan = run_case(native, xh, data, name, "no_bins", n_cols, size=7, inverse=True)
        prefix, none = DESCRIBE[name]
        line = plan.describe()
        assert line.startswith(prefix) and none in line, line
