"""bin_order on the GPU: every comparison is bit for bit against tests/bin_order_oracle.py (numpy's stable argsort of the oracle's
bin indices), and every direct case asserts from the plan's describe() that it ran the geometry the restatement predicts.

Direct cases go through Plan.execute_group with both outputs inside one DeviceBuffer filled with a sentinel: lead | order |
gap | offsets | tail.  The sentinel must be intact in the lead, the gap and the tail and gone from every element of the two
blocks (no position and no offset can equal it).  The lead is odd in every second case, so the blocks start 8 bytes off 16-byte
alignment there.  The case tables are tests/bin_order_cases.py's; tests/test_bin_order_cpu.py holds them to what they claim."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import bin_order_cases as bc
import bin_order_oracle as bo
import extreme_cases as xc
import map_oracle as mo
from test_gpu_map import generic_inputs
from test_gpu_parity import _plan_for, xh  # noqa: F401  (xh: the module fixture)
from test_gpu_values_census import _cus

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F64, F32 = np.float64, np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A5A5A5A5A5A5A5A
CASE_NO = [0]
GAP = 64


_STREAMS = []


def side_streams(n):
    """n of the eight side streams of this file, made once and together: later test files then find torch's stream pool, and the
    hardware queues the runtime hands its streams in the order they are made, where a session without this file leaves them
    (eight is a multiple of the queues a process opens)"""
    if not _STREAMS:
        _STREAMS.extend(torch.cuda.Stream() for _ in range(8))
    return _STREAMS[:n]


def _tag(native, dt):
    return native.dtype_tag(np.dtype(np.int64) if np.dtype(dt).kind in "mM" else dt)


def _dev(x):
    x = np.ascontiguousarray(x)
    return torch.as_tensor(x.view(np.int64) if x.dtype.kind in "mM" else x).cuda()


def guarded_group(native, plan, views, n_rows, n_cols, n_bins, stream=0):
    """Plan.execute_group into the middle of a DeviceBuffer of sentinels -> (order [n_rows, n_cols], offsets [n_rows, n_bins + 1])"""
    CASE_NO[0] += 1
    lead, tail = 64 + CASE_NO[0] % 2, 64
    n, m = n_rows * n_cols, n_rows * (n_bins + 1)
    host = np.full(lead + n + GAP + m + tail, SENTINEL, np.int64)
    buf = native.DeviceBuffer(0, host.nbytes)
    buf.upload(host)
    torch.cuda.synchronize()
    plan.execute_group(views, n_rows, n_cols, buf.ptr + 8 * lead, buf.ptr + 8 * (lead + n + GAP), stream=stream)
    torch.cuda.synchronize()
    buf.download(host)
    buf.close()
    guards = (host[:lead], host[lead + n:lead + n + GAP], host[lead + n + GAP + m:])
    assert all((g == SENTINEL).all() for g in guards), "the guard bands were written"
    order = host[lead:lead + n].reshape(n_rows, n_cols)
    offsets = host[lead + n + GAP:lead + n + GAP + m].reshape(n_rows, n_bins + 1)
    for name, block in (("order", order), ("offsets", offsets)):
        assert not (block == SENTINEL).any(), "%d elements of %s were never written" % ((block == SENTINEL).sum(), name)
    return order, offsets


def run_direct(core, xs, edges, cmp=0, what="", layout_fast=True):
    """contiguous [R, C] host arrays through Plan.execute_group: the describe() line, the guard bands, the oracle's bits"""
    from xhistogram_amd import _native as native

    n_rows, n_cols = xs[0].shape
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    xs_t = [_dev(x) for x in xs]
    plan = _plan_for(core, xs, edges)
    views = [native.make_view(t.data_ptr(), _tag(native, x.dtype), n_cols, 1) for t, x in zip(xs_t, xs)]
    order, offsets = guarded_group(native, plan, views, n_rows, n_cols, n_bins)
    hit = bo.assert_variant(plan.describe(), bo.predict(_cus(), edges, cmp, xs[0].dtype, n_rows, n_cols, layout_fast=layout_fast))
    want_order, want_offsets = bo.order_offsets(mo.index(xs, edges), n_bins)
    mo.assert_bits(offsets, want_offsets, what + " offsets")
    mo.assert_bits(order, want_order, what + " order")
    return hit


# ---------------------------------------------------------------------------------------------------------------------
# 1. the case tables: sizes around a step and a chunk, ballot widths, waves per workgroup, the LDS bound, key patterns
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bc.gpu_cases(bc.CUS), ids=lambda c: c["name"])
def test_case_table(xh, case):
    cus = _cus()
    if cus != bc.CUS:  # (the table is a function of the device: the same names, this device's sizes)
        case = {c["name"]: c for c in bc.gpu_cases(cus)}.get(case["name"])
        if case is None:
            pytest.skip("the size list of this device has no such size")
    edges, idx, xs = bc.case_data(case, cus)
    bc.check_claims(case, idx, cus)
    hit = run_direct(xh, xs, edges, what=case["name"])
    assert hit["keys"] == "fast"


def test_more_rows_than_one_launch(xh):
    """one launch's rows and five more, two samples each in one bin: every row past the first batch is written, from its own
    keys into its own rows of both blocks"""
    g = bo.geometry(_cus(), 1, 1 << 25, 2)
    n_rows = g["rows_per_launch"] + 5
    assert g["chunks"] == 1 and n_rows < (1 << 25)
    rng = np.random.default_rng(5)
    x = rng.integers(0, 3, (n_rows, 2)).astype(F32) - 0.5  # -0.5: dropped, 0.5: the bin, 1.5: dropped
    edges = [np.array([0.0, 1.0])]
    hit = run_direct(xh, [x], edges, what="row batches")
    assert hit["rows_per_launch"] == g["rows_per_launch"] < n_rows


def test_the_lds_bound_plus_one_is_refused_and_nothing_is_launched(xh):
    from xhistogram_amd import _native as native

    edges = [np.linspace(-4.0, 4.0, bo.MAX_BINS + 2)]
    x = np.random.default_rng(6).uniform(-4, 4, (2, 500))
    x_t = _dev(x)
    plan = _plan_for(xh, [x], edges)
    before = plan.describe()
    out = torch.full((2 * 500 + 2 * (bo.MAX_BINS + 2),), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    lib = native.load()
    rc = lib.xhist_plan_execute_group(plan._h, (native.XhistArray * 1)(native.make_view(x_t.data_ptr(), native.F64, 500, 1)), 2, 500,
                                      C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr() + 8000), native.MEM_DEVICE, C.c_void_p(0))
    assert rc == native.ERR_UNSUPPORTED
    assert "at most %d bins" % bo.MAX_BINS in lib.xhist_last_error().decode()
    torch.cuda.synchronize()
    assert plan.describe() == before and bool((out == -7).all())
    with pytest.raises(NotImplementedError, match="at most %d bins" % bo.MAX_BINS):
        xh.bin_order(x_t, bins=edges, axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# 2. both families of bin_index in step 0: compare domains, sample types, input counts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dom", ["f64", "i64", "mixed"])
def test_generic_keys(xh, dom):
    """int32 samples on float64 edges (domain 0), int64 on int64 (1), int64 next to float64 (3): the generic family makes the keys"""
    for i, (n_rows, n_cols) in enumerate(((3, 1500), (1, 4000))):
        edges, xs, cmp = generic_inputs(dom, 100, n_rows, n_cols, 900 + i)
        hit = run_direct(xh, xs, edges, cmp=cmp, what="%s %dx%d" % (dom, n_rows, n_cols))
        assert hit["keys"] == "generic" and hit["cmp"] == cmp and hit["D"] == len(edges)


def test_datetime_samples(xh):
    t0 = np.datetime64("2020-01-01", "s")
    edges = [t0 + np.arange(0, 25 * 3600, 3600).astype("timedelta64[s]")]
    x = t0 + np.random.default_rng(7).integers(-4000, 26 * 3600, (2, 3000)).astype("timedelta64[s]")
    hit = run_direct(xh, [x], edges, cmp=1, what="datetime64[s]")
    assert hit["keys"] == "generic"


def test_eight_inputs_of_three_bins(xh):
    nbs = [3] * 8
    idx = bc.indices("random", 2, 3000, 3 ** 8, seed=8)
    edges = bc.edges_for(nbs)
    xs = xc.emit(idx, edges, F64)
    hit = run_direct(xh, xs, edges, what="eight inputs")
    assert (hit["keys"], hit["D"], hit["bits"]) == ("generic", 8, 13)


# ---------------------------------------------------------------------------------------------------------------------
# 3. layouts through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_base_pointer_off_16_byte_alignment(xh, sdt):
    from xhistogram_amd import _native as native

    st = F64 if sdt == "f64" else F32
    n_rows, n_cols = 3, 1001
    edges = bc.edges_for([50])
    flat = np.concatenate([[0], xc.emit(bc.indices("random", 1, n_rows * n_cols, 50, seed=9), edges, st)[0].reshape(-1)]).astype(st)
    x_t = _dev(flat)
    assert x_t.data_ptr() % 16 == 0
    plan = _plan_for(xh, [flat], edges)
    views = [native.make_view(x_t.data_ptr() + flat.itemsize, _tag(native, st), n_cols, 1)]
    order, offsets = guarded_group(native, plan, views, n_rows, n_cols, 50)
    bo.assert_variant(plan.describe(), bo.predict(_cus(), edges, 0, st, n_rows, n_cols))
    want = bo.order_offsets(mo.index([flat[1:].reshape(n_rows, n_cols)], edges), 50)
    mo.assert_bits(order, want[0], "x[1:] order")
    mo.assert_bits(offsets, want[1], "x[1:] offsets")


@pytest.mark.parametrize("layout", ["row_broadcast", "transposed"])
def test_strided_views(xh, layout):
    """rows broadcast at stride 0 (still the fast family) and a transposed block (row stride 1: the generic family)"""
    from xhistogram_amd import _native as native

    edges = bc.edges_for([40])
    n_rows, n_cols = 3, 2500
    if layout == "row_broadcast":
        base = xc.emit(bc.indices("random", 1, n_cols, 40, seed=10), edges, F64)[0]
        logical, (rs, cs) = np.broadcast_to(base, (n_rows, n_cols)), (0, 1)
    else:
        base = xc.emit(bc.indices("random", n_cols, n_rows, 40, seed=11), edges, F64)[0]  # [C, R] in memory
        logical, (rs, cs) = base.T, (1, n_rows)
    x_t = _dev(base)
    plan = _plan_for(xh, [base], edges)
    order, offsets = guarded_group(native, plan, [native.make_view(x_t.data_ptr(), native.F64, rs, cs)], n_rows, n_cols, 40)
    fast = layout == "row_broadcast"
    hit = bo.assert_variant(plan.describe(), bo.predict(_cus(), edges, 0, F64, n_rows, n_cols, layout_fast=fast))
    assert hit["keys"] == ("fast" if fast else "generic")
    want = bo.order_offsets(mo.index([np.ascontiguousarray(logical)], edges), 40)
    mo.assert_bits(order, want[0], layout + " order")
    mo.assert_bits(offsets, want[1], layout + " offsets")


# ---------------------------------------------------------------------------------------------------------------------
# 4. determinism: twice, and on two streams at once
# ---------------------------------------------------------------------------------------------------------------------
def test_twice_and_on_two_streams_at_once(xh):
    from xhistogram_amd import _native as native

    n_rows, n_cols, nb = 2, 200_000, 37
    edges = bc.edges_for([nb])
    x = xc.emit(bc.indices("random", n_rows, n_cols, nb, seed=12), edges, F64)[0]
    x_t = _dev(x)
    plan = _plan_for(xh, [x], edges)
    views = [native.make_view(x_t.data_ptr(), native.F64, n_cols, 1)]
    want = bo.order_offsets(mo.index([x], edges), nb)
    first = guarded_group(native, plan, views, n_rows, n_cols, nb)
    second = guarded_group(native, plan, views, n_rows, n_cols, nb)
    for a, b, w in zip(first, second, want):
        mo.assert_bits(a, w, "first run")
        mo.assert_bits(b, a, "second run")
    streams = side_streams(2)
    outs = [(torch.empty((n_rows, n_cols), dtype=torch.int64, device="cuda"), torch.empty((n_rows, nb + 1), dtype=torch.int64, device="cuda"))
            for _ in streams]
    torch.cuda.synchronize()
    for _ in range(3):
        for s, (o, f) in zip(streams, outs):
            plan.execute_group(views, n_rows, n_cols, o.data_ptr(), f.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    for o, f in outs:
        mo.assert_bits(o.cpu().numpy(), want[0], "two streams order")
        mo.assert_bits(f.cpu().numpy(), want[1], "two streams offsets")


# ---------------------------------------------------------------------------------------------------------------------
# 5. the public API
# ---------------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


API_AXES = [(2,), (1,), (0,), (0, 2), (2, 0), None]


@pytest.mark.parametrize("backend", ["torch", "numpy", "device"])
@pytest.mark.parametrize("axis", API_AXES, ids=[str(a) for a in API_AXES])
def test_public_api_backends_and_axes(xh, backend, axis):
    """a 3-D block over trailing, middle, leading and split axes (listed in both orders): the oracle's bits, and the identities
    with the library's own histogram, bin_index and histogram_extrema"""
    from xhistogram_amd.devicearray import DeviceArray

    rng = np.random.default_rng(300)
    shape = (5, 37, 11)
    edges = np.linspace(-1.0, 1.0, 9)
    x = rng.uniform(-1.2, 1.2, shape)
    x[rng.random(shape) < 0.05] = np.nan
    v = rng.standard_normal(shape)
    put = {"torch": lambda a: torch.as_tensor(a).cuda(), "numpy": lambda a: a, "device": lambda a: DeviceArray.from_numpy(a, 0)}[backend]
    xd, vd = put(x), put(v)
    kind = torch.Tensor if backend == "torch" else np.ndarray

    order, offsets, e = xh.bin_order(xd, bins=[edges], axis=axis)
    assert isinstance(order, kind) and isinstance(offsets, kind) and np.array_equal(e[0], edges)
    order, offsets = _np(order), _np(offsets)
    idx = mo.index([x], [edges])
    rows = bo.rows_of(idx, axis)
    want_order, want_offsets = bo.order_offsets(rows, 8)
    mo.assert_bits(order, want_order, "order")
    mo.assert_bits(offsets, want_offsets, "offsets")

    h, _ = xh.histogram(xd, bins=[edges], axis=axis)
    np.testing.assert_array_equal(np.diff(offsets, axis=-1), _np(h))
    got_idx, _ = xh.bin_index(xd, bins=[edges])
    keys = bo.keys_of(bo.rows_of(_np(got_idx), axis), 8)
    sorted_keys = np.take_along_axis(keys, order, axis=-1)
    assert (np.diff(sorted_keys, axis=-1) >= 0).all()
    flat_order, flat_offsets, flat_rows = order.reshape(-1, order.shape[-1]), offsets.reshape(-1, 9), rows.reshape(-1, rows.shape[-1])
    for r in range(flat_order.shape[0]):
        bo.assert_grouped(flat_order[r], flat_offsets[r], flat_rows[r], 8, "row %d" % r)

    # a per-bin statistic rebuilt from the order: the maximum of every non-empty segment is histogram_extrema's, bit for bit
    _, vmax, _ = xh.histogram_extrema(xd, values=vd, bins=[edges], axis=axis)
    vmax = _np(vmax).reshape(-1, 8)
    v_rows = bo.rows_of(v, axis).reshape(flat_rows.shape)
    for r in range(flat_order.shape[0]):
        counts = np.diff(flat_offsets[r])
        full = np.flatnonzero(counts > 0)
        assert np.isnan(vmax[r][counts == 0]).all()
        if len(full):
            sorted_v = v_rows[r][flat_order[r]][:flat_offsets[r][-1]]
            mo.assert_bits(np.maximum.reduceat(sorted_v, flat_offsets[r][full]), vmax[r][full], "vmax rebuilt, row %d" % r)


def test_both_listings_of_the_axes_give_the_same(xh):
    x = torch.as_tensor(np.random.default_rng(301).uniform(-1.2, 1.2, (4, 9, 13))).cuda()
    a = xh.bin_order(x, bins=[np.linspace(-1, 1, 6)], axis=(0, 2))
    b = xh.bin_order(x, bins=[np.linspace(-1, 1, 6)], axis=(2, 0))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("backend", ["torch", "numpy"])
def test_a_plan_without_bins(xh, backend):
    """one edge, no bin: every sample is dropped, offsets == [0] and the order is the positions; through Plan.execute_group too"""
    from xhistogram_amd import _native as native

    x = np.random.default_rng(302).uniform(-1.0, 1.0, (3, 515))
    edges = [np.array([0.25])]
    xd = torch.as_tensor(x).cuda() if backend == "torch" else x
    order, offsets, _ = xh.bin_order(xd, bins=edges, axis=1)
    assert _np(order).dtype == _np(offsets).dtype == np.int64
    np.testing.assert_array_equal(_np(order), np.broadcast_to(np.arange(515), (3, 515)))
    np.testing.assert_array_equal(_np(offsets), np.zeros((3, 1), np.int64))
    order, offsets, _ = xh.bin_order(xd, bins=edges)
    np.testing.assert_array_equal(_np(order), np.arange(3 * 515))
    np.testing.assert_array_equal(_np(offsets), [0])
    x_t = _dev(x)
    plan = _plan_for(xh, [x], edges)
    got = guarded_group(native, plan, [native.make_view(x_t.data_ptr(), native.F64, 515, 1)], 3, 515, 0)
    np.testing.assert_array_equal(got[0], np.broadcast_to(np.arange(515), (3, 515)))
    assert (got[1] == 0).all()


@pytest.mark.parametrize("backend", ["torch", "numpy"])
def test_extents_of_zero(xh, backend):
    edges = [np.linspace(0.0, 1.0, 5)]
    put = (lambda a: torch.as_tensor(a).cuda()) if backend == "torch" else (lambda a: a)
    order, offsets, _ = xh.bin_order(put(np.zeros((3, 0))), bins=edges, axis=1)  # c == 0
    assert _np(order).shape == (3, 0) and _np(order).dtype == np.int64
    np.testing.assert_array_equal(_np(offsets), np.zeros((3, 5), np.int64))
    order, offsets, _ = xh.bin_order(put(np.zeros((0, 7))), bins=edges, axis=1)  # no kept index
    assert _np(order).shape == (0, 7) and _np(offsets).shape == (0, 5)
    order, offsets, _ = xh.bin_order(put(np.zeros((0,))), bins=edges)
    assert _np(order).shape == (0,)
    np.testing.assert_array_equal(_np(offsets), np.zeros(5, np.int64))


def test_zero_columns_through_the_plan(xh):
    from xhistogram_amd import _native as native

    edges = bc.edges_for([4])
    x = np.zeros((3, 1))
    x_t = _dev(x)
    plan = _plan_for(xh, [x], edges)
    got = guarded_group(native, plan, [native.make_view(x_t.data_ptr(), native.F64, 0, 1)], 3, 0, 4)
    assert got[0].shape == (3, 0) and (got[1] == 0).all()
    bo.assert_variant(plan.describe(), bo.predict(_cus(), edges, 0, F64, 3, 0))


def test_eight_threads_on_one_plan(xh):
    edges = [np.linspace(-1.0, 1.0, 33)]
    rng = np.random.default_rng(303)
    xs = [rng.uniform(-1.1, 1.1, (3, 5000 + 17 * t)) for t in range(8)]
    results, errors = [None] * 8, []

    streams = side_streams(8)

    def work(t):
        try:
            with torch.cuda.stream(streams[t]):
                for _ in range(3):
                    o, f, _e = xh.bin_order(torch.as_tensor(xs[t]).cuda(), bins=edges, axis=1)
                torch.cuda.current_stream().synchronize()
                results[t] = (o.cpu().numpy(), f.cpu().numpy())
        except Exception as err:  # noqa: BLE001
            errors.append(err)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(8):
        want = bo.order_offsets(mo.index([xs[t]], edges), 32)
        mo.assert_bits(results[t][0], want[0], "thread %d order" % t)
        mo.assert_bits(results[t][1], want[1], "thread %d offsets" % t)


def test_torch_results_follow_the_current_stream(xh):
    x = np.random.default_rng(304).uniform(-1.0, 1.0, 40_000)
    edges = [np.linspace(-1.0, 1.0, 101)]
    s = side_streams(1)[0]
    with torch.cuda.stream(s):
        order, offsets, _ = xh.bin_order(torch.as_tensor(x).cuda(), bins=edges)
        s.synchronize()
        got = order.cpu().numpy(), offsets.cpu().numpy()
    want = bo.order_offsets(mo.index([x], edges), 100)
    mo.assert_bits(got[0], want[0], "side stream order")
    mo.assert_bits(got[1], want[1], "side stream offsets")


def test_edges_from_a_bin_count_and_two_inputs(xh):
    rng = np.random.default_rng(305)
    x, y = rng.uniform(0, 1, (2, 4, 600))
    order, offsets, e = xh.bin_order(torch.as_tensor(x).cuda(), torch.as_tensor(y).cuda(), bins=[4, 3], axis=1)
    edges = [np.asarray(b) for b in e]
    want = bo.order_offsets(mo.index([x, y], edges), 12)
    mo.assert_bits(_np(order), want[0], "order")
    mo.assert_bits(_np(offsets), want[1], "offsets")


def test_xarray_wrapper(xh, monkeypatch):
    try:
        import xarray as xr
    except ImportError:
        monkeypatch.syspath_prepend(os.path.join(ROOT, "tests", "doubles"))
        import xarray as xr
    from xhistogram_amd import xarray as xhx

    rng = np.random.default_rng(306)
    edges = np.linspace(-1.0, 1.0, 9)
    x = rng.uniform(-1.2, 1.2, (4, 60))
    temp = xr.DataArray(x, dims=("time", "x"), coords={"time": np.arange(4.0)}, name="temp")
    order, offsets = xhx.bin_order(temp, bins=[edges], dim=["x"])
    assert (order.name, tuple(order.dims)) == ("temp_bin_order", ("time", "temp_order"))
    assert (offsets.name, tuple(offsets.dims)) == ("temp_bin_offsets", ("time", "temp_bin_offset"))
    want = bo.order_offsets(mo.index([x], [edges]), 8)
    mo.assert_bits(np.asarray(order.data), want[0], "xarray order")
    mo.assert_bits(np.asarray(offsets.data), want[1], "xarray offsets")
    np.testing.assert_array_equal(np.asarray(order["time"].data), np.arange(4.0))
    flat_order, flat_offsets = xhx.bin_order(temp, bins=[edges])
    assert tuple(flat_order.dims) == ("temp_order",) and tuple(flat_offsets.dims) == ("temp_bin_offset",)
    mo.assert_bits(np.asarray(flat_order.data), bo.order_offsets(mo.index([x], [edges]).reshape(-1), 8)[0], "xarray flat order")
    with pytest.raises(TypeError, match="accepts only xarray.DataArray"):
        xhx.bin_order(x, bins=[edges])


def test_dask_branch(monkeypatch):
    """blocks over the kept axes give what the numpy call gives, bit for bit: tests/bin_order_dask_script.py in the interpreter
    that has dask, started as tests/test_dask_branch.py starts its own script"""
    import test_dask_branch as tdb

    if not tdb._have_dask_python():
        pytest.skip("no interpreter with dask in this image")
    monkeypatch.setattr(tdb, "SCRIPT", os.path.join(ROOT, "tests", "bin_order_dask_script.py"))
    assert "BIN-ORDER-DASK-OK" in tdb._run("bin_order")
