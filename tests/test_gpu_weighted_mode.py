"""histogram_weighted_mode on the GPU, bit for bit against tests/weighted_unique_oracle.py: count and nunique by value, mode and
mode_weight by their bits (the entry sums are math.fsum over each run on exactly summable weights, tests/exact_weights.py).  On
N(0, 1) weights mode_weight is held, bit for bit, to the first maximal entry of the segment as bin_weighted_unique stores it.

Direct cases go through Plan.execute_mode_weighted with the four outputs as one block inside a DeviceBuffer filled with a
sentinel (0x5A5A...: neither 0, -1 nor a NaN), intact around the block and gone from every element of it.  The case tables are
tests/weighted_unique_cases.py's."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import bin_order_cases as bc
import bin_order_oracle as bo
import exact_weights as xw
import extreme_cases as xc
import map_oracle as mo
import mode_oracle as mdo
import weighted_unique_cases as wc
import weighted_unique_oracle as wo
from test_gpu_bin_order import side_streams
from test_gpu_bin_sort import _dev, _tag, _upload
from test_gpu_bin_weighted_unique import _normal_block, _tie_block, guarded_wunique
from test_gpu_mode import guarded_mode
from test_gpu_parity import _plan_for, xh  # noqa: F401  (xh: the module fixture)
from test_gpu_values_census import _cus

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F64, F32 = np.float64, np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A5A5A5A5A5A5A5A
CASE_NO = [0]


def guarded_wmode(native, plan, views, vview, wview, n_rows, n_cols, stream=0, fill=SENTINEL):
    """Plan.execute_mode_weighted into the middle of a DeviceBuffer of `fill` -> (count, nunique, mode, mode_weight)"""
    CASE_NO[0] += 1
    lead, tail = 64 + CASE_NO[0] % 2, 64
    n = n_rows * plan.n_bins
    host = np.full(lead + 4 * n + tail, fill, np.uint64).view(np.int64)
    guard = host[0]
    buf = native.DeviceBuffer(0, host.nbytes)
    buf.upload(host)
    torch.cuda.synchronize()
    base = buf.ptr + 8 * lead
    plan.execute_mode_weighted(views, vview, wview, n_rows, n_cols, base, base + 8 * n, base + 16 * n, base + 24 * n, stream=stream)
    torch.cuda.synchronize()
    buf.download(host)
    buf.close()
    assert (host[:lead] == guard).all() and (host[lead + 4 * n:] == guard).all(), "the guard bands were written"
    block = host[lead:lead + 4 * n]
    assert not (block == guard).any(), "%d elements were never written" % (block == guard).sum()
    parts = [block[i * n:(i + 1) * n].reshape(n_rows, plan.n_bins).copy() for i in range(4)]
    return parts[0], parts[1], parts[2].view(F64), parts[3].view(F64)


def run_direct(core, xs, v, w, edges, cmp=0, what="", want=None, fill=SENTINEL):
    from xhistogram_amd import _native as native

    n_rows, n_cols = xs[0].shape
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    xs_t = [_dev(x) for x in xs]
    vb, wb = _upload(native, v), _upload(native, w)
    plan = _plan_for(core, xs, edges)
    views = [native.make_view(t.data_ptr(), _tag(native, x.dtype), n_cols, 1) for t, x in zip(xs_t, xs)]
    got = guarded_wmode(native, plan, views, native.make_view(vb.ptr, _tag(native, v.dtype), n_cols, 1),
                        native.make_view(wb.ptr, _tag(native, w.dtype), n_cols, 1), n_rows, n_cols, fill=fill)
    hit = wo.assert_variant(plan.describe(), "wmode", wo.predict_mode(_cus(), edges, cmp, xs[0].dtype, v.dtype, n_rows, n_cols))
    if want is None:
        want = wo.wmode_rows(mo.index(xs, edges), v, w, n_bins)
    wo.assert_mode_same(got, want, what)
    vb.close()
    wb.close()
    return hit, got


def from_runs(runs, seed=0):
    """(idx [1, c], v [1, c], w [1, c]) of runs (bin, value, [weights]), shuffled"""
    idx = np.concatenate([np.full(len(ws), b, np.int32) for b, _, ws in runs])
    v = np.concatenate([np.full(len(ws), x, F64) for _, x, ws in runs])
    w = np.concatenate([np.asarray(ws, F64) for _, _, ws in runs])
    p = np.random.default_rng(seed).permutation(len(idx))
    return idx[p][None], v[p][None], w[p][None]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the case tables
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wc.gpu_cases(wc.CUS), ids=lambda c: c["name"])
def test_case_table(xh, case):
    cus = _cus()
    edges, idx, xs, v, w = wc.case_data(case, cus)
    hit, got = run_direct(xh, xs, v, w, edges, what=case["name"])
    assert hit["words"] == -(-case["n_cols"] // 64)
    empty = got[0] == 0
    assert (wo.bits(got[2])[empty] == wo.NAN_BITS).all() and (wo.bits(got[3])[empty] == 0).all() and not got[1][empty].any()


def test_more_rows_than_one_launch(xh):
    """one launch's rows and five more, two samples each in one bin: the slots of every batch are filled anew"""
    import bin_sort_oracle as so

    g = so.geometry(_cus(), 1 << 25, 2)
    n_rows = g["rows_per_launch"] + 5
    rng = np.random.default_rng(6)
    x = rng.integers(0, 2, (n_rows, 2)).astype(F32) + 0.5  # 0.5: bin 0, 1.5: dropped
    v = rng.integers(0, 2, (n_rows, 2)).astype(np.uint8)
    w = xw.f64(rng, (n_rows, 2), "both")
    edges = [np.array([0.0, 1.0])]
    ok = x < 1
    n = ok.sum(1)
    same = (n == 2) & (v[:, 0] == v[:, 1])
    count, nunique = n.astype(np.int64), np.where(same, 1, n).astype(np.int64)
    # two entries: the larger weight, the smaller value among equal ones (equal weights of two samples do not occur here)
    first_wins = np.where(n == 2, w[:, 0] > w[:, 1], ok[:, 0])
    mode = np.where(n == 0, wo.PAD, np.where(same, v[:, 0], np.where(first_wins, v[:, 0], v[:, 1])).astype(F64))
    weight = np.where(n == 0, 0.0, np.where(same, w[:, 0] + w[:, 1], np.where(first_wins, w[:, 0], w[:, 1])))
    assert not ((n == 2) & (w[:, 0] == w[:, 1])).any()
    want = tuple(a[:, None] for a in (count, nunique, mode, weight))
    hit, _ = run_direct(xh, [x], v, w, edges, what="row batches", want=want)
    assert hit["rows_per_launch"] == g["rows_per_launch"] < n_rows
    sel = slice(n_rows - 200, n_rows)
    wo.assert_mode_same(wo.wmode_rows(mo.index([x[sel]], edges), v[sel], w[sel], 1), tuple(a[sel] for a in want), "the closed form")


# ---------------------------------------------------------------------------------------------------------------------
# 2. what decides the winner
# ---------------------------------------------------------------------------------------------------------------------
def _check_runs(xh, runs, n_bins, what, seed=0):
    idx, v, w = from_runs(runs, seed)
    edges = bc.edges_for([n_bins])
    _, got = run_direct(xh, xc.emit(idx, edges, F64), v, w, edges, what=what)
    return got


def test_equal_sums_the_smallest_value_wins(xh):
    """two and three entries of equal sum in one word and in different words, next to lighter ones before and after them"""
    half = [0.5] * 70
    got = _check_runs(xh, [(0, 1.0, [0.25]), (0, 2.0, [0.5, 0.25, 0.25]), (0, 3.0, [0.5, 0.5]), (0, 4.0, [1.0]), (0, 5.0, [0.75]),
                           (1, 1.0, [2.0]), (1, 2.0, [1.0, 1.0]),
                           (2, 1.0, [0.5] * 10), (2, 2.0, half), (2, 3.0, half), (2, 4.0, half), (2, 5.0, [0.5] * 69),
                           (3, 7.0, half), (3, 8.0, [0.5] * 6), (3, 9.0, half)], 4, "equal sums")
    assert got[2][0].tolist() == [2.0, 1.0, 2.0, 7.0] and got[3][0].tolist() == [1.0, 2.0, 35.0, 35.0]


def test_zero_sums_of_both_signs_are_equal(xh):
    """a -0.0 sum against a +0.0 sum: the smaller value wins either way, and mode_weight carries that entry's own bits"""
    got = _check_runs(xh, [(0, 1.0, [1.0, -1.0]), (0, 2.0, [-0.0, -0.0]), (0, 3.0, [-1.0]),
                           (1, 1.0, [-0.0, -0.0]), (1, 2.0, [1.0, -1.0]), (1, 3.0, [-0.5])], 2, "zero sums")
    assert got[2][0].tolist() == [1.0, 1.0] and wo.bits(got[3][0]).tolist() == [0, 1 << 63]


def test_the_heaviest_is_not_the_most_frequent(xh):
    """counts used for sums would name 1.0 in bin 0 and 4.0 in bin 1"""
    runs = [(0, 1.0, [0.5] * 100), (0, 2.0, [30.0, 30.0]), (0, 3.0, [1.0] * 3), (1, 4.0, [-1.0] * 80), (1, 5.0, [-0.5])]
    got = _check_runs(xh, runs, 2, "heavy and rare")
    assert got[2][0].tolist() == [2.0, 5.0] and got[3][0].tolist() == [60.0, -0.5]
    idx, v, _ = from_runs(runs)
    assert mdo.mode_rows(idx, v, 2)[2][0].tolist() == [1.0, 4.0]


def test_a_nan_sum_takes_its_bin_and_no_other(xh):
    runs = [(0, 1.0, [1.0] * 70), (0, 2.0, [9.0] + [np.nan] + [1.0] * 80), (1, 1.0, [np.inf, 1.0]), (1, 2.0, [5.0]),
            (2, 1.0, [np.inf, -np.inf]), (2, 2.0, [7.0]), (3, 3.0, [-np.inf]), (3, 4.0, [-np.inf, 1.0])]
    got = _check_runs(xh, runs, 4, "nan sums")
    assert wo.bits(got[2][0]).tolist()[0] == wo.bits(got[3][0]).tolist()[0] == wo.NAN_BITS
    assert got[2][0, 1] == 1.0 and got[3][0, 1] == np.inf and wo.bits(got[3][0])[2] == wo.NAN_BITS and got[2][0, 3] == 3.0


# ---------------------------------------------------------------------------------------------------------------------
# 3. reproducibility and identities
# ---------------------------------------------------------------------------------------------------------------------
def test_mode_weight_is_the_first_maximal_entry_by_bits(xh):
    """N(0, 1) weights: mode_weight and mode are bitwise the first entry of the segment that holds the largest of
    bin_weighted_unique's sums, twice and on two streams at once; count and nunique are histogram_mode's"""
    from xhistogram_amd import _native as native

    edges, x, v, w = _normal_block(n_rows=2, n_cols=100_000, nb=7, seed=41)
    n_rows, n_cols = x.shape
    x_t, v_t, w_t = _dev(x), _dev(v), _dev(w)
    plan = _plan_for(xh, [x], edges)
    args = ([native.make_view(x_t.data_ptr(), native.F64, n_cols, 1)], native.make_view(v_t.data_ptr(), native.F64, n_cols, 1),
            native.make_view(w_t.data_ptr(), native.F64, n_cols, 1), n_rows, n_cols)
    uniques, _, sums, offsets = guarded_wunique(native, plan, *args, n_cols, False)
    got = guarded_wmode(native, plan, *args)
    plain = guarded_mode(native, plan, args[0], args[1], n_rows, n_cols)
    np.testing.assert_array_equal(got[0], plain[0])
    np.testing.assert_array_equal(got[1], plain[1])
    for r in range(n_rows):
        for b in range(7):
            seg = slice(offsets[r, b], offsets[r, b + 1])
            first = offsets[r, b] + int(np.argmax(sums[r, seg]))
            assert wo.bits(got[3][r, b:b + 1])[0] == wo.bits(sums[r, first:first + 1])[0], (r, b)
            assert wo.bits(got[2][r, b:b + 1])[0] == wo.bits(uniques[r, first:first + 1])[0], (r, b)
    again = guarded_wmode(native, plan, *args)
    assert all(np.array_equal(a.view(np.int64), g.view(np.int64)) for a, g in zip(again, got)), "the second call"
    streams = side_streams(2)
    outs = [torch.full((4, n_rows, 7), 7, dtype=torch.int64, device="cuda") for _ in streams]
    torch.cuda.synchronize()
    for _ in range(2):
        for s, o in zip(streams, outs):
            plan.execute_mode_weighted(*args, *[o[i].data_ptr() for i in range(4)], stream=s.cuda_stream)
    torch.cuda.synchronize()
    for o in outs:
        h = o.cpu().numpy()
        assert all(np.array_equal(h[i], g.view(np.int64)) for i, g in enumerate(got)), "two streams"


def test_unit_weights_give_histogram_mode(xh):
    from xhistogram_amd import _native as native

    edges, x, v, _ = _tie_block(3, 6000, 23, 52)
    n_rows, n_cols = x.shape
    x_t, v_t, one_t = _dev(x), _dev(v), _dev(np.ones(1, np.int32))
    plan = _plan_for(xh, [x], edges)
    views, vview = [native.make_view(x_t.data_ptr(), native.F64, n_cols, 1)], native.make_view(v_t.data_ptr(), native.F32, n_cols, 1)
    got = guarded_wmode(native, plan, views, vview, native.make_view(one_t.data_ptr(), native.I32, 0, 0), n_rows, n_cols)
    plain = guarded_mode(native, plan, views, vview, n_rows, n_cols)
    mdo.assert_same((got[0], got[1], got[2], got[3].astype(np.int64)), plain, "unit weights")
    assert (got[3] == plain[3]).all()


def test_slots_full_of_set_bits_and_zero_columns(xh):
    from xhistogram_amd import _native as native

    edges, x, v, w = _tie_block(3, 5000, 20, 14)
    run_direct(xh, [x], v, w, edges, what="all ones", fill=0xFFFFFFFFFFFFFFFF)
    run_direct(xh, [x[:, :0]], v[:, :0], w[:, :0], edges, what="all ones, no columns", fill=0xFFFFFFFFFFFFFFFF)
    plan = _plan_for(xh, [x], edges)
    assert plan.describe() == "wmode words=0 rows_per_launch=0 | none"


# ---------------------------------------------------------------------------------------------------------------------
# 4. the public API
# ---------------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


API_AXES = [(2,), (1,), (0,), (0, 2), None]


def _api_block(seed=300, shape=(5, 37, 11)):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.2, 1.2, shape)
    x[rng.random(shape) < 0.05] = np.nan
    v = np.round(rng.standard_normal(shape) * 2, 0)
    v[rng.random(shape) < 0.05] = np.nan
    v[rng.random(shape) < 0.05] = -0.0
    return x, v, xw.f64(rng, shape, "both"), np.linspace(-1.0, 1.0, 9)


def _want(x, v, w, edges, axis):
    idx = mo.index([x], [edges])
    return wo.wmode_rows(bo.rows_of(idx, axis), bo.rows_of(v, axis), bo.rows_of(w, axis), len(edges) - 1)


@pytest.mark.parametrize("backend", ["torch", "numpy", "device"])
@pytest.mark.parametrize("axis", API_AXES, ids=[str(a) for a in API_AXES])
def test_public_api_backends_and_axes(xh, backend, axis):
    from xhistogram_amd.devicearray import DeviceArray

    x, v, w, edges = _api_block()
    put = {"torch": lambda a: torch.as_tensor(a).cuda(), "numpy": lambda a: a, "device": lambda a: DeviceArray.from_numpy(a, 0)}[backend]
    kind = torch.Tensor if backend == "torch" else np.ndarray
    *got, e = xh.histogram_weighted_mode(put(x), values=put(v), weights=put(w), bins=[edges], axis=axis)
    want = _want(x, v, w, edges, axis)
    assert all(isinstance(g, kind) and tuple(g.shape) == want[0].shape for g in got) and np.array_equal(e[0], edges)
    wo.assert_mode_same([_np(g) for g in got], want, "%s %s" % (backend, axis))


def test_the_blocks_dask_hands_over(xh):
    x, v, w, edges = _api_block(312, (6, 300))
    for lo, hi in ((0, 2), (2, 6)):
        out = xh._value_block(x[lo:hi], v[lo:hi], w[lo:hi], stat="mode_w", axis=[1], bins=[edges])
        assert out.shape == (4, hi - lo, 1, 8) and out.dtype == F64
        got = (out[0, :, 0].view(np.int64), out[1, :, 0].view(np.int64), out[2, :, 0], out[3, :, 0])
        wo.assert_mode_same(got, _want(x[lo:hi], v[lo:hi], w[lo:hi], edges, (1,)), "rows %d..%d" % (lo, hi))


@pytest.mark.parametrize("backend", ["torch", "numpy"])
def test_extents_of_zero(xh, backend):
    edges = [np.linspace(0.0, 1.0, 5)]
    put = (lambda a: torch.as_tensor(a).cuda()) if backend == "torch" else (lambda a: a)
    for shape, axis, kept in (((3, 0), 1, (3,)), ((0, 7), 1, (0,)), ((0,), None, ()), ((2, 0, 3), (0, 2), (0,))):
        z = put(np.zeros(shape))
        count, nunique, mode, weight, _ = (_np(a) if not isinstance(a, list) else a
                                           for a in xh.histogram_weighted_mode(z, values=z, weights=z, bins=edges, axis=axis))
        for a, dt in ((count, np.int64), (nunique, np.int64), (mode, F64), (weight, F64)):
            assert a.shape == kept + (4,) and a.dtype == dt
        assert not count.any() and not nunique.any() and (wo.bits(weight) == 0).all() and (wo.bits(mode) == wo.NAN_BITS).all()


def test_refusals_through_the_c_abi(xh):
    from xhistogram_amd import _native as native

    x = torch.zeros(8, dtype=torch.float64, device="cuda")
    edges = [np.linspace(0.0, 1.0, 5)]
    plan = _plan_for(xh, [np.zeros((2, 4))], edges)
    xh.histogram_weighted_mode(x, values=x, weights=x, bins=edges)
    before = plan.describe()
    n = 1 << 31
    wide = torch.full((1,), 0.5, dtype=torch.float64, device="cuda").expand(n)
    for fn, name in ((xh.histogram_weighted_mode, "histogram_weighted_mode"), (xh.bin_weighted_unique, "bin_weighted_unique")):
        with pytest.raises(NotImplementedError, match=r"%s takes fewer than 2\^31" % name):
            fn(wide, values=wide, weights=wide, bins=edges)
    out = torch.full((5, 2, 5), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    lib = native.load()
    view = native.make_view(x.data_ptr(), native.F64, 4, 1)
    wide_view = native.make_view(wide.data_ptr(), native.F64, 0, 0)
    ptrs = [C.c_void_p(out[i].data_ptr()) for i in range(5)]
    arr, wide_arr = (native.XhistArray * 1)(view), (native.XhistArray * 1)(wide_view)
    dev, null = native.MEM_DEVICE, C.c_void_p(0)
    assert lib.xhist_plan_execute_mode_weighted(plan._h, wide_arr, C.byref(wide_view), C.byref(wide_view), 1, n, *ptrs[:4], dev, null) == native.ERR_UNSUPPORTED
    assert "histogram_weighted_mode takes fewer than 2^31 samples per output row" in lib.xhist_last_error().decode()
    assert lib.xhist_plan_execute_unique_weighted(plan._h, wide_arr, C.byref(wide_view), C.byref(wide_view), 1, n, 3, *ptrs, dev, null) == native.ERR_UNSUPPORTED
    assert "bin_weighted_unique takes fewer than 2^31 samples per output row" in lib.xhist_last_error().decode()
    margs = (plan._h, arr, C.byref(view), C.byref(view), 2, 4)
    for missing in range(4):
        holed = [null if i == missing else p for i, p in enumerate(ptrs[:4])]
        assert lib.xhist_plan_execute_mode_weighted(*margs, *holed, dev, null) == native.ERR_INVALID and "NULL" in lib.xhist_last_error().decode()
    for missing in range(4):  # (the inverse may be NULL)
        holed = [null if i == missing else p for i, p in enumerate(ptrs)]
        assert lib.xhist_plan_execute_unique_weighted(*margs, 3, *holed, dev, null) == native.ERR_INVALID and "NULL" in lib.xhist_last_error().decode()
    assert lib.xhist_plan_execute_mode_weighted(plan._h, arr, C.byref(view), None, 2, 4, *ptrs[:4], dev, null) == native.ERR_INVALID
    assert "weights are required" in lib.xhist_last_error().decode()
    assert lib.xhist_plan_execute_unique_weighted(*margs, -1, *ptrs, dev, null) == native.ERR_INVALID
    assert lib.xhist_plan_execute_mode_weighted(*margs, *ptrs[:4], native.MEM_HOST, null) == native.ERR_INVALID
    assert "mem_kind XHIST_MEM_DEVICE" in lib.xhist_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and plan.describe() == before
    assert lib.xhist_plan_execute_mode_weighted(*margs, *ptrs[:4], dev, null) == native.OK
    torch.cuda.synchronize()
    h = out.cpu().numpy().reshape(5, 10)[:, :8].reshape(5, 2, 4)  # (each block is [2, 4] at the head of its plane of 10)
    # four zeros of weight 0 in bin 0 of each of two rows
    want = (np.array([[4, 0, 0, 0]] * 2), np.array([[1, 0, 0, 0]] * 2), np.array([[0.0, np.nan, np.nan, np.nan]] * 2), np.zeros((2, 4)))
    wo.assert_mode_same((h[0], h[1], h[2].view(F64), h[3].view(F64)),
                        tuple(np.ascontiguousarray(a) for a in want), "a valid call still runs")


def test_eight_threads_on_one_plan(xh):
    edges = [np.linspace(-1.0, 1.0, 33)]
    rng = np.random.default_rng(303)
    xs = [rng.uniform(-1.1, 1.1, (3, 5000 + 17 * t)) for t in range(8)]
    vs = [rng.integers(0, 6, (3, 5000 + 17 * t)).astype(F32) for t in range(8)]
    ws = [xw.f64(rng, (3, 5000 + 17 * t), "both") for t in range(8)]
    results, errors = [None] * 8, []
    streams = side_streams(8)

    def work(t):
        try:
            with torch.cuda.stream(streams[t]):
                for _ in range(3):
                    got = xh.histogram_weighted_mode(torch.as_tensor(xs[t]).cuda(), values=torch.as_tensor(vs[t]).cuda(),
                                                     weights=torch.as_tensor(ws[t]).cuda(), bins=edges, axis=1)[:4]
                torch.cuda.current_stream().synchronize()
                results[t] = [g.cpu().numpy() for g in got]
        except Exception as err:  # noqa: BLE001
            errors.append(err)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(8):
        wo.assert_mode_same(results[t], wo.wmode_rows(mo.index([xs[t]], edges), vs[t], ws[t], 32), "thread %d" % t)


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
    v = np.round(rng.standard_normal((4, 60)), 0)
    w = xw.f64(rng, (60,))
    temp = xr.DataArray(x, dims=("time", "x"), coords={"time": np.arange(4.0)}, name="temp")
    cls = xr.DataArray(v, dims=("time", "x"), coords={"time": np.arange(4.0)}, name="cls")
    area = xr.DataArray(w, dims=("x",), name="area")
    got = xhx.histogram_weighted_mode(temp, values=cls, weights=area, bins=[edges], dim=["x"])
    assert [g.name for g in got] == ["cls_count", "cls_nunique", "cls_weighted_mode", "cls_mode_weight"]
    assert all(tuple(g.dims) == ("time", "temp_bin") for g in got)
    wo.assert_mode_same([np.asarray(g.data) for g in got], wo.wmode_rows(mo.index([x], [edges]), v, np.broadcast_to(w, x.shape), 8), "xarray")
    with pytest.raises(TypeError, match="accepts only xarray.DataArray"):
        xhx.histogram_weighted_mode(temp, values=cls, weights=w, bins=[edges])
