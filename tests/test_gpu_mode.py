"""histogram_mode on the GPU: every comparison is bit for bit against tests/mode_oracle.py (tests/bin_rank_oracle.py's sorted
domain, the runs of non-NaN values of each bin, the first of the longest), int64 by value and `mode` by its bit pattern, and
every direct case asserts from the plan's describe() that it ran the words and the sort the restatement predicts.

Direct cases go through Plan.execute_mode with the four outputs as one block inside a DeviceBuffer filled with a sentinel:
lead | count | nunique | mode | mode_count | tail.  The sentinel must be intact in the lead and the tail and gone from every
element of the block; 0x5A5A... is neither 0 nor a NaN, so no result is mistaken for it.  The lead is odd in every second case,
so the block starts 8 bytes off 16-byte alignment there.  The slots of the call's atomic maximum are the mode_count block
itself: the sentinel there is larger than any packed run, so a call that forgot to zero its slots would report it (and
test_slots_full_of_set_bits hands over a block of all ones).  The case tables are tests/mode_cases.py's; tests/test_mode_cpu.py
holds them to what they claim."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import bin_order_cases as bc
import bin_order_oracle as bo
import bin_rank_oracle as ro
import bin_sort_cases as sc
import bin_sort_oracle as so
import extreme_cases as xc
import map_oracle as mo
import mode_cases as mc
import mode_oracle as mdo
from test_gpu_bin_order import side_streams
from test_gpu_bin_sort import _dev, _tag, _upload
from test_gpu_map import generic_inputs
from test_gpu_parity import _plan_for, xh  # noqa: F401  (xh: the module fixture)
from test_gpu_values_census import _cus

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F64, F32 = np.float64, np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A5A5A5A5A5A5A5A
CASE_NO = [0]


def guarded_mode(native, plan, views, vview, n_rows, n_cols, stream=0, fill=SENTINEL):
    """Plan.execute_mode into the middle of a DeviceBuffer of `fill` -> (count, nunique, mode, mode_count), [n_rows, bins] each"""
    CASE_NO[0] += 1
    lead, tail = 64 + CASE_NO[0] % 2, 64
    n = n_rows * plan.n_bins
    host = np.full(lead + 4 * n + tail, fill, np.uint64).view(np.int64)
    guard = host[0]
    buf = native.DeviceBuffer(0, host.nbytes)
    buf.upload(host)
    torch.cuda.synchronize()
    base = buf.ptr + 8 * lead
    plan.execute_mode(views, vview, n_rows, n_cols, base, base + 8 * n, base + 16 * n, base + 24 * n, stream=stream)
    torch.cuda.synchronize()
    buf.download(host)
    buf.close()
    assert (host[:lead] == guard).all() and (host[lead + 4 * n:] == guard).all(), "the guard bands were written"
    block = host[lead:lead + 4 * n]
    assert not (block == guard).any(), "%d elements were never written" % (block == guard).sum()
    parts = [block[i * n:(i + 1) * n].reshape(n_rows, plan.n_bins).copy() for i in range(4)]
    return parts[0], parts[1], parts[2].view(np.float64), parts[3]


def run_direct(core, xs, v, edges, cmp=0, what="", layout_fast=True, want=None, fill=SENTINEL):
    """contiguous [R, C] host arrays through Plan.execute_mode: the describe() line, the guard bands, the oracle's bits"""
    from xhistogram_amd import _native as native

    n_rows, n_cols = xs[0].shape
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    xs_t = [_dev(x) for x in xs]
    vb = _upload(native, v)
    plan = _plan_for(core, xs, edges)
    views = [native.make_view(t.data_ptr(), _tag(native, x.dtype), n_cols, 1) for t, x in zip(xs_t, xs)]
    vview = native.make_view(vb.ptr, _tag(native, v.dtype), n_cols, 1)
    got = guarded_mode(native, plan, views, vview, n_rows, n_cols, fill=fill)
    hit = mdo.assert_variant(plan.describe(), mdo.predict(_cus(), edges, cmp, xs[0].dtype, v.dtype, n_rows, n_cols, layout_fast=layout_fast))
    if want is None:
        want = mdo.mode_rows(mo.index(xs, edges), v, n_bins)
    mdo.assert_same(got, want, what)
    vb.close()
    return hit, got


# ---------------------------------------------------------------------------------------------------------------------
# 1. the case tables: where the winning run, bin borders and segment ends fall among the words; sizes; dtypes; bin counts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.gpu_cases(mc.CUS), ids=lambda c: c["name"])
def test_case_table(xh, case):
    cus = _cus()
    edges, idx, xs, v = mc.case_data(case, cus)
    mc.check_claims(case, idx, v, cus)
    hit, got = run_direct(xh, xs, v, edges, what=case["name"])
    assert hit["words"] == -(-case["n_cols"] // 64)
    assert hit["sort"]["vdtype"] == so.DTYPE_NAME[case["vt"]] and hit["sort"]["bin_passes"] == so.bin_passes(int(np.prod(case["nbs"])))
    if "all dropped" in case["claims"]:
        assert not got[0].any() and not got[1].any() and not got[3].any() and (got[2].view(np.uint64) == mdo.NAN_BITS).all()


def test_more_rows_than_one_launch(xh):
    """one launch's rows and five more, two samples each in one bin: every row past the first batch takes its own words,
    offsets and slots, against the closed form of a row of two"""
    g = so.geometry(_cus(), 1 << 25, 2)
    n_rows = g["rows_per_launch"] + 5
    assert g["chunks"] == 1 and n_rows < (1 << 20)
    rng = np.random.default_rng(5)
    x = rng.integers(0, 3, (n_rows, 2)).astype(F32) - 0.5  # -0.5: dropped, 0.5: the bin, 1.5: dropped
    v = rng.integers(0, 2, (n_rows, 2)).astype(np.uint8)
    edges = [np.array([0.0, 1.0])]
    counted = mo.index([x], edges) == 0
    n = counted.sum(1)
    vf = v.astype(F64)
    same = vf[:, 0] == vf[:, 1]
    nunique = np.where(n == 2, np.where(same, 1, 2), n)
    mode_count = np.where(n == 2, np.where(same, 2, 1), n)
    low = np.where(n == 2, vf.min(1), np.where(counted[:, 0], vf[:, 0], vf[:, 1]))
    want = tuple(a[:, None] for a in (n, nunique, np.where(n > 0, low, np.nan), mode_count))
    hit, _ = run_direct(xh, [x], v, edges, what="row batches", want=want)
    assert hit["rows_per_launch"] == g["rows_per_launch"] < n_rows
    sel = slice(n_rows - 300, n_rows)
    mdo.assert_same(mdo.mode_rows(mo.index([x[sel]], edges), v[sel], 1), tuple(w[sel] for w in want), "the closed form")


# ---------------------------------------------------------------------------------------------------------------------
# 2. both families of bin_index in the sort's step 0: compare domains, sample types, input counts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dom", ["f64", "i64", "mixed"])
def test_generic_keys(xh, dom):
    """int32 samples on float64 edges (domain 0), int64 on int64 (1), int64 next to float64 (3): the generic family makes the keys"""
    for i, (n_rows, n_cols) in enumerate(((3, 1500), (1, 4000))):
        edges, xs, cmp = generic_inputs(dom, 100, n_rows, n_cols, 900 + i)
        v = sc.values("random", [F64, np.int32][i], n_rows, n_cols, 40 + i)
        hit, _ = run_direct(xh, xs, v, edges, cmp=cmp, what="%s %dx%d" % (dom, n_rows, n_cols))
        assert hit["sort"]["keys"] == "generic" and hit["sort"]["cmp"] == cmp and hit["sort"]["D"] == len(edges)


def test_datetime_samples(xh):
    t0 = np.datetime64("2020-01-01", "s")
    edges = [t0 + np.arange(0, 25 * 3600, 3600).astype("timedelta64[s]")]
    x = t0 + np.random.default_rng(7).integers(-4000, 26 * 3600, (2, 3000)).astype("timedelta64[s]")
    hit, _ = run_direct(xh, [x], sc.values("random", F32, 2, 3000, 41), edges, cmp=1, what="datetime64[s]")
    assert hit["sort"]["keys"] == "generic"


def test_eight_inputs_of_three_bins(xh):
    idx = bc.indices("random", 2, 3000, 3 ** 8, seed=8)
    edges = bc.edges_for([3] * 8)
    xs = xc.emit(idx, edges, F64)
    v = np.random.default_rng(42).integers(0, 4, (2, 3000)).astype(np.int16)
    hit, _ = run_direct(xh, xs, v, edges, what="eight inputs")
    assert (hit["sort"]["keys"], hit["sort"]["D"], hit["sort"]["bin_passes"]) == ("generic", 8, 2)


def test_two_inputs(xh):
    idx = bc.indices("random", 3, 2000, 12, seed=9)
    edges = bc.edges_for([4, 3])
    hit, _ = run_direct(xh, xc.emit(idx, edges, F32), sc.values("random", F32, 3, 2000, 48), edges, what="two inputs")
    assert hit["sort"]["D"] == 2


# ---------------------------------------------------------------------------------------------------------------------
# 3. layouts through the C ABI: samples and values
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_base_pointers_off_16_byte_alignment(xh, sdt):
    from xhistogram_amd import _native as native

    st = F64 if sdt == "f64" else F32
    n_rows, n_cols = 3, 1001
    edges = bc.edges_for([50])
    flat = np.concatenate([[0], xc.emit(bc.indices("random", 1, n_rows * n_cols, 50, seed=9), edges, st)[0].reshape(-1)]).astype(st)
    vflat = np.concatenate([[0], sc.values("random", st, 1, n_rows * n_cols, 43).reshape(-1)]).astype(st)
    x_t, v_t = _dev(flat), _dev(vflat)
    assert x_t.data_ptr() % 16 == 0 and v_t.data_ptr() % 16 == 0
    plan = _plan_for(xh, [flat], edges)
    views = [native.make_view(x_t.data_ptr() + flat.itemsize, _tag(native, st), n_cols, 1)]
    vview = native.make_view(v_t.data_ptr() + flat.itemsize, _tag(native, st), n_cols, 1)
    got = guarded_mode(native, plan, views, vview, n_rows, n_cols)
    mdo.assert_variant(plan.describe(), mdo.predict(_cus(), edges, 0, st, st, n_rows, n_cols))
    mdo.assert_same(got, mdo.mode_rows(mo.index([flat[1:].reshape(n_rows, n_cols)], edges), vflat[1:].reshape(n_rows, n_cols), 50), "x[1:]")


@pytest.mark.parametrize("layout", ["row_broadcast", "transposed", "values_col_broadcast", "values_strided"])
def test_strided_views(xh, layout):
    """rows of samples broadcast at stride 0 (still the fast family) and a transposed block (row stride 1: the generic family),
    each with values laid out the same way; values broadcast along the columns (one run per bin) and values at a column
    stride of 3"""
    from xhistogram_amd import _native as native

    edges = bc.edges_for([40])
    n_rows, n_cols = 3, 2500
    vals = sc.values("random", F64, n_rows, 3 * n_cols, 44)
    if layout == "row_broadcast":
        base = xc.emit(bc.indices("random", 1, n_cols, 40, seed=10), edges, F64)[0]
        logical, (rs, cs) = np.broadcast_to(base, (n_rows, n_cols)), (0, 1)
        vbase = vals[:1, :n_cols]
        vlogical, (vrs, vcs) = np.broadcast_to(vbase, (n_rows, n_cols)), (0, 1)
    elif layout == "transposed":
        base = xc.emit(bc.indices("random", n_cols, n_rows, 40, seed=11), edges, F64)[0]  # [C, R] in memory
        logical, (rs, cs) = base.T, (1, n_rows)
        vbase = np.ascontiguousarray(vals[:, :n_cols].T)
        vlogical, (vrs, vcs) = vbase.T, (1, n_rows)
    else:
        base = xc.emit(bc.indices("random", n_rows, n_cols, 40, seed=12), edges, F64)[0]
        logical, (rs, cs) = base, (n_cols, 1)
        if layout == "values_col_broadcast":
            vbase = np.ascontiguousarray(vals[:, :1])
            vlogical, (vrs, vcs) = np.broadcast_to(vbase, (n_rows, n_cols)), (1, 0)
        else:
            vbase = vals
            vlogical, (vrs, vcs) = vals[:, ::3], (3 * n_cols, 3)
    x_t, v_t = _dev(base), _dev(vbase)
    plan = _plan_for(xh, [base], edges)
    got = guarded_mode(native, plan, [native.make_view(x_t.data_ptr(), native.F64, rs, cs)],
                       native.make_view(v_t.data_ptr(), native.F64, vrs, vcs), n_rows, n_cols)
    fast = layout != "transposed"
    hit = mdo.assert_variant(plan.describe(), mdo.predict(_cus(), edges, 0, F64, F64, n_rows, n_cols, layout_fast=fast))
    assert hit["sort"]["keys"] == ("fast" if fast else "generic")
    mdo.assert_same(got, mdo.mode_rows(mo.index([np.ascontiguousarray(logical)], edges), np.ascontiguousarray(vlogical), 40), layout)


# ---------------------------------------------------------------------------------------------------------------------
# 4. determinism: twice, on two streams at once, and slots that start full of set bits
# ---------------------------------------------------------------------------------------------------------------------
def _tie_block(n_rows, n_cols, nb, seed):
    edges = bc.edges_for([nb])
    x = xc.emit(bc.indices("random", n_rows, n_cols, nb, seed=seed), edges, F64)[0]
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 10, (n_rows, n_cols)).astype(F32)  # ten categories: many runs of nearly equal length
    v[rng.random(v.shape) < 0.05] = np.nan
    return edges, x, v


def test_twice_and_on_two_streams_at_once(xh):
    from xhistogram_amd import _native as native

    n_rows, n_cols, nb = 2, 60_000, 37
    edges, x, v = _tie_block(n_rows, n_cols, nb, 12)
    x_t, v_t = _dev(x), _dev(v)
    plan = _plan_for(xh, [x], edges)
    views = [native.make_view(x_t.data_ptr(), native.F64, n_cols, 1)]
    vview = native.make_view(v_t.data_ptr(), native.F32, n_cols, 1)
    want = mdo.mode_rows(mo.index([x], edges), v, nb)
    first = guarded_mode(native, plan, views, vview, n_rows, n_cols)
    second = guarded_mode(native, plan, views, vview, n_rows, n_cols)
    mdo.assert_same(first, want, "first run")
    mdo.assert_same(second, first, "the second run")
    streams = side_streams(2)
    outs = [torch.full((4, n_rows, nb), 7, dtype=torch.int64, device="cuda") for _ in streams]
    torch.cuda.synchronize()
    for _ in range(3):
        for s, o in zip(streams, outs):
            plan.execute_mode(views, vview, n_rows, n_cols, *[o[i].data_ptr() for i in range(4)], stream=s.cuda_stream)
    torch.cuda.synchronize()
    for o in outs:
        h = o.cpu().numpy()
        mdo.assert_same((h[0], h[1], h[2].view(F64), h[3]), want, "two streams")


def test_slots_full_of_set_bits(xh):
    """the slots are the mode_count block: handed over as bytes of all ones, larger than any packed run, a call that did not
    zero them (for every batch of rows) would keep them"""
    edges, x, v = _tie_block(3, 5000, 20, 14)
    run_direct(xh, [x], v, edges, what="all ones", fill=0xFFFFFFFFFFFFFFFF)
    run_direct(xh, [x[:, :0]], v[:, :0], edges, what="all ones, no columns", fill=0xFFFFFFFFFFFFFFFF)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the public API
# ---------------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


API_AXES = [(2,), (1,), (0,), (0, 2), (2, 0), None]


def _api_block(seed=300, shape=(5, 37, 11)):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.2, 1.2, shape)
    x[rng.random(shape) < 0.05] = np.nan
    v = np.round(rng.standard_normal(shape) * 3, 0)  # (ties)
    v[rng.random(shape) < 0.05] = np.nan
    v[rng.random(shape) < 0.05] = -0.0
    return x, v, np.linspace(-1.0, 1.0, 9)


def _want(x, v, edges, axis):
    """the oracle's four outputs in the shape histogram gives: kept axes, then the bins"""
    idx = mo.index([x], [edges])
    return mdo.mode_rows(bo.rows_of(idx, axis), bo.rows_of(v, axis), len(edges) - 1)


@pytest.mark.parametrize("backend", ["torch", "numpy", "device"])
@pytest.mark.parametrize("axis", API_AXES, ids=[str(a) for a in API_AXES])
def test_public_api_backends_and_axes(xh, backend, axis):
    """a 3-D block over trailing, middle, leading and split axes (listed in both orders): the oracle's bits, kept axes then bins"""
    from xhistogram_amd.devicearray import DeviceArray

    x, v, edges = _api_block()
    put = {"torch": lambda a: torch.as_tensor(a).cuda(), "numpy": lambda a: a, "device": lambda a: DeviceArray.from_numpy(a, 0)}[backend]
    kind = torch.Tensor if backend == "torch" else np.ndarray
    *got, e = xh.histogram_mode(put(x), values=put(v), bins=[edges], axis=axis)
    want = _want(x, v, edges, axis)
    assert all(isinstance(g, kind) and tuple(g.shape) == want[0].shape for g in got) and np.array_equal(e[0], edges)
    mdo.assert_same([_np(g) for g in got], want, "%s %s" % (backend, axis))


def test_identities_with_the_librarys_own_results(xh):
    """count is histogram_mean_var's; nunique the largest dense rank of the bin; mode_count the largest max - min + 1; and where
    every value of a bin is distinct, mode is histogram_extrema's vmin bit for bit"""
    x, v, edges = _api_block(310, (6, 900))
    v2 = v.copy()
    v2[3:] = np.random.default_rng(311).permutation(v2[3:].size).reshape(v2[3:].shape) - 1000.0  # (three rows of distinct values)
    xd, vd = torch.as_tensor(x).cuda(), torch.as_tensor(v2).cuda()
    kw = dict(values=vd, bins=[edges], axis=1)
    count, nunique, mode, mode_count, _ = (_np(a) if hasattr(a, "detach") else a for a in xh.histogram_mode(xd, **kw))
    mdo.assert_same((count, nunique, mode, mode_count), _want(x, v2, edges, (1,)), "the block")
    np.testing.assert_array_equal(count, _np(xh.histogram_mean_var(xd, **kw)[0]))
    r = {m: _np(xh.bin_rank(xd, method=m, **kw)[0]) for m in ("dense", "max", "min")}
    vmin = _np(xh.histogram_extrema(xd, **kw)[0])
    idx = mo.index([x], [edges])
    for row in range(x.shape[0]):
        for b in range(8):
            sel = (idx[row] == b) & ~np.isnan(v2[row])
            if not sel.any():
                assert count[row, b] == nunique[row, b] == mode_count[row, b] == 0
                continue
            assert nunique[row, b] == r["dense"][row][sel].max()
            assert mode_count[row, b] == (r["max"][row][sel] - r["min"][row][sel] + 1).max()
            if nunique[row, b] == count[row, b]:
                assert mode[row, b].view(np.uint64) == vmin[row, b].view(np.uint64) and mode_count[row, b] == 1
    assert (nunique[3:] == count[3:]).all() and (nunique[:3] < count[:3]).any()


def test_values_broadcast_against_the_samples(xh):
    rng = np.random.default_rng(307)
    x = rng.uniform(-1.2, 1.2, (6, 400))
    v = rng.integers(-5, 6, (400,)).astype(np.int16)
    edges = [np.linspace(-1.0, 1.0, 9)]
    got = xh.histogram_mode(torch.as_tensor(x).cuda(), values=torch.as_tensor(v).cuda(), bins=edges, axis=1)[:4]
    mdo.assert_same([_np(g) for g in got], mdo.mode_rows(mo.index([x], edges), np.broadcast_to(v, x.shape), 8), "broadcast values")
    count, nunique, mode, mode_count, _ = xh.histogram_mode(x, values=2.5, bins=edges, axis=1)  # a scalar: one run per bin
    assert (nunique == (count > 0)).all() and (mode_count == count).all() and (mode[count > 0] == 2.5).all()


def test_the_blocks_dask_hands_over(xh):
    """core._value_block as a dask task calls it, on host blocks over the kept axis: [4, rows, 1, bins] float64, the int64
    outputs as the bits they are (they are never merged)"""
    x, v, edges = _api_block(312, (6, 300))
    for lo, hi in ((0, 2), (2, 6)):
        out = xh._value_block(x[lo:hi], v[lo:hi], stat="mode", axis=[1], bins=[edges])
        assert out.shape == (4, hi - lo, 1, 8) and out.dtype == F64
        got = (out[0, :, 0].view(np.int64), out[1, :, 0].view(np.int64), out[2, :, 0], out[3, :, 0].view(np.int64))
        mdo.assert_same(got, _want(x[lo:hi], v[lo:hi], edges, (1,)), "rows %d..%d" % (lo, hi))


@pytest.mark.parametrize("backend", ["torch", "numpy"])
def test_extents_of_zero(xh, backend):
    edges = [np.linspace(0.0, 1.0, 5)]
    put = (lambda a: torch.as_tensor(a).cuda()) if backend == "torch" else (lambda a: a)
    for shape, axis, kept in (((3, 0), 1, (3,)), ((0, 7), 1, (0,)), ((0,), None, ()), ((2, 0, 3), (0, 2), (0,))):
        count, nunique, mode, mode_count, _ = (_np(a) if not isinstance(a, list) else a
                                               for a in xh.histogram_mode(put(np.zeros(shape)), values=put(np.zeros(shape)), bins=edges, axis=axis))
        for a, dt in ((count, np.int64), (nunique, np.int64), (mode, F64), (mode_count, np.int64)):
            assert a.shape == kept + (4,) and a.dtype == dt
        assert not count.any() and not nunique.any() and not mode_count.any()
        assert (np.ascontiguousarray(mode).view(np.uint64) == mdo.NAN_BITS).all()


def test_zero_columns_through_the_plan(xh):
    from xhistogram_amd import _native as native

    edges = bc.edges_for([4])
    x = np.zeros((3, 1))
    x_t = _dev(x)
    plan = _plan_for(xh, [x], edges)
    view = native.make_view(x_t.data_ptr(), native.F64, 0, 1)
    got = guarded_mode(native, plan, [view], view, 3, 0)
    mdo.assert_same(got, mdo.mode_rows(np.zeros((3, 0), np.int64), np.zeros((3, 0)), 4), "no columns")
    mdo.assert_variant(plan.describe(), mdo.predict(_cus(), edges, 0, F64, F64, 3, 0))


def test_refusals(xh):
    from xhistogram_amd import _native as native

    x = torch.zeros(8, dtype=torch.float64, device="cuda")
    edges = [np.linspace(0.0, 1.0, 5)]
    with pytest.raises(TypeError, match="complex values have no order"):
        xh.histogram_mode(x, values=torch.zeros(8, dtype=torch.complex64, device="cuda"), bins=edges)
    with pytest.raises(NotImplementedError, match="histogram_mode does not take weights"):
        xh.histogram_mode(x, values=x, weights=x, bins=edges)
    with pytest.raises(TypeError, match="histogram_mode needs values"):
        xh.histogram_mode(x, values=None, bins=edges)
    # 2^31 columns by shape only: one element expanded at stride 0, refused by the front and by the library before any launch
    n = 1 << 31
    wide = torch.full((1,), 0.5, dtype=torch.float64, device="cuda").expand(n)
    assert wide.stride() == (0,)
    plan = _plan_for(xh, [np.zeros((2, 4))], edges)
    xh.histogram_mode(x, values=x, bins=edges)
    before = plan.describe()
    with pytest.raises(NotImplementedError, match=r"histogram_mode takes fewer than 2\^31"):
        xh.histogram_mode(wide, values=wide, bins=edges)
    out = torch.full((4, 2, 4), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    lib = native.load()
    view = native.make_view(x.data_ptr(), native.F64, 4, 1)
    ptrs = [C.c_void_p(out[i].data_ptr()) for i in range(4)]
    args = (plan._h, (native.XhistArray * 1)(view), C.byref(view), 2, 4)
    wide_view = native.make_view(wide.data_ptr(), native.F64, 0, 0)
    assert lib.xhist_plan_execute_mode(plan._h, (native.XhistArray * 1)(wide_view), C.byref(wide_view), 1, n, *ptrs, native.MEM_DEVICE,
                                       C.c_void_p(0)) == native.ERR_UNSUPPORTED
    assert "fewer than 2^31 samples per output row" in lib.xhist_last_error().decode()
    for missing in range(4):
        holed = [C.c_void_p(0) if i == missing else p for i, p in enumerate(ptrs)]
        assert lib.xhist_plan_execute_mode(*args, *holed, native.MEM_DEVICE, C.c_void_p(0)) == native.ERR_INVALID
        assert "NULL" in lib.xhist_last_error().decode()
    assert lib.xhist_plan_execute_mode(*args, *ptrs, native.MEM_HOST, C.c_void_p(0)) == native.ERR_INVALID
    assert "mem_kind XHIST_MEM_DEVICE" in lib.xhist_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and plan.describe() == before
    assert lib.xhist_plan_execute_mode(*args, *ptrs, native.MEM_DEVICE, C.c_void_p(0)) == native.OK
    torch.cuda.synchronize()
    h = out.cpu().numpy()  # (four zeros in bin 0 of each of two rows)
    want = (np.array([[4, 0, 0, 0]] * 2), np.array([[1, 0, 0, 0]] * 2), np.array([[0.0, np.nan, np.nan, np.nan]] * 2), np.array([[4, 0, 0, 0]] * 2))
    mdo.assert_same((h[0], h[1], h[2].view(F64), h[3]), want, "a valid call still runs")


def test_eight_threads_on_one_plan(xh):
    edges = [np.linspace(-1.0, 1.0, 33)]
    rng = np.random.default_rng(303)
    xs = [rng.uniform(-1.1, 1.1, (3, 5000 + 17 * t)) for t in range(8)]
    vs = [rng.integers(0, 6, (3, 5000 + 17 * t)).astype(F32) for t in range(8)]
    results, errors = [None] * 8, []
    streams = side_streams(8)

    def work(t):
        try:
            with torch.cuda.stream(streams[t]):
                for _ in range(3):
                    got = xh.histogram_mode(torch.as_tensor(xs[t]).cuda(), values=torch.as_tensor(vs[t]).cuda(), bins=edges, axis=1)[:4]
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
        mdo.assert_same(results[t], mdo.mode_rows(mo.index([xs[t]], edges), vs[t], 32), "thread %d" % t)


def test_torch_results_follow_the_current_stream(xh):
    edges, x, v = _tie_block(1, 40_000, 100, 304)
    s = side_streams(1)[0]
    with torch.cuda.stream(s):
        got = xh.histogram_mode(torch.as_tensor(x[0]).cuda(), values=torch.as_tensor(v[0]).cuda(), bins=edges)[:4]
        s.synchronize()
        got = [g.cpu().numpy() for g in got]
    mdo.assert_same(got, mdo.mode_rows(mo.index([x[0]], edges), v[0], 100), "side stream")


def test_edges_from_a_bin_count_and_two_inputs(xh):
    rng = np.random.default_rng(305)
    x, y = rng.uniform(0, 1, (2, 4, 600))
    v = rng.integers(0, 9, (4, 600))
    *got, e = xh.histogram_mode(torch.as_tensor(x).cuda(), torch.as_tensor(y).cuda(), values=torch.as_tensor(v).cuda(), bins=[4, 3], axis=1)
    edges = [np.asarray(b) for b in e]
    want = [w.reshape(4, 4, 3) for w in mdo.mode_rows(mo.index([x, y], edges), v, 12)]
    mdo.assert_same([_np(g) for g in got], want, "two inputs")


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
    temp = xr.DataArray(x, dims=("time", "x"), coords={"time": np.arange(4.0)}, name="temp")
    cls = xr.DataArray(v, dims=("time", "x"), coords={"time": np.arange(4.0)}, name="cls")
    got = xhx.histogram_mode(temp, values=cls, bins=[edges], dim=["x"])
    assert [g.name for g in got] == ["cls_count", "cls_nunique", "cls_mode", "cls_mode_count"]
    assert all(tuple(g.dims) == ("time", "temp_bin") for g in got)
    mdo.assert_same([np.asarray(g.data) for g in got], mdo.mode_rows(mo.index([x], [edges]), v, 8), "xarray")
    np.testing.assert_array_equal(np.asarray(got[2]["time"].data), np.arange(4.0))
    flat = xhx.histogram_mode(temp, values=cls, bins=[edges])
    mdo.assert_same([np.asarray(g.data) for g in flat], mdo.mode_rows(mo.index([x], [edges]).reshape(-1), v.reshape(-1), 8), "flat")
    with pytest.raises(TypeError, match="accepts only xarray.DataArray"):
        xhx.histogram_mode(x, values=cls, bins=[edges])


def test_dask_branch(monkeypatch):
    """blocks over the kept axes give what the numpy call gives, bit for bit: tests/mode_dask_script.py in the interpreter that
    has dask, started as tests/test_dask_branch.py starts its own script"""
    import test_dask_branch as tdb

    if not tdb._have_dask_python():
        pytest.skip("no interpreter with dask in this image")
    monkeypatch.setattr(tdb, "SCRIPT", os.path.join(ROOT, "tests", "mode_dask_script.py"))
    assert "MODE-DASK-OK" in tdb._run("mode")
