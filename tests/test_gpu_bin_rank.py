"""bin_rank on the GPU: every comparison is bit for bit against tests/bin_rank_oracle.py (np.lexsort over the oracle's bin
indices and core.extrema_keys, tie runs by == inside each bin), and every direct case asserts from the plan's describe() that it
ran the words and the sort the restatement predicts.

Direct cases go through Plan.execute_rank with the output inside one DeviceBuffer filled with a sentinel: lead | out | tail.
The sentinel must be intact in the lead and the tail and gone from every element of the block; 0x5A5A... is no NaN, so a NaN
result is not mistaken for it.  The lead is odd in every second case, so the block starts 8 bytes off 16-byte alignment there.
The case tables are tests/bin_rank_cases.py's; tests/test_bin_rank_cpu.py holds them to what they claim."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import bin_order_cases as bc
import bin_order_oracle as bo
import bin_rank_cases as rc
import bin_rank_oracle as ro
import bin_sort_cases as sc
import bin_sort_oracle as so
import extreme_cases as xc
import map_oracle as mo
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


def guarded_rank(native, plan, views, vview, n_rows, n_cols, method, descending, pct, stream=0):
    """Plan.execute_rank into the middle of a DeviceBuffer of sentinels -> rank float64 [n_rows, n_cols]"""
    CASE_NO[0] += 1
    lead, tail = 64 + CASE_NO[0] % 2, 64
    n = n_rows * n_cols
    host = np.full(lead + n + tail, SENTINEL, np.int64)
    buf = native.DeviceBuffer(0, host.nbytes)
    buf.upload(host)
    torch.cuda.synchronize()
    plan.execute_rank(views, vview, n_rows, n_cols, native.RANK_METHODS[method], descending, pct, buf.ptr + 8 * lead, stream=stream)
    torch.cuda.synchronize()
    buf.download(host)
    buf.close()
    assert (host[:lead] == SENTINEL).all() and (host[lead + n:] == SENTINEL).all(), "the guard bands were written"
    block = host[lead:lead + n]
    assert not (block == SENTINEL).any(), "%d elements were never written" % (block == SENTINEL).sum()
    return block.view(np.float64).reshape(n_rows, n_cols)


def run_direct(core, xs, v, edges, mode, cmp=0, what="", layout_fast=True, want=None):
    """contiguous [R, C] host arrays through Plan.execute_rank: the describe() line, the guard bands, the oracle's bits"""
    from xhistogram_amd import _native as native

    method, descending, pct = mode
    n_rows, n_cols = xs[0].shape
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    xs_t = [_dev(x) for x in xs]
    vb = _upload(native, v)
    plan = _plan_for(core, xs, edges)
    views = [native.make_view(t.data_ptr(), _tag(native, x.dtype), n_cols, 1) for t, x in zip(xs_t, xs)]
    vview = native.make_view(vb.ptr, _tag(native, v.dtype), n_cols, 1)
    got = guarded_rank(native, plan, views, vview, n_rows, n_cols, method, descending, pct)
    hit = ro.assert_variant(plan.describe(), ro.predict(_cus(), edges, cmp, xs[0].dtype, v.dtype, n_rows, n_cols, method, descending, pct,
                                                        layout_fast=layout_fast))
    if want is None:
        want = ro.rank_rows(mo.index(xs, edges), v, n_bins, method, descending, pct)
    mo.assert_bits(got, want, "%s %s" % (what, mode))
    vb.close()
    return hit, got


# ---------------------------------------------------------------------------------------------------------------------
# 1. the case tables: where tie runs, bin borders and NaN runs fall among the words; sizes; value dtypes; bin counts
# ---------------------------------------------------------------------------------------------------------------------
LAYOUT_CASES = [c for c in rc.gpu_cases(rc.CUS) if c["layout"]]
OTHER_CASES = [c for c in rc.gpu_cases(rc.CUS) if not c["layout"]]


@pytest.mark.parametrize("method", ro.METHODS)
@pytest.mark.parametrize("case", LAYOUT_CASES, ids=lambda c: c["name"])
def test_layout_cases_in_every_mode(xh, case, method):
    """each method, in both directions, plain and pct"""
    cus = _cus()
    for descending in (False, True):
        edges, idx, xs, v = rc.case_data(case, cus, descending)
        rc.check_claims(case, idx, v, cus, descending)
        for pct in (False, True):
            hit, _ = run_direct(xh, xs, v, edges, (method, descending, pct), what=case["name"])
            assert hit["sort"]["keys"] == "fast" and hit["words"] == -(-case["n_cols"] // 64)


@pytest.mark.parametrize("case", OTHER_CASES, ids=lambda c: c["name"])
def test_case_table(xh, case):
    """method average, and one more mode that goes round the twenty from case to case"""
    cus = _cus()
    k = OTHER_CASES.index(case)
    for mode in (("average", False, False), rc.MODES[(7 * k + 3) % len(rc.MODES)]):
        edges, idx, xs, v = rc.case_data(case, cus, mode[1])
        rc.check_claims(case, idx, v, cus, mode[1])
        hit, got = run_direct(xh, xs, v, edges, mode, what=case["name"])
        assert hit["sort"]["vdtype"] == so.DTYPE_NAME[case["vt"]] and hit["sort"]["bin_passes"] == so.bin_passes(int(np.prod(case["nbs"])))
        if "all dropped" in case["claims"] or "all values NaN" in case["claims"]:
            assert np.isnan(got).all()


def test_more_rows_than_one_launch(xh):
    """one launch's rows and five more, two samples each in one bin: every row past the first batch is ranked from its own words,
    offsets and divisors (pct), against the closed form of a row of two"""
    g = so.geometry(_cus(), 1 << 25, 2)
    n_rows = g["rows_per_launch"] + 5
    assert g["chunks"] == 1 and n_rows < (1 << 20)
    rng = np.random.default_rng(5)
    x = rng.integers(0, 3, (n_rows, 2)).astype(F32) - 0.5  # -0.5: dropped, 0.5: the bin, 1.5: dropped
    v = rng.integers(0, 2, (n_rows, 2)).astype(np.uint8)
    edges = [np.array([0.0, 1.0])]
    counted = mo.index([x], edges) == 0
    n = counted.sum(1, keepdims=True).astype(F64)
    vf, other = v.astype(F64), v[:, ::-1].astype(F64)
    alone = np.ones_like(vf)
    both = np.where(vf == other, 1.5, np.where(vf < other, 1.0, 2.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.where(counted, np.where(n == 2, both, alone) / n, np.nan)
    hit, _ = run_direct(xh, [x], v, edges, ("average", False, True), what="row batches", want=want)
    assert hit["rows_per_launch"] == g["rows_per_launch"] < n_rows
    sel = slice(n_rows - 300, n_rows)
    mo.assert_bits(ro.rank_rows(mo.index([x[sel]], edges), v[sel], 1, "average", False, True), want[sel], "the closed form")


# ---------------------------------------------------------------------------------------------------------------------
# 2. both families of bin_index in the sort's step 0: compare domains, sample types, input counts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dom", ["f64", "i64", "mixed"])
def test_generic_keys(xh, dom):
    """int32 samples on float64 edges (domain 0), int64 on int64 (1), int64 next to float64 (3): the generic family makes the keys"""
    for i, (n_rows, n_cols) in enumerate(((3, 1500), (1, 4000))):
        edges, xs, cmp = generic_inputs(dom, 100, n_rows, n_cols, 900 + i)
        v = sc.values("random", [F64, np.int32][i], n_rows, n_cols, 40 + i)
        hit, _ = run_direct(xh, xs, v, edges, (["max", "dense"][i], bool(i), True), cmp=cmp, what="%s %dx%d" % (dom, n_rows, n_cols))
        assert hit["sort"]["keys"] == "generic" and hit["sort"]["cmp"] == cmp and hit["sort"]["D"] == len(edges)


def test_datetime_samples(xh):
    t0 = np.datetime64("2020-01-01", "s")
    edges = [t0 + np.arange(0, 25 * 3600, 3600).astype("timedelta64[s]")]
    x = t0 + np.random.default_rng(7).integers(-4000, 26 * 3600, (2, 3000)).astype("timedelta64[s]")
    hit, _ = run_direct(xh, [x], sc.values("random", F32, 2, 3000, 41), edges, ("min", False, False), cmp=1, what="datetime64[s]")
    assert hit["sort"]["keys"] == "generic"


def test_eight_inputs_of_three_bins(xh):
    idx = bc.indices("random", 2, 3000, 3 ** 8, seed=8)
    edges = bc.edges_for([3] * 8)
    xs = xc.emit(idx, edges, F64)
    hit, _ = run_direct(xh, xs, sc.values("random", F64, 2, 3000, 42), edges, ("ordinal", True, True), what="eight inputs")
    assert (hit["sort"]["keys"], hit["sort"]["D"], hit["sort"]["bin_passes"]) == ("generic", 8, 2)


def test_two_inputs(xh):
    idx = bc.indices("random", 3, 2000, 12, seed=9)
    edges = bc.edges_for([4, 3])
    hit, _ = run_direct(xh, xc.emit(idx, edges, F32), sc.values("random", F32, 3, 2000, 48), edges, ("average", True, True), what="two inputs")
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
    got = guarded_rank(native, plan, views, vview, n_rows, n_cols, "average", False, True)
    ro.assert_variant(plan.describe(), ro.predict(_cus(), edges, 0, st, st, n_rows, n_cols, "average", False, True))
    want = ro.rank_rows(mo.index([flat[1:].reshape(n_rows, n_cols)], edges), vflat[1:].reshape(n_rows, n_cols), 50, "average", False, True)
    mo.assert_bits(got, want, "x[1:]")


@pytest.mark.parametrize("layout", ["row_broadcast", "transposed", "values_col_broadcast", "values_strided"])
def test_strided_views(xh, layout):
    """rows of samples broadcast at stride 0 (still the fast family) and a transposed block (row stride 1: the generic family),
    each with values laid out the same way; values broadcast along the columns (one tie run per bin) and values at a column
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
    mode = {"row_broadcast": ("dense", False, True), "transposed": ("max", True, False), "values_col_broadcast": ("average", False, False),
            "values_strided": ("min", True, True)}[layout]
    got = guarded_rank(native, plan, [native.make_view(x_t.data_ptr(), native.F64, rs, cs)],
                       native.make_view(v_t.data_ptr(), native.F64, vrs, vcs), n_rows, n_cols, *mode)
    fast = layout != "transposed"
    hit = ro.assert_variant(plan.describe(), ro.predict(_cus(), edges, 0, F64, F64, n_rows, n_cols, *mode, layout_fast=fast))
    assert hit["sort"]["keys"] == ("fast" if fast else "generic")
    want = ro.rank_rows(mo.index([np.ascontiguousarray(logical)], edges), np.ascontiguousarray(vlogical), 40, *mode)
    mo.assert_bits(got, want, layout)


# ---------------------------------------------------------------------------------------------------------------------
# 4. determinism: twice, and on two streams at once
# ---------------------------------------------------------------------------------------------------------------------
def test_twice_and_on_two_streams_at_once(xh):
    from xhistogram_amd import _native as native

    n_rows, n_cols, nb = 2, 60_000, 37
    edges = bc.edges_for([nb])
    x = xc.emit(bc.indices("random", n_rows, n_cols, nb, seed=12), edges, F64)[0]
    v = sc.values("random", F32, n_rows, n_cols, 45)
    x_t, v_t = _dev(x), _dev(v)
    plan = _plan_for(xh, [x], edges)
    views = [native.make_view(x_t.data_ptr(), native.F64, n_cols, 1)]
    vview = native.make_view(v_t.data_ptr(), native.F32, n_cols, 1)
    want = ro.rank_rows(mo.index([x], edges), v, nb, "average", False, True)
    first = guarded_rank(native, plan, views, vview, n_rows, n_cols, "average", False, True)
    second = guarded_rank(native, plan, views, vview, n_rows, n_cols, "average", False, True)
    mo.assert_bits(first, want, "first run")
    assert np.array_equal(first.view(np.int64), second.view(np.int64)), "the second run differs in its bits"
    streams = side_streams(2)
    outs = [torch.empty((n_rows, n_cols), dtype=torch.float64, device="cuda") for _ in streams]
    torch.cuda.synchronize()
    for _ in range(3):
        for s, o in zip(streams, outs):
            plan.execute_rank(views, vview, n_rows, n_cols, native.RANK_AVERAGE, False, True, o.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    for o in outs:
        mo.assert_bits(o.cpu().numpy(), want, "two streams")


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


def _want(x, v, edges, axis, *mode):
    """the oracle's ranks in the shape of x: rows over the kept axes, moved back"""
    idx = mo.index([x], [edges])
    rows, v_rows = bo.rows_of(idx, axis), bo.rows_of(v, axis)
    flat = ro.rank_rows(rows, v_rows, len(edges) - 1, *mode)
    if axis is None:
        return flat.reshape(x.shape)
    red = sorted(a % x.ndim for a in axis)
    kept = [i for i in range(x.ndim) if i not in red]
    full = flat.reshape([x.shape[i] for i in kept] + [x.shape[i] for i in red])
    return np.moveaxis(full, range(len(kept), x.ndim), red) if kept else full


@pytest.mark.parametrize("backend", ["torch", "numpy", "device"])
@pytest.mark.parametrize("axis", API_AXES, ids=[str(a) for a in API_AXES])
def test_public_api_backends_and_axes(xh, backend, axis):
    """a 3-D block over trailing, middle, leading and split axes (listed in both orders), three modes each: the oracle's bits in
    the inputs' shape"""
    from xhistogram_amd.devicearray import DeviceArray

    x, v, edges = _api_block()
    put = {"torch": lambda a: torch.as_tensor(a).cuda(), "numpy": lambda a: a, "device": lambda a: DeviceArray.from_numpy(a, 0)}[backend]
    xd, vd = put(x), put(v)
    kind = torch.Tensor if backend == "torch" else np.ndarray
    for mode in (("average", False, False), ("dense", True, True), ("ordinal", False, True)):
        rank, e = xh.bin_rank(xd, values=vd, bins=[edges], axis=axis, method=mode[0], descending=mode[1], pct=mode[2])
        assert isinstance(rank, kind) and tuple(rank.shape) == x.shape and np.array_equal(e[0], edges)
        assert _np(rank).dtype == np.float64
        mo.assert_bits(_np(rank), _want(x, v, edges, axis, *mode), "%s %s" % (axis, mode))


@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
def test_identities_with_the_librarys_own_results(xh, descending):
    """the ECDF and the percentile-of-score kinds from pct; ordinal against bin_sort; min rank 1 against histogram_extrema; the
    largest max rank against histogram_mean_var's count"""
    x, v, edges = _api_block(310, (6, 900))
    xd, vd = torch.as_tensor(x).cuda(), torch.as_tensor(v).cuda()
    kw = dict(values=vd, bins=[edges], axis=1, descending=descending)
    r = {(m, p): _np(xh.bin_rank(xd, method=m, pct=p, **kw)[0]) for m in ro.METHODS for p in (False, True)}
    idx = mo.index([x], [edges])
    ok = (idx >= 0) & ~np.isnan(v)
    count, _, _, _ = xh.histogram_mean_var(xd, values=vd, bins=[edges], axis=1)
    count = _np(count)
    vmin, vmax, _ = xh.histogram_extrema(xd, values=vd, bins=[edges], axis=1)
    extreme = _np(vmax if descending else vmin)
    order, offsets, _ = xh.bin_sort(xd, **kw)
    order, offsets = _np(order), _np(offsets)
    for row in range(x.shape[0]):
        n = count[row][np.maximum(idx[row], 0)].astype(F64)
        sel = ok[row]
        before = (v[row][None, :] > v[row][:, None]) if descending else (v[row][None, :] < v[row][:, None])
        same_bin = (idx[row][None, :] == idx[row][:, None]) & sel[None, :]
        le = ((before | (v[row][None, :] == v[row][:, None])) & same_bin).sum(1)
        lt = (before & same_bin).sum(1)
        mo.assert_bits(r["max", True][row][sel], (le / n)[sel], "the ECDF: percentileofscore(kind='weak') / 100")
        mo.assert_bits(((r["min", False][row] - 1) / n)[sel], (lt / n)[sel], "kind='strict'")
        mo.assert_bits((r["average", False][row] / n)[sel], ((lt + le + 1) / 2.0 / n)[sel], "kind='rank'")
        mo.assert_bits(r["average", True][row][sel], (r["average", False][row] / n)[sel], "pct is one division")
        i = np.arange(x.shape[1])
        at = np.searchsorted(offsets[row], i, side="right") - 1
        place = (i - offsets[row][np.minimum(at, 7)] + 1).astype(F64)
        got = r["ordinal", False][row][order[row]]
        keep = ~np.isnan(got)
        assert np.array_equal(keep, (at < 8) & ~np.isnan(v[row][order[row]]))
        mo.assert_bits(got[keep], place[keep], "ordinal is the place in bin_sort's segment")
        for b in range(8):
            inb = sel & (idx[row] == b)
            if not inb.any():
                assert count[row, b] == 0
                continue
            assert np.array_equal(r["min", False][row][inb] == 1, v[row][inb] == extreme[row, b])
            assert r["max", False][row][inb].max() == count[row, b]
    assert np.isnan(r["average", False][~ok]).all()


def test_values_broadcast_against_the_samples(xh):
    rng = np.random.default_rng(307)
    x = rng.uniform(-1.2, 1.2, (6, 400))
    v = rng.integers(-5, 6, (400,)).astype(np.int16)
    edges = [np.linspace(-1.0, 1.0, 9)]
    rank, _ = xh.bin_rank(torch.as_tensor(x).cuda(), values=torch.as_tensor(v).cuda(), bins=edges, axis=1, method="min")
    mo.assert_bits(_np(rank), ro.rank_rows(mo.index([x], edges), np.broadcast_to(v, x.shape), 8, "min"), "broadcast values")
    rank, _ = xh.bin_rank(x, values=2.5, bins=edges, axis=1, method="max", pct=True)  # a scalar: every counted sample ties
    assert np.array_equal(_np(rank) == 1.0, mo.index([x], edges) >= 0) and np.isnan(_np(rank)[mo.index([x], edges) < 0]).all()


@pytest.mark.parametrize("backend", ["torch", "numpy"])
def test_a_plan_without_bins(xh, backend):
    """one edge, no bin: no sample is counted and every rank is NaN; through Plan.execute_rank too, guard bands intact"""
    from xhistogram_amd import _native as native

    x = np.random.default_rng(302).uniform(-1.0, 1.0, (3, 1515))
    v = sc.values("random", F64, 3, 1515, 46)
    edges = [np.array([0.25])]
    put = (lambda a: torch.as_tensor(a).cuda()) if backend == "torch" else (lambda a: a)
    for pct in (False, True):
        rank, _ = xh.bin_rank(put(x), values=put(v), bins=edges, axis=1, pct=pct)
        assert _np(rank).shape == x.shape and _np(rank).dtype == np.float64 and np.isnan(_np(rank)).all()
    rank, _ = xh.bin_rank(put(x), values=put(v), bins=edges)
    assert _np(rank).shape == x.shape and np.isnan(_np(rank)).all()
    x_t, v_t = _dev(x), _dev(v)
    plan = _plan_for(xh, [x], edges)
    got = guarded_rank(native, plan, [native.make_view(x_t.data_ptr(), native.F64, 1515, 1)], native.make_view(v_t.data_ptr(), native.F64, 1515, 1),
                       3, 1515, "dense", True, True)
    assert np.isnan(got).all()


@pytest.mark.parametrize("backend", ["torch", "numpy"])
def test_extents_of_zero(xh, backend):
    edges = [np.linspace(0.0, 1.0, 5)]
    put = (lambda a: torch.as_tensor(a).cuda()) if backend == "torch" else (lambda a: a)
    for shape, axis in (((3, 0), 1), ((0, 7), 1), ((0,), None), ((2, 0, 3), (0, 2))):
        rank, _ = xh.bin_rank(put(np.zeros(shape)), values=put(np.zeros(shape)), bins=edges, axis=axis, pct=True)
        assert _np(rank).shape == shape and _np(rank).dtype == np.float64


def test_zero_columns_through_the_plan(xh):
    from xhistogram_amd import _native as native

    edges = bc.edges_for([4])
    x = np.zeros((3, 1))
    x_t = _dev(x)
    plan = _plan_for(xh, [x], edges)
    got = guarded_rank(native, plan, [native.make_view(x_t.data_ptr(), native.F64, 0, 1)], native.make_view(x_t.data_ptr(), native.F64, 0, 1),
                       3, 0, "max", False, True)
    assert got.shape == (3, 0)
    ro.assert_variant(plan.describe(), ro.predict(_cus(), edges, 0, F64, F64, 3, 0, "max", False, True))


def test_refusals(xh):
    from xhistogram_amd import _native as native

    x = torch.zeros(8, dtype=torch.float64, device="cuda")
    edges = [np.linspace(0.0, 1.0, 5)]
    with pytest.raises(TypeError, match="complex values have no order"):
        xh.bin_rank(x, values=torch.zeros(8, dtype=torch.complex64, device="cuda"), bins=edges)
    with pytest.raises(TypeError):
        xh.bin_rank(x, values=x, weights=x, bins=edges)
    with pytest.raises(TypeError, match="bin_rank needs values"):
        xh.bin_rank(x, values=None, bins=edges)
    with pytest.raises(ValueError, match="unknown rank method 'first'"):
        xh.bin_rank(x, values=x, bins=edges, method="first")
    with pytest.raises(TypeError, match="pct must be a bool"):
        xh.bin_rank(x, values=x, bins=edges, pct="yes")
    # the C ABI: an unknown method, a host call and a row of 2^31 columns end before any launch, and nothing is written
    plan = _plan_for(xh, [np.zeros((2, 4))], edges)
    xa = torch.zeros(8, dtype=torch.float64, device="cuda")
    out = torch.full((8,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    lib = native.load()
    view = native.make_view(xa.data_ptr(), native.F64, 4, 1)
    args = (plan._h, (native.XhistArray * 1)(view), C.byref(view), 2, 4)
    tail = (C.c_void_p(out.data_ptr()), native.MEM_DEVICE, C.c_void_p(0))
    for method in (-1, 5):
        assert lib.xhist_plan_execute_rank(*args, method, 0, 0, *tail) == native.ERR_INVALID
        assert "unknown rank method %d" % method in lib.xhist_last_error().decode()
    assert lib.xhist_plan_execute_rank(*args, 0, 0, 0, C.c_void_p(out.data_ptr()), native.MEM_HOST, C.c_void_p(0)) == native.ERR_INVALID
    assert "mem_kind XHIST_MEM_DEVICE" in lib.xhist_last_error().decode()
    assert lib.xhist_plan_execute_rank(plan._h, (native.XhistArray * 1)(view), C.byref(view), 1, 1 << 31, 0, 0, 0, *tail) == native.ERR_UNSUPPORTED
    assert "fewer than 2^31 samples per output row" in lib.xhist_last_error().decode()
    with pytest.raises(ValueError, match="unknown rank method 9"):
        plan.execute_rank([view], view, 2, 4, 9, False, False, out.data_ptr())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert lib.xhist_plan_execute_rank(*args, native.RANK_MAX, 0, 1, *tail) == native.OK
    torch.cuda.synchronize()
    assert bool((out == 1.0).all())  # (eight zeros in bin 0 of two rows: the ECDF of a tie of everything)


def test_eight_threads_on_one_plan(xh):
    edges = [np.linspace(-1.0, 1.0, 33)]
    rng = np.random.default_rng(303)
    xs = [rng.uniform(-1.1, 1.1, (3, 5000 + 17 * t)) for t in range(8)]
    vs = [sc.values("random", F32, 3, 5000 + 17 * t, 50 + t) for t in range(8)]
    modes = [rc.MODES[(5 * t + 1) % len(rc.MODES)] for t in range(8)]
    results, errors = [None] * 8, []
    streams = side_streams(8)

    def work(t):
        try:
            with torch.cuda.stream(streams[t]):
                for _ in range(3):
                    r, _e = xh.bin_rank(torch.as_tensor(xs[t]).cuda(), values=torch.as_tensor(vs[t]).cuda(), bins=edges, axis=1,
                                        method=modes[t][0], descending=modes[t][1], pct=modes[t][2])
                torch.cuda.current_stream().synchronize()
                results[t] = r.cpu().numpy()
        except Exception as err:  # noqa: BLE001
            errors.append(err)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(8):
        mo.assert_bits(results[t], ro.rank_rows(mo.index([xs[t]], edges), vs[t], 32, *modes[t]), "thread %d" % t)


def test_torch_results_follow_the_current_stream(xh):
    x = np.random.default_rng(304).uniform(-1.0, 1.0, 40_000)
    v = sc.values("random", F64, 1, 40_000, 47).reshape(-1)
    edges = [np.linspace(-1.0, 1.0, 101)]
    s = side_streams(1)[0]
    with torch.cuda.stream(s):
        rank, _ = xh.bin_rank(torch.as_tensor(x).cuda(), values=torch.as_tensor(v).cuda(), bins=edges, pct=True)
        s.synchronize()
        got = rank.cpu().numpy()
    mo.assert_bits(got, ro.rank_rows(mo.index([x], edges), v, 100, "average", False, True), "side stream")


def test_edges_from_a_bin_count_and_two_inputs(xh):
    rng = np.random.default_rng(305)
    x, y = rng.uniform(0, 1, (2, 4, 600))
    v = rng.integers(0, 9, (4, 600))
    rank, e = xh.bin_rank(torch.as_tensor(x).cuda(), torch.as_tensor(y).cuda(), values=torch.as_tensor(v).cuda(), bins=[4, 3], axis=1,
                          method="dense")
    edges = [np.asarray(b) for b in e]
    mo.assert_bits(_np(rank), ro.rank_rows(mo.index([x, y], edges), v, 12, "dense"), "two inputs")


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
    v = np.round(rng.standard_normal((4, 60)), 1)
    temp = xr.DataArray(x, dims=("time", "x"), coords={"time": np.arange(4.0)}, name="temp")
    oxy = xr.DataArray(v, dims=("time", "x"), coords={"time": np.arange(4.0)}, name="oxy")
    rank = xhx.bin_rank(temp, values=oxy, bins=[edges], dim=["x"], method="max", descending=True, pct=True)
    assert (rank.name, tuple(rank.dims)) == ("oxy_bin_rank", ("time", "x"))
    mo.assert_bits(np.asarray(rank.data), ro.rank_rows(mo.index([x], [edges]), v, 8, "max", True, True), "xarray")
    np.testing.assert_array_equal(np.asarray(rank["time"].data), np.arange(4.0))
    flat = xhx.bin_rank(temp, values=oxy, bins=[edges])
    assert tuple(flat.dims) == ("time", "x")
    mo.assert_bits(np.asarray(flat.data), ro.rank_rows(mo.index([x], [edges]).reshape(-1), v.reshape(-1), 8).reshape(4, 60), "flat")
    with pytest.raises(TypeError, match="accepts only xarray.DataArray"):
        xhx.bin_rank(x, values=oxy, bins=[edges])


def test_dask_branch(monkeypatch):
    """blocks over the kept axes give what the numpy call gives, bit for bit: tests/bin_rank_dask_script.py in the interpreter
    that has dask, started as tests/test_dask_branch.py starts its own script"""
    import test_dask_branch as tdb

    if not tdb._have_dask_python():
        pytest.skip("no interpreter with dask in this image")
    monkeypatch.setattr(tdb, "SCRIPT", os.path.join(ROOT, "tests", "bin_rank_dask_script.py"))
    assert "BIN-RANK-DASK-OK" in tdb._run("bin_rank")
