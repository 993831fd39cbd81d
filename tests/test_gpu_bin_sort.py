"""bin_sort on the GPU: every comparison is bit for bit against tests/bin_sort_oracle.py (np.lexsort over the oracle's bin
indices and core.extrema_keys), and every direct case asserts from the plan's describe() that it ran the geometry and the passes
the restatement predicts.

Direct cases go through Plan.execute_sort with both outputs inside one DeviceBuffer filled with a sentinel: lead | order |
gap | offsets | tail.  The sentinel must be intact in the lead, the gap and the tail and gone from every element of the two
blocks (no position and no offset can equal it).  The lead is odd in every second case, so the blocks start 8 bytes off 16-byte
alignment there.  The case tables are tests/bin_sort_cases.py's; tests/test_bin_sort_cpu.py holds them to what they claim."""
import os
import threading

import numpy as np
import pytest

import bin_order_cases as bc
import bin_order_oracle as bo
import bin_sort_cases as sc
import bin_sort_oracle as so
import extreme_cases as xc
import map_oracle as mo
from test_gpu_bin_order import side_streams
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


def _tag(native, dt):
    return native.dtype_tag(np.dtype(np.int64) if np.dtype(dt).kind in "mM" else dt)


def _dev(x):
    x = np.ascontiguousarray(x)
    return torch.as_tensor(x.view(np.int64) if x.dtype.kind in "mM" else x).cuda()


def _upload(native, a):
    """any dtype, torch's or not, as the bytes it is"""
    a = np.ascontiguousarray(a)
    buf = native.DeviceBuffer(0, max(a.nbytes, 8))
    if a.nbytes:
        buf.upload(a.view(np.uint8) if a.dtype == np.bool_ else a)
    return buf


def guarded_sort(native, plan, views, vview, n_rows, n_cols, n_bins, descending, stream=0):
    """Plan.execute_sort into the middle of a DeviceBuffer of sentinels -> (order [n_rows, n_cols], offsets [n_rows, n_bins + 1])"""
    CASE_NO[0] += 1
    lead, tail = 64 + CASE_NO[0] % 2, 64
    n, m = n_rows * n_cols, n_rows * (n_bins + 1)
    host = np.full(lead + n + GAP + m + tail, SENTINEL, np.int64)
    buf = native.DeviceBuffer(0, host.nbytes)
    buf.upload(host)
    torch.cuda.synchronize()
    plan.execute_sort(views, vview, n_rows, n_cols, descending, buf.ptr + 8 * lead, buf.ptr + 8 * (lead + n + GAP), stream=stream)
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


def run_direct(core, xs, v, edges, descending, cmp=0, what="", layout_fast=True, want=None):
    """contiguous [R, C] host arrays through Plan.execute_sort: the describe() line, the guard bands, the oracle's bits"""
    from xhistogram_amd import _native as native

    n_rows, n_cols = xs[0].shape
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    xs_t = [_dev(x) for x in xs]
    vb = _upload(native, v)
    plan = _plan_for(core, xs, edges)
    views = [native.make_view(t.data_ptr(), _tag(native, x.dtype), n_cols, 1) for t, x in zip(xs_t, xs)]
    vview = native.make_view(vb.ptr, _tag(native, v.dtype), n_cols, 1)
    order, offsets = guarded_sort(native, plan, views, vview, n_rows, n_cols, n_bins, descending)
    hit = so.assert_variant(plan.describe(), so.predict(_cus(), edges, cmp, xs[0].dtype, v.dtype, n_rows, n_cols, layout_fast=layout_fast))
    if want is None:
        want = so.order_offsets(mo.index(xs, edges), v, n_bins, descending)
    mo.assert_bits(offsets, want[1], what + " offsets")
    mo.assert_bits(order, want[0], what + " order")
    vb.close()
    return hit, order, offsets


# ---------------------------------------------------------------------------------------------------------------------
# 1. the case tables: sizes around a step and a chunk, slices, value patterns, value dtypes, bin counts, both directions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
@pytest.mark.parametrize("case", sc.gpu_cases(sc.CUS), ids=lambda c: c["name"])
def test_case_table(xh, case, descending):
    cus = _cus()
    edges, idx, xs, v = sc.case_data(case, cus)
    sc.check_claims(case, idx, v, cus)
    hit, order, offsets = run_direct(xh, xs, v, edges, descending, what=case["name"])
    assert hit["keys"] == "fast"
    name = so.DTYPE_NAME[case["vt"]]
    assert (hit["value_passes"], hit["bin_passes"], hit["vdtype"]) == (so.value_passes(name), so.bin_passes(int(np.prod(case["nbs"]))), name)
    n_bins = int(np.prod(case["nbs"]))
    if "all values equal" in case["claims"]:  # every value pass is an identity: bin_order's result
        grouped = bo.order_offsets(idx, n_bins)
        mo.assert_bits(order, grouped[0], "bin_order's order")
        mo.assert_bits(offsets, grouped[1], "bin_order's offsets")
    if n_bins <= bo.MAX_BINS and case["n_cols"] <= 5000:  # the offsets are bin_order's own, from the library
        from xhistogram_amd import _native as native

        plan = _plan_for(xh, xs, edges)
        got = torch.empty(case["n_rows"] * (case["n_cols"] + n_bins + 1), dtype=torch.int64, device="cuda")
        xs_t = [_dev(x) for x in xs]
        views = [native.make_view(t.data_ptr(), _tag(native, x.dtype), case["n_cols"], 1) for t, x in zip(xs_t, xs)]
        plan.execute_group(views, case["n_rows"], case["n_cols"], got.data_ptr(), got.data_ptr() + 8 * idx.size)
        torch.cuda.synchronize()
        mo.assert_bits(got[idx.size:].cpu().numpy().reshape(offsets.shape), offsets, "offsets against execute_group")


def test_more_rows_than_one_launch(xh):
    """one launch's rows and five more, two samples each in one bin: every row past the first batch is written, from its own
    records into its own rows of both blocks"""
    g = so.geometry(_cus(), 1 << 25, 2)
    n_rows = g["rows_per_launch"] + 5
    assert g["chunks"] == 1 and n_rows < (1 << 20)
    rng = np.random.default_rng(5)
    x = rng.integers(0, 3, (n_rows, 2)).astype(F32) - 0.5  # -0.5: dropped, 0.5: the bin, 1.5: dropped
    v = rng.integers(0, 2, (n_rows, 2)).astype(np.uint8)
    edges = [np.array([0.0, 1.0])]
    key = bo.keys_of(mo.index([x], edges), 1)
    vk = v.astype(np.int64)
    swap = (key[:, 0] > key[:, 1]) | ((key[:, 0] == key[:, 1]) & (vk[:, 0] > vk[:, 1]))  # the closed form of a row of two
    want_order = np.where(swap[:, None], [1, 0], [0, 1]).astype(np.int64)
    want_offsets = np.stack([np.zeros(n_rows, np.int64), (key == 0).sum(1)], 1)
    hit, _, _ = run_direct(xh, [x], v, edges, False, what="row batches", want=(want_order, want_offsets))
    assert hit["rows_per_launch"] == g["rows_per_launch"] < n_rows
    sel = slice(n_rows - 300, n_rows)
    got = so.order_offsets(mo.index([x[sel]], edges), v[sel], 1)
    np.testing.assert_array_equal(got[0], want_order[sel])
    np.testing.assert_array_equal(got[1], want_offsets[sel])


# ---------------------------------------------------------------------------------------------------------------------
# 2. both families of bin_index in step 0: compare domains, sample types, input counts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dom", ["f64", "i64", "mixed"])
def test_generic_keys(xh, dom):
    """int32 samples on float64 edges (domain 0), int64 on int64 (1), int64 next to float64 (3): the generic family makes the keys"""
    for i, (n_rows, n_cols) in enumerate(((3, 1500), (1, 4000))):
        edges, xs, cmp = generic_inputs(dom, 100, n_rows, n_cols, 900 + i)
        v = sc.values("random", [F64, np.int32][i], n_rows, n_cols, 40 + i)
        hit, _, _ = run_direct(xh, xs, v, edges, bool(i), cmp=cmp, what="%s %dx%d" % (dom, n_rows, n_cols))
        assert hit["keys"] == "generic" and hit["cmp"] == cmp and hit["D"] == len(edges)


def test_datetime_samples(xh):
    t0 = np.datetime64("2020-01-01", "s")
    edges = [t0 + np.arange(0, 25 * 3600, 3600).astype("timedelta64[s]")]
    x = t0 + np.random.default_rng(7).integers(-4000, 26 * 3600, (2, 3000)).astype("timedelta64[s]")
    hit, _, _ = run_direct(xh, [x], sc.values("random", F32, 2, 3000, 41), edges, False, cmp=1, what="datetime64[s]")
    assert hit["keys"] == "generic"


def test_eight_inputs_of_three_bins(xh):
    idx = bc.indices("random", 2, 3000, 3 ** 8, seed=8)
    edges = bc.edges_for([3] * 8)
    xs = xc.emit(idx, edges, F64)
    hit, _, _ = run_direct(xh, xs, sc.values("random", F64, 2, 3000, 42), edges, True, what="eight inputs")
    assert (hit["keys"], hit["D"], hit["bin_passes"]) == ("generic", 8, 2)


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
    order, offsets = guarded_sort(native, plan, views, vview, n_rows, n_cols, 50, False)
    so.assert_variant(plan.describe(), so.predict(_cus(), edges, 0, st, st, n_rows, n_cols))
    want = so.order_offsets(mo.index([flat[1:].reshape(n_rows, n_cols)], edges), vflat[1:].reshape(n_rows, n_cols), 50)
    mo.assert_bits(order, want[0], "x[1:] order")
    mo.assert_bits(offsets, want[1], "x[1:] offsets")


@pytest.mark.parametrize("layout", ["row_broadcast", "transposed", "values_col_broadcast", "values_strided"])
def test_strided_views(xh, layout):
    """rows of samples broadcast at stride 0 (still the fast family) and a transposed block (row stride 1: the generic family),
    each with values laid out the same way; values broadcast along the columns and values at a column stride of 3"""
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
        if layout == "values_col_broadcast":  # one value per row: every tie is broken by position
            vbase = np.ascontiguousarray(vals[:, :1])
            vlogical, (vrs, vcs) = np.broadcast_to(vbase, (n_rows, n_cols)), (1, 0)
        else:
            vbase = vals
            vlogical, (vrs, vcs) = vals[:, ::3], (3 * n_cols, 3)
    x_t, v_t = _dev(base), _dev(vbase)
    plan = _plan_for(xh, [base], edges)
    order, offsets = guarded_sort(native, plan, [native.make_view(x_t.data_ptr(), native.F64, rs, cs)],
                                  native.make_view(v_t.data_ptr(), native.F64, vrs, vcs), n_rows, n_cols, 40, layout == "transposed")
    fast = layout != "transposed"
    hit = so.assert_variant(plan.describe(), so.predict(_cus(), edges, 0, F64, F64, n_rows, n_cols, layout_fast=fast))
    assert hit["keys"] == ("fast" if fast else "generic")
    want = so.order_offsets(mo.index([np.ascontiguousarray(logical)], edges), np.ascontiguousarray(vlogical), 40, layout == "transposed")
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
    v = sc.values("random", F32, n_rows, n_cols, 45)
    x_t, v_t = _dev(x), _dev(v)
    plan = _plan_for(xh, [x], edges)
    views = [native.make_view(x_t.data_ptr(), native.F64, n_cols, 1)]
    vview = native.make_view(v_t.data_ptr(), native.F32, n_cols, 1)
    want = so.order_offsets(mo.index([x], edges), v, nb)
    first = guarded_sort(native, plan, views, vview, n_rows, n_cols, nb, False)
    second = guarded_sort(native, plan, views, vview, n_rows, n_cols, nb, False)
    for a, b, w in zip(first, second, want):
        mo.assert_bits(a, w, "first run")
        mo.assert_bits(b, a, "second run")
    streams = side_streams(2)
    outs = [(torch.empty((n_rows, n_cols), dtype=torch.int64, device="cuda"), torch.empty((n_rows, nb + 1), dtype=torch.int64, device="cuda"))
            for _ in streams]
    torch.cuda.synchronize()
    for _ in range(3):
        for s, (o, f) in zip(streams, outs):
            plan.execute_sort(views, vview, n_rows, n_cols, False, o.data_ptr(), f.data_ptr(), stream=s.cuda_stream)
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
    with the library's own bin_order, histogram, histogram_extrema, histogram_argextrema and histogram_quantile"""
    from xhistogram_amd.devicearray import DeviceArray

    rng = np.random.default_rng(300)
    shape = (5, 37, 11)
    edges = np.linspace(-1.0, 1.0, 9)
    x = rng.uniform(-1.2, 1.2, shape)
    x[rng.random(shape) < 0.05] = np.nan
    v = np.round(rng.standard_normal(shape) * 3, 0)  # (ties)
    v[rng.random(shape) < 0.05] = np.nan
    v[rng.random(shape) < 0.05] = -0.0
    put = {"torch": lambda a: torch.as_tensor(a).cuda(), "numpy": lambda a: a, "device": lambda a: DeviceArray.from_numpy(a, 0)}[backend]
    xd, vd = put(x), put(v)
    kind = torch.Tensor if backend == "torch" else np.ndarray
    idx = mo.index([x], [edges])
    rows, v_rows = bo.rows_of(idx, axis), bo.rows_of(v, axis)
    flat_rows, flat_v = rows.reshape(-1, rows.shape[-1]), v_rows.reshape(-1, rows.shape[-1])

    grouped, grouped_offsets, _ = xh.bin_order(xd, bins=[edges], axis=axis)
    grouped = _np(grouped).reshape(flat_rows.shape)
    h, _ = xh.histogram(xd, bins=[edges], axis=axis)
    vmin, vmax, _ = xh.histogram_extrema(xd, values=vd, bins=[edges], axis=axis)
    arg = xh.histogram_argextrema(xd, values=vd, bins=[edges], axis=axis)
    argmin, argmax = _np(arg[0]).reshape(-1, 8), _np(arg[1]).reshape(-1, 8)
    qs = [0.0, 0.3, 0.5, 1.0]
    quant, _ = xh.histogram_quantile(xd, values=vd, q=qs, bins=[edges], axis=axis, method="lower")
    quant = _np(quant).reshape(len(qs), -1, 8)
    ext = {False: (_np(vmin).reshape(-1, 8), argmin), True: (_np(vmax).reshape(-1, 8), argmax)}

    for descending in (False, True):
        order, offsets, e = xh.bin_sort(xd, values=vd, bins=[edges], axis=axis, descending=descending)
        assert isinstance(order, kind) and isinstance(offsets, kind) and np.array_equal(e[0], edges)
        order, offsets = _np(order), _np(offsets)
        want_order, want_offsets = so.order_offsets(rows, v_rows, 8, descending)
        mo.assert_bits(order, want_order, "order")
        mo.assert_bits(offsets, want_offsets, "offsets")
        mo.assert_bits(offsets, _np(grouped_offsets), "bin_order's offsets")
        np.testing.assert_array_equal(np.diff(offsets, axis=-1), _np(h))
        flat_order, flat_offsets = order.reshape(flat_rows.shape), offsets.reshape(-1, 9)
        for r in range(flat_order.shape[0]):
            so.assert_sorted(flat_order[r], flat_offsets[r], flat_rows[r], flat_v[r], 8, descending, "row %d" % r)
            for b in range(9):
                seg = slice(flat_offsets[r][b], flat_offsets[r][b + 1] if b < 8 else None)
                np.testing.assert_array_equal(np.sort(flat_order[r][seg]), grouped[r][seg])  # bin_order's segment
                if b == 8:
                    continue
                sv = flat_v[r][flat_order[r][seg]]
                n = int((~np.isnan(sv)).sum())
                if n == 0:
                    assert np.isnan(ext[descending][0][r, b]) and ext[descending][1][r, b] == -1
                    continue
                mo.assert_bits(sv[:1], ext[descending][0][r, b:b + 1], "the first of the bin is the extreme")
                assert flat_order[r][seg][0] == ext[descending][1][r, b]
                if not descending:
                    for qi, q in enumerate(qs):
                        # floor(q * (n - 1)) as histogram_quantile's "lower" takes it, from the same float64 product
                        at = int(np.floor(np.float64(q) * np.float64(n - 1)))
                        mo.assert_bits(sv[at:at + 1], quant[qi, r, b:b + 1], "quantile lower q=%s" % q)


def test_both_listings_of_the_axes_give_the_same(xh):
    rng = np.random.default_rng(301)
    x = torch.as_tensor(rng.uniform(-1.2, 1.2, (4, 9, 13))).cuda()
    v = torch.as_tensor(rng.integers(-3, 4, (4, 9, 13))).cuda()
    a = xh.bin_sort(x, values=v, bins=[np.linspace(-1, 1, 6)], axis=(0, 2))
    b = xh.bin_sort(x, values=v, bins=[np.linspace(-1, 1, 6)], axis=(2, 0))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_values_broadcast_against_the_samples(xh):
    rng = np.random.default_rng(307)
    x = rng.uniform(-1.2, 1.2, (6, 400))
    v = rng.integers(-5, 6, (400,)).astype(np.int16)
    edges = [np.linspace(-1.0, 1.0, 9)]
    order, offsets, _ = xh.bin_sort(torch.as_tensor(x).cuda(), values=torch.as_tensor(v).cuda(), bins=edges, axis=1)
    want = so.order_offsets(mo.index([x], edges), np.broadcast_to(v, x.shape), 8)
    mo.assert_bits(_np(order), want[0], "order")
    mo.assert_bits(_np(offsets), want[1], "offsets")
    order, offsets, _ = xh.bin_sort(x, values=2.5, bins=edges, axis=1)  # a scalar: bin_order
    grouped = bo.order_offsets(mo.index([x], edges), 8)
    mo.assert_bits(order, grouped[0], "scalar values order")
    mo.assert_bits(offsets, grouped[1], "scalar values offsets")


@pytest.mark.parametrize("backend", ["torch", "numpy"])
def test_a_plan_without_bins(xh, backend):
    """one edge, no bin: every sample is dropped, offsets == [0] and the whole row is sorted by value; through Plan.execute_sort too"""
    x = np.random.default_rng(302).uniform(-1.0, 1.0, (3, 1515))
    v = sc.values("random", F64, 3, 1515, 46)
    edges = [np.array([0.25])]
    put = (lambda a: torch.as_tensor(a).cuda()) if backend == "torch" else (lambda a: a)
    for descending in (False, True):
        order, offsets, _ = xh.bin_sort(put(x), values=put(v), bins=edges, axis=1, descending=descending)
        assert _np(order).dtype == _np(offsets).dtype == np.int64
        want = so.order_offsets(np.full(x.shape, -1), v, 0, descending)
        mo.assert_bits(_np(order), want[0], "order")
        np.testing.assert_array_equal(_np(offsets), np.zeros((3, 1), np.int64))
    order, offsets, _ = xh.bin_sort(put(x), values=put(v), bins=edges)
    mo.assert_bits(_np(order), so.order_offsets(np.full(x.size, -1), v.reshape(-1), 0)[0], "flat order")
    np.testing.assert_array_equal(_np(offsets), [0])
    v32 = v.astype(F32)
    hit, _, _ = run_direct(xh, [x], v32, edges, False, what="no bins",
                           want=(so.order_offsets(np.full(x.shape, -1), v32, 0)[0], np.zeros((3, 1), np.int64)))
    assert (hit["keys"], hit["bin_passes"], hit["value_passes"], hit["chunks"]) == ("none", 0, 5, 2)


@pytest.mark.parametrize("backend", ["torch", "numpy"])
def test_extents_of_zero(xh, backend):
    edges = [np.linspace(0.0, 1.0, 5)]
    put = (lambda a: torch.as_tensor(a).cuda()) if backend == "torch" else (lambda a: a)
    order, offsets, _ = xh.bin_sort(put(np.zeros((3, 0))), values=put(np.zeros((3, 0))), bins=edges, axis=1)  # c == 0
    assert _np(order).shape == (3, 0) and _np(order).dtype == np.int64
    np.testing.assert_array_equal(_np(offsets), np.zeros((3, 5), np.int64))
    order, offsets, _ = xh.bin_sort(put(np.zeros((0, 7))), values=put(np.zeros((0, 7))), bins=edges, axis=1)  # no kept index
    assert _np(order).shape == (0, 7) and _np(offsets).shape == (0, 5)
    order, offsets, _ = xh.bin_sort(put(np.zeros((0,))), values=put(np.zeros((0,))), bins=edges)
    assert _np(order).shape == (0,)
    np.testing.assert_array_equal(_np(offsets), np.zeros(5, np.int64))


def test_zero_columns_through_the_plan(xh):
    from xhistogram_amd import _native as native

    edges = bc.edges_for([4])
    x = np.zeros((3, 1))
    x_t = _dev(x)
    plan = _plan_for(xh, [x], edges)
    got = guarded_sort(native, plan, [native.make_view(x_t.data_ptr(), native.F64, 0, 1)], native.make_view(x_t.data_ptr(), native.F64, 0, 1),
                       3, 0, 4, False)
    assert got[0].shape == (3, 0) and (got[1] == 0).all()
    so.assert_variant(plan.describe(), so.predict(_cus(), edges, 0, F64, F64, 3, 0))


def test_refusals(xh):
    x = torch.zeros(8, dtype=torch.float64, device="cuda")
    edges = [np.linspace(0.0, 1.0, 5)]
    with pytest.raises(TypeError, match="complex values have no order"):
        xh.bin_sort(x, values=torch.zeros(8, dtype=torch.complex64, device="cuda"), bins=edges)
    with pytest.raises(TypeError):
        xh.bin_sort(x, values=x, weights=x, bins=edges)
    with pytest.raises(TypeError, match="bin_sort needs values"):
        xh.bin_sort(x, values=None, bins=edges)
    # one bin past bin_order's bound: refused there, sorted here
    many = [np.linspace(0.0, 1.0, bo.MAX_BINS + 2)]
    with pytest.raises(NotImplementedError, match="at most %d bins" % bo.MAX_BINS):
        xh.bin_order(x, bins=many)
    order, offsets, _ = xh.bin_sort(x, values=x, bins=many)
    assert _np(order).tolist() == list(range(8)) and _np(offsets).shape == (bo.MAX_BINS + 2,)


def test_eight_threads_on_one_plan(xh):
    edges = [np.linspace(-1.0, 1.0, 33)]
    rng = np.random.default_rng(303)
    xs = [rng.uniform(-1.1, 1.1, (3, 5000 + 17 * t)) for t in range(8)]
    vs = [sc.values("random", F32, 3, 5000 + 17 * t, 50 + t) for t in range(8)]
    results, errors = [None] * 8, []
    streams = side_streams(8)

    def work(t):
        try:
            with torch.cuda.stream(streams[t]):
                for _ in range(3):
                    o, f, _e = xh.bin_sort(torch.as_tensor(xs[t]).cuda(), values=torch.as_tensor(vs[t]).cuda(), bins=edges, axis=1,
                                           descending=bool(t % 2))
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
        want = so.order_offsets(mo.index([xs[t]], edges), vs[t], 32, bool(t % 2))
        mo.assert_bits(results[t][0], want[0], "thread %d order" % t)
        mo.assert_bits(results[t][1], want[1], "thread %d offsets" % t)


def test_torch_results_follow_the_current_stream(xh):
    x = np.random.default_rng(304).uniform(-1.0, 1.0, 40_000)
    v = sc.values("random", F64, 1, 40_000, 47).reshape(-1)
    edges = [np.linspace(-1.0, 1.0, 101)]
    s = side_streams(1)[0]
    with torch.cuda.stream(s):
        order, offsets, _ = xh.bin_sort(torch.as_tensor(x).cuda(), values=torch.as_tensor(v).cuda(), bins=edges)
        s.synchronize()
        got = order.cpu().numpy(), offsets.cpu().numpy()
    want = so.order_offsets(mo.index([x], edges), v, 100)
    mo.assert_bits(got[0], want[0], "side stream order")
    mo.assert_bits(got[1], want[1], "side stream offsets")


def test_edges_from_a_bin_count_and_two_inputs(xh):
    rng = np.random.default_rng(305)
    x, y = rng.uniform(0, 1, (2, 4, 600))
    v = rng.integers(0, 9, (4, 600))
    order, offsets, e = xh.bin_sort(torch.as_tensor(x).cuda(), torch.as_tensor(y).cuda(), values=torch.as_tensor(v).cuda(), bins=[4, 3], axis=1)
    edges = [np.asarray(b) for b in e]
    want = so.order_offsets(mo.index([x, y], edges), v, 12)
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
    v = np.round(rng.standard_normal((4, 60)), 1)
    temp = xr.DataArray(x, dims=("time", "x"), coords={"time": np.arange(4.0)}, name="temp")
    oxy = xr.DataArray(v, dims=("time", "x"), coords={"time": np.arange(4.0)}, name="oxy")
    order, offsets = xhx.bin_sort(temp, values=oxy, bins=[edges], dim=["x"], descending=True)
    assert (order.name, tuple(order.dims)) == ("oxy_bin_sort", ("time", "oxy_order"))
    assert (offsets.name, tuple(offsets.dims)) == ("oxy_bin_offsets", ("time", "oxy_bin_offset"))
    want = so.order_offsets(mo.index([x], [edges]), v, 8, True)
    mo.assert_bits(np.asarray(order.data), want[0], "xarray order")
    mo.assert_bits(np.asarray(offsets.data), want[1], "xarray offsets")
    np.testing.assert_array_equal(np.asarray(order["time"].data), np.arange(4.0))
    flat_order, flat_offsets = xhx.bin_sort(temp, values=oxy, bins=[edges])
    assert tuple(flat_order.dims) == ("oxy_order",) and tuple(flat_offsets.dims) == ("oxy_bin_offset",)
    mo.assert_bits(np.asarray(flat_order.data), so.order_offsets(mo.index([x], [edges]).reshape(-1), v.reshape(-1), 8)[0], "flat order")
    with pytest.raises(TypeError, match="accepts only xarray.DataArray"):
        xhx.bin_sort(x, values=oxy, bins=[edges])


def test_dask_branch(monkeypatch):
    """blocks over the kept axes give what the numpy call gives, bit for bit: tests/bin_sort_dask_script.py in the interpreter
    that has dask, started as tests/test_dask_branch.py starts its own script"""
    import test_dask_branch as tdb

    if not tdb._have_dask_python():
        pytest.skip("no interpreter with dask in this image")
    monkeypatch.setattr(tdb, "SCRIPT", os.path.join(ROOT, "tests", "bin_sort_dask_script.py"))
    assert "BIN-SORT-DASK-OK" in tdb._run("bin_sort")
