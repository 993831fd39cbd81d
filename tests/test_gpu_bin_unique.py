"""bin_unique on the GPU: every comparison is bit for bit against tests/bin_unique_oracle.py (tests/bin_rank_oracle.py's sorted
domain, the runs of non-NaN values of each bin, the cut at `size` and the padding), int64 by value and `uniques` by its bit
pattern, and every direct case asserts from the plan's describe() that it ran the words and the sort the restatement predicts.

Direct cases go through Plan.execute_unique with all outputs as one block inside a DeviceBuffer filled with a sentinel:
lead | uniques | counts | offsets | inverse | tail, the inverse block absent (and its pointer NULL) in a call without one, so that
the tail then starts right behind the offsets.  The sentinel must be intact in the lead and the tail and gone from every element
of the block; 0x5A5A... is neither 0, -1 nor a NaN, so no result is mistaken for it.  The lead is odd in every second case, so
the block starts 8 bytes off 16-byte alignment there.  A row's uniques and counts are exactly `size` wide, so an entry stored
past the width would land in the next row or the next block and differ from the oracle there.  The case tables are
tests/bin_unique_cases.py's; tests/test_bin_unique_cpu.py holds them to what they claim."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import bin_order_cases as bc
import bin_order_oracle as bo
import bin_sort_cases as sc
import bin_sort_oracle as so
import bin_unique_cases as uc
import bin_unique_oracle as uo
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
ONES = 0xFFFFFFFFFFFFFFFF
CASE_NO = [0]


def guarded_unique(native, plan, views, vview, n_rows, n_cols, size, inverse, stream=0, fill=SENTINEL):
    """Plan.execute_unique into the middle of a DeviceBuffer of `fill` -> (uniques [n_rows, size], counts [n_rows, size], offsets
    [n_rows, bins + 1][, inverse [n_rows, n_cols]])"""
    CASE_NO[0] += 1
    lead, tail = 64 + CASE_NO[0] % 2, 64
    nb1 = plan.n_bins + 1
    parts = [n_rows * size, n_rows * size, n_rows * nb1] + ([n_rows * n_cols] if inverse else [])
    at = np.concatenate([[0], np.cumsum(parts)]) + lead
    host = np.full(int(at[-1]) + tail, fill, np.uint64).view(np.int64)
    guard = host[0]
    buf = native.DeviceBuffer(0, host.nbytes)
    buf.upload(host)
    torch.cuda.synchronize()
    ptrs = [buf.ptr + 8 * int(a) for a in at[:-1]]
    plan.execute_unique(views, vview, n_rows, n_cols, size, ptrs[0], ptrs[1], ptrs[2], ptrs[3] if inverse else None, stream=stream)
    torch.cuda.synchronize()
    buf.download(host)
    buf.close()
    assert (host[:lead] == guard).all() and (host[at[-1]:] == guard).all(), "the guard bands were written"
    block = host[lead:at[-1]]
    if fill == SENTINEL:
        assert not (block == guard).any(), "%d elements were never written" % (block == guard).sum()
    shapes = [(n_rows, size), (n_rows, size), (n_rows, nb1), (n_rows, n_cols)]
    out = [host[at[i]:at[i + 1]].reshape(shapes[i]).copy() for i in range(len(parts))]
    out[0] = out[0].view(np.float64)
    return tuple(out)


def want_of(idx, v, n_bins, size, inverse):
    w = uo.unique_rows(idx, v, n_bins, size)
    return w if inverse else w[:3]


def run_direct(core, xs, v, edges, size=None, inverse=True, cmp=0, what="", layout_fast=True, want=None, fill=SENTINEL):
    """contiguous [R, C] host arrays through Plan.execute_unique: the describe() line, the guard bands, the oracle's bits"""
    from xhistogram_amd import _native as native

    n_rows, n_cols = xs[0].shape
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    width = n_cols if size is None else size
    xs_t = [_dev(x) for x in xs]
    vb = _upload(native, v)
    plan = _plan_for(core, xs, edges)
    views = [native.make_view(t.data_ptr(), _tag(native, x.dtype), n_cols, 1) for t, x in zip(xs_t, xs)]
    vview = native.make_view(vb.ptr, _tag(native, v.dtype), n_cols, 1)
    got = guarded_unique(native, plan, views, vview, n_rows, n_cols, width, inverse, fill=fill)
    hit = uo.assert_variant(plan.describe(), uo.predict(_cus(), edges, cmp, xs[0].dtype, v.dtype, n_rows, n_cols, width, inverse,
                                                        layout_fast=layout_fast))
    if want is None:
        want = want_of(mo.index(xs, edges), v, n_bins, width, inverse)
    uo.assert_same(got, want, what)
    vb.close()
    return hit, got


# ---------------------------------------------------------------------------------------------------------------------
# 1. the case tables: where runs, bin borders and segment ends fall among the words; sizes; dtypes; bin counts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", uc.gpu_cases(uc.CUS), ids=lambda c: c["name"])
def test_case_table(xh, case):
    cus = _cus()
    edges, idx, xs, v = uc.case_data(case, cus)
    uc.check_claims(case, idx, v, cus)
    hit, got = run_direct(xh, xs, v, edges, inverse=case["inverse"], what=case["name"])
    assert hit["words"] == -(-case["n_cols"] // 64) and hit["size"] == case["n_cols"] and hit["inverse"] == int(case["inverse"])
    assert hit["sort"]["vdtype"] == so.DTYPE_NAME[case["vt"]] and hit["sort"]["bin_passes"] == so.bin_passes(int(np.prod(case["nbs"])))
    if any(c.endswith("(U = 0)") for c in case["claims"]):
        assert not got[2].any() and not got[1].any() and (got[0].view(np.uint64) == uo.NAN_BITS).all()


def test_more_rows_than_one_launch(xh):
    """one launch's rows and five more, two samples each in two bins, with 0, 1 or 2 entries per row: every row past the first
    batch takes its own words, offsets, padding start and inverse, against the closed form of a row of two"""
    g = so.geometry(_cus(), 1 << 25, 2)
    n_rows = g["rows_per_launch"] + 5
    assert g["chunks"] == 1 and n_rows < (1 << 20)
    rng = np.random.default_rng(5)
    x = rng.integers(0, 4, (n_rows, 2)).astype(F32) - 0.5  # -0.5: dropped, 0.5: bin 0, 1.5: bin 1, 2.5: dropped
    v = rng.integers(0, 2, (n_rows, 2)).astype(np.uint8)
    edges = [np.array([0.0, 1.0, 2.0])]
    idx = mo.index([x], edges)
    big = 99
    key = np.where(idx >= 0, idx * 2 + v, big)  # (bin, value) in one number
    k0, k1 = key.min(1), key.max(1)
    two = (k1 < big) & (k1 != k0)
    total = (k0 < big).astype(np.int64) + two
    ent = np.stack([k0, np.where(two, k1, big)], 1)  # a row's entries, `big`: padding
    uniques = np.where(ent < big, (ent % 2).astype(F64), uo.PAD)
    counts = np.where(ent < big, (key[:, :, None] == ent[:, None, :]).sum(1), 0)
    offsets = np.stack([np.zeros(n_rows, np.int64), ((ent < big) & (ent < 2)).sum(1), total], 1)
    inverse = np.where(key < big, (key != k0[:, None]).astype(np.int64), -1)
    want = (uniques, counts, offsets, inverse)
    hit, _ = run_direct(xh, [x], v, edges, what="row batches", want=want)
    assert hit["rows_per_launch"] == g["rows_per_launch"] < n_rows and set(total[-5:]) | set(total[:5]) <= {0, 1, 2} and len(set(total)) == 3
    sel = slice(n_rows - 300, n_rows)
    uo.assert_same(uo.unique_rows(idx[sel], v[sel], 2), tuple(w[sel] for w in want), "the closed form")


# ---------------------------------------------------------------------------------------------------------------------
# 2. size: the cut and the padding
# ---------------------------------------------------------------------------------------------------------------------
def _tie_block(n_rows, n_cols, nb, seed, cats=10):
    edges = bc.edges_for([nb])
    x = xc.emit(bc.indices("random", n_rows, n_cols, nb, seed=seed), edges, F64)[0]
    rng = np.random.default_rng(seed)
    v = rng.integers(0, cats, (n_rows, n_cols)).astype(F32)  # a few categories: many runs
    v[rng.random(v.shape) < 0.05] = np.nan
    return edges, x, v


def test_sizes_around_the_number_of_entries(xh):
    """size in {None, 0, 1, U - 1, U, U + 1, c + 7} for a row with 1 < U < c, three rows of different U: the cut leaves offsets
    and inverse as they are, and nothing is stored past the width"""
    edges, x, v = _tie_block(3, 700, 13, 21)
    v[1] = np.where(v[1] > 3, 3, v[1])  # (rows 1 and 2 have fewer entries, row 2 more NaNs)
    v[2] = np.where(v[2] > 6, 6, v[2])
    v[2, ::3] = np.nan
    idx = mo.index([x], edges)
    full = uo.unique_rows(idx, v, 13)
    totals = full[2][:, -1]
    assert len(set(totals)) == 3 and all(1 < t < 700 for t in totals)
    for size in uc.sizes_for(int(totals[0]), 700):
        for inverse in (True, False):
            hit, got = run_direct(xh, [x], v, edges, size=size, inverse=inverse, what="size=%s inverse=%s" % (size, inverse))
            np.testing.assert_array_equal(got[2], full[2])
            if inverse:
                np.testing.assert_array_equal(got[3], full[3])
            assert hit["size"] == (700 if size is None else size)


# ---------------------------------------------------------------------------------------------------------------------
# 3. both families of bin_index in the sort's step 0: compare domains, sample types, input counts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dom", ["f64", "i64", "mixed"])
def test_generic_keys(xh, dom):
    """int32 samples on float64 edges (domain 0), int64 on int64 (1), int64 next to float64 (3): the generic family makes the keys"""
    for i, (n_rows, n_cols) in enumerate(((3, 1500), (1, 4000))):
        edges, xs, cmp = generic_inputs(dom, 100, n_rows, n_cols, 900 + i)
        v = np.random.default_rng(40 + i).integers(-3, 4, (n_rows, n_cols)).astype([F64, np.int32][i])
        hit, _ = run_direct(xh, xs, v, edges, cmp=cmp, inverse=bool(i), size=[None, 300][i], what="%s %dx%d" % (dom, n_rows, n_cols))
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
    hit, _ = run_direct(xh, xc.emit(idx, edges, F32), np.round(sc.values("random", F32, 3, 2000, 48), 1), edges, what="two inputs")
    assert hit["sort"]["D"] == 2


# ---------------------------------------------------------------------------------------------------------------------
# 4. layouts through the C ABI: samples and values
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_base_pointers_off_16_byte_alignment(xh, sdt):
    from xhistogram_amd import _native as native

    st = F64 if sdt == "f64" else F32
    n_rows, n_cols = 3, 1001
    edges = bc.edges_for([50])
    flat = np.concatenate([[0], xc.emit(bc.indices("random", 1, n_rows * n_cols, 50, seed=9), edges, st)[0].reshape(-1)]).astype(st)
    vflat = np.concatenate([[0], np.round(sc.values("random", st, 1, n_rows * n_cols, 43).reshape(-1), 1)]).astype(st)
    x_t, v_t = _dev(flat), _dev(vflat)
    assert x_t.data_ptr() % 16 == 0 and v_t.data_ptr() % 16 == 0
    plan = _plan_for(xh, [flat], edges)
    views = [native.make_view(x_t.data_ptr() + flat.itemsize, _tag(native, st), n_cols, 1)]
    vview = native.make_view(v_t.data_ptr() + flat.itemsize, _tag(native, st), n_cols, 1)
    got = guarded_unique(native, plan, views, vview, n_rows, n_cols, n_cols, True)
    uo.assert_variant(plan.describe(), uo.predict(_cus(), edges, 0, st, st, n_rows, n_cols, n_cols, True))
    uo.assert_same(got, uo.unique_rows(mo.index([flat[1:].reshape(n_rows, n_cols)], edges), vflat[1:].reshape(n_rows, n_cols), 50), "x[1:]")


@pytest.mark.parametrize("layout", ["row_broadcast", "transposed", "values_col_broadcast", "values_strided"])
def test_strided_views(xh, layout):
    """rows of samples broadcast at stride 0 (still the fast family) and a transposed block (row stride 1: the generic family),
    each with values laid out the same way; values broadcast along the columns (one entry per bin) and values at a column
    stride of 3"""
    from xhistogram_amd import _native as native

    edges = bc.edges_for([40])
    n_rows, n_cols = 3, 2500
    vals = np.round(sc.values("random", F64, n_rows, 3 * n_cols, 44), 1)
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
    size, inverse = (900, False) if layout == "values_strided" else (n_cols, True)
    got = guarded_unique(native, plan, [native.make_view(x_t.data_ptr(), native.F64, rs, cs)],
                         native.make_view(v_t.data_ptr(), native.F64, vrs, vcs), n_rows, n_cols, size, inverse)
    fast = layout != "transposed"
    hit = uo.assert_variant(plan.describe(), uo.predict(_cus(), edges, 0, F64, F64, n_rows, n_cols, size, inverse, layout_fast=fast))
    assert hit["sort"]["keys"] == ("fast" if fast else "generic")
    uo.assert_same(got, want_of(mo.index([np.ascontiguousarray(logical)], edges), np.ascontiguousarray(vlogical), 40, size, inverse), layout)


# ---------------------------------------------------------------------------------------------------------------------
# 5. determinism: twice, on two streams at once, and outputs that start full of set bits
# ---------------------------------------------------------------------------------------------------------------------
def test_twice_and_on_two_streams_at_once(xh):
    from xhistogram_amd import _native as native

    n_rows, n_cols, nb, size = 2, 60_000, 37, 500
    edges, x, v = _tie_block(n_rows, n_cols, nb, 12)
    x_t, v_t = _dev(x), _dev(v)
    plan = _plan_for(xh, [x], edges)
    views = [native.make_view(x_t.data_ptr(), native.F64, n_cols, 1)]
    vview = native.make_view(v_t.data_ptr(), native.F32, n_cols, 1)
    want = uo.unique_rows(mo.index([x], edges), v, nb, size)
    first = guarded_unique(native, plan, views, vview, n_rows, n_cols, size, True)
    second = guarded_unique(native, plan, views, vview, n_rows, n_cols, size, True)
    uo.assert_same(first, want, "first run")
    uo.assert_same(second, first, "the second run")
    streams = side_streams(2)
    outs = [[torch.full(s, 7, dtype=torch.int64, device="cuda") for s in ((n_rows, size), (n_rows, size), (n_rows, nb + 1), (n_rows, n_cols))]
            for _ in streams]
    torch.cuda.synchronize()
    for _ in range(3):
        for s, o in zip(streams, outs):
            plan.execute_unique(views, vview, n_rows, n_cols, size, *[t.data_ptr() for t in o], stream=s.cuda_stream)
    torch.cuda.synchronize()
    for o in outs:
        h = [t.cpu().numpy() for t in o]
        uo.assert_same((h[0].view(F64), h[1], h[2], h[3]), want, "two streams")


def test_outputs_full_of_set_bits(xh):
    """every output is its own working space: handed over as bytes of all ones, a call that added to what it found, or left an
    element out, would show it"""
    edges, x, v = _tie_block(3, 5000, 20, 14)
    run_direct(xh, [x], v, edges, what="all ones", fill=ONES)
    run_direct(xh, [x], v, edges, size=64, inverse=False, what="all ones, cut", fill=ONES)
    run_direct(xh, [x[:, :0]], v[:, :0], edges, size=5, what="all ones, no columns", fill=ONES)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the public API
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


def _want(x, v, edges, axis, size=None):
    """the oracle's outputs: uniques, counts and offsets over the kept axes, the inverse moved back into the shape of x"""
    idx = mo.index([x], [edges])
    uniques, counts, offsets, flat = uo.unique_rows(bo.rows_of(idx, axis), bo.rows_of(v, axis), len(edges) - 1, size)
    if axis is None:
        return uniques, counts, offsets, flat.reshape(x.shape)
    red = sorted(a % x.ndim for a in axis)
    kept = [i for i in range(x.ndim) if i not in red]
    full = flat.reshape([x.shape[i] for i in kept] + [x.shape[i] for i in red])
    return uniques, counts, offsets, (np.moveaxis(full, range(len(kept), x.ndim), red) if kept else full)


@pytest.mark.parametrize("backend", ["torch", "numpy", "device"])
@pytest.mark.parametrize("axis", API_AXES, ids=[str(a) for a in API_AXES])
def test_public_api_backends_and_axes(xh, backend, axis):
    """a 3-D block over trailing, middle, leading and split axes (listed in both orders): the oracle's bits, with and without
    the inverse, at size=None and at a cut"""
    from xhistogram_amd.devicearray import DeviceArray

    x, v, edges = _api_block()
    put = {"torch": lambda a: torch.as_tensor(a).cuda(), "numpy": lambda a: a, "device": lambda a: DeviceArray.from_numpy(a, 0)}[backend]
    kind = torch.Tensor if backend == "torch" else np.ndarray
    *got, e = xh.bin_unique(put(x), values=put(v), bins=[edges], axis=axis, return_inverse=True)
    want = _want(x, v, edges, axis)
    assert all(isinstance(g, kind) for g in got) and np.array_equal(e[0], edges) and tuple(got[3].shape) == x.shape
    uo.assert_same([_np(g) for g in got], want, "%s %s" % (backend, axis))
    *got, e = xh.bin_unique(put(x), values=put(v), bins=[edges], axis=axis, size=12)
    assert len(got) == 3
    uo.assert_same([_np(g) for g in got], _want(x, v, edges, axis, 12)[:3], "%s %s size=12" % (backend, axis))


def test_identities_with_the_librarys_own_results(xh):
    """np.diff(offsets) is histogram_mode's nunique; the segment sums of counts its count; a segment's largest count its
    mode_count and the first entry that holds it its mode, by bits; a segment's ends == histogram_extrema's vmin and vmax;
    inverse == offsets[bin_index] + dense rank - 1; the bincount of the inverse is counts; uniques[inverse] == values"""
    x, v, edges = _api_block(310, (6, 900))
    xd, vd = torch.as_tensor(x).cuda(), torch.as_tensor(v).cuda()
    kw = dict(values=vd, bins=[edges], axis=1)
    uniques, counts, offsets, inverse, _ = (_np(a) if hasattr(a, "detach") else a for a in xh.bin_unique(xd, return_inverse=True, **kw))
    uo.assert_same((uniques, counts, offsets, inverse), _want(x, v, edges, (1,)), "the block")
    count, nunique, mode, mode_count = (_np(a) for a in xh.histogram_mode(xd, **kw)[:4])
    vmin, vmax = (_np(a) for a in xh.histogram_extrema(xd, **kw)[:2])
    dense = _np(xh.bin_rank(xd, method="dense", **kw)[0])
    index = _np(xh.bin_index(xd, bins=[edges])[0])
    np.testing.assert_array_equal(np.diff(offsets, axis=1), nunique)
    for row in range(x.shape[0]):
        total = offsets[row, -1]
        for b in range(8):
            seg = slice(offsets[row, b], offsets[row, b + 1])
            assert counts[row, seg].sum() == count[row, b]
            if count[row, b]:
                assert counts[row, seg].max() == mode_count[row, b]
                first = offsets[row, b] + int(np.argmax(counts[row, seg]))
                assert uniques[row, first:first + 1].view(np.uint64)[0] == mode[row, b:b + 1].view(np.uint64)[0]
                assert uniques[row, seg][0] == vmin[row, b] and uniques[row, seg][-1] == vmax[row, b]
        on = (index[row] >= 0) & ~np.isnan(v[row])
        assert on.any() and (inverse[row][~on] == -1).all()
        np.testing.assert_array_equal(inverse[row][on], offsets[row][index[row][on]] + dense[row][on].astype(np.int64) - 1)
        np.testing.assert_array_equal(np.bincount(inverse[row][on], minlength=total), counts[row, :total])
        np.testing.assert_array_equal(uniques[row][inverse[row][on]], v[row][on])


def test_values_broadcast_against_the_samples(xh):
    rng = np.random.default_rng(307)
    x = rng.uniform(-1.2, 1.2, (6, 400))
    v = rng.integers(-5, 6, (400,)).astype(np.int16)
    edges = [np.linspace(-1.0, 1.0, 9)]
    got = xh.bin_unique(torch.as_tensor(x).cuda(), values=torch.as_tensor(v).cuda(), bins=edges, axis=1, return_inverse=True)[:4]
    uo.assert_same([_np(g) for g in got], uo.unique_rows(mo.index([x], edges), np.broadcast_to(v, x.shape), 8), "broadcast values")
    uniques, counts, offsets, _ = xh.bin_unique(x, values=2.5, bins=edges, axis=1, size=8)  # a scalar: one entry per bin that has a sample
    hist = np.stack([np.histogram(r, edges[0])[0] for r in x])
    assert (np.diff(offsets, axis=1) == (hist > 0)).all() and (uniques[counts > 0] == 2.5).all() and (counts.sum(1) == hist.sum(1)).all()


def test_the_blocks_dask_hands_over(xh):
    """core._bin_unique_block and core._bin_unique_inverse_block as a dask task calls them, on host blocks over the kept axis:
    int64 [rows, 1, 2 W + B + 1], uniques as the bits they are, and the inverse in the block's own shape"""
    x, v, edges = _api_block(312, (6, 300))
    for lo, hi in ((0, 2), (2, 6)):
        want = _want(x[lo:hi], v[lo:hi], edges, (1,), 20)
        out = xh._bin_unique_block(x[lo:hi], v[lo:hi], axis=[1], bins=[edges], size=20)
        assert out.shape == (hi - lo, 1, 2 * 20 + 9) and out.dtype == np.int64
        got = (np.ascontiguousarray(out[:, 0, :20]).view(F64), out[:, 0, 20:40], out[:, 0, 40:])
        uo.assert_same(got, want[:3], "rows %d..%d" % (lo, hi))
        inv = xh._bin_unique_inverse_block(x[lo:hi], v[lo:hi], axis=[1], bins=[edges])
        uo.assert_same((got[0], got[1], got[2], inv), want, "the inverse of rows %d..%d" % (lo, hi))


@pytest.mark.parametrize("backend", ["torch", "numpy"])
def test_extents_of_zero(xh, backend):
    edges = [np.linspace(0.0, 1.0, 5)]
    put = (lambda a: torch.as_tensor(a).cuda()) if backend == "torch" else (lambda a: a)
    for shape, axis, kept, c in (((3, 0), 1, (3,), 0), ((0, 7), 1, (0,), 7), ((0,), None, (), 0), ((2, 0, 3), (0, 2), (0,), 6)):
        for size in (None, 4):
            uniques, counts, offsets, inverse, _ = (_np(a) if not isinstance(a, list) else a for a in xh.bin_unique(
                put(np.zeros(shape)), values=put(np.zeros(shape)), bins=edges, axis=axis, size=size, return_inverse=True))
            width = c if size is None else size
            assert uniques.shape == counts.shape == kept + (width,) and offsets.shape == kept + (5,) and inverse.shape == shape
            assert uniques.dtype == F64 and counts.dtype == offsets.dtype == inverse.dtype == np.int64
            assert not counts.any() and not offsets.any() and (np.ascontiguousarray(uniques).view(np.uint64) == uo.NAN_BITS).all()


def test_zero_columns_and_zero_width_through_the_plan(xh):
    from xhistogram_amd import _native as native

    edges = bc.edges_for([4])
    x = np.zeros((3, 1))
    x_t = _dev(x)
    plan = _plan_for(xh, [x], edges)
    view = native.make_view(x_t.data_ptr(), native.F64, 0, 1)
    for size in (0, 6):
        got = guarded_unique(native, plan, [view], view, 3, 0, size, True)
        uo.assert_same(got, uo.unique_rows(np.zeros((3, 0), np.int64), np.zeros((3, 0)), 4, size), "no columns, size=%d" % size)
        uo.assert_variant(plan.describe(), uo.predict(_cus(), edges, 0, F64, F64, 3, 0, size, True))
    run_direct(xh, [np.full((2, 300), 0.5)], np.arange(600.0).reshape(2, 300) % 7, edges, size=0, what="no width")


@pytest.mark.parametrize("backend", ["torch", "numpy"])
def test_plan_without_bins(xh, backend):
    """one edge, no bin: offsets == [0], padding only, an inverse of -1; through Plan.execute_unique too, guard bands intact"""
    from xhistogram_amd import _native as native

    x = np.random.default_rng(302).uniform(-1.0, 1.0, (3, 1515))
    v = np.round(sc.values("random", F64, 3, 1515, 46), 1)
    edges = [np.array([0.25])]
    put = (lambda a: torch.as_tensor(a).cuda()) if backend == "torch" else (lambda a: a)
    for size in (None, 9, 0):
        got = xh.bin_unique(put(x), values=put(v), bins=edges, axis=1, size=size, return_inverse=True)[:4]
        uo.assert_same([_np(g) for g in got], uo.unique_rows(np.full(x.shape, -1), v, 0, size), "no bins, size=%s" % size)
    x_t, v_t = _dev(x), _dev(v)
    plan = _plan_for(xh, [x], edges)
    views, vview = [native.make_view(x_t.data_ptr(), native.F64, 1515, 1)], native.make_view(v_t.data_ptr(), native.F64, 1515, 1)
    for size, inverse in ((3000, True), (7, False)):
        got = guarded_unique(native, plan, views, vview, 3, 1515, size, inverse)
        uo.assert_same(got, want_of(np.full(x.shape, -1), v, 0, size, inverse), "no bins, direct")


def test_refusals(xh):
    from xhistogram_amd import _native as native

    x = torch.zeros(8, dtype=torch.float64, device="cuda")
    edges = [np.linspace(0.0, 1.0, 5)]
    with pytest.raises(TypeError, match="complex values have no order"):
        xh.bin_unique(x, values=torch.zeros(8, dtype=torch.complex64, device="cuda"), bins=edges)
    with pytest.raises(TypeError, match="unexpected keyword argument 'weights'"):
        xh.bin_unique(x, values=x, weights=x, bins=edges)
    with pytest.raises(TypeError, match="bin_unique needs values"):
        xh.bin_unique(x, values=None, bins=edges)
    for bad in (-1, True, 2.0):
        with pytest.raises(ValueError, match="size must be None or an integer >= 0"):
            xh.bin_unique(x, values=x, bins=edges, size=bad)
    # 2^31 columns by shape only: one element expanded at stride 0, refused by the front and by the library before any launch
    n = 1 << 31
    wide = torch.full((1,), 0.5, dtype=torch.float64, device="cuda").expand(n)
    assert wide.stride() == (0,)
    plan = _plan_for(xh, [np.zeros((2, 4))], edges)
    xh.bin_unique(x, values=x, bins=edges)
    before = plan.describe()
    with pytest.raises(NotImplementedError, match=r"bin_unique takes fewer than 2\^31"):
        xh.bin_unique(wide, values=wide, bins=edges, size=4)
    outs = [torch.full(s, -7, dtype=torch.int64, device="cuda") for s in ((2, 3), (2, 3), (2, 5), (2, 4))]
    torch.cuda.synchronize()
    lib = native.load()
    view = native.make_view(x.data_ptr(), native.F64, 4, 1)
    ptrs = [C.c_void_p(o.data_ptr()) for o in outs]
    args = (plan._h, (native.XhistArray * 1)(view), C.byref(view), 2, 4)
    wide_view = native.make_view(wide.data_ptr(), native.F64, 0, 0)
    assert lib.xhist_plan_execute_unique(plan._h, (native.XhistArray * 1)(wide_view), C.byref(wide_view), 1, n, 3, *ptrs, native.MEM_DEVICE,
                                         C.c_void_p(0)) == native.ERR_UNSUPPORTED
    assert "fewer than 2^31 samples per output row" in lib.xhist_last_error().decode()
    for missing in range(3):  # (the inverse may be NULL: a call without one)
        holed = [C.c_void_p(0) if i == missing else p for i, p in enumerate(ptrs)]
        assert lib.xhist_plan_execute_unique(*args, 3, *holed, native.MEM_DEVICE, C.c_void_p(0)) == native.ERR_INVALID
        assert "NULL" in lib.xhist_last_error().decode()
    assert lib.xhist_plan_execute_unique(*args, -1, *ptrs, native.MEM_DEVICE, C.c_void_p(0)) == native.ERR_INVALID
    assert "size of 0 or more" in lib.xhist_last_error().decode()
    assert lib.xhist_plan_execute_unique(*args, 3, *ptrs, native.MEM_HOST, C.c_void_p(0)) == native.ERR_INVALID
    assert "mem_kind XHIST_MEM_DEVICE" in lib.xhist_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool((o == -7).all()) for o in outs) and plan.describe() == before
    assert lib.xhist_plan_execute_unique(*args, 3, *ptrs, native.MEM_DEVICE, C.c_void_p(0)) == native.OK
    torch.cuda.synchronize()
    h = [o.cpu().numpy() for o in outs]  # (four zeros in bin 0 of each of two rows)
    want = (np.array([[0.0, uo.PAD, uo.PAD]] * 2), np.array([[4, 0, 0]] * 2), np.array([[0, 1, 1, 1, 1]] * 2), np.zeros((2, 4), np.int64))
    uo.assert_same((h[0].view(F64), h[1], h[2], h[3]), want, "a valid call still runs")


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
                    got = xh.bin_unique(torch.as_tensor(xs[t]).cuda(), values=torch.as_tensor(vs[t]).cuda(), bins=edges, axis=1, size=250,
                                        return_inverse=True)[:4]
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
        uo.assert_same(results[t], uo.unique_rows(mo.index([xs[t]], edges), vs[t], 32, 250), "thread %d" % t)


def test_torch_results_follow_the_current_stream(xh):
    edges, x, v = _tie_block(1, 40_000, 100, 304)
    s = side_streams(1)[0]
    with torch.cuda.stream(s):
        got = xh.bin_unique(torch.as_tensor(x[0]).cuda(), values=torch.as_tensor(v[0]).cuda(), bins=edges, size=1500, return_inverse=True)[:4]
        s.synchronize()
        got = [g.cpu().numpy() for g in got]
    uo.assert_same(got, uo.unique_rows(mo.index([x[0]], edges), v[0], 100, 1500), "side stream")


def test_edges_from_a_bin_count_and_two_inputs(xh):
    rng = np.random.default_rng(305)
    x, y = rng.uniform(0, 1, (2, 4, 600))
    v = rng.integers(0, 9, (4, 600))
    *got, e = xh.bin_unique(torch.as_tensor(x).cuda(), torch.as_tensor(y).cuda(), values=torch.as_tensor(v).cuda(), bins=[4, 3], axis=1,
                            return_inverse=True)
    edges = [np.asarray(b) for b in e]
    uo.assert_same([_np(g) for g in got], uo.unique_rows(mo.index([x, y], edges), v, 12), "two inputs")


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
    got = xhx.bin_unique(temp, values=cls, bins=[edges], dim=["x"], return_inverse=True)
    assert [g.name for g in got] == ["cls_unique", "cls_unique_counts", "cls_unique_offsets", "cls_unique_inverse"]
    assert [tuple(g.dims) for g in got] == [("time", "cls_unique"), ("time", "cls_unique"), ("time", "cls_bin_offset"), ("time", "x")]
    uo.assert_same([np.asarray(g.data) for g in got], uo.unique_rows(mo.index([x], [edges]), v, 8), "xarray")
    np.testing.assert_array_equal(np.asarray(got[0]["time"].data), np.arange(4.0))
    flat = xhx.bin_unique(temp, values=xr.DataArray(v, dims=("time", "x")), bins=[edges], size=30)
    assert [g.name for g in flat] == ["values_unique", "values_unique_counts", "values_unique_offsets"]
    assert [tuple(g.dims) for g in flat] == [("values_unique",), ("values_unique",), ("values_bin_offset",)]
    uo.assert_same([np.asarray(g.data) for g in flat], uo.unique_rows(mo.index([x], [edges]).reshape(-1), v.reshape(-1), 8, 30)[:3], "flat")
    with pytest.raises(TypeError, match="accepts only xarray.DataArray"):
        xhx.bin_unique(x, values=cls, bins=[edges])


def test_dask_branch(monkeypatch):
    """blocks over the kept axes give what the numpy call gives, bit for bit: tests/bin_unique_dask_script.py in the interpreter
    that has dask, started as tests/test_dask_branch.py starts its own script"""
    import test_dask_branch as tdb

    if not tdb._have_dask_python():
        pytest.skip("no interpreter with dask in this image")
    monkeypatch.setattr(tdb, "SCRIPT", os.path.join(ROOT, "tests", "bin_unique_dask_script.py"))
    assert "BIN-UNIQUE-DASK-OK" in tdb._run("bin_unique")
