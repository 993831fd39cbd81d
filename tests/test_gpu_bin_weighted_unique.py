"""bin_weighted_unique on the GPU.  Every comparison is bit for bit against tests/weighted_unique_oracle.py unless it says
otherwise: bin_unique's four outputs as tests/bin_unique_oracle.py states them, and every weight sum against math.fsum over its
run on exactly summable weights (tests/exact_weights.py), where any order of additions gives the same float64.  On N(0, 1)
weights the sums are held to each other across calls, streams, row batches, sizes and with or without an inverse, bit for bit,
and to math.fsum within exact_weights.assert_within_f64_bound.

Direct cases go through Plan.execute_unique_weighted with all outputs as one block inside a DeviceBuffer filled with a sentinel:
lead | uniques | counts | weight_sums | offsets | inverse | tail (the inverse block absent, and its pointer NULL, in a call
without one).  The sentinel must be intact in the lead and the tail and gone from every element of the block; 0x5A5A... is
neither 0, -1 nor a NaN.  The case tables are tests/weighted_unique_cases.py's; tests/test_bin_weighted_unique_cpu.py holds them
to what they claim."""
import os
import threading

import numpy as np
import pytest

import bin_order_cases as bc
import bin_order_oracle as bo
import bin_sort_oracle as so
import bin_unique_oracle as uo
import exact_weights as xw
import extreme_cases as xc
import map_oracle as mo
import weighted_unique_cases as wc
import weighted_unique_oracle as wo
from test_gpu_bin_order import side_streams
from test_gpu_bin_sort import _dev, _tag, _upload
from test_gpu_bin_unique import guarded_unique
from test_gpu_parity import _plan_for, xh  # noqa: F401  (xh: the module fixture)
from test_gpu_values_census import _cus

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F64, F32 = np.float64, np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A5A5A5A5A5A5A5A
ONES = 0xFFFFFFFFFFFFFFFF
CASE_NO = [0]


def guarded_wunique(native, plan, views, vview, wview, n_rows, n_cols, size, inverse, stream=0, fill=SENTINEL):
    """Plan.execute_unique_weighted into the middle of a DeviceBuffer of `fill` -> (uniques, counts, weight_sums [n_rows, size],
    offsets [n_rows, bins + 1][, inverse [n_rows, n_cols]])"""
    CASE_NO[0] += 1
    lead, tail = 64 + CASE_NO[0] % 2, 64
    nb1 = plan.n_bins + 1
    parts = [n_rows * size] * 3 + [n_rows * nb1] + ([n_rows * n_cols] if inverse else [])
    at = np.concatenate([[0], np.cumsum(parts)]) + lead
    host = np.full(int(at[-1]) + tail, fill, np.uint64).view(np.int64)
    guard = host[0]
    buf = native.DeviceBuffer(0, host.nbytes)
    buf.upload(host)
    torch.cuda.synchronize()
    ptrs = [buf.ptr + 8 * int(a) for a in at[:-1]]
    plan.execute_unique_weighted(views, vview, wview, n_rows, n_cols, size, ptrs[0], ptrs[1], ptrs[2], ptrs[3],
                                 ptrs[4] if inverse else None, stream=stream)
    torch.cuda.synchronize()
    buf.download(host)
    buf.close()
    assert (host[:lead] == guard).all() and (host[at[-1]:] == guard).all(), "the guard bands were written"
    block = host[lead:at[-1]]
    if fill == SENTINEL:
        assert not (block == guard).any(), "%d elements were never written" % (block == guard).sum()
    shapes = [(n_rows, size)] * 3 + [(n_rows, nb1), (n_rows, n_cols)]
    out = [host[at[i]:at[i + 1]].reshape(shapes[i]).copy() for i in range(len(parts))]
    out[0], out[2] = out[0].view(F64), out[2].view(F64)
    return tuple(out)


def want_of(idx, v, w, n_bins, size, inverse):
    want = wo.wunique_rows(idx, v, w, n_bins, size)
    return want if inverse else want[:4]


def run_direct(core, xs, v, w, edges, size=None, inverse=True, cmp=0, what="", layout_fast=True, want=None, fill=SENTINEL):
    """contiguous [R, C] host arrays through Plan.execute_unique_weighted: the describe() line, the guard bands, the oracle's bits"""
    from xhistogram_amd import _native as native

    n_rows, n_cols = xs[0].shape
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    width = n_cols if size is None else size
    xs_t = [_dev(x) for x in xs]
    vb, wb = _upload(native, v), _upload(native, w)
    plan = _plan_for(core, xs, edges)
    views = [native.make_view(t.data_ptr(), _tag(native, x.dtype), n_cols, 1) for t, x in zip(xs_t, xs)]
    vview = native.make_view(vb.ptr, _tag(native, v.dtype), n_cols, 1)
    wview = native.make_view(wb.ptr, _tag(native, w.dtype), n_cols, 1)
    got = guarded_wunique(native, plan, views, vview, wview, n_rows, n_cols, width, inverse, fill=fill)
    hit = wo.assert_variant(plan.describe(), "wunique", wo.predict_unique(_cus(), edges, cmp, xs[0].dtype, v.dtype, n_rows, n_cols, width,
                                                                          inverse, layout_fast=layout_fast))
    if want is None:
        want = want_of(mo.index(xs, edges), v, w, n_bins, width, inverse)
    wo.assert_same(got, want, what)
    vb.close()
    wb.close()
    return hit, got


# ---------------------------------------------------------------------------------------------------------------------
# 1. the case tables: where a run lies against words and tiles; column counts; value and weight dtypes; bin counts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wc.gpu_cases(wc.CUS), ids=lambda c: c["name"])
def test_case_table(xh, case):
    cus = _cus()
    edges, idx, xs, v, w = wc.case_data(case, cus)
    wc.check_claims(case, idx, v, w, cus)
    hit, got = run_direct(xh, xs, v, w, edges, inverse=case["inverse"], what=case["name"])
    assert hit["words"] == -(-case["n_cols"] // 64) and hit["size"] == case["n_cols"] and hit["inverse"] == int(case["inverse"])
    if any(c.endswith("(U = 0)") for c in case["claims"]):
        assert not got[3].any() and not got[1].any() and (wo.bits(got[2]) == 0).all()


def test_more_rows_than_one_launch(xh):
    """one launch's rows and five more, two samples each in two bins: every row past the first batch takes its own words, sums,
    offsets and padding start, against the closed form of a row of two"""
    g = so.geometry(_cus(), 1 << 25, 2)
    n_rows = g["rows_per_launch"] + 5
    assert g["chunks"] == 1 and n_rows < (1 << 20)
    rng = np.random.default_rng(5)
    x = rng.integers(0, 4, (n_rows, 2)).astype(F32) - 0.5  # -0.5: dropped, 0.5: bin 0, 1.5: bin 1, 2.5: dropped
    v = rng.integers(0, 2, (n_rows, 2)).astype(np.uint8)
    w = xw.f64(rng, (n_rows, 2), "both")
    edges = [np.array([0.0, 1.0, 2.0])]
    idx = mo.index([x], edges)
    big = 99
    key = np.where(idx >= 0, idx * 2 + v, big)  # (bin, value) in one number
    k0, k1 = key.min(1), key.max(1)
    two = (k1 < big) & (k1 != k0)
    total = (k0 < big).astype(np.int64) + two
    ent = np.stack([k0, np.where(two, k1, big)], 1)  # a row's entries, `big`: padding
    uniques = np.where(ent < big, (ent % 2).astype(F64), uo.PAD)
    member = key[:, :, None] == ent[:, None, :]
    counts = np.where(ent < big, member.sum(1), 0)
    both = member.all(1)  # an entry both samples hold: one float64 addition, exact on these weights
    sums = np.where(ent < big, np.where(both, (w[:, 0] + w[:, 1])[:, None], np.where(member[:, 0], w[:, :1], w[:, 1:])), 0.0)
    offsets = np.stack([np.zeros(n_rows, np.int64), ((ent < big) & (ent < 2)).sum(1), total], 1)
    inverse = np.where(key < big, (key != k0[:, None]).astype(np.int64), -1)
    want = (uniques, counts, sums, offsets, inverse)
    hit, _ = run_direct(xh, [x], v, w, edges, what="row batches", want=want)
    assert hit["rows_per_launch"] == g["rows_per_launch"] < n_rows and len(set(total)) == 3
    sel = slice(n_rows - 200, n_rows)
    wo.assert_same(wo.wunique_rows(idx[sel], v[sel], w[sel], 2), tuple(a[sel] for a in want), "the closed form")


# ---------------------------------------------------------------------------------------------------------------------
# 2. size, inverse, inputs, views of the weights
# ---------------------------------------------------------------------------------------------------------------------
def _tie_block(n_rows, n_cols, nb, seed, cats=10, signs="both"):
    edges = bc.edges_for([nb])
    x = xc.emit(bc.indices("random", n_rows, n_cols, nb, seed=seed), edges, F64)[0]
    rng = np.random.default_rng(seed)
    v = rng.integers(0, cats, (n_rows, n_cols)).astype(F32)  # a few categories: many runs
    v[rng.random(v.shape) < 0.05] = np.nan
    return edges, x, v, xw.f64(rng, (n_rows, n_cols), signs)


def test_sizes_around_the_number_of_entries(xh):
    """size in {None, 0, 1, U - 1, U, U + 1} for a row with 1 < U < c, three rows of different U, with and without an inverse:
    the cut leaves the stored sums, the offsets and the inverse as they are, and nothing is stored past the width"""
    edges, x, v, w = _tie_block(3, 700, 13, 21)
    v[1] = np.where(v[1] > 3, 3, v[1])
    v[2] = np.where(v[2] > 6, 6, v[2])
    v[2, ::3] = np.nan
    idx = mo.index([x], edges)
    full = wo.wunique_rows(idx, v, w, 13)
    totals = full[3][:, -1]
    assert len(set(totals)) == 3 and all(1 < t < 700 for t in totals)
    u = int(totals[0])
    for size in (None, 0, 1, u - 1, u, u + 1):
        for inverse in (True, False):
            hit, got = run_direct(xh, [x], v, w, edges, size=size, inverse=inverse, what="size=%s inverse=%s" % (size, inverse))
            np.testing.assert_array_equal(got[3], full[3])
            assert hit["size"] == (700 if size is None else size)


def test_two_and_eight_inputs(xh):
    idx = bc.indices("random", 3, 2000, 12, seed=9)
    edges = bc.edges_for([4, 3])
    rng = np.random.default_rng(48)
    v = rng.integers(0, 5, (3, 2000)).astype(F32)
    hit, _ = run_direct(xh, xc.emit(idx, edges, F32), v, xw.f64(rng, v.shape, "both"), edges, what="two inputs")
    assert hit["sort"]["D"] == 2
    idx = bc.indices("random", 2, 3000, 3 ** 8, seed=8)
    edges = bc.edges_for([3] * 8)
    v = rng.integers(0, 4, (2, 3000)).astype(np.int16)
    hit, _ = run_direct(xh, xc.emit(idx, edges, F64), v, xw.f32(rng, v.shape, "both"), edges, what="eight inputs")
    assert (hit["sort"]["keys"], hit["sort"]["D"]) == ("generic", 8)


@pytest.mark.parametrize("layout", ["broadcast_rows", "broadcast_cols", "strided", "transposed", "unaligned"])
def test_views_of_the_weights(xh, layout):
    """weights broadcast at row stride 0 and at column stride 0, at a column stride of 3, transposed in memory, and from a base
    pointer 8 bytes off 16-byte alignment; samples and values contiguous"""
    from xhistogram_amd import _native as native

    n_rows, n_cols, nb = 3, 1500, 20
    edges, x, v, _ = _tie_block(n_rows, n_cols, nb, 31)
    rng = np.random.default_rng(32)
    base = xw.f64(rng, (n_rows, 3 * n_cols + 1), "both")
    off = 0
    if layout == "broadcast_rows":
        mem, logical, (rs, cs) = base[:1, :n_cols], np.broadcast_to(base[:1, :n_cols], (n_rows, n_cols)), (0, 1)
    elif layout == "broadcast_cols":
        mem, logical, (rs, cs) = base[:, :1], np.broadcast_to(base[:, :1], (n_rows, n_cols)), (1, 0)
    elif layout == "strided":
        mem, logical, (rs, cs) = base[:, :3 * n_cols], base[:, :3 * n_cols:3], (3 * n_cols, 3)
    elif layout == "transposed":
        mem = np.ascontiguousarray(base[:, :n_cols].T)  # [C, R] in memory
        logical, (rs, cs) = mem.T, (1, n_rows)
    else:
        mem, logical, (rs, cs), off = base.reshape(-1)[:n_rows * n_cols + 1], base.reshape(-1)[1:n_rows * n_cols + 1].reshape(n_rows, n_cols), (n_cols, 1), 8
    x_t, v_t, w_t = _dev(x), _dev(v), _dev(mem)
    assert w_t.data_ptr() % 16 == 0
    plan = _plan_for(xh, [x], edges)
    got = guarded_wunique(native, plan, [native.make_view(x_t.data_ptr(), native.F64, n_cols, 1)], native.make_view(v_t.data_ptr(), native.F32, n_cols, 1),
                          native.make_view(w_t.data_ptr() + off, native.F64, rs, cs), n_rows, n_cols, n_cols, True)
    wo.assert_same(got, wo.wunique_rows(mo.index([x], edges), v, np.ascontiguousarray(logical), nb), layout)


# ---------------------------------------------------------------------------------------------------------------------
# 3. what the weights hold
# ---------------------------------------------------------------------------------------------------------------------
def test_nan_and_infinite_weights_stay_in_their_own_entry(xh):
    """a NaN weight in one run, +inf and -inf in another, +inf alone in a third; the runs between them stay exact.  The runs are
    long enough to cross words, so the NaN travels through lead and tail sums"""
    runs = [(0, 1.0, 50), (0, 2.0, 100), (0, 3.0, 90), (1, 3.0, 70), (1, 4.0, 5), (2, 1.0, 200)]
    idx = np.concatenate([np.full(n, b, np.int32) for b, _, n in runs])[None]
    v = np.concatenate([np.full(n, x, F64) for _, x, n in runs])[None]
    rng = np.random.default_rng(7)
    w = xw.f64(rng, idx.shape, "both")
    w[0, 60] = np.nan  # in run (0, 2.0)
    w[0, 245], w[0, 300] = np.inf, -np.inf  # in run (1, 3.0)
    w[0, 320] = np.inf  # in run (2, 1.0)
    perm = rng.permutation(idx.shape[1])
    idx, v, w = idx[:, perm], v[:, perm], w[:, perm]
    edges = bc.edges_for([4])
    _, got = run_direct(xh, xc.emit(idx, edges, F64), v, w, edges, what="nan and inf weights")
    s = got[2][0]
    assert np.isnan(s[1]) and np.isnan(s[3]) and s[5] == np.inf and np.isfinite(s[[0, 2, 4]]).all() and got[3][0, -1] == 6


def test_all_zero_weights(xh):
    edges, x, v, _ = _tie_block(2, 3000, 11, 33)
    _, got = run_direct(xh, [x], v, np.zeros(v.shape), edges, what="zero weights")
    assert (wo.bits(got[2]) == 0).all() and got[1].sum() > 0
    _, got = run_direct(xh, [x], v, np.full(v.shape, -0.0), edges, what="minus zero weights")
    u = got[3][:, -1]
    assert all((wo.bits(got[2][r, :u[r]]) == 1 << 63).all() and (wo.bits(got[2][r, u[r]:]) == 0).all() for r in range(2))


# ---------------------------------------------------------------------------------------------------------------------
# 4. reproducibility on weights with full mantissas
# ---------------------------------------------------------------------------------------------------------------------
def _normal_block(n_rows=3, n_cols=150_000, nb=5, seed=40):
    """rounded values: runs of thousands that cross words and tiles at places the data decides"""
    rng = np.random.default_rng(seed)
    edges = bc.edges_for([nb])
    x = xc.emit(bc.indices("random", n_rows, n_cols, nb, seed=seed), edges, F64)[0]
    v = np.round(rng.standard_normal((n_rows, n_cols)), 1)
    v[-1] = np.round(v[-1])  # (the last row: runs of ten thousand)
    v[rng.random(v.shape) < 0.01] = np.nan
    return edges, x, v, rng.standard_normal((n_rows, n_cols))


def test_the_same_bits_whatever_the_call(xh):
    """N(0, 1) weights: twice, on two streams at once, a row alone against the same row as the middle of three, size=None against
    a cut size, with and without an inverse: the same bits; and every sum within the float64 bound of math.fsum"""
    from xhistogram_amd import _native as native

    edges, x, v, w = _normal_block()
    n_rows, n_cols = x.shape
    nb = 5
    x_t, v_t, w_t = _dev(x), _dev(v), _dev(w)
    plan = _plan_for(xh, [x], edges)

    def views(r0, nr):
        at = 8 * r0 * n_cols
        return ([native.make_view(x_t.data_ptr() + at, native.F64, n_cols, 1)], native.make_view(v_t.data_ptr() + at, native.F64, n_cols, 1),
                native.make_view(w_t.data_ptr() + at, native.F64, n_cols, 1), nr, n_cols)

    first = guarded_wunique(native, plan, *views(0, 3), n_cols, True)
    idx = mo.index([x], edges)
    uo.assert_same(first[:2] + first[3:], uo.unique_rows(idx, v, nb), "bin_unique's outputs")
    wo.assert_within_bound(first[2], idx, v, w, nb, "N(0, 1) weights")
    total = first[3][:, -1]
    assert (total > 20).all() and first[1].max() > 5000
    again = guarded_wunique(native, plan, *views(0, 3), n_cols, True)
    assert np.array_equal(wo.bits(again[2]), wo.bits(first[2])), "the second call"
    plain = guarded_wunique(native, plan, *views(0, 3), n_cols, False)
    assert np.array_equal(wo.bits(plain[2]), wo.bits(first[2])), "without an inverse"
    cut = int(total.min()) // 2
    short = guarded_wunique(native, plan, *views(0, 3), cut, False)
    assert np.array_equal(wo.bits(short[2]), wo.bits(first[2][:, :cut])), "a cut size"
    alone = guarded_wunique(native, plan, *views(1, 1), n_cols, True)
    assert np.array_equal(wo.bits(alone[2][0]), wo.bits(first[2][1])), "the middle row alone"
    streams = side_streams(2)
    outs = [torch.full((4, n_rows, n_cols), 7, dtype=torch.int64, device="cuda") for _ in streams]
    offs = [torch.full((n_rows, nb + 1), 7, dtype=torch.int64, device="cuda") for _ in streams]
    torch.cuda.synchronize()
    for _ in range(2):
        for s, o, f in zip(streams, outs, offs):
            plan.execute_unique_weighted(*views(0, 3), n_cols, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), f.data_ptr(), o[3].data_ptr(),
                                         stream=s.cuda_stream)
    torch.cuda.synchronize()
    for o in outs:
        assert np.array_equal(o[2].cpu().numpy().view(np.uint64), wo.bits(first[2])), "two streams"


def test_a_run_over_more_than_256_tiles(xh):
    """wruns_scan walks a row's tiles in groups of 256 with a carry from group to group, so only a run of more than 256 tiles of
    65 536 samples takes its sum across a group border: the size at which that code can first go wrong.  One bin, a run of 1000
    and a run of the rest; the closed form is the exact sum of each part's exactly summable weights, and with a unit weight
    the counts.  The weighted mode names the heavier of the two."""
    n = 256 * wo.TILE + 5_000 + 1000
    assert (n - 1) // wo.TILE - 1000 // wo.TILE == 256  # (the long run starts in tile 0 and ends in tile 256, the second group)
    xw.assert_summable(n)
    w = xw.f64(np.random.default_rng(60), n, "both")
    sums = [float(w[:1000].sum()), float(w[1000:].sum())]  # (exact in any order)
    edges = [np.array([0.0, 1.0])]
    x = torch.full((1,), 0.5, dtype=torch.float64, device="cuda").expand(n)
    v = torch.where(torch.arange(n, device="cuda") < 1000, 1.0, 2.0).to(torch.float32)
    w_t = torch.as_tensor(w).cuda()
    pad = [uo.PAD, uo.PAD]
    for weights, want in ((w_t, sums), (1.0, [1000.0, float(n - 1000)])):
        uniques, counts, got, offsets, _ = xh.bin_weighted_unique(x, values=v, weights=weights, bins=edges, size=4)
        wo.assert_same([_np(a) for a in (uniques, counts, got, offsets)],
                       (np.array([1.0, 2.0] + pad), np.array([1000, n - 1000, 0, 0]), np.array(want + [0.0, 0.0]), np.array([0, 2])), "257 tiles")
    count, nunique, mode, weight, _ = xh.histogram_weighted_mode(x, values=v, weights=w_t, bins=edges)
    first = int(np.argmax(sums))
    wo.assert_mode_same([_np(a) for a in (count, nunique, mode, weight)],
                        (np.array([n]), np.array([2]), np.array([[1.0, 2.0][first]]), np.array([sums[first]])), "257 tiles, mode")


# ---------------------------------------------------------------------------------------------------------------------
# 5. identities with the library's own results
# ---------------------------------------------------------------------------------------------------------------------
def test_identities(xh):
    """uniques, counts, offsets and inverse are bin_unique's by bits; unit weights give the counts; np.bincount over the inverse
    gives the sums; the segment sums are histogram(weights=w) where no value is NaN (exactly summable weights)"""
    from xhistogram_amd import _native as native

    edges, x, v, w = _tie_block(3, 4000, 17, 50, signs="one")
    v = np.where(np.isnan(v), 1.0, v).astype(F32)  # (no NaN value: every counted sample is in an entry)
    n_rows, n_cols = x.shape
    x_t, v_t, w_t, one_t = _dev(x), _dev(v), _dev(w), _dev(np.ones(1))
    plan = _plan_for(xh, [x], edges)
    views = [native.make_view(x_t.data_ptr(), native.F64, n_cols, 1)]
    vview = native.make_view(v_t.data_ptr(), native.F32, n_cols, 1)
    got = guarded_wunique(native, plan, views, vview, native.make_view(w_t.data_ptr(), native.F64, n_cols, 1), n_rows, n_cols, n_cols, True)
    plain = guarded_unique(native, plan, views, vview, n_rows, n_cols, n_cols, True)
    uo.assert_same(got[:2] + got[3:], plain, "bin_unique")
    ones = guarded_wunique(native, plan, views, vview, native.make_view(one_t.data_ptr(), native.F64, 0, 0), n_rows, n_cols, n_cols, False)
    wo.assert_sums(ones[2], ones[1].astype(F64), "unit weights")
    hist = xh.histogram(x, bins=edges, weights=w, axis=1)[0]
    for r in range(n_rows):
        u, inv = int(got[3][r, -1]), got[4][r]
        wo.assert_sums(np.bincount(inv[inv >= 0], weights=w[r][inv >= 0], minlength=u)[:u], got[2][r, :u], "bincount over the inverse")
        seg = np.array([got[2][r, got[3][r, b]:got[3][r, b + 1]].sum() for b in range(17)])
        wo.assert_sums(seg, np.asarray(hist[r], F64), "segment sums against histogram(weights=)")


# ---------------------------------------------------------------------------------------------------------------------
# 6. the public API
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


def _want(x, v, w, edges, axis, size=None):
    idx = mo.index([x], [edges])
    out = wo.wunique_rows(bo.rows_of(idx, axis), bo.rows_of(v, axis), bo.rows_of(w, axis), len(edges) - 1, size)
    ndim = x.ndim
    red = list(range(ndim)) if axis is None else sorted(axis)
    kept = [i for i in range(ndim) if i not in red]
    inv = out[4].reshape([x.shape[i] for i in kept] + [x.shape[i] for i in red])
    inv = np.moveaxis(inv, list(range(len(kept), ndim)), red) if kept else inv
    return out[:4] + (inv,)


@pytest.mark.parametrize("backend", ["torch", "numpy", "device"])
@pytest.mark.parametrize("axis", API_AXES, ids=[str(a) for a in API_AXES])
def test_public_api_backends_and_axes(xh, backend, axis):
    from xhistogram_amd.devicearray import DeviceArray

    x, v, w, edges = _api_block()
    put = {"torch": lambda a: torch.as_tensor(a).cuda(), "numpy": lambda a: a, "device": lambda a: DeviceArray.from_numpy(a, 0)}[backend]
    kind = torch.Tensor if backend == "torch" else np.ndarray
    *got, e = xh.bin_weighted_unique(put(x), values=put(v), weights=put(w), bins=[edges], axis=axis, return_inverse=True)
    assert all(isinstance(g, kind) for g in got) and np.array_equal(e[0], edges)
    wo.assert_same([_np(g) for g in got], _want(x, v, w, edges, axis), "%s %s" % (backend, axis))
    *cut, _ = xh.bin_weighted_unique(put(x), values=put(v), weights=put(w), bins=[edges], axis=axis, size=6)
    wo.assert_same([_np(g) for g in cut], _want(x, v, w, edges, axis, 6)[:4], "%s %s size=6" % (backend, axis))


def test_weights_broadcast_and_of_other_dtypes(xh):
    rng = np.random.default_rng(307)
    x = rng.uniform(-1.2, 1.2, (6, 400))
    v = rng.integers(-5, 6, (6, 400)).astype(np.int16)
    edges = [np.linspace(-1.0, 1.0, 9)]
    idx = mo.index([x], edges)
    for w in (rng.integers(-9, 10, 400).astype(np.int32), xw.f32(rng, (6, 1)), (rng.integers(1, 9, (6, 400)) / 8).astype(np.float16), 2.5):
        *got, _ = xh.bin_weighted_unique(torch.as_tensor(x).cuda(), values=torch.as_tensor(v).cuda(),
                                         weights=torch.as_tensor(w).cuda() if isinstance(w, np.ndarray) else w, bins=edges, axis=1)
        wo.assert_same([_np(g) for g in got], wo.wunique_rows(idx, v, np.broadcast_to(w, x.shape), 8)[:4], "weights %s" % getattr(w, "dtype", "scalar"))


def test_the_blocks_dask_hands_over(xh):
    """core._bin_weighted_unique_block as a dask task calls it, on host blocks over the kept axis: uniques, counts and weight_sums
    side by side as int64 bits, then the offsets"""
    x, v, w, edges = _api_block(312, (6, 300))
    for lo, hi in ((0, 2), (2, 6)):
        out = xh._bin_weighted_unique_block(x[lo:hi], v[lo:hi], w[lo:hi], axis=[1], bins=[edges], size=40)
        assert out.shape == (hi - lo, 1, 3 * 40 + 9) and out.dtype == np.int64
        flat = out[:, 0]
        got = (flat[:, :40].copy().view(F64), flat[:, 40:80], flat[:, 80:120].copy().view(F64), flat[:, 120:])
        wo.assert_same(got, _want(x[lo:hi], v[lo:hi], w[lo:hi], edges, (1,), 40)[:4], "rows %d..%d" % (lo, hi))


def test_dask_branch(monkeypatch):
    import test_dask_branch as tdb

    if not tdb._have_dask_python():
        pytest.skip("no interpreter with dask in this image")
    monkeypatch.setattr(tdb, "SCRIPT", os.path.join(ROOT, "tests", "bin_weighted_unique_dask_script.py"))
    assert "WUNIQUE-DASK-OK" in tdb._run("wunique")


@pytest.mark.parametrize("backend", ["torch", "numpy"])
def test_extents_of_zero_and_a_plan_without_bins(xh, backend):
    edges = [np.linspace(0.0, 1.0, 5)]
    put = (lambda a: torch.as_tensor(a).cuda()) if backend == "torch" else (lambda a: a)
    for shape, axis, kept, c in (((3, 0), 1, (3,), 0), ((0, 7), 1, (0,), 7), ((0,), None, (), 0)):
        z = put(np.zeros(shape))
        uniques, counts, sums, offsets, inverse, _ = xh.bin_weighted_unique(z, values=z, weights=z, bins=edges, axis=axis, return_inverse=True)
        assert tuple(uniques.shape) == tuple(counts.shape) == tuple(sums.shape) == kept + (c,) and tuple(offsets.shape) == kept + (5,)
        assert tuple(inverse.shape) == shape and not _np(offsets).any()
        *cut, _ = xh.bin_weighted_unique(z, values=z, weights=z, bins=edges, axis=axis, size=3)
        assert tuple(cut[2].shape) == kept + (3,) and (wo.bits(_np(cut[2])) == 0).all() and (wo.bits(_np(cut[0])) == wo.NAN_BITS).all()
    x = put(np.linspace(0, 1, 12).reshape(3, 4))
    uniques, counts, sums, offsets, inverse, _ = xh.bin_weighted_unique(x, values=x, weights=x, bins=[np.array([0.5])], axis=1, return_inverse=True)
    assert tuple(offsets.shape) == (3, 1) and not _np(offsets).any() and (_np(inverse) == -1).all()
    assert (wo.bits(_np(sums)) == 0).all() and not _np(counts).any() and (wo.bits(_np(uniques)) == wo.NAN_BITS).all()


def test_outputs_full_of_set_bits_and_zero_columns(xh):
    from xhistogram_amd import _native as native

    edges, x, v, w = _tie_block(3, 5000, 20, 14)
    run_direct(xh, [x], v, w, edges, size=4000, what="all ones", fill=ONES)
    run_direct(xh, [x[:, :0]], v[:, :0], w[:, :0], edges, size=5, what="all ones, no columns", fill=ONES)
    x_t = _dev(np.zeros((3, 1)))
    plan = _plan_for(xh, [x], edges)
    view = native.make_view(x_t.data_ptr(), native.F64, 0, 1)
    got = guarded_wunique(native, plan, [view], view, view, 3, 0, 4, False)
    wo.assert_same(got, wo.wunique_rows(np.zeros((3, 0), np.int64), np.zeros((3, 0)), np.zeros((3, 0)), 20, 4)[:4], "no columns")
    wo.assert_variant(plan.describe(), "wunique", wo.predict_unique(_cus(), edges, 0, F64, F64, 3, 0, 4, False))


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
                    got = xh.bin_weighted_unique(torch.as_tensor(xs[t]).cuda(), values=torch.as_tensor(vs[t]).cuda(),
                                                 weights=torch.as_tensor(ws[t]).cuda(), bins=edges, axis=1, size=300)[:4]
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
        wo.assert_same(results[t], wo.wunique_rows(mo.index([xs[t]], edges), vs[t], ws[t], 32, 300)[:4], "thread %d" % t)


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
    got = xhx.bin_weighted_unique(temp, values=cls, weights=area, bins=[edges], dim=["x"], size=20, return_inverse=True)
    assert [g.name for g in got] == ["cls_unique", "cls_unique_counts", "cls_unique_weight_sums", "cls_unique_offsets", "cls_unique_inverse"]
    assert all(tuple(g.dims) == ("time", "cls_unique") for g in got[:3]) and tuple(got[3].dims) == ("time", "cls_bin_offset")
    wo.assert_same([np.asarray(g.data) for g in got], wo.wunique_rows(mo.index([x], [edges]), v, np.broadcast_to(w, x.shape), 8, 20), "xarray")
    with pytest.raises(TypeError, match="accepts only xarray.DataArray"):
        xhx.bin_weighted_unique(temp, values=cls, weights=w, bins=[edges])
