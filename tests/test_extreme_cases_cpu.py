"""What tests/test_gpu_extremes.py relies on, checked where no GPU is needed.

Its answers are constructed, not computed (tests/extreme_cases.py): for every case that file runs, the samples are generated
here with the same generator and patterns, the column count cut to at most 50 000, and the constructed expectation must equal
oracle_np.bincount_rows of the generated samples — counts exactly, weighted sums bit for bit.  That holds every midpoint inside
its bin after the cast to float32 for every edge kind used, and shows that each dropped kind is dropped.  The samples the GPU
file emits on the device (emit_torch) are held to the host's, bit for bit.  The three host restatements are checked at their
borders on numbers written out by hand."""
import numpy as np
import pytest

import exact_weights as ew
import extreme_cases as xc
from oracle import oracle_np as onp

torch = pytest.importorskip("torch")  # (the GPU files' helpers import it; none of this needs a GPU)
F64 = np.float64


def _check(b, what):
    case = b.case
    want = onp.bincount_rows([x.astype(F64) for x in b.xs], b.edges, None if b.w is None else b.w.astype(F64))
    if b.w is None:
        assert want.dtype.kind in "iu" and b.want.dtype == np.int64
        np.testing.assert_array_equal(b.want, want, err_msg=what)
    else:
        ew.assert_summable(b.top, b.w.dtype)
        ew.assert_bits_equal(b.want, want, what)
    assert b.top == onp.bincount_rows([x.astype(F64) for x in b.xs], b.edges, None).max(), what
    dropped = int((b.idx < 0).sum())
    assert int(onp.bincount_rows([x.astype(F64) for x in b.xs], b.edges, None).sum()) == b.idx.size - dropped, what
    # the device's emit gives the host's samples
    for xt, x in zip(xc.emit_torch(torch.from_numpy(b.idx.copy()), b.edges, xc.ST[case["st"]]), b.xs):
        assert xt.numpy().dtype == x.dtype and np.array_equal(xt.numpy().view(np.uint8), x.view(np.uint8)), what
    return dropped


@pytest.mark.parametrize("home", xc.HOT_HOMES)
def test_hot_cases_against_the_oracle(home):
    """part 1: every (sample dtype, weight dtype, inputs, edge kind, pattern, shift, signs) of the home, at its shape and — what
    an unweighted case runs again when its histogram is packed16 — at the longer row"""
    n = dropped = 0
    seen = set()
    for st in ("f64", "f32"):
        for wt in ("none", "f32", "f64"):
            for case in xc.hot_cases(home, st, wt):
                # (packed16 is a home of the streaming kernels with a few rows; the GPU file asserts that where it runs the longer row)
                shapes = [case["shape"]] + ([(case["shape"][0], xc.PACKED16_COLS)] if wt == "none" and case["shape"][0] <= xc.PACKED16_ROWS else [])
                for shape in shapes:
                    c = dict(case, shape=shape)
                    key = (st, wt, case["signs"], case["D"], case["kind"], case["pattern"], case["shift"], min(shape[1], xc.CPU_COLS))
                    if key in seen:  # (both shapes cut to the same columns)
                        continue
                    seen.add(key)
                    dropped += _check(xc.Built(c, n_cols=xc.CPU_COLS), repr(c))
                    n += 1
    assert n > 0 and dropped > 0  # (pattern pair drops samples of every kind)


def test_every_dropped_kind_is_dropped():
    """a row of nothing but dropped samples, each kind in each input: nothing is counted"""
    for st in (np.float64, np.float32):
        for D in (1, 2, 3):
            edges = [xc.edges_of(kind, 12, seed=d) for d, kind in zip(range(D), ("lin", "k3", "lin"))]
            idx = np.full((2, 5 * D * 4), -1, np.int32)
            xs = xc.emit(idx, edges, st)
            for d in range(D):  # every kind turns up in every input
                col = xs[d].reshape(-1)
                assert np.isnan(col).any() and (col == np.inf).any() and (col == -np.inf).any()
                assert (col < edges[d][0]).any() and ((col > edges[d][-1]) & np.isfinite(col)).any()
            assert onp.bincount_rows([x.astype(F64) for x in xs], edges, None).sum() == 0
            assert xc.expected(idx, [12] * D).sum() == 0


def test_capacity_cases_against_the_oracle():
    """part 2: the value every sample of a row has lies in the row's hot bin (both halves of the middle word, the first and the
    last bin), for float32, float64 and uint8 samples; the ordered packed16 input counts what its closed form says"""
    for c in xc.capacity_cases():
        edges = xc.case_edges(c)
        dt = xc.CAP_ST[c["st"]]
        vals, flat = xc.one_values(edges, dt, c["n_rows"], c["shift"])
        n_cols = 7
        xs = [np.repeat(v[:, None], n_cols, axis=1) for v in vals]
        assert xs[0].dtype == dt
        want = onp.bincount_rows([x.astype(F64) for x in xs], edges, None)
        np.testing.assert_array_equal(xc.one_expected(flat, c["nbs"], n_cols), want, err_msg=repr(c))
        hot = xc.hot_bins(int(np.prod(c["nbs"])))
        assert hot[2] % 2 == 0 and hot[3] == hot[2] + 1 and list(flat[:4]) == hot[:min(4, c["n_rows"])]
        if dt != np.uint8:  # pattern one as the index construction gives it
            idx = xc.indices("one", min(c["n_rows"], 9), n_cols, int(np.prod(c["nbs"])), c["shift"], 0)
            for x, e in zip(xs, xc.emit(idx, edges, dt)):
                np.testing.assert_array_equal(x[:idx.shape[0]], e)
    c = [c for c in xc.capacity_cases() if c["name"] == "packed16_both_halves"][0]
    e = xc.case_edges(c)
    mids = xc.midpoints(e[0], F64)
    m = xc.hot_bins(c["nbs"][0])[2]
    x = xc.both_halves_samples(mids[m], mids[m + 1])
    got = onp.bincount_rows([x], e, None)
    assert (got[0, m], got[0, m + 1]) == xc.BOTH_HALVES_WANT and got.sum() == sum(xc.BOTH_HALVES_WANT)
    # every phase starts on a multiple of 8192 (a tile of 64 lanes has at most 64 x 4 x 8 samples) and has one value
    starts = np.flatnonzero(~np.isnan(x[0]) & np.isnan(np.concatenate([[np.nan], x[0, :-1]])))
    assert len(starts) == 4 and not (starts % 8192).any()
    assert [x[0, i] for i in starts] == [mids[m + 1], mids[m], mids[m], mids[m + 1]]


@pytest.mark.parametrize("pattern", ["spread", "pair"])
def test_route_cases_against_the_oracle(pattern):
    """part 3: every variant (float64 and float32 pairs, counts, float32 / float64 weights of one sign and both, three rows)"""
    for variant in xc.ROUTE_VARIANTS:
        b = xc.Built(xc.route_case(variant, pattern, 2 * xc.ROUTE_N), n_cols=xc.CPU_COLS)
        _check(b, variant + " " + pattern)
        # the first half of the columns, as the GPU file runs it with route_grid = 1
        h = xc.CPU_COLS // 2
        want = onp.bincount_rows([x[:, :h].astype(F64) for x in b.xs], b.edges, None if b.w is None else b.w[:, :h].astype(F64))
        got = xc.expected(b.idx[:, :h], b.case["nbs"], None if b.w is None else b.w[:, :h])
        assert np.array_equal(got.view(np.int64), want.view(np.int64))


def test_periodic_closed_form_against_the_oracle():
    """part 4: the 7-element sample pattern (uint8 and float32) and the 11- and 13-element weight patterns, at lengths around
    whole periods: the closed form against the oracle over the written-out arrays"""
    for dt in (np.uint8, np.float32):
        pat = xc.chunk_sample_pattern(dt)
        e = [xc.chunk_edges(dt)]
        assert len(pat) == 7 and sorted(b for b in xc.CHUNK_BINS_PAT if b >= 0) == [0, 1, 2, 3, 4]
        for n in (1, 6, 7, 8, 76, 77, 78, 1001, 50_000):
            x = np.tile(pat, n // 7 + 1)[:n][None, :]
            np.testing.assert_array_equal(xc.periodic_expected(n, xc.CHUNK_BINS_PAT, 5)[None, :], onp.bincount_rows([x.astype(F64)], e, None))
            for period, seed in ((11, 41), (11, 42), (13, 43)):
                wp = xc.chunk_weight_pattern(period, seed)
                assert wp.dtype == np.float32 and (wp > 0).any() and (wp < 0).any()
                w = np.tile(wp, n // period + 1)[:n][None, :]
                ew.assert_bits_equal(xc.periodic_expected(n, xc.CHUNK_BINS_PAT, 5, wp)[None, :], onp.bincount_rows([x.astype(F64)], e, w.astype(F64)),
                                     "%s n=%d period=%d" % (np.dtype(dt).name, n, period))
    # at the GPU file's length no bin holds 2^29 samples (sums of exact float32 weights stay exact) and the sums fit 53 bits
    ew.assert_summable(xc.periodic_expected(xc.CHUNK_N, xc.CHUNK_BINS_PAT, 5).max(), np.float32)
    xc.periodic_expected(xc.CHUNK_N, xc.CHUNK_BINS_PAT, 5, xc.chunk_weight_pattern(11, 41))
    # neither period divides a column chunk (a multiple of the tile, itself a power of two times 64 lanes)
    assert all((1 << 30) % p for p in (7, 11, 13))


def test_borders_of_the_host_restatements():
    """per_wg_samples around 2^31, route_chunks_per_wg around block * 2^14 per workgroup, lane_cols_per_seg around 65535"""
    stream = "family=fast hist=lds vec=4 unroll=4 block=256 grid=1 segs=1 lds_bytes=1024 copies=32 table_bytes=0"
    tile = 256 * 4 * 4  # 4096
    assert xc.per_wg_samples(stream, 2**31 - tile) == 2147479552 == 2**31 - tile  # whole tiles below 2^31: one launch
    assert xc.per_wg_samples(stream, 2**31 - tile + 1) == 2147483648 == 2**31    # one sample more is a tile more: chunked
    assert xc.per_wg_samples(stream, 2**31) == 2**31
    assert xc.per_wg_samples(stream, 2**31 + 12_345) == 2147500032 == 2**31 + 4 * tile
    assert xc.per_wg_samples(stream.replace("unroll=4", "unroll=8").replace("block=256", "block=64"), 5) == 2048
    with pytest.raises(AssertionError):
        xc.per_wg_samples(stream.replace("segs=1", "segs=2"), 100)
    route = "family=fast hist=partitioned route=fused rows_per_pass=1 parts=64 chunk=16384 chunks<=2000 tile=4096 block=1024 grid=1 acc_grid=7 lds_route=1"
    full = 1024 * 2**14  # 16 777 216 samples: block chunks of 2^14 records
    assert xc.route_chunks_per_wg(route, full - 1) == 1023
    assert xc.route_chunks_per_wg(route, full) == 1024       # == block: the list holds them
    assert xc.route_chunks_per_wg(route, full + 1) == 1024
    assert xc.route_chunks_per_wg(route, full + 2**14) == 1025  # > block: the list is full
    assert xc.route_chunks_per_wg(route, 20_000_003) == 1220
    two = route.replace(" grid=1 ", " grid=2 ")
    assert xc.route_chunks_per_wg(two, 40_000_006) == 1220 and xc.route_chunks_per_wg(two, 2 * full + 1) == 1024
    assert xc.route_chunks_per_wg(route.replace("chunk=16384", "chunk=1024"), 6_000_011) == 5859
    assert xc.field(route, "grid") == "1" and xc.field(route, "acc_grid") == "7"  # (grid= is not the tail of acc_grid=)
    lanes = "family=lanes hist=lds16(shared) rows_per_wg=4 transpose=0 direct_store=0 block=256 grid=1x4096 lds_bytes=4000"
    assert xc.lane_cols_per_seg(lanes, 4096 * 65535) == 65535 and 4096 * 65535 == 268_431_360
    assert xc.lane_cols_per_seg(lanes, 4096 * 65535 + 1) == 65536
    assert xc.lane_cols_per_seg(lanes, 4096 * 65535 - 4095) == 65535 and xc.lane_cols_per_seg(lanes, 4096 * 65534) == 65534
