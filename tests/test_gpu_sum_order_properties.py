"""Property, thread, scratch and row-batch tests of histogram_sum and bin_order on an MI355X: what
tests/test_gpu_values_properties.py is to the ten per-bin statistics and tests/test_gpu_map_properties.py to the maps.
tests/test_gpu_sum.py and tests/test_gpu_bin_order.py build each case for one launch variant on contiguous arrays; these walk what
feeds the launchers (core._value_views, _value_rows, _value_block, _upload_host, core._order_offsets_rows, _launch_outputs, _bin_order_block) and the row
loop of launch_values_pass, whose second iteration no other test reaches.  Every comparison is bit for bit or integer equality
(totals by sum_cases.same_bits: zeros by value, NaN by place); there is no tolerance.  The cases, their data and what they
claim are tests/sum_order_cases.py's, held to the oracles by tests/test_sum_order_cases_cpu.py.

(a) test_sum_cases_match_oracle[stat], test_order_cases_match_oracle[stat]: the very 60 derandomised cases per statistic that
    tests/test_gpu_values_properties.py draws (D = 1..3 inputs of ndim 1..4, a dtype and a layout per array, axis in any order
    and sign, extents of 0, three backends).  histogram_sum on "extrema" as drawn (+-inf, +-0.0, int64 near 2^62, float16,
    bool, small integers) and on "mean_var" with full-mantissa values in place of its grid values (float64, float32, float16,
    laid out as the case lays out its values), against sum_oracle.histogram_sum; its count against histogram_mean_var's on the
    same call.  bin_order on the samples of "argextrema" and "quantile" against bin_order_oracle.order_offsets, the library's own
    histogram and assert_grouped; on "argextrema" the first maximum found through the order is histogram_argextrema's argmax.
(b) test_sum_blocks_as_dask_hands_them[stat], test_order_blocks_as_dask_hands_them[stat]: the kept axes cut into 1..3 chunks
    (neither result merges: every reduced axis is one chunk), core._value_block(stat="sum") and core._bin_order_block on every
    block of host arrays, each against the oracle on that block, the blocks put together against the unchunked public call.
(d) test_sum_and_bin_order_initialise_the_scratch_they_inherit: histogram_sum's block of five planes and bin_order's key,
    counter and slice blocks come back from the scratch cache full of set bits.
(c) test_one_plan_many_threads: 8 threads, a stream each from test_gpu_bin_order.side_streams, one cached plan, both entry
    points, inputs made on the thread's stream and not synchronised, sliced along both axes on every other thread.
(e) test_more_rows_than_one_launch[family]: Plan.execute_sum on 4099 rows more than one launch of a pass takes, the whole
    block of counts and totals against a closed form, between guard bands.

What the 60 examples per statistic of (a) hold (printed by tests/test_sum_order_cases_cpu.py, which asserts the floors):
histogram_sum, extrema / mean_var: cases that count no sample 3 / 2 (at most 6), with an extent 0 3 / 2, with a finite total
in a bin of two or more values 53 / 51 (at least 50), with an infinite or NaN total 8 / 46; of the mean_var cases 38 hold a bin
whose total is not what float64 additions in column order give; replacement values float64 50, float32 3, float16 7.
bin_order, argextrema / quantile: cases that count nothing 2 / 3, with an extent 0 2 / 3, with a bin of two or more positions
53 / 55 (at least 50), axis listed out of order 17 / 13, every axis listed and out of order 12 / 9; 58 argextrema cases tie the
positions to histogram_argextrema.
A drawn case that failed once stays below as a directed case (DIRECTED_*), whatever becomes of the bug."""
import threading
import time

import numpy as np
import pytest

import bin_order_oracle as bo
import map_cases as mc
import map_oracle as mo
import sum_cases as sc
import sum_oracle as so
import sum_order_cases as soc
import values_cases as vc
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
hyp = pytest.importorskip("hypothesis")

from test_gpu_bin_order import side_streams  # noqa: E402
from test_gpu_map_properties import _need, check_output  # noqa: E402
from test_gpu_sum import parse  # noqa: E402
from test_gpu_values_census import _cus  # noqa: E402
from test_gpu_values_properties import BLOCK_EXAMPLES, EXAMPLES, cuts_of, for_each_case, kept_shape, xh  # noqa: E402,F401  (xh: the fixture)

F64 = np.float64
SENTINEL = -0x0123456789ABCDEF  # (no count, and as a float64 -3.5e-303: no total of any data here)


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _bins_kw(built):
    return built.edges if built.d > 1 else built.edges[0]


# ---------------------------------------------------------------------------------------------------------------------
# (a) the public calls on the drawn cases
# ---------------------------------------------------------------------------------------------------------------------
def check_sum_case(core, case):
    built = soc.build_sum(case)
    d, backend = built.d, case["backend"]
    want_cnt, want_tot = soc.sum_want(built.host[:d], built.host[d], built.edges, case["axis"])
    arrays = built.inputs(backend)
    args, kw = soc.sum_call(built, arrays)
    cnt, tot, edges = core.histogram_sum(*args, **kw)
    for got, mine in zip(edges, built.edges):
        np.testing.assert_array_equal(_np(got), mine)
    shape = kept_shape(case) + tuple(len(e) - 1 for e in built.edges)
    cnt = check_output(cnt, arrays, backend, shape, np.int64, "count")
    tot = check_output(tot, arrays, backend, shape, F64, "total")
    np.testing.assert_array_equal(cnt, want_cnt, err_msg="count")
    sc.same_bits(tot, want_tot, "total")
    if want_cnt.sum() > 0:  # the samples histogram counts whose value is not NaN: histogram_mean_var's count on the same call
        np.testing.assert_array_equal(_np(core.histogram_mean_var(*args, **kw)[0]), cnt, err_msg="histogram_mean_var's count")


def check_order_case(core, case):
    built = vc.build(case)
    d, backend, axis, shape = built.d, case["backend"], case["axis"], case["shape"]
    n_bins = soc.n_bins_of(built.edges)
    want_order, want_offsets, rows = soc.order_want(built.host[:d], built.edges, axis)
    arrays = built.inputs(backend)
    xs, bins = arrays[:d], _bins_kw(built)
    order, offsets, edges = core.bin_order(*xs, bins=bins, axis=axis)
    for got, mine in zip(edges, built.edges):
        np.testing.assert_array_equal(_np(got), mine)
    kept = kept_shape(case)
    c = int(np.prod([shape[i] for i in set(vc.reduced_axes(case))], dtype=np.int64))
    m = int(np.prod(kept, dtype=np.int64))
    order = check_output(order, arrays, backend, kept + (c,), np.int64, "order")
    offsets = check_output(offsets, arrays, backend, kept + (n_bins + 1,), np.int64, "offsets")
    mo.assert_bits(offsets, want_offsets, "offsets")
    mo.assert_bits(order, want_order, "order")
    counts = np.diff(offsets, axis=-1)
    if 0 not in shape:  # (arrays without elements: see test_gpu_values_properties.run_public)
        h = _np(core.histogram(*xs, bins=bins, axis=axis)[0])
        np.testing.assert_array_equal(counts.reshape(h.shape), h)
    flat_o, flat_f, flat_r = order.reshape(m, c), offsets.reshape(m, n_bins + 1), rows.reshape(m, c)
    for r in range(m):
        bo.assert_grouped(flat_o[r], flat_f[r], flat_r[r], n_bins, "row %d" % r)
    if case["stat"] == "argextrema" and (counts > 0).any():
        # the two definitions of a position, on this layout: the first maximum found through the order is the library's argmax
        _, amax, _, _, _ = core.histogram_argextrema(*xs, values=arrays[d], bins=bins, axis=axis)
        amax = _np(amax).reshape(m, n_bins)
        v_rows = bo.rows_of(built.host[d], axis).reshape(m, c)
        for r in range(m):
            np.testing.assert_array_equal(soc.argmax_through_order(flat_o[r], flat_f[r], v_rows[r]), amax[r], err_msg="argmax, row %d" % r)


@pytest.mark.parametrize("stat", soc.SUM_STATS)
def test_sum_cases_match_oracle(xh, stat):
    for_each_case(stat, EXAMPLES, lambda case: check_sum_case(xh, case))


@pytest.mark.parametrize("stat", soc.ORDER_STATS)
def test_order_cases_match_oracle(xh, stat):
    for_each_case(stat, EXAMPLES, lambda case: check_order_case(xh, case))


# Drawn cases that failed once, kept as they were drawn (none so far: the tests are loops, so that an empty list does not skip).
DIRECTED_SUM = [
]
DIRECTED_ORDER = [
]


def test_drawn_cases_that_failed_once(xh):
    for case in DIRECTED_SUM:
        check_sum_case(xh, case)
    for case in DIRECTED_ORDER:
        check_order_case(xh, case)


# ---------------------------------------------------------------------------------------------------------------------
# (b) the blocks of a chunked call, as dask's tasks hand them to core._value_block and core._bin_order_block
# ---------------------------------------------------------------------------------------------------------------------
def _kept_cuts(case, salt):
    """(reduced axes sorted, per axis its chunks: 1..3 along a kept axis, one along a reduced one)"""
    shape = case["shape"]
    rng = np.random.default_rng(case["seed"] + salt)
    red = sorted(set(vc.reduced_axes(case)))
    return red, [[(0, n)] if i in red else cuts_of(rng, n) for i, n in enumerate(shape)]


def _blocks(cuts):
    for at in np.ndindex(*[len(c) for c in cuts]):
        yield tuple(slice(*c[j]) for c, j in zip(cuts, at))


def check_sum_blocks(core, case):
    built = soc.build_sum(case)
    shape, d, edges = case["shape"], built.d, built.edges
    axis = onp.normalise_axis(case["axis"], len(shape))  # (what _values_blockwise hands on)
    red, cuts = _kept_cuts(case, 3)
    full = [np.broadcast_to(a, shape) for a in built.views]  # (dask broadcasts its arrays before it cuts them)
    bins_shape = tuple(len(e) - 1 for e in edges)
    whole = np.full((2,) + tuple(1 if i in red else n for i, n in enumerate(shape)) + bins_shape, np.nan)
    for sl in _blocks(cuts):
        out = core._value_block(*[a[sl] for a in full], stat="sum", axis=axis, bins=edges)
        lead = tuple(1 if i in red else s.stop - s.start for i, s in enumerate(sl))
        assert out.dtype == F64 and out.shape == (2,) + lead + bins_shape, (out.dtype, out.shape)
        host = [np.ascontiguousarray(h[sl]) for h in built.host]
        want_cnt, want_tot = soc.sum_want(host[:d], host[d], edges, axis)
        got = [np.ascontiguousarray(o.squeeze(tuple(red))) for o in out]
        np.testing.assert_array_equal(got[0].view(np.int64), want_cnt, err_msg="count of block %s" % (sl,))  # (never merged: the bits)
        sc.same_bits(got[1], want_tot, "total of block %s" % (sl,))
        whole[(slice(None),) + tuple(slice(None) if i in red else s for i, s in enumerate(sl))] = out
    args, kw = soc.sum_call(built, full)
    cnt, tot, _ = core.histogram_sum(*args, **kw)
    whole = [np.ascontiguousarray(w.squeeze(tuple(red))) for w in whole]
    np.testing.assert_array_equal(whole[0].view(np.int64), cnt, err_msg="the blocks' counts put together")
    sc.same_bits(whole[1], tot, "the blocks' totals put together")


def check_order_blocks(core, case):
    built = vc.build(case)
    shape, d, edges = case["shape"], built.d, built.edges
    ndim = len(shape)
    axis = onp.normalise_axis(case["axis"], ndim) or list(range(ndim))  # (bin_order hands its blocks list(drop_axes))
    red, cuts = _kept_cuts(case, 4)
    full = [np.broadcast_to(a, shape) for a in built.views[:d]]
    n_bins = soc.n_bins_of(edges)
    c = int(np.prod([shape[i] for i in red], dtype=np.int64))
    whole = np.full(tuple(1 if i in red else n for i, n in enumerate(shape)) + (c + n_bins + 1,), -7, np.int64)
    for sl in _blocks(cuts):
        out = core._bin_order_block(*[a[sl] for a in full], axis=axis, bins=edges)
        lead = tuple(1 if i in red else s.stop - s.start for i, s in enumerate(sl))
        assert out.dtype == np.int64 and out.shape == lead + (c + n_bins + 1,), (out.dtype, out.shape)
        want_order, want_offsets, _ = soc.order_want([np.ascontiguousarray(h[sl]) for h in built.host[:d]], edges, axis)
        got = out.squeeze(tuple(red))
        mo.assert_bits(np.ascontiguousarray(got[..., :c]), want_order, "order of block %s" % (sl,))
        mo.assert_bits(np.ascontiguousarray(got[..., c:]), want_offsets, "offsets of block %s" % (sl,))
        whole[tuple(slice(None) if i in red else s for i, s in enumerate(sl))] = out
    order, offsets, _ = core.bin_order(*full, bins=_bins_kw(built), axis=case["axis"])
    whole = whole.squeeze(tuple(red))
    mo.assert_bits(np.ascontiguousarray(whole[..., :c]), order, "the blocks' orders put together")
    mo.assert_bits(np.ascontiguousarray(whole[..., c:]), offsets, "the blocks' offsets put together")


@pytest.mark.parametrize("stat", soc.SUM_STATS)
def test_sum_blocks_as_dask_hands_them(xh, stat):
    for_each_case(stat, BLOCK_EXAMPLES, lambda case: check_sum_blocks(xh, case))


@pytest.mark.parametrize("stat", soc.ORDER_STATS)
def test_order_blocks_as_dask_hands_them(xh, stat):
    for_each_case(stat, BLOCK_EXAMPLES, lambda case: check_order_blocks(xh, case))


DIRECTED_SUM_BLOCKS = [
]
DIRECTED_ORDER_BLOCKS = [
]


def test_blocks_of_drawn_cases_that_failed_once(xh):
    for case in DIRECTED_SUM_BLOCKS:
        check_sum_blocks(xh, case)
    for case in DIRECTED_ORDER_BLOCKS:
        check_order_blocks(xh, case)


# ---------------------------------------------------------------------------------------------------------------------
# (d) dirty scratch  (before (c): the threads leave staging blocks in the cache)
# ---------------------------------------------------------------------------------------------------------------------
def test_sum_and_bin_order_initialise_the_scratch_they_inherit(xh):
    """The method of test_gpu_values_properties.test_a_statistic_initialises_the_scratch_it_inherits, for the two entry points
    that came after it.  histogram_sum takes one block of 5 * R * B 8-byte words from the stream-ordered scratch cache: two key
    planes that pass 1 must initialise and three limb planes that zero_words must clear before the integer atomics add into
    them.  bin_order takes its keys (R * C * 8 bytes), its counters (R * chunks * (B + 1) * 4) and, where a row is more than
    one chunk, its slice bases (R * slices * (B + 1) * 4).  Every cached block that a request of one of these sizes could be
    given is held out of the cache; a call on other data makes the blocks; host-route histograms of samples whose bytes are
    all ones stage them into those very blocks, on the same stream or on another one, and allocate nothing (their output
    takes a smallest block put there for it, each staging request the only block left that fits it); then the entry runs on
    the real data, allocates nothing either, and gives the oracle's bits.  At this shape the counter and slice blocks are
    13 312 and 6 656 bytes, above the smallest size class of the cache (4096), so each can be isolated and is dirtied too."""
    from xhistogram_amd import _native

    R, C, B = 13, 600, 127
    edges = np.linspace(-4.0, 4.0, B + 1)

    def data_of(seed):
        rng = np.random.default_rng(seed)
        return vc.edge_relative(rng, (R, C), edges, F64), soc.full_mantissa(rng, (R, C))

    (x, v), (x2, v2) = data_of(31), data_of(32)
    xd, vd, xd2, vd2 = (torch.as_tensor(a).cuda() for a in (x, v, x2, v2))
    want_sum = so.sum_rows([x], [edges], v)
    want_order = bo.order_offsets(mo.index([x], [edges]), B)
    g = bo.geometry(_cus(), B, R, C)
    sum_block = 5 * R * B * 8
    group_blocks = [R * C * 8, R * g["chunks"] * (B + 1) * 4]
    if g["chunks"] > 1:
        group_blocks.append(R * -(-g["chunks"] // bo.SLICE) * (B + 1) * 4)
    assert min(group_blocks) > 4096 and len(set(group_blocks + [sum_block])) == len(group_blocks) + 1, group_blocks
    dirty_plan = _native.Plan([np.array([0.0, 0.5, 1.0])], _native.CMP_F64, 0)
    side = side_streams(1)[0]

    def total():
        s = _native.scratch_stats(0)
        return s["cached"] + s["live"]

    def dirty(nbytes, stream):
        ones = np.frombuffer(b"\xff" * nbytes, np.float64)  # (NaN samples: nothing is counted)
        out = np.empty(2, np.int64)
        dirty_plan.execute([_native.make_view(ones.ctypes.data, _native.F64, ones.size, 1)], None, 1, ones.size, out.ctypes.data,
                           False, _native.MEM_HOST, stream=stream)
        assert not out.any()

    torch.cuda.synchronize()
    held = []
    try:
        for size in [sum_block] + group_blocks:  # hold every cached block a request of this size could be given
            for _ in range(20_000):
                before = _native.scratch_stats(0)["cached"]
                held.append(_native.DeviceBuffer(0, size))
                if _native.scratch_stats(0)["cached"] == before:  # (a fresh allocation: the cache had nothing left for it)
                    break
            else:
                raise AssertionError("the scratch cache never ran out of blocks")
        _native.DeviceBuffer(0, 16).close()  # (whatever the cache held before, it now holds a block smaller than all of these)
        for where in ("same stream", "another stream"):
            stream = 0 if where == "same stream" else side.cuda_stream
            for name, blocks in (("histogram_sum", [sum_block]), ("bin_order", group_blocks)):
                if name == "histogram_sum":  # makes the blocks of this shape
                    xh.histogram_sum(xd2, values=vd2, bins=[edges], axis=1)
                else:
                    xh.bin_order(xd2, bins=[edges], axis=1)
                torch.cuda.synchronize()
                _native.DeviceBuffer(0, 16).close()  # (a smallest block for the histograms' own output: it is asked for first)
                before = total()
                for nbytes in blocks:
                    dirty(nbytes, stream)
                    torch.cuda.synchronize()
                assert total() == before, "the all-ones samples were staged into a fresh block, not into the cached ones (%s)" % name
                if name == "histogram_sum":
                    cnt, tot, _ = xh.histogram_sum(xd, values=vd, bins=[edges], axis=1)
                else:
                    order, offsets, _ = xh.bin_order(xd, bins=[edges], axis=1)
                torch.cuda.synchronize()
                assert total() == before, "%s allocated scratch of its own (%s)" % (name, where)
                if name == "histogram_sum":
                    np.testing.assert_array_equal(_np(cnt), want_sum[0], err_msg="count, " + where)
                    sc.same_bits(_np(tot), want_sum[1], "total, " + where)
                else:
                    mo.assert_bits(_np(offsets), want_order[1], "offsets, " + where)
                    mo.assert_bits(_np(order), want_order[0], "order, " + where)
    finally:
        for h in held:
            h.close()
        dirty_plan.close()


# ---------------------------------------------------------------------------------------------------------------------
# (c) one plan, many threads
# ---------------------------------------------------------------------------------------------------------------------
THREAD_COLS = [5000 + 17 * t for t in range(8)]
WIDE_COLS = 22_000  # 3 rows of these are 2^16 elements and more: sliced along both axes, such an input is copied


def _laid(a, sliced):
    """the array itself, or a block of twice its extents that holds it at [::2, ::2] and its elements in another order elsewhere"""
    if not sliced:
        return a
    big = np.resize(a.reshape(-1)[::-1], (2 * a.shape[0], 2 * a.shape[1])).astype(a.dtype)
    big[::2, ::2] = a
    return big


def test_one_plan_many_threads(xh):
    """8 threads with a stream (test_gpu_bin_order.side_streams: no stream is made here) and data of their own share one edge
    array, so one cached plan, and run histogram_sum and bin_order three times each; resident torch inputs and numpy inputs
    take turns.  The resident inputs are made on the thread's stream by device arithmetic (twice the halves uploaded
    beforehand: exact) and handed over without synchronising: the library must queue behind that arithmetic.  On every other
    thread the inputs are [::2, ::2] views of a block twice the size.  At (3, 5000 + 17 t) such a view is handed to the kernels
    by its strides (below 2^16 elements nothing is copied); those threads therefore also run a second input of 3 x 22 000 and
    more, which the front copies, and whose copies it lets go of while the kernels are still queued.  Every round of every
    thread is held to oracles computed beforehand, bit for bit."""
    edges = [np.linspace(-1.0, 1.0, 33)]
    jobs = []  # (thread, sliced, halves on the host, halves on the device, what the calls must give)
    for t in range(8):
        sliced = t % 2 == 1
        for n_cols in [THREAD_COLS[t]] + ([WIDE_COLS + 17 * t] if sliced else []):
            rng = np.random.default_rng(6000 + 10 * t + (n_cols >= WIDE_COLS))
            x = vc.edge_relative(rng, (3, n_cols), edges[0], F64)
            v = soc.full_mantissa(rng, (3, n_cols))
            halves = [_laid(a * 0.5, sliced) for a in (x, v)]
            x, v = (h[::2, ::2] * 2.0 if sliced else h * 2.0 for h in halves)  # (what the device makes of the halves)
            want = so.sum_rows([x], edges, v) + bo.order_offsets(mo.index([x], edges), 32)
            jobs.append((t, sliced, halves, [torch.as_tensor(h).cuda() for h in halves], want))
    torch.cuda.synchronize()
    streams = side_streams(8)
    results = [[] for _ in jobs]
    errors = []

    def work(t):
        try:
            for rnd in range(3):
                for j, (owner, sliced, host, dev, _) in enumerate(jobs):
                    if owner != t:
                        continue
                    with torch.cuda.stream(streams[t]):
                        if (rnd + t) % 2 == 0:
                            x, v = (h * 2.0 for h in dev)  # (on this stream, and nobody waits for it)
                        else:
                            x, v = (h * 2.0 for h in host)
                        if sliced:
                            x, v = x[::2, ::2], v[::2, ::2]
                        outs = xh.histogram_sum(x, values=v, bins=edges, axis=1)[:2] + xh.bin_order(x, bins=edges, axis=1)[:2]
                        streams[t].synchronize()
                        assert all(isinstance(o, torch.Tensor if (rnd + t) % 2 == 0 else np.ndarray) for o in outs)
                        results[j].append([_np(o) for o in outs])
        except Exception as e:  # pragma: no cover
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for j, (t, sliced, _, _, want) in enumerate(jobs):
        assert len(results[j]) == 3
        for rnd, (cnt, tot, order, offsets) in enumerate(results[j]):
            what = "thread %d round %d, %d columns" % (t, rnd, want[2].shape[1])
            np.testing.assert_array_equal(cnt, want[0], err_msg=what + " count")
            sc.same_bits(tot, want[1], what + " total")
            mo.assert_bits(offsets, want[3], what + " offsets")
            mo.assert_bits(order, want[2], what + " order")


# ---------------------------------------------------------------------------------------------------------------------
# (e) more rows than one launch of the value passes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", soc.ROW_FAMILIES)
def test_more_rows_than_one_launch(xh, family):
    """launch_values_pass's loop over the rows of a launch, second iteration included, for the statistic for which it does the
    most: it advances the limb plane 0 (`out`), the counts (`out2`) and pass 1's minimum keys (`w2_ptr`) to the batch's first
    row, the other planes and the maximum keys lie CovParams::plane = the whole call's rows x bins on, and the kernels add
    Params::row0 to the row of the inputs.  Plan.execute_sum on 4099 rows more than one launch takes; rows are grouped views of
    periodic [P, 3] arrays (row r reads row r mod P; coprime periods for samples and values), the values full mantissas whose
    exponent steps by 50 from one value row to the next, so that a unit taken from another row's keys shows in the total
    (tests/test_sum_order_cases_cpu.py holds that, and the closed form, to the oracle by brute force).  The 31 877 distinct rows
    go through sum_oracle.sum_rows on the host; the WHOLE block of counts and totals is compared with them on the GPU, between
    guard bands.  fast: float64 samples and values, block 256; generic: int64 samples on int64 edges, float32 values, block 512.
    The cost is the launch of 2^24 (2^23) small workgroups per pass: measured 0.10 s (fast) and 0.11 s (generic) for the call,
    0.7 s and 0.4 s for the test."""
    from xhistogram_amd import _native as native

    edges, xs, vs = soc.rows_data(family)
    n_cols, n_bins = soc.ROWS_COLS, soc.ROWS_BINS
    cmp, plan_edges, _ = xh._compare_domain([xs.dtype], edges)
    assert cmp == (native.CMP_I64 if family == "generic" else native.CMP_F64)
    plan = xh._get_plan(plan_edges, cmp, 0)
    xs_t, vs_t = torch.as_tensor(xs).cuda(), torch.as_tensor(vs).cuda()
    views = [native.make_view(xs_t.data_ptr(), native.dtype_tag(xs.dtype), n_cols, 1, inner_rows=soc.P_S, outer_stride=0)]
    vview = native.make_view(vs_t.data_ptr(), native.dtype_tag(vs.dtype), n_cols, 1, inner_rows=soc.P_V, outer_stride=0)
    want_cnt, want_tot = (torch.as_tensor(a).cuda() for a in soc.rows_table(family))  # (once per distinct row, on the host)

    def run(n_rows, cnt_ptr, tot_ptr):
        plan.execute_sum(views, vview, n_rows, n_cols, cnt_ptr, tot_ptr)
        torch.cuda.synchronize()
        return parse(plan.describe())

    # a few rows first: the launch geometry of this case, from describe()
    small = torch.empty((2, 8, n_bins), dtype=torch.int64, device="cuda")
    hit = run(8, small[0].data_ptr(), small[1].data_ptr())
    assert (hit["family"], hit["block"], hit["segs"], hit["cmp"]) == (family, soc.ROW_BLOCK[family], [1, 1], int(family == "generic")), hit
    chunk = mc.launch_rows(hit["block"], hit["segs"][1])
    n_rows = chunk + soc.ROWS_EXTRA
    assert chunk < n_rows <= 2 * chunk  # (two launches of each pass)
    n = n_rows * n_bins
    lead, tail = 65, 64
    _need(8 * (2 * (lead + n + tail) + 5 * n) + (1 << 30),
          "2 x %d of outputs, %d of the call's scratch, about 2^30 for the comparison" % (8 * n, 40 * n))
    bufs = [torch.full((lead + n + tail,), SENTINEL, dtype=torch.int64, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hit = run(n_rows, bufs[0].data_ptr() + 8 * lead, bufs[1].data_ptr() + 8 * lead)
    print("\n%s: %d rows, chunk %d, %.3f s for the call; %s" % (family, n_rows, chunk, time.perf_counter() - t0, plan.describe()))
    assert (hit["family"], hit["block"], hit["segs"]) == (family, soc.ROW_BLOCK[family], [1, 1]), hit
    assert mc.launch_rows(hit["block"], hit["segs"][1]) == chunk
    for buf in bufs:
        assert bool((buf[:lead] == SENTINEL).all()) and bool((buf[lead + n:] == SENTINEL).all()), "the guard bands were written"
    got_cnt, got_tot = (buf[lead:lead + n].view(n_rows, n_bins) for buf in bufs)
    bad = {"count": 0, "total": 0}
    first = {}
    step = 1 << 21
    for r0 in range(0, n_rows, step):
        rows = torch.arange(r0, min(n_rows, r0 + step), device="cuda")
        at = soc.rows_index(rows)
        wc, wt = want_cnt[at], want_tot[at]
        gc, gt = got_cnt[r0:r0 + len(rows)], got_tot[r0:r0 + len(rows)]
        gf = gt.view(torch.float64)
        wn = torch.isnan(wt)
        wrong_t = (torch.isnan(gf) != wn) | (~wn & (gt != wt.view(torch.int64)) & ~((gf == 0) & (wt == 0)))  # (zeros by value)
        for name, wrong, got, want in (("count", gc != wc, gc, wc), ("total", wrong_t, gt, wt.view(torch.int64))):
            k = int(wrong.sum())
            if k and name not in first:
                i, b = torch.nonzero(wrong)[0].tolist()
                first[name] = (r0 + i, b, got[i, b].item(), want[i, b].item())
            bad[name] += k
    assert not bad["count"] and not bad["total"], "%d counts and %d totals of %d differ; first at (row, bin, got, expected; totals as bits) %s" % (
        bad["count"], bad["total"], n, first)
