"""Property, scratch, long-row and thread tests of the six calls built on the sorted order (bin_sort, bin_rank, histogram_mode,
bin_unique, bin_weighted_unique, histogram_weighted_mode) on an MI355X: what tests/test_gpu_values_properties.py is to the ten
per-bin statistics, tests/test_gpu_map_properties.py to the maps and tests/test_gpu_sum_order_properties.py to histogram_sum and
bin_order.  Each call's own file builds its cases for one launch variant on contiguous [R, C] arrays; these walk what feeds the
launchers (core._sample_call, _value_views, _launch_outputs, _order_offsets_rows, _sample_block, _bin_unique, _value_stat and the
per-block callables of the dask graphs), the scratch every kernel of a call reads, rank_scan beyond one tile per thread, and the
scratch cache under eight streams that ask it for overlapping sizes.  Every comparison is bit for bit or integer equality (zeros
by sign, NaN by place and, where the design fixes them, by its bits 0x7ff8000000000000); there is no tolerance.  The cases, their
data and what they claim are tests/sorted_cases.py's, held to the oracles by tests/test_sorted_cases_cpu.py.

(a) test_drawn_cases_match_oracle[call-stat]: the very 60 derandomised cases per statistic that tests/test_gpu_values_properties.py
    draws (D = 1..3 inputs of ndim 1..4, a dtype and a layout per array, axis in any order and sign, extents of 0, three
    backends), and the directed ones of sorted_cases.DIRECTED_EXTRA.  bin_sort and bin_rank on "argextrema" and "quantile"
    (descending, and the mode out of bin_rank_cases.MODES, from the case's seed) against bin_sort_oracle and bin_rank_oracle;
    np.diff(offsets) against the library's histogram and, ascending, the order against bin_order's sorted stably by value key.
    histogram_mode and bin_unique on "argextrema" and "mean_var" (size out of None, 0, 1, U // 2, U, U + 3 and return_inverse from
    the seed) against mode_oracle and bin_unique_oracle; np.diff(offsets) against nunique and the count against
    histogram_mean_var's.  The weighted twins on "mean_var_w" and "quantile_w", whose integer weights sum exactly, against
    weighted_unique_oracle (math.fsum's bits) and against the unweighted twin on the same arrays.
(b) test_blocks_as_dask_hands_them[call-stat]: the kept axes cut into 1..3 chunks, the per-block callables of the dask graphs
    (core._bin_sort_block, _bin_rank_block, _bin_unique_block with its packed int64 block, _bin_unique_inverse_block,
    _bin_weighted_unique_block, _value_block(stat="mode" / "mode_w")) on every block of host arrays, each against the oracle on
    that block, the blocks put together against the unchunked public call.  test_a_cut_reduced_axis_is_refused[call]: the message
    of core._check_one_chunk, before any device work.
(c) test_a_call_initialises_the_scratch_it_inherits[call]: 3 rows of 70 001 samples in 127 bins; every block of the sort's seven
    requests and the sorted domain's carved block comes back from the scratch cache full of set bits, on the same stream and on
    another one; a block of the carved size read back before the call is all ones, and the call allocates nothing.
(d) test_long_row_*: one row of 256 * 65 536 + 70 001 samples, 258 tiles, so two per thread of rank_scan, with heads in the
    tiles of every thread that owns one; ranks, modes, distinct values, their counts, the inverse and the weight sums against a
    closed form (sorted_cases.LongRow), bin_sort and the ordinal rank against each other on the device.
(e) test_different_calls_at_once: 8 threads, a stream each from test_gpu_bin_order.side_streams, one cached plan, eight different
    calls that rotate over three rounds, inputs made on the thread's stream and not synchronised, every result against the same
    call made alone beforehand.

What the 60 examples per statistic of (a) hold (printed by tests/test_sorted_cases_cpu.py, which asserts the floors; argextrema /
quantile / mean_var / mean_var_w / quantile_w, the directed cases not counted): cases with an extent of 0 2 / 3 / 2 / 3 / 3, that
count no sample 2 / 3 / 2 / 3 / 3 (at most 6), with a bin of two or more counted values 53 / 55 / 53 / 56 / 54 (at least 50),
with a tie run of two or more equal values inside a bin 40 / 37 / 43 / 44 / 39 (at least 40), with a NaN value in a counted bin
16 / 26 / 15 / 18 / 16 (at least 10), with the same value in two bins of one row 48 / 40 / 47 / 43 / 39 (at least 40), with rows
longer than one word of 64 39 / 35 / 43 / 33 / 39 (at least 35), with both zeros in one bin 5 / 0 / 0 / 0 / 0; the longest row is
41 160 samples and the most rows 3 708.  Where the 60 miss a floor (quantile, mean_var_w, quantile_w) the 5, 4 and 3 directed cases
lift the tally over it.  All twenty modes of bin_rank occur over its 120 cases (2 .. 12 times each), every size 15 .. 27 times,
an inverse in 60 of 120, descending in 62 of 120.
A drawn case that failed once stays below as a directed case (DIRECTED_*), whatever becomes of the bug."""
import functools
import threading

import numpy as np
import pytest

import bin_order_oracle as bo
import bin_unique_oracle as uo
import exact_weights as xw
import mode_oracle as mdo
import sorted_cases as sdc
import values_cases as vc
import weighted_unique_oracle as wo
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
hyp = pytest.importorskip("hypothesis")

from test_gpu_bin_order import side_streams  # noqa: E402
from test_gpu_map_properties import check_output  # noqa: E402
from test_gpu_values_census import _cus  # noqa: E402
from test_gpu_values_properties import BLOCK_EXAMPLES, EXAMPLES, cuts_of, for_each_case, kept_shape, xh  # noqa: E402,F401  (xh: the fixture)

F64 = np.float64
NAN_BITS = np.uint64(uo.NAN_BITS)
PAIR_IDS = ["%s-%s" % p for p in sdc.PAIRS]


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _bins_kw(built):
    return built.edges if built.d > 1 else built.edges[0]


def same(got, want, what, nan_bits=True):
    """the same shape, dtype and 8 bytes per element: int64 by value, float64 by its bits, so -0.0 is not +0.0.  A NaN of `want`
    stands for 0x7ff8000000000000, the one NaN these calls write; `nan_bits` False (a rank, whose NaN the interface does not
    spell out): any NaN in its place"""
    got, want = np.ascontiguousarray(_np(got)), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert got.dtype in (np.int64, F64), (what, got.dtype)
    if got.dtype == F64:
        gb, wb = got.view(np.uint64), np.where(np.isnan(want), NAN_BITS, want.view(np.uint64))
        if not nan_bits:
            gb = np.where(np.isnan(got), NAN_BITS, gb)
    else:
        gb, wb = got, want
    bad = np.flatnonzero((gb != wb).reshape(-1))
    assert bad.size == 0, "%s: %d of %d elements differ, first at flat %d: got %r, want %r" % (
        what, bad.size, gb.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


def all_same(got, want, names, what, loose=()):
    assert len(got) == len(want) == len(names), (what, len(got), len(want))
    for g, w, name in zip(got, want, names):
        same(g, w, "%s %s" % (what, name), nan_bits=name not in loose)


def each_case(stat, n, body):
    """body(case) on the first n drawn cases of the statistic, then on the directed ones that go with it"""
    for_each_case(stat, n, body)
    for case in sdc.directed(stat):
        try:
            body(case)
        except Exception as e:
            raise AssertionError("%s: %s\ndirected case = %r" % (type(e).__name__, e, case)) from e


# ---------------------------------------------------------------------------------------------------------------------
# (a) the public calls on the drawn cases
# ---------------------------------------------------------------------------------------------------------------------
def _reduced_extent(case):
    return int(np.prod([case["shape"][i] for i in set(vc.reduced_axes(case))], dtype=np.int64))


def _check_edges(got, built):
    for e, mine in zip(got, built.edges):
        np.testing.assert_array_equal(_np(e), mine)


def check_sort_case(core, case):
    built = vc.build(case)
    d, backend, axis = built.d, case["backend"], case["axis"]
    kept, c, nb = kept_shape(case), _reduced_extent(case), sdc.n_bins_of(built.edges)
    arrays = built.inputs(backend)
    xs, bins, descending = arrays[:d], _bins_kw(built), sdc.descending_of(case)
    order, offsets, edges = core.bin_sort(*xs, values=arrays[d], bins=bins, axis=axis, descending=descending)
    _check_edges(edges, built)
    order = check_output(order, arrays, backend, kept + (c,), np.int64, "order")
    offsets = check_output(offsets, arrays, backend, kept + (nb + 1,), np.int64, "offsets")
    all_same((order, offsets), sdc.sort_want(built.host, d, built.edges, axis, descending), ("order", "offsets"), "bin_sort")
    if 0 not in case["shape"]:  # (arrays without elements: see test_gpu_values_properties.run_public)
        h = _np(core.histogram(*xs, bins=bins, axis=axis)[0])
        np.testing.assert_array_equal(np.diff(offsets, axis=-1).reshape(h.shape), h, err_msg="np.diff(offsets) against histogram")
    if not descending:
        plain_order, plain_offsets, _ = core.bin_order(*xs, bins=bins, axis=axis)
        same(plain_offsets, offsets, "bin_order's offsets")
        v_rows = bo.rows_of(built.host[d], axis)
        same(sdc.stable_by_value(_np(plain_order), _np(plain_offsets), v_rows), order, "bin_order's order sorted stably by value key")


def check_rank_case(core, case):
    built = vc.build(case)
    d, backend, axis = built.d, case["backend"], case["axis"]
    arrays = built.inputs(backend)
    method, descending, pct = sdc.rank_mode_of(case)
    rank, edges = core.bin_rank(*arrays[:d], values=arrays[d], bins=_bins_kw(built), axis=axis, method=method, descending=descending, pct=pct)
    _check_edges(edges, built)
    rank = check_output(rank, arrays, backend, case["shape"], F64, "rank")
    same(rank, sdc.rank_want(built.host, d, built.edges, axis, method, descending, pct), "bin_rank %s descending=%s pct=%s" % (method, descending, pct),
         nan_bits=False)


def _binned_outputs(outs, arrays, backend, shape, last, names):
    dts = (np.int64, np.int64, F64, last)
    return [check_output(o, arrays, backend, shape, dt, name) for o, dt, name in zip(outs, dts, names)]


def check_mode_case(core, case):
    built = vc.build(case)
    d, backend, axis = built.d, case["backend"], case["axis"]
    arrays = built.inputs(backend)
    *outs, edges = core.histogram_mode(*arrays[:d], values=arrays[d], bins=_bins_kw(built), axis=axis)
    _check_edges(edges, built)
    names = ("count", "nunique", "mode", "mode_count")
    got = _binned_outputs(outs, arrays, backend, kept_shape(case) + sdc.bins_shape(built.edges), np.int64, names)
    all_same(got, sdc.mode_want(built.host, d, built.edges, axis), names, "histogram_mode")


def _unique_outputs(outs, arrays, backend, case, built, width, weighted, inverse):
    kept, nb = kept_shape(case), sdc.n_bins_of(built.edges)
    spec = [("uniques", kept + (width,), F64), ("counts", kept + (width,), np.int64)]
    spec += [("weight_sums", kept + (width,), F64)] if weighted else []
    spec += [("offsets", kept + (nb + 1,), np.int64)] + ([("inverse", case["shape"], np.int64)] if inverse else [])
    assert len(outs) == len(spec), (len(outs), [s[0] for s in spec])
    return [check_output(o, arrays, backend, shape, dt, name) for o, (name, shape, dt) in zip(outs, spec)], tuple(s[0] for s in spec)


def check_unique_case(core, case):
    built = vc.build(case)
    d, backend, axis = built.d, case["backend"], case["axis"]
    arrays = built.inputs(backend)
    xs, bins = arrays[:d], _bins_kw(built)
    full = sdc.unique_want(built.host, d, built.edges, axis)
    size, inverse = sdc.size_of(case, sdc.u_max(full[2])), sdc.inverse_of(case)
    *outs, edges = core.bin_unique(*xs, values=arrays[d], bins=bins, axis=axis, size=size, return_inverse=inverse)
    _check_edges(edges, built)
    width = _reduced_extent(case) if size is None else size
    got, names = _unique_outputs(outs, arrays, backend, case, built, width, False, inverse)
    want = sdc.unique_want(built.host, d, built.edges, axis, size)
    all_same(got, want[:len(got)], names, "bin_unique size=%s" % size)
    count, nunique, _, _, _ = core.histogram_mode(*xs, values=arrays[d], bins=bins, axis=axis)
    count, nunique = _np(count), _np(nunique)
    np.testing.assert_array_equal(np.diff(got[2], axis=-1).reshape(nunique.shape), nunique, err_msg="np.diff(offsets) against nunique")
    if count.sum() > 0:
        np.testing.assert_array_equal(_np(core.histogram_mean_var(*xs, values=arrays[d], bins=bins, axis=axis)[0]), count,
                                      err_msg="histogram_mean_var's count")


def check_wunique_case(core, case):
    built = vc.build(case)
    d, backend, axis = built.d, case["backend"], case["axis"]
    arrays = built.inputs(backend)
    xs, bins = arrays[:d], _bins_kw(built)
    full = sdc.wunique_want(built.host, d, built.edges, axis)
    size, inverse = sdc.size_of(case, sdc.u_max(full[3])), sdc.inverse_of(case)
    kw = dict(values=arrays[d], bins=bins, axis=axis, size=size, return_inverse=inverse)
    *outs, edges = core.bin_weighted_unique(*xs, weights=arrays[d + 1], **kw)
    _check_edges(edges, built)
    width = _reduced_extent(case) if size is None else size
    got, names = _unique_outputs(outs, arrays, backend, case, built, width, True, inverse)
    want = sdc.wunique_want(built.host, d, built.edges, axis, size)
    all_same(got, want[:len(got)], names, "bin_weighted_unique size=%s" % size)
    twin = [_np(o) for o in core.bin_unique(*xs, **kw)[:-1]]  # the unweighted twin on the same arrays: every output but the sums
    all_same(got[:2] + got[3:], twin, names[:2] + names[3:], "bin_weighted_unique against bin_unique")


def check_wmode_case(core, case):
    built = vc.build(case)
    d, backend, axis = built.d, case["backend"], case["axis"]
    arrays = built.inputs(backend)
    xs, bins = arrays[:d], _bins_kw(built)
    *outs, edges = core.histogram_weighted_mode(*xs, values=arrays[d], weights=arrays[d + 1], bins=bins, axis=axis)
    _check_edges(edges, built)
    names = ("count", "nunique", "mode", "mode_weight")
    got = _binned_outputs(outs, arrays, backend, kept_shape(case) + sdc.bins_shape(built.edges), F64, names)
    all_same(got, sdc.wmode_want(built.host, d, built.edges, axis), names, "histogram_weighted_mode")
    twin = core.histogram_mode(*xs, values=arrays[d], bins=bins, axis=axis)
    all_same(got[:2], [_np(o) for o in twin[:2]], names[:2], "histogram_weighted_mode against histogram_mode")


CHECK_CASE = {"bin_sort": check_sort_case, "bin_rank": check_rank_case, "histogram_mode": check_mode_case, "bin_unique": check_unique_case,
              "bin_weighted_unique": check_wunique_case, "histogram_weighted_mode": check_wmode_case}


@pytest.mark.parametrize("call,stat", sdc.PAIRS, ids=PAIR_IDS)
def test_drawn_cases_match_oracle(xh, call, stat):
    each_case(stat, EXAMPLES, lambda case: CHECK_CASE[call](xh, case))


# Drawn cases that failed once, kept as they were drawn: (call, case) pairs (none so far: the test is a loop, so that an empty
# list does not skip).
DIRECTED_CASES = [
]


def test_drawn_cases_that_failed_once(xh):
    for call, case in DIRECTED_CASES:
        CHECK_CASE[call](xh, case)


# ---------------------------------------------------------------------------------------------------------------------
# (b) the blocks of a chunked call, as dask's tasks hand them to the per-block callables
# ---------------------------------------------------------------------------------------------------------------------
def _kept_cuts(case, salt):
    """(reduced axes sorted, per axis its chunks: 1..3 along a kept axis, one along a reduced one)"""
    rng = np.random.default_rng(case["seed"] + salt)
    red = sorted(set(vc.reduced_axes(case)))
    return red, [[(0, n)] if i in red else cuts_of(rng, n) for i, n in enumerate(case["shape"])]


def _blocks(cuts):
    for at in np.ndindex(*[len(c) for c in cuts]):
        yield tuple(slice(*c[j]) for c, j in zip(cuts, at))


def _bits(a):
    return np.ascontiguousarray(a).view(F64)


def _ints(a):
    return np.ascontiguousarray(a).view(np.int64)


def block_spec(core, call, case, built):
    """how one call is run blockwise: (run(blocks) -> the block's parts, want(host block) -> the oracle's parts, public(full) ->
    the unchunked call's parts, names, which parts are per sample, which are ranks).  A part that is not per sample is [block
    axes (reduced ones of extent 1), its own axes]; what the callables carry as bits is read back as what it is."""
    d, edges, shape = built.d, built.edges, case["shape"]
    ndim = len(shape)
    axis = onp.normalise_axis(case["axis"], ndim)  # (what _values_blockwise hands on)
    drop = axis or list(range(ndim))  # (what the grouped calls hand their blocks: list(drop_axes))
    c, nb, bins = _reduced_extent(case), sdc.n_bins_of(edges), _bins_kw(built)
    if call == "bin_sort":
        descending = sdc.descending_of(case)

        def run(blocks):
            out = core._bin_sort_block(*blocks, axis=drop, bins=edges, descending=descending)
            assert out.dtype == np.int64 and out.shape[-1] == c + nb + 1, (out.dtype, out.shape)
            return [out[..., :c], out[..., c:]]

        return (run, lambda host: sdc.sort_want(host, d, edges, drop, descending),
                lambda full: core.bin_sort(*full[:d], values=full[d], bins=bins, axis=case["axis"], descending=descending)[:2],
                ("order", "offsets"), (), ())
    if call == "bin_rank":
        method, descending, pct = sdc.rank_mode_of(case)
        kw = dict(method=method, descending=descending, pct=pct)
        return (lambda blocks: [core._bin_rank_block(*blocks, axis=drop, bins=edges, **kw)],
                lambda host: [sdc.rank_want(host, d, edges, drop, method, descending, pct)],
                lambda full: core.bin_rank(*full[:d], values=full[d], bins=bins, axis=case["axis"], **kw)[:1], ("rank",), (0,), (0,))
    if call in ("histogram_mode", "histogram_weighted_mode"):
        weighted = call == "histogram_weighted_mode"
        names = ("count", "nunique", "mode", "mode_weight" if weighted else "mode_count")

        def run(blocks):
            out = core._value_block(*blocks, stat="mode_w" if weighted else "mode", axis=axis, bins=edges)
            assert out.dtype == F64 and out.shape[0] == 4, (out.dtype, out.shape)
            return [_ints(out[0]), _ints(out[1]), out[2], out[3] if weighted else _ints(out[3])]

        def public(full):
            if weighted:
                return core.histogram_weighted_mode(*full[:d], values=full[d], weights=full[d + 1], bins=bins, axis=case["axis"])[:4]
            return core.histogram_mode(*full[:d], values=full[d], bins=bins, axis=case["axis"])[:4]

        return run, lambda host: (sdc.wmode_want if weighted else sdc.mode_want)(host, d, edges, drop), public, names, (), ()
    weighted = call == "bin_weighted_unique"
    want_fn = sdc.wunique_want if weighted else sdc.unique_want
    offsets = want_fn(built.host, d, edges, drop)[-2]
    width = sdc.size_of(case, sdc.u_max(offsets), none=c)  # (the dask graph hands its blocks the width, never None)
    k = 3 if weighted else 2

    def run(blocks):
        out = (core._bin_weighted_unique_block if weighted else core._bin_unique_block)(*blocks, axis=drop, bins=edges, size=width)
        assert out.dtype == np.int64 and out.shape[-1] == k * width + nb + 1, (out.dtype, out.shape)  # the packed block
        parts = [_bits(out[..., :width]), out[..., width:2 * width]] + ([_bits(out[..., 2 * width:3 * width])] if weighted else [])
        return parts + [out[..., k * width:], core._bin_unique_inverse_block(*blocks[:d + 1], axis=drop, bins=edges)]

    def public(full):
        kw = dict(values=full[d], bins=bins, axis=case["axis"], size=width, return_inverse=True)
        return (core.bin_weighted_unique(*full[:d], weights=full[d + 1], **kw) if weighted else core.bin_unique(*full[:d], **kw))[:-1]

    names = ("uniques", "counts") + (("weight_sums",) if weighted else ()) + ("offsets", "inverse")
    return run, lambda host: want_fn(host, d, edges, drop, width), public, names, (len(names) - 1,), ()


def check_blocks(core, call, case):
    built = vc.build(case)
    shape = case["shape"]
    red, cuts = _kept_cuts(case, 5 + sdc.CALLS.index(call))
    run, want, public, names, per_sample, ranks = block_spec(core, call, case, built)
    loose = tuple(names[i] for i in ranks)
    full = [np.broadcast_to(a, shape) for a in built.views]  # (dask broadcasts its arrays before it cuts them)
    lead = tuple(1 if i in red else n for i, n in enumerate(shape))
    whole = None
    for sl in _blocks(cuts):
        parts = run([a[sl] for a in full])
        here = tuple(1 if i in red else s.stop - s.start for i, s in enumerate(sl))
        for i, p in enumerate(parts):
            assert p.shape[:len(shape)] == (tuple(s.stop - s.start for s in sl) if i in per_sample else here), (names[i], p.shape, sl)
        got = [p if i in per_sample else p.squeeze(tuple(red)) for i, p in enumerate(parts)]
        all_same(got, want([np.ascontiguousarray(h[sl]) for h in built.host]), names, "%s of block %s" % (call, sl), loose)
        if whole is None:
            whole = [np.zeros((tuple(shape) if i in per_sample else lead) + p.shape[len(shape):], p.dtype) for i, p in enumerate(parts)]
        for i, p in enumerate(parts):
            whole[i][sl if i in per_sample else tuple(slice(None) if j in red else s for j, s in enumerate(sl))] = p
    outs = [_np(o) for o in public(full)]
    whole = [w if i in per_sample else w.squeeze(tuple(red)) for i, w in enumerate(whole)]
    all_same(whole, outs, names, "%s: the blocks put together against the unchunked call" % call, loose)


@pytest.mark.parametrize("call,stat", sdc.PAIRS, ids=PAIR_IDS)
def test_blocks_as_dask_hands_them(xh, call, stat):
    each_case(stat, BLOCK_EXAMPLES, lambda case: check_blocks(xh, call, case))


DIRECTED_BLOCKS = [
]


def test_blocks_of_drawn_cases_that_failed_once(xh):
    for call, case in DIRECTED_BLOCKS:
        check_blocks(xh, call, case)


class _Chunked:
    """just enough of a dask array for the front of a call: its shape, its dtype and its chunks along each axis"""
    def __init__(self, shape, chunks):
        self.shape, self.ndim, self.chunks, self.dtype = tuple(shape), len(shape), chunks, np.dtype(F64)


@pytest.mark.parametrize("call", sdc.CALLS)
def test_a_cut_reduced_axis_is_refused(xh, monkeypatch, call):
    """The first drawn case of the call with a reduced axis of two elements or more, that axis cut into two chunks and the kept
    axes as (b) cuts them: the public call raises the ValueError of core._check_one_chunk, word for word, with the call's own noun,
    before any device work and before any graph is made; with the axis whole it goes on to make the graph."""
    cases = []
    for_each_case(sdc.DRAWS[call][0], BLOCK_EXAMPLES, cases.append)
    case = next(c for c in cases if any(c["shape"][a] >= 2 for a in vc.reduced_axes(c)) and 0 not in c["shape"])
    built = vc.build(case)
    shape, ndim = case["shape"], len(case["shape"])
    red, cuts = _kept_cuts(case, 11)
    cut = next(a for a in red if shape[a] >= 2)
    axis = onp.normalise_axis(case["axis"], ndim)
    drop = tuple(axis) if axis is not None else tuple(range(ndim))
    n_arrays = built.d + (2 if "weighted" in call else 1)

    def boom(*a, **k):
        pytest.fail("device work, or a graph")

    for fn in ("_upload_host", "_value_views", "_get_plan", "_value_rows", "_resident", "_sample_blockwise", "_packed_blockwise", "_values_blockwise"):
        monkeypatch.setattr(xh, fn, boom)

    def call_with(chunks):
        arrays = [_Chunked(shape, chunks)] * n_arrays
        monkeypatch.setattr(xh, "_values_call", lambda *a, **k: ("dask", arrays, None, built.edges, axis, drop))
        kw = dict(values=arrays[built.d], bins=built.edges, axis=case["axis"])
        if "weighted" in call:
            kw["weights"] = arrays[built.d + 1]
        return arrays, lambda: getattr(xh, call)(*arrays[:built.d], **kw)

    whole = tuple(tuple(b - a for a, b in c) for c in cuts)
    halves = tuple((1, shape[i] - 1) if i == cut else ch for i, ch in enumerate(whole))
    arrays, go = call_with(halves)
    with pytest.raises(ValueError) as mine:
        xh._check_one_chunk(sdc.NOUNS[call], arrays, drop)
    assert str(mine.value).startswith("%s of several chunks cannot be merged: rechunk the reduced axes" % sdc.NOUNS[call])
    with pytest.raises(ValueError) as theirs:
        go()
    assert str(theirs.value) == str(mine.value)
    _, go = call_with(whole)
    with pytest.raises(pytest.fail.Exception, match="device work, or a graph"):
        go()


# ---------------------------------------------------------------------------------------------------------------------
# (c) dirty scratch  (before (d) and (e): they leave hundreds of megabytes of blocks in the cache)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scratch_host(seed):
    return sdc.scratch_data(seed)


@functools.lru_cache(maxsize=None)
def _scratch_dev(seed):
    return tuple(torch.as_tensor(a).cuda() for a in _scratch_host(seed))


def scratch_call(core, name, x, v, w):
    """one of sorted_cases.SCRATCH_CALLS (or bin_order) on [3, 70 001] arrays over axis 1: its outputs without the edges"""
    if name == "bin_order":
        return core.bin_order(x, bins=[sdc.SCRATCH_EDGES], axis=1)[:-1]
    fn, kw, weighted = sdc.SCRATCH_CALLS[name]
    return getattr(core, fn)(x, values=v, bins=[sdc.SCRATCH_EDGES], axis=1, **kw, **(dict(weights=w) if weighted else {}))[:-1]


def _drain(native, size):
    """every cached block a request of `size` bytes could be given, and the fresh one that shows there is none left"""
    out = []
    for _ in range(20_000):
        before = native.scratch_stats(0)["cached"]
        out.append(native.DeviceBuffer(0, size))
        if native.scratch_stats(0)["cached"] == before:  # (a fresh allocation: the cache had nothing left for it)
            return out
    raise AssertionError("the scratch cache never ran out of blocks")


@pytest.mark.parametrize("name", list(sdc.SCRATCH_CALLS))
def test_a_call_initialises_the_scratch_it_inherits(xh, name):
    """The method of test_gpu_values_properties.test_a_statistic_initialises_the_scratch_it_inherits, for the calls that hold the
    most scratch.  A call takes the sort's seven blocks (three of R * C * 8 bytes, two of R * C * 4, the counters of the chunks and
    of the slices) and, all but bin_sort, one block that sorted_domain_run carves into order, offsets, head and NaN words, before /
    last / next, the tiles' part, the divisors (pct) and the weighted twins' lead, tail, tsum, tflag and per-position sums;
    sorted_cases.scratch_requests restates the sizes.  First every cached block that a request of one of these sizes could be
    given is held out of the cache for the whole test, so that a call on other data of the same shape makes blocks of exactly
    its sizes.  Then, for the same stream and for another one: those blocks (and one more of each size) are taken out of the cache,
    filled with bytes of all ones and given back; a block of the largest size, taken and read back right then, is all ones; the
    call runs on the real data, allocates nothing (cached + live does not grow: every block it took was a dirty one) and gives
    the oracle's bits.  A call's requests are below 11 MB, twice over below the 64 MiB the cache always keeps: nothing is
    evicted."""
    from xhistogram_amd import _native

    sizes = sorted(set(sdc.scratch_requests(name, _cus())), reverse=True)  # (descending: every size takes the blocks of its own class)
    want = sdc.scratch_want(name, *_scratch_host(31))
    names = ["output %d" % i for i in range(len(want))]
    loose = names if name.startswith("bin_rank") else ()
    data, other = _scratch_dev(31), _scratch_dev(32)
    side = side_streams(1)[0]

    def total():
        s = _native.scratch_stats(0)
        return s["cached"] + s["live"]

    torch.cuda.synchronize()
    held = []
    try:
        for size in sizes:
            held += _drain(_native, size)
        scratch_call(xh, name, *other)  # makes the blocks of this call
        torch.cuda.synchronize()
        made = total()
        scratch_call(xh, name, *other)
        torch.cuda.synchronize()
        assert total() <= made, "a second call of the same shape allocated scratch: sorted_cases.scratch_requests misses a request"
        for where in ("same stream", "another stream"):
            taken = [(size, buf) for size in sizes for buf in _drain(_native, size)]
            assert len(taken) >= len(sdc.scratch_requests(name, _cus())) and sum(s for s, _ in taken) < 32 << 20, [s for s, _ in taken]
            for size, buf in taken:
                buf.upload(np.full(size, 0xFF, np.uint8))
            for _, buf in taken:
                buf.close()
            torch.cuda.synchronize()
            probe = _native.DeviceBuffer(0, sizes[0])  # the control: what a request of the carved block's size is handed
            back = np.zeros(sizes[0], np.uint8)
            probe.download(back)
            probe.close()
            assert (back == 0xFF).all(), "a cached block of %d bytes does not read all ones before the call" % sizes[0]
            torch.cuda.synchronize()
            before = total()
            if where == "same stream":
                outs = scratch_call(xh, name, *data)
            else:
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    outs = scratch_call(xh, name, *data)
            torch.cuda.synchronize()
            assert total() <= before, "%s took a fresh block from the driver, not the dirty ones (%s): %d -> %d bytes" % (name, where, before, total())
            all_same(outs, want, names, "%s on dirty scratch, %s" % (name, where), loose)
    finally:
        for h in held:
            h.close()


# ---------------------------------------------------------------------------------------------------------------------
# (d) a row of more than 256 tiles with heads everywhere
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_row(xh):
    """(the closed form, samples float64 and values float32 on the device)"""
    row = sdc.LongRow()
    x, v = torch.as_tensor(row.samples()).cuda(), torch.as_tensor(row.values()).cuda()
    yield row, x, v
    del x, v
    torch.cuda.empty_cache()


LONG_RANKS = [("average", False), ("average", True), ("dense", False), ("dense", True)]


@pytest.mark.parametrize("method,descending", LONG_RANKS, ids=["%s-%s" % (m, "descending" if d else "ascending") for m, d in LONG_RANKS])
def test_long_row_rank(xh, long_row, method, descending):
    """rank_scan with two tiles per thread: `before` of every word of a thread's second tile holds the heads of its first
    (run_sum += a), `last` of a word in a tile without a head comes from the tiles before (run_max) and `next` from those after
    (the reversed run_min walk), over the border of two threads' tiles too; threads 129..255 own no tile.  pct: the divisors of
    rank_bins, which for dense are head counts over the whole bin.  (Measured once on a build without `run_sum += a;`: 8 396 433
    of the 16 847 217 dense ranks differ here, while every test of tests/test_gpu_bin_rank.py passes on that build.)"""
    row, x, v = long_row
    rank, _ = xh.bin_rank(x, values=v, bins=[sdc.LONG_EDGES], method=method, descending=descending, pct=True)
    same(rank, row.rank(method, descending, True), "bin_rank %s descending=%s pct on 258 tiles" % (method, descending), nan_bits=False)
    if method == "average":  # min and max are its two halves: once each, without pct
        other = "max" if descending else "min"
        same(xh.bin_rank(x, values=v, bins=[sdc.LONG_EDGES], method=other, descending=descending)[0], row.rank(other, descending), other, nan_bits=False)


def test_long_row_mode_and_unique(xh, long_row):
    row, x, v = long_row
    got = xh.histogram_mode(x, values=v, bins=[sdc.LONG_EDGES])[:4]
    mdo.assert_same([_np(o) for o in got], row.mode(), "histogram_mode on 258 tiles")
    uniques, counts, offsets, inverse = row.unique()
    u, n = int(offsets[2]), row.n
    got = xh.bin_unique(x, values=v, bins=[sdc.LONG_EDGES], return_inverse=True)[:4]  # (size=None: the width is the row)
    pad = n - u
    all_same(got, (np.concatenate([uniques, np.full(pad, uo.PAD)]), np.concatenate([counts, np.zeros(pad, np.int64)]), offsets, inverse),
             ("uniques", "counts", "offsets", "inverse"), "bin_unique on 258 tiles")


def test_long_row_weighted(xh, long_row):
    """exactly summable weights: a run's sum is the same float64 in any order, so np.bincount by entry is the closed form"""
    row, x, v = long_row
    xw.assert_summable(row.n)
    w = xw.f64(np.random.default_rng(258), row.n, "both")
    w_t = torch.as_tensor(w).cuda()
    uniques, counts, offsets, inverse = row.unique()
    u = int(offsets[2])
    size = u + 3
    got = xh.bin_weighted_unique(x, values=v, weights=w_t, bins=[sdc.LONG_EDGES], size=size, return_inverse=True)[:5]
    want = (np.concatenate([uniques, np.full(3, uo.PAD)]), np.concatenate([counts, np.zeros(3, np.int64)]),
            np.concatenate([row.weight_sums(w), np.zeros(3)]), offsets, inverse)
    all_same(got, want, ("uniques", "counts", "weight_sums", "offsets", "inverse"), "bin_weighted_unique on 258 tiles")
    got = xh.histogram_weighted_mode(x, values=v, weights=w_t, bins=[sdc.LONG_EDGES])[:4]
    wo.assert_mode_same([_np(o) for o in got], row.weighted_mode(w), "histogram_weighted_mode on 258 tiles")


def test_long_row_sort_and_ordinal(xh, long_row):
    """The order inside a run depends on the input positions, which no closed form of the slots gives: bin_sort's order and the
    ordinal rank are held to each other and to the runs, on the device.  rank_ordinal[order[j]] == j - offsets[key] + 1; the
    run of order[j] is the run of j (so values[order] ascends inside every segment, NaN last); positions ascend inside a run."""
    row, x, v = long_row
    n = row.n
    order, offsets, _ = xh.bin_sort(x, values=v, bins=[sdc.LONG_EDGES])
    ordinal, _ = xh.bin_rank(x, values=v, bins=[sdc.LONG_EDGES], method="ordinal")
    same(offsets, np.array([0, row.n0, row.n0 + row.n1]), "offsets")
    assert order.shape == (n,) and order.dtype == torch.int64
    dev = lambda a: torch.as_tensor(a).cuda()  # noqa: E731
    j = torch.arange(n, device="cuda")
    assert bool((torch.sort(order).values == j).all()), "order is not a permutation"
    start, length = dev(row.start), dev(row.length)
    key = (j >= row.n0).long() + (j >= row.n0 + row.n1).long()  # the segment of a sorted position: bin 0, bin 1, dropped
    got_bin = dev(np.where(row.bin < 0, 2, row.bin))[order]
    assert bool((got_bin == key).all()), "a sample sorted into another segment than its bin's"
    is_nan = dev(row.nan)[order]
    nan_zone = (j >= row.n0 - row.nans) & (j < row.n0)
    assert bool((is_nan == nan_zone).all()), "the NaN values are not the last of bin 0"
    run_of_j = (j - start[key]) // length[key]
    there = ~nan_zone
    assert bool((dev(row.run)[order][there] == run_of_j[there]).all()), "a sample sorted into another run than its value's"
    sorted_v = v[order].double()
    inside = (key[1:] == key[:-1]) & there[1:] & there[:-1]
    assert bool((sorted_v[1:][inside] >= sorted_v[:-1][inside]).all()), "values[order] descends inside a segment"
    tie = inside & (run_of_j[1:] == run_of_j[:-1])
    tie |= nan_zone[1:] & nan_zone[:-1]  # (the NaN values are one run of equal keys)
    assert bool((order[1:][tie] > order[:-1][tie]).all()), "positions do not ascend inside a run"
    valid = there & (key < 2)
    want = (j - dev(np.array([0, row.n0, row.n0 + row.n1]))[key] + 1).double()
    got = ordinal[order]
    assert bool((got[valid] == want[valid]).all()), "the ordinal rank is not the place in bin_sort's segment"
    assert bool(torch.isnan(got[~valid]).all()), "an ordinal rank for a dropped sample or a NaN value"


# ---------------------------------------------------------------------------------------------------------------------
# (e) different calls at once
# ---------------------------------------------------------------------------------------------------------------------
def test_different_calls_at_once(xh):
    """8 threads with a stream (test_gpu_bin_order.side_streams: no stream is made here) and rows of their own share one edge
    array, so one cached plan, and run bin_sort, bin_rank (average), bin_rank (dense, pct), histogram_mode, bin_unique with an
    inverse, bin_weighted_unique, histogram_weighted_mode and bin_order: thread t runs call (t + round) mod 8 in each of three
    rounds.  The calls ask the scratch cache for three blocks of n * 8 bytes, two of n * 4, the counters, and a carved block whose
    size differs by call (bin_order: its own three), so a block freed by one call on one stream is what another call on another
    stream asks for next; the cache hands it over once an event has passed.  The inputs are made on the thread's stream by device
    arithmetic (twice the halves uploaded beforehand: exact) and handed over without synchronising.  Every result carries the
    bits of the same call on the same rows made alone beforehand; what those bits must be is (c)'s business."""
    n_threads, rounds = 8, 3
    calls = sdc.THREAD_CALLS
    halves = [[torch.as_tensor(a * 0.5).cuda() for a in sdc.scratch_data(100 + t)] for t in range(n_threads)]
    torch.cuda.synchronize()
    alone = {}
    for t in range(n_threads):
        for rnd in range(rounds):
            name = calls[(t + rnd) % len(calls)]
            alone[t, name] = [_np(o) for o in scratch_call(xh, name, *[h * 2.0 for h in halves[t]])]
    torch.cuda.synchronize()
    streams = side_streams(n_threads)
    results = [[] for _ in range(n_threads)]
    errors = []

    def work(t):
        try:
            for rnd in range(rounds):
                name = calls[(t + rnd) % len(calls)]
                with torch.cuda.stream(streams[t]):
                    outs = scratch_call(xh, name, *[h * 2.0 for h in halves[t]])  # (on this stream, and nobody waits for it)
                    streams[t].synchronize()
                    results[t].append((name, [_np(o) for o in outs]))
        except Exception as e:  # pragma: no cover
            errors.append("thread %d: %r" % (t, e))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(n_threads)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(n_threads):
        assert [name for name, _ in results[t]] == [calls[(t + rnd) % len(calls)] for rnd in range(rounds)]
        for rnd, (name, outs) in enumerate(results[t]):
            want = alone[t, name]
            assert len(outs) == len(want)
            for i, (g, w) in enumerate(zip(outs, want)):
                assert g.shape == w.shape and g.dtype == w.dtype and g.dtype in (np.int64, F64), (name, i, g.shape, g.dtype)
                assert np.array_equal(_ints(g), _ints(w)), "thread %d round %d: output %d of %s differs from the call made alone" % (t, rnd, i, name)
