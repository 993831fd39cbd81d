"""tests/sorted_cases.py held to what it claims, without a GPU: the cases tests/test_gpu_sorted_properties.py replays on the six
calls of the sorted order hold bins, tie runs, NaN values and rows that can go wrong, every per-call parameter drawn from a seed
occurs, the oracles give every public shape on every drawn case (the empty ones included), the dirty-scratch shape is what its
comments say and its requests are restated from the drivers, and the closed form of the row of 258 tiles is the oracles' on a row
small enough to sort.  pytest -s prints the tallies the GPU file's docstring quotes."""
import collections
import functools

import numpy as np
import pytest

import bin_order_oracle as bo
import bin_rank_cases as rc
import bin_rank_oracle as ro
import bin_sort_oracle as so
import bin_unique_oracle as uo
import exact_weights as xw
import map_oracle as mo
import mode_oracle as mdo
import sorted_cases as sdc
import values_cases as vc
import weighted_unique_oracle as wo

hyp = pytest.importorskip("hypothesis")
torch = pytest.importorskip("torch")  # (for_each_case lives in a GPU file that imports it; none of this needs a GPU)

import test_gpu_values_properties as tgp  # noqa: E402

F64 = np.float64
CUS = rc.CUS
FLOORS = {"a bin of two or more values": 50, "a tie run inside a bin": 40, "a NaN in a counted bin": 10,
          "the same value in two bins of a row": 40, "rows longer than 64": 35}


@functools.lru_cache(maxsize=None)
def drawn(stat, n=tgp.EXAMPLES):
    out = []
    tgp.for_each_case(stat, n, out.append)
    assert len(out) == n
    return out


def test_the_calls_replay_existing_draws():
    assert set(sdc.ALL_DRAWS) == {s for stats in sdc.DRAWS.values() for s in stats} <= set(vc.STATS)
    assert len(sdc.PAIRS) == 12 and set(sdc.NOUNS) == set(sdc.CALLS)
    for call in ("bin_weighted_unique", "histogram_weighted_mode"):
        assert set(sdc.DRAWS[call]) <= set(vc.WEIGHTED)
    for stat in sdc.ALL_DRAWS:
        assert repr(drawn(stat, tgp.BLOCK_EXAMPLES)) == repr(drawn(stat)[:tgp.BLOCK_EXAMPLES])


# ---------------------------------------------------------------------------------------------------------------------
# (a) what the drawn cases hold
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stat", sdc.ALL_DRAWS)
def test_drawn_cases_meet_their_conditions(stat):
    t = collections.Counter()
    longest = most = 0
    for case in drawn(stat) + sdc.directed(stat):
        b = vc.build(case)
        got = sdc.census(b, case["axis"])
        longest, most = max(longest, got.pop("row")), max(most, got.pop("rows"))
        for k, v in got.items():
            t[k] += bool(v)
        t["values " + b.host[b.d].dtype.name] += 1
        t["backend " + case["backend"]] += 1
    print("\n%s, 60 drawn cases and %d directed ones: %s; the longest row %d, the most rows %d" % (
        stat, len(sdc.directed(stat)), ", ".join("%s %d" % kv for kv in sorted(t.items())), longest, most))
    for what, floor in FLOORS.items():
        assert t[what] >= floor, (stat, what, t[what])
    assert t["no counted sample"] <= 6 and t["an extent of 0"] >= 1
    if stat == "argextrema":
        assert t["both zeros in one bin"] >= 1
        assert t["values int64"] >= 1 and t["values float16"] >= 1 and t["values bool"] >= 1


@pytest.mark.parametrize("call,stat", sdc.PAIRS)
def test_the_oracles_give_the_public_shapes(call, stat):
    """every want of sorted_cases on every drawn case, the empty ones included: shapes and dtypes of the public call"""
    for case in drawn(stat) + sdc.directed(stat):
        b = vc.build(case)
        d, edges, axis, shape = b.d, b.edges, case["axis"], case["shape"]
        kept = tgp.kept_shape(case)
        c = int(np.prod([shape[i] for i in set(vc.reduced_axes(case))], dtype=np.int64))
        nb, binned = sdc.n_bins_of(edges), kept + sdc.bins_shape(edges)
        if call == "bin_sort":
            order, offsets = sdc.sort_want(b.host, d, edges, axis, sdc.descending_of(case))
            assert order.shape == kept + (c,) and offsets.shape == kept + (nb + 1,) and order.dtype == offsets.dtype == np.int64
            idx, (v,) = sdc.rows(b.host[:d + 1], d, edges, axis)
            plain = bo.order_offsets(idx, nb)
            mo.assert_bits(plain[1], offsets, "bin_order's offsets")
            if not sdc.descending_of(case):  # the identity the GPU file holds bin_sort and bin_order to
                mo.assert_bits(sdc.stable_by_value(plain[0], plain[1], v), order, "bin_order's order sorted stably by value")
        elif call == "bin_rank":
            rank = sdc.rank_want(b.host, d, edges, axis, *sdc.rank_mode_of(case))
            assert rank.shape == shape and rank.dtype == F64
        elif call in ("histogram_mode", "histogram_weighted_mode"):
            outs = (sdc.mode_want if call == "histogram_mode" else sdc.wmode_want)(b.host, d, edges, axis)
            last = np.int64 if call == "histogram_mode" else F64  # (mode_count, mode_weight)
            assert all(o.shape == binned for o in outs) and [o.dtype for o in outs] == [np.int64, np.int64, F64, last]
        else:
            want = sdc.unique_want if call == "bin_unique" else sdc.wunique_want
            full = want(b.host, d, edges, axis)
            size = sdc.size_of(case, sdc.u_max(full[-2]))
            outs = want(b.host, d, edges, axis, size)
            w = c if size is None else size
            assert all(o.shape == kept + (w,) for o in outs[:-2]) and outs[-2].shape == kept + (nb + 1,) and outs[-1].shape == shape
            mo.assert_bits(outs[-2], full[-2], "the offsets whatever the size")
            mo.assert_bits(outs[-1], full[-1], "the inverse whatever the size")
            if call == "bin_weighted_unique":  # the weights of build(): integers 0..7, exactly summable
                assert np.array_equal(b.host[d + 1].astype(F64), np.rint(b.host[d + 1].astype(F64))) and np.abs(b.host[d + 1].astype(F64)).max(initial=0) <= 7


def test_every_parameter_drawn_from_a_seed_occurs():
    modes = collections.Counter(sdc.rank_mode_of(c) for stat in sdc.DRAWS["bin_rank"] for c in drawn(stat))
    print("\nbin_rank's modes over the 120 cases: %s" % sorted(modes.values()))
    assert set(modes) == set(rc.MODES) and len(rc.MODES) == 20
    for call in ("bin_unique", "bin_weighted_unique"):
        cases = [c for stat in sdc.DRAWS[call] for c in drawn(stat)]
        sizes = collections.Counter(c["seed"] % 6 for c in cases)
        inverse = collections.Counter(sdc.inverse_of(c) for c in cases)
        print("%s: sizes (None, 0, 1, U // 2, U, U + 3) %s, with an inverse %d of %d" % (call, [sizes[i] for i in range(6)], inverse[True], len(cases)))
        assert all(sizes[i] >= 5 for i in range(6)) and min(inverse.values()) >= 30
    down = collections.Counter(sdc.descending_of(c) for stat in sdc.DRAWS["bin_sort"] for c in drawn(stat))
    print("bin_sort: descending %d of 120" % down[True])
    assert min(down.values()) >= 30
    assert sdc.size_of({"seed": 12}, 9, none=77) == 77 and [sdc.size_of({"seed": i}, 9) for i in range(1, 6)] == [0, 1, 4, 9, 12]


# ---------------------------------------------------------------------------------------------------------------------
# (c), (e) the dirty-scratch shape
# ---------------------------------------------------------------------------------------------------------------------
def test_scratch_data_is_what_it_says():
    R, C, B = sdc.SCRATCH_ROWS, sdc.SCRATCH_COLS, sdc.SCRATCH_BINS
    words = -(-C // 64)
    assert (R, C, B) == (3, 70_001, 127) and words == 1094 and C - (words - 1) * 64 == 49 and C % 64 != 0
    assert -(-words // sdc.TILE_WORDS) == 2 and words - sdc.TILE_WORDS == 70
    xw.assert_summable(C)
    x, v, w = sdc.scratch_data(0)
    x2, v2, _ = sdc.scratch_data(1)
    assert x.shape == v.shape == w.shape == (R, C) and not np.array_equal(x, x2, equal_nan=True) and not np.array_equal(v, v2, equal_nan=True)
    rest = v[v != sdc.SCRATCH_RUN_VALUE]  # (the values outside the run of 66 000: one in a hundred is NaN)
    assert rest.size == R * (C - sdc.SCRATCH_RUN) and 0.005 < np.isnan(rest).mean() < 0.015
    assert np.isnan(x).any() and (w < 0).any() and (w > 0).any()
    assert np.array_equal(v[~np.isnan(v)], np.round(v[~np.isnan(v)], 1))
    idx = mo.index([x], [sdc.SCRATCH_EDGES])
    assert (idx < 0).any() and len(np.unique(idx)) > 100
    crossing = heads_in_both = 0
    for r in range(R):
        _, ks, vs, head = ro.sorted_domain(idx[r], v[r], B)
        s, e = rc.runs_of(head)
        long = np.flatnonzero((e - s >= sdc.SCRATCH_RUN) & (ks[s] == sdc.SCRATCH_RUN_BIN))
        assert len(long) == 1 and vs[s[long[0]]] == sdc.SCRATCH_RUN_VALUE
        crossing += s[long[0]] < sdc.TILE < e[long[0]]  # the run crosses the border of the two tiles
        heads_in_both += (s < sdc.TILE).sum() > 1000 and (s >= sdc.TILE).sum() > 1000
        assert np.isnan(vs[ks < B]).sum() > 10
    print("\nscratch data: %d words a row, the last 49 wide; the run of %d crosses the tile border in %d of %d rows" % (words, sdc.SCRATCH_RUN, crossing, R))
    assert crossing == R and heads_in_both == R
    u = sdc.unique_want([x, v], 1, [sdc.SCRATCH_EDGES], 1)[2][:, -1]
    assert (u > 1000).all() and sdc.SCRATCH_CUT < C  # (a cut size that keeps entries and pads none away is still a cut: below c)


def test_scratch_requests_are_restated_from_the_drivers():
    R, C, B = sdc.SCRATCH_ROWS, sdc.SCRATCH_COLS, sdc.SCRATCH_BINS
    n = R * C
    sort = sdc.sort_requests(CUS, R, C)
    g = so.geometry(CUS, R, C)
    assert g["chunks"] > 1 and g["slices"] == 2 and g["rows_per_launch"] >= R
    assert sort == [n * 8] * 3 + [n * 4] * 2 + [R * g["chunks"] * 1024, R * 2 * 1024] and len(sort) == 7 and min(sort) > 4096
    nw = R * 1094
    plain = (n + R * (B + 1) + 2 * nw) * 8 + (3 * nw + 3 * R * 2) * 4
    assert sdc.domain_bytes(R, C, B) == plain and sdc.domain_bytes(R, C, B, pct=True) == plain + R * B * 8
    assert sdc.wruns_bytes(R, C, False) == (2 * nw + 2 * R * 2) * 8 and sdc.wruns_bytes(R, C, True) == (2 * nw + 2 * R * 2 + n) * 8
    carved = {}
    for name in sdc.SCRATCH_CALLS:
        req = sdc.scratch_requests(name, CUS)
        assert req[-7:] == sort and len(req) == (7 if name == "bin_sort" else 8)
        assert sum(req) < 16 << 20  # (with one block more per size, far below the 64 MiB the cache always keeps)
        carved[name] = req[0] if len(req) == 8 else None
    assert carved["bin_rank"] == carved["histogram_mode"] == carved["bin_unique"] == carved["bin_unique_inverse"] == plain
    assert carved["bin_rank_pct"] == plain + R * B * 8
    assert carved["bin_weighted_unique"] == carved["bin_weighted_unique_cut"] == plain + sdc.wruns_bytes(R, C, False)
    assert carved["histogram_weighted_mode"] == plain + sdc.wruns_bytes(R, C, True)
    assert set(sdc.THREAD_CALLS) - {"bin_order"} <= set(sdc.SCRATCH_CALLS) and len(sdc.THREAD_CALLS) == 8
    print("\nscratch of a call at %d x %d, %d bins: %s" % (R, C, B, {k: sum(sdc.scratch_requests(k, CUS)) for k in sdc.SCRATCH_CALLS}))


# ---------------------------------------------------------------------------------------------------------------------
# (d) the row of 258 tiles
# ---------------------------------------------------------------------------------------------------------------------
def test_long_row_claims():
    """the full-size row: 258 tiles, so two per thread of rank_scan; tiles without a head; a run across the border of thread 0's
    and thread 1's tiles; heads in the tiles of most threads"""
    row = sdc.LongRow()
    n = row.n
    assert n == 256 * 65_536 + 70_001 and np.array_equal(np.sort(row.s), np.arange(n))
    words = -(-n // 64)
    tiles = -(-words // sdc.TILE_WORDS)
    per = -(-tiles // 256)
    assert tiles == 258 and per == 2 and row.n0 % 64 != 0 and abs(row.n0 / n - 0.6) < 0.001 and abs(row.n1 / n - 0.3) < 0.001
    assert 128 * per < tiles <= 129 * per  # (thread 128 owns the last two tiles, threads 129..255 none)
    v = row.values()
    assert v.dtype == np.float32 and np.nanmax(v) < 1 << 24 and np.isnan(v).sum() == sdc.LONG_NANS
    xw.assert_summable(n)
    heads = row.heads()
    assert np.all(np.diff(heads) > 0) and heads[0] == 0
    per_tile = np.bincount(heads // sdc.TILE, minlength=tiles)
    empty = np.flatnonzero(per_tile == 0)
    assert len(empty) >= 10 and empty.max() < row.n0 // sdc.TILE  # (bin 0's runs are longer than a tile)
    border = per * sdc.TILE  # the end of tile 1: where thread 0's tiles end and thread 1's begin
    k = border // sdc.LONG_RUN0
    assert k * sdc.LONG_RUN0 < border < (k + 1) * sdc.LONG_RUN0 <= row.m[0], "no run of bin 0 crosses the border of two threads' tiles"
    threads = lambda h: np.unique(h // sdc.TILE // per)  # noqa: E731
    in1 = heads[(heads >= row.n0) & (heads < row.n0 + row.n1)]
    in0 = heads[heads < row.n0 - row.nans]
    # bin 1 is 0.3 n, 78 of the 258 tiles, so its heads lie in the tiles of 39 or 40 threads and no more; with bin 0's and the
    # dropped samples' runs every thread that owns a tile carries heads into the next one's
    print("\nlong row: %d tiles, %d without a head; heads of bin 0 in the tiles of %d threads, of bin 1 of %d, of all of %d; a word of bin 1 holds %d heads"
          % (tiles, len(empty), len(threads(in0)), len(threads(in1)), len(threads(heads)), 64 // sdc.LONG_RUN1))
    assert len(threads(in1)) >= 39 and len(threads(in0)) >= 60 and len(threads(heads)) >= 125
    assert (per_tile[1::2] > 0).sum() >= 100  # (the second tile of a thread adds heads: run_sum += a carries something)
    assert int(row.offsets[2]) + 3 < n


SMALL = dict(n=5003, m=1237, n0=3001, n1=1500, run0=211, run1=3, nans=50)


def test_long_row_closed_form_is_the_oracle():
    """the same construction at 5003 samples (runs of 211 over words of 64, a last run that is cut short by the NaNs) against
    the oracles on the arrays themselves"""
    row = sdc.LongRow(**SMALL)
    x, v = row.samples(), row.values()
    idx = mo.index([x], [sdc.LONG_EDGES])
    np.testing.assert_array_equal(idx, row.bin)
    _, ks, vs, head = ro.sorted_domain(idx, v, 2)
    np.testing.assert_array_equal(np.flatnonzero(head), row.heads())
    for method in ("min", "max", "average", "dense"):
        for descending in (False, True):
            for pct in (False, True):
                mo.assert_bits(row.rank(method, descending, pct), ro.rank_row(idx, v, 2, method, descending, pct), "%s %s %s" % (method, descending, pct))
    mdo.assert_same(row.mode(), mdo.mode_row(idx, v, 2), "mode")
    uniques, counts, offsets, inverse = row.unique()
    u = int(offsets[2])
    want = uo.unique_row(idx, v, 2)
    uo.assert_same((np.concatenate([uniques, np.full(row.n - u, uo.PAD)]), np.concatenate([counts, np.zeros(row.n - u, np.int64)]), offsets, inverse), want, "unique")
    w = xw.f64(np.random.default_rng(5), row.n, "both")
    wu = wo.wunique_row(idx, v, w, 2)
    wo.assert_sums(row.weight_sums(w), wu[2][:u], "weight sums")
    wo.assert_mode_same(row.weighted_mode(w), wo.wmode_row(idx, v, w, 2), "weighted mode")
    # the two identities the GPU file holds bin_sort and the ordinal rank to each other with
    order, off = so.order_offsets(idx, v, 2)
    ordinal = ro.rank_row(idx, v, 2, "ordinal")
    j = np.arange(row.n)
    ok = row.valid[order]
    np.testing.assert_array_equal(ordinal[order][ok], (j - off[np.minimum(ks, 1)] + 1)[ok])
    there = ~row.nan[order]  # (the NaN values of bin 0 are one run of equal keys: in position order, whatever their slots)
    np.testing.assert_array_equal(row.run[order][there], ((j - row.start[row.bin[order]]) // row.length[row.bin[order]])[there])
