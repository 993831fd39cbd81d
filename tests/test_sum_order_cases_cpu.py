"""tests/sum_order_cases.py held to what it claims, without a GPU: the replayed cases of tests/test_gpu_sum_order_properties.py
count something and hold bins that can go wrong, the replacement values leave the case's own stream alone and tell integer
limbs from float additions, the position of a maximum found through the order is histogram_argextrema's, and the row-batch
test's closed form is the oracle on real rows on both sides of the batch boundary, with values that make another row's keys
visible.  pytest -s prints the tallies the GPU file's docstring quotes."""
import collections
import functools
import math

import numpy as np
import pytest

import argextrema_oracle as ao
import bin_order_oracle as bo
import map_cases as mc
import map_oracle as mo
import sum_cases as sc
import sum_oracle as so
import sum_order_cases as soc
import values_cases as vc

hyp = pytest.importorskip("hypothesis")
torch = pytest.importorskip("torch")  # (for_each_case lives in a GPU file that imports it; none of this needs a GPU)

import test_gpu_sum as tgs  # noqa: E402
import test_gpu_values_properties as tgp  # noqa: E402

F64 = np.float64


@functools.lru_cache(maxsize=None)
def drawn(stat, n=tgp.EXAMPLES):
    out = []
    tgp.for_each_case(stat, n, out.append)
    assert len(out) == n
    return out


def test_replayed_statistics_exist_and_the_blocks_replay_their_first_cases():
    assert set(soc.SUM_STATS + soc.ORDER_STATS) <= set(vc.STATS) and set(soc.REPLACED) <= set(soc.SUM_STATS)
    assert "sum" not in vc.STATS  # (the reason the cases are replayed: values_cases.py draws none for it)
    for stat in soc.SUM_STATS + soc.ORDER_STATS:
        assert repr(drawn(stat, tgp.BLOCK_EXAMPLES)) == repr(drawn(stat)[:tgp.BLOCK_EXAMPLES])


# ---------------------------------------------------------------------------------------------------------------------
# (a) histogram_sum's replayed cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stat", soc.SUM_STATS)
def test_sum_cases_meet_their_conditions(stat):
    t = collections.Counter()
    for case in drawn(stat):
        b = soc.build_sum(case)
        d = b.d
        v = b.host[d]
        assert v.shape == case["shape"] and v.flags.c_contiguous and len(b.host) == len(b.views) == d + 1
        full = np.broadcast_to(b.views[d], case["shape"])
        assert full.dtype == v.dtype and np.array_equal(full, v, equal_nan=v.dtype.kind == "f")
        mine, theirs = mo.compare_domain(b.host[:d], b.edges), tgs._cmp_domain(b.host[:d], b.edges)
        for x, y in zip(mine[0] + mine[1], theirs[0] + theirs[1]):
            assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f")
        cnt, tot = soc.sum_want(b.host[:d], v, b.edges, case["axis"])
        kept = tgp.kept_shape(case)
        assert cnt.shape == tot.shape == kept + tuple(len(e) - 1 for e in b.edges) and cnt.dtype == np.int64 and tot.dtype == F64
        t["count nothing"] += not (mo.index(b.host[:d], b.edges) >= 0).any()
        t["a finite total of two or more values"] += bool(((cnt >= 2) & np.isfinite(tot)).any())
        t["an infinite or NaN total"] += bool((~np.isfinite(tot)).any())
        t["an extent 0"] += 0 in case["shape"]
        t["values " + v.dtype.name] += 1
        t["backend " + case["backend"]] += 1
        t["values layout " + case["layouts"][d]["kind"]] += 1
        # what tells integer limbs from float additions: a bin whose total is not what adding in the given order gives
        if cnt.size and stat in soc.REPLACED:
            xs, es = mo.compare_domain(b.host[:d], b.edges)
            rows = [ao.rows_cols_sorted(x, onp_axis(case)) for x in xs]
            v_rows = ao.rows_cols_sorted(v.astype(F64), onp_axis(case))
            naive = naive_sums(rows, es, v_rows)
            differ = np.isfinite(tot.reshape(-1)) & (naive != tot.reshape(-1))
            t["a total that adding in order misses"] += bool(differ.any())
    print("\n%s: %s" % (stat, ", ".join("%s %d" % kv for kv in sorted(t.items()))))
    assert t["count nothing"] <= 6
    assert t["a finite total of two or more values"] >= 50
    if stat in soc.REPLACED:
        assert t["a total that adding in order misses"] >= 30
        dtypes = {k.split()[1] for k in t if k.startswith("values ") and not k.startswith("values layout")}
        assert dtypes == {"float64", "float32", "float16"} and t["an infinite or NaN total"]
    else:  # as drawn: the kinds the issue names are there
        kinds = collections.Counter(c["values"][0] for c in drawn(stat))
        for k in ("special:float64", "special:float32", "big:int64", "small:float16", "small:bool", "small:int8", "small:uint8", "small:int16"):
            assert kinds[k] >= 1, k


def onp_axis(case):
    from oracle import oracle_np as onp

    return onp.normalise_axis(case["axis"], len(case["shape"]))


def naive_sums(rows, edges, v_rows):
    """per (row, bin), flat: the float64 additions in the order of the columns (np.add.at), NaN values skipped"""
    m = rows[0].shape[0]
    ok, flat, nbs = ao.counted_bins(rows, edges, v_rows)
    n_bins = int(np.prod(nbs, dtype=np.int64))
    out = np.zeros(m * n_bins)
    with np.errstate(invalid="ignore", over="ignore"):
        np.add.at(out, (flat + (np.arange(m, dtype=np.int64) * n_bins)[:, None])[ok], v_rows[ok])
    return out


def test_the_replacement_values_leave_the_case_alone():
    """a case built with and without drawing its replacement gives the same arrays, and the replacement is laid out as the
    case's values are: the same shape and strides as the view it replaces, the dtype kept where it is a float type"""
    for case in drawn("mean_var"):
        first = vc.build(case)
        buf, view = soc.replacement(case)
        again = vc.build(case)
        for a, b in zip(first.bufs + first.views + first.host, again.bufs + again.views + again.host):
            assert a.dtype == b.dtype and a.shape == b.shape and a.strides == b.strides and a.tobytes() == b.tobytes()
        own = first.views[first.d]
        assert view.shape == own.shape and view.dtype == soc.value_dtype(case)
        assert [s // view.itemsize for s in view.strides] == [s // own.itemsize for s in own.strides]
        assert view.dtype == own.dtype or own.dtype.kind != "f"
        buf2, view2 = soc.replacement(case)
        assert buf.tobytes() == buf2.tobytes()  # (drawn from the case alone)
        if view.size:
            item = view.itemsize
            off = (view.__array_interface__["data"][0] - buf.__array_interface__["data"][0]) // item
            reach = [(n - 1) * (st // item) for n, st in zip(view.shape, view.strides)]
            assert 0 <= off + sum(r for r in reach if r < 0) and off + sum(r for r in reach if r > 0) < buf.size


@pytest.mark.parametrize("dt", ["float64", "float32", "float16"])
def test_full_mantissa_values(dt):
    v = soc.full_mantissa(np.random.default_rng(1), (7, 300), dt)
    assert v.dtype == np.dtype(dt) and v.shape == (7, 300)
    f = v.astype(F64)
    fin = f[np.isfinite(f) & (f != 0)]
    assert np.isnan(f).sum() == 21 and np.isinf(f).sum() == 3 and (f == 0).sum() >= 2 and np.signbit(f[f == 0]).any()
    assert (np.abs(fin) == float(np.finfo(v.dtype).smallest_subnormal)).sum() == 1
    k = soc.EXPONENTS[dt]
    assert fin.min() < 0 < fin.max() and np.abs(fin).max() > 2.0 ** (k - 2) and np.median(np.abs(fin)) < 2.0
    bits = np.finfo(v.dtype).nmant + 1
    m, _ = np.frexp(fin)
    assert (np.ldexp(m, bits) % 2 == 1).mean() > 0.3  # (the last mantissa bit is set in about half of them)
    tiny = float(np.finfo(v.dtype).smallest_subnormal)
    for n, nans, specials in ((0, 0, 0), (1, 0, 0), (7, 0, 0), (8, 1, 1), (47, 1, 5), (48, 1, 6), (300, 3, 6)):
        w = soc.full_mantissa(np.random.default_rng(2), (n,), dt).astype(F64)
        assert np.isnan(w).sum() == nans and ((w == 0) | np.isinf(w) | (np.abs(w) == tiny)).sum() == specials, (n, w)


# ---------------------------------------------------------------------------------------------------------------------
# (a) bin_order's replayed cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stat", soc.ORDER_STATS)
def test_order_cases_meet_their_conditions(stat):
    t = collections.Counter()
    for case in drawn(stat):
        b = vc.build(case)
        d, axis = b.d, case["axis"]
        n_bins = soc.n_bins_of(b.edges)
        order, offsets, rows = soc.order_want(b.host[:d], b.edges, axis)
        kept = tgp.kept_shape(case)
        c = int(np.prod([case["shape"][i] for i in set(vc.reduced_axes(case))], dtype=np.int64))
        assert order.shape == kept + (c,) and offsets.shape == kept + (n_bins + 1,) and order.dtype == offsets.dtype == np.int64
        counts = np.diff(offsets, axis=-1)
        t["count nothing"] += not (counts > 0).any()
        t["an extent 0"] += 0 in case["shape"]
        t["two or more positions in a bin"] += bool((counts >= 2).any())
        ndim = len(case["shape"])
        norm = [a % ndim for a in axis] if axis is not None else []
        t["axis out of order"] += norm != sorted(norm)
        t["every axis, out of order"] += norm != sorted(norm) and len(norm) == ndim
        t["backend " + case["backend"]] += 1
        m = int(np.prod(kept, dtype=np.int64))  # (said outright: numpy infers no extent next to 0)
        flat_o, flat_f, flat_r = order.reshape(m, c), offsets.reshape(m, n_bins + 1), rows.reshape(m, c)
        for r in range(m):
            bo.assert_grouped(flat_o[r], flat_f[r], flat_r[r], n_bins, "row %d" % r)
        if stat == "argextrema" and (counts > 0).any():
            # the two definitions of a position: the first maximum found through the order is the oracle's argmax
            amax = vc.oracle(stat, b.host, b.edges, axis, case["params"])[1].reshape(m, n_bins)
            v_rows = bo.rows_of(b.host[d], axis).reshape(m, c)
            for r in range(m):
                np.testing.assert_array_equal(soc.argmax_through_order(flat_o[r], flat_f[r], v_rows[r]), amax[r])
            t["positions tied to argextrema"] += 1
    print("\n%s: %s" % (stat, ", ".join("%s %d" % kv for kv in sorted(t.items()))))
    assert t["count nothing"] <= 6 and t["two or more positions in a bin"] >= 50
    assert t["an extent 0"] >= 1 and t["axis out of order"] >= 5
    if stat == "argextrema":
        assert t["positions tied to argextrema"] >= 50


def test_argmax_through_order_written_down():
    order, offsets = np.array([4, 1, 3, 0, 5, 2]), np.array([0, 3, 3, 5])  # bin 0: 4, 1, 3 is not ascending on purpose
    v = np.array([-0.0, 7.0, np.nan, 7.0, np.nan, 0.0])
    np.testing.assert_array_equal(soc.argmax_through_order(order, offsets, v), [1, -1, 5])
    np.testing.assert_array_equal(soc.argmax_through_order(order, offsets, np.full(6, np.nan)), [-1, -1, -1])


# ---------------------------------------------------------------------------------------------------------------------
# (e) the row batches
# ---------------------------------------------------------------------------------------------------------------------
def _chunk(family):
    chunk = mc.launch_rows(soc.ROW_BLOCK[family], 1)
    assert chunk == {"fast": 16_777_215, "generic": 8_388_607}[family]
    return chunk


@pytest.mark.parametrize("family", soc.ROW_FAMILIES)
def test_rows_data_is_what_it_says(family):
    edges, xs, vs = soc.rows_data(family)
    assert math.gcd(soc.P_S, soc.P_V) == 1 and soc.ROWS_COLS != soc.ROWS_BINS and min(soc.ROWS_COLS, soc.ROWS_BINS) > 1
    assert xs.shape == (soc.P_S, soc.ROWS_COLS) and vs.shape == (soc.P_V, soc.ROWS_COLS) and len(edges[0]) - 1 == soc.ROWS_BINS
    vdt, bits, e0, shifts = soc.ROW_VALUES[family]
    assert (xs.dtype, edges[0].dtype, vs.dtype) == ((np.int64, np.int64, np.float32) if family == "generic" else (F64, F64, F64))
    assert np.finfo(vdt).nmant + 1 == bits and max(shifts) < soc.ROW_EXP_STEP
    idx = mo.index([xs], edges)
    assert 0.25 < (idx < 0).mean() < 0.45 and set(np.unique(idx)) == {-1, 0, 1}
    if xs.dtype.kind == "f":
        assert np.isnan(xs).sum() >= 10
    assert np.isnan(vs).sum() == 20
    v = vs.astype(F64)
    m, e = np.frexp(np.where(np.isnan(v), 1.0, v))
    full = np.ldexp(np.abs(m), bits)  # the mantissa as an integer of `bits` bits
    assert ((full == np.round(full)) & (full % 2 == 1) & (full >= 2.0 ** (bits - 1)))[~np.isnan(v)].all(), "not every mantissa bit is in use"
    p = np.arange(soc.P_V)[:, None]
    below = soc.ROW_EXP_STEP * (p % 5) + e0 + 1 - e  # how far below its row's exponent a value lies
    assert set(np.unique(below[~np.isnan(v)])) == set(shifts)
    assert (np.signbit(v) & ~np.isnan(v)).any() and (~np.signbit(v) & ~np.isnan(v)).any()
    # the limbs the totals are made of: all three planes take non-zero words
    cnt, tot = soc.rows_table(family)
    used = np.zeros(3, bool)
    for bins in soc.rows_bins(family, np.arange(300)):
        for vals in bins:
            vals = vals[~np.isnan(vals)]
            if vals.size:
                u = so.unit_exponent(float(np.abs(vals).max()))
                for x in vals.tolist():
                    q = so.quantum(x, u)[1]
                    used |= [bool((q >> (32 * j)) & 0xFFFFFFFF) for j in range(3)]
    assert used.all(), used
    # (a column meets a given bin one time in three: two or more of three do in about a quarter of the bins, less the NaN)
    assert np.isfinite(tot).all() and (cnt >= 2).mean() > 0.15 and (cnt == 0).any() and (tot[cnt > 0] != 0).all()


@pytest.mark.parametrize("family", soc.ROW_FAMILIES)
def test_rows_closed_form_is_the_oracle(family):
    """soc.rows_table read at soc.rows_index, the expectation of test_more_rows_than_one_launch, against sum_oracle.sum_rows
    on the rows themselves: the first 2048 rows, 1024 on each side of the first launch's last row, and the last 2048"""
    chunk = _chunk(family)
    n_rows = chunk + soc.ROWS_EXTRA
    assert chunk < n_rows <= 2 * chunk
    edges, xs, vs = soc.rows_data(family)
    cnt, tot = soc.rows_table(family)
    assert cnt.shape == tot.shape == (soc.P_S * soc.P_V, soc.ROWS_BINS)
    for rows in (np.arange(0, 2048), np.arange(chunk - 1024, chunk + 1024), np.arange(n_rows - 2048, n_rows)):
        want_cnt, want_tot = so.sum_rows([xs[rows % soc.P_S]], edges, vs[rows % soc.P_V].astype(F64))
        at = soc.rows_index(rows)
        np.testing.assert_array_equal(cnt[at], want_cnt)
        sc.same_bits(tot[at], want_tot, "%s rows %d.." % (family, rows[0]))
    r = torch.arange(chunk - 5, chunk + 5)
    np.testing.assert_array_equal(soc.rows_index(r).numpy(), soc.rows_index(r.numpy()))


@pytest.mark.parametrize("family", soc.ROW_FAMILIES)
def test_another_rows_keys_change_the_total(family):
    """the unit is all a total takes from pass 1's keys: with the keys of row r + 1, r - 1 or r - chunk (what a key pointer
    that is not advanced reads in the second launch) the total of row r changes, in at least 9 of 10 of the rows that count
    two or more values in a bin, and total_with_keys with the row's own keys is the oracle's total"""
    chunk = _chunk(family)
    rows = np.concatenate([np.arange(chunk, chunk + 600), np.arange(chunk + soc.ROWS_EXTRA - 600, chunk + soc.ROWS_EXTRA)])
    own = soc.rows_bins(family, rows)
    cnt, tot = soc.rows_table(family)
    for shift in (1, -1, -chunk):
        other = soc.rows_bins(family, rows + shift)
        held = changed = 0
        for i, r in enumerate(rows.tolist()):
            want = tot[soc.rows_index(r)]
            two = [b for b in range(soc.ROWS_BINS) if (~np.isnan(own[i][b])).sum() >= 2]
            for b in range(soc.ROWS_BINS):
                sc.same_bits(soc.total_with_keys(own[i][b], own[i][b]), want[b], "row %d bin %d, its own keys" % (r, b))
            if two:
                held += 1
                changed += any(soc.total_with_keys(own[i][b], other[i][b]) != want[b] for b in two)
        print("\n%s, keys of row r%+d: the total changes in %d of %d rows with two or more values in a bin" % (family, shift, changed, held))
        assert held >= 300 and changed * 10 >= held * 9
