"""What tests/test_gpu_quantile_census.py derives, spelled out where no GPU is needed: the borders of the quantile drivers'
choices, found by search over the restatement (`predict_quantile`) and held as numbers; that each GPU case's prediction has the
tier, d, G, homes and chunks its name claims; and the conditions its data must meet for the checks to bite: enough bins of
several distinct keys, a bin only the last digit separates, a bin the first digit separates, the R, N and last workgroup of every
short case, and q values whose virtual index falls on and beside whole numbers and halves."""
import numpy as np
import pytest

import test_gpu_quantile_census as qc
from test_gpu_quantile_census import F32, F64, border, cap_border, generic_border, last_true

U, W = False, True
MIN_DISTINCT_BINS = 20  # the chosen bins of every row of a radix case that must hold at least two distinct keys


# ---------------------------------------------------------------------------------------------------------------------
# the restatement's constants and borders
# ---------------------------------------------------------------------------------------------------------------------
def test_slot_and_scratch_sizes():
    """the sizes read off xhist_quantile.hip.h, xhist_quantile_w.hip.h and the two drivers"""
    assert qc.Q_LDS_MAX == 160 * 1024 - 64
    assert [qc.digit_bytes(U, 1, d) for d in (8, 4, 1)] == [1048, 88, 32] and qc.digit_bytes(U, 8, 4) == 704
    assert [qc.digit_bytes(W, 1, d) for d in (8, 4, 1)] == [2072, 152, 40]
    assert (qc.win_bytes(U, 1), qc.win_bytes(U, 5), qc.win_bytes(W, 1)) == (36, 180, 24)
    assert qc.radix_row_bytes(U, 100, 2, 5) == 100 * 712  # (tests/test_gpu_quantile.py::test_row_chunks: 712 bytes per (row, bin))
    assert qc.radix_row_bytes(W, 100, 2, 4) == 100 * 344  # (tests/test_gpu_weighted_quantile.py::test_row_chunks)
    assert qc.radix_row_bytes(U, 1, 1, 4) == 248 and qc.radix_row_bytes(W, 1, 1, 4) == 184


def test_existing_chunk_tests_are_predicted():
    """the chunk counts the two row-chunk tests of the existing suites assert"""
    lin = [np.linspace(-2.0, 3.0, 101)]
    p = qc.predict_quantile(U, 256, lin, 0, F32, F32, None, None, 9000, 4200, 2)
    assert (p["group"], p["d"], p["chunks"], p["rows_per_chunk"]) == (2, 5, 3, 3770)
    p = qc.predict_quantile(W, 256, lin, 0, F32, F32, F32, None, 9000, 4200, 2)
    assert (p["group"], p["d"], p["chunks"], p["rows_per_chunk"]) == (2, 4, 2, 7803)


def test_budget_border():
    """two targets at d = 8 take 2 * 1048 bytes a bin: 19 bins are the last within kQLdsBudget next to the fine tables"""
    def within(n):
        p = qc._p(U, (n,), 2)
        return p["d"] == 8 and p["group"] == 2
    assert last_true(within, 2, 100) == 19
    assert qc._p(U, (19,), 2)["lds_bytes"] == "1388/40528" and qc._p(U, (20,), 2)["d"] == 7
    assert last_true(lambda n: qc._p(W, (n,), 1)["d"] == 8, 2, 100) == 19
    assert qc._p(W, (19,), 1)["lds_bytes"] == "1160/40072" and qc._p(W, (20,), 1)["d"] == 7
    # float32 samples: smaller fine tables, the same border
    assert last_true(lambda n: qc._p(U, (n,), 2, F32)["d"] == 8 and qc._p(U, (n,), 2, F32)["group"] == 2, 2, 100) == 19
    assert last_true(lambda n: qc._p(W, (n,), 1, F32)["d"] == 8, 2, 100) == 19
    assert (qc._p(U, (19,), 2, F32)["lds_bytes"], qc._p(W, (19,), 1, F32)["lds_bytes"]) == ("1292/40432", "1064/39976")


def test_home_borders():
    """the last 1-D bin count of arithmetic edges at which the d = 4 digit pass of one target, the successor pass of two
    targets and pass 0 still have their slots in LDS: (float64, float32) samples and values.  The arithmetic form carries no
    table, so the sample type moves none of them: 163 776 bytes over 88, 72, 36 (weighted: 152, 24) bytes a bin"""
    got = {(wt, what): tuple(border(wt, st, what) for st in (F64, F32))
           for wt, what in ((U, "digits"), (U, "successor"), (U, "pass0"), (W, "digits"), (W, "pass0"))}
    assert got == {(U, "digits"): (1861, 1861), (U, "successor"): (2274, 2274), (U, "pass0"): (4549, 4549),
                   (W, "digits"): (1077, 1077), (W, "pass0"): (6824, 6824)}
    for (wt, what), (n64, n32) in got.items():
        slot = {"digits": qc.digit_bytes(wt, 1, 4), "successor": qc.win_bytes(U, 2), "pass0": qc.win_bytes(wt, 1)}[what]
        assert n64 == n32 == qc.Q_LDS_MAX // slot
    # past the digit border the search is in tier 2 and takes the widest digit; with the fine tables (not arithmetic edges) the
    # float32 tables are smaller and the borders do differ
    assert qc._p(U, (1862,), 1)["digits"] == "generic/global" and qc._p(U, (1862,), 1)["d"] == 8
    k1 = {st: last_true(lambda n: qc.predict_quantile(U, 256, [np.zeros(n + 1)], 0, st, st, None, None, 1, 4200, 1, arith=False)
                        ["digits"] == "fast/lds", 100, 20_000) for st in (F64, F32)}
    assert k1[F64] < k1[F32] < 1861, k1


def test_scratch_cap_borders():
    """the bin counts up to which a digit of d bits (one target) stays under kQScratchCap: beyond d = 4's the search drops to 3,
    2, 1, and beyond d = 1's only the exemption of (g, d) = (1, 1) is left"""
    assert [cap_border(U, d) for d in (4, 3, 2, 1)] == [1_082_401, 1_458_888, 1_766_022, 1_973_790]
    assert [cap_border(W, d) for d in (4, 3, 2, 1)] == [1_458_888, 2_236_962, 3_050_402, 3_728_270]
    for wt in (U, W):
        for d in (4, 3, 2, 1):
            n = cap_border(wt, d)
            assert n == qc.SCRATCH_CAP // qc.radix_row_bytes(wt, 1, 1, d)
            lo, hi = (int(n ** 0.5),) * 2, (int(n ** 0.5) + 1,) * 2  # the 2-D histograms on either side
            assert qc._p(wt, lo, 1, n_rows=3)["d"] == d and qc._p(wt, hi, 1, n_rows=3)["d"] == max(1, d - 1)
        beyond = qc._p(wt, (int(cap_border(wt, 1) ** 0.5) + 1,) * 2, 1, n_rows=3)
        assert (beyond["d"], beyond["passes"], beyond["rows_per_chunk"], beyond["chunks"]) == (1, 64, 1, 3)
    # the GPU cases sit on the side their names say
    for s, d in ((1024, 4), (1100, 3), (1300, 2), (1400, 1)):
        assert s * s <= cap_border(U, d) and (d == 4 or s * s > cap_border(U, d + 1))
    assert 1500 * 1500 > cap_border(U, 1)
    for s, d in ((1200, 4), (1300, 3), (1600, 2), (1800, 1)):
        assert s * s <= cap_border(W, d) and (d == 4 or s * s > cap_border(W, d + 1))
    assert 2000 * 2000 > cap_border(W, 1)


def test_generic_borders():
    """the generic family's d = 4 digit pass next to the native tables, per domain (unweighted, weighted)"""
    assert [(generic_border(wt, dom)) for wt in (U, W) for dom in ("i64", "mixed")] == [1534, 541, 920, 334]


def test_short_bound_and_threshold():
    lin = [np.linspace(0.0, 1.0, 11)]
    for wt, cols in ((U, 4096), (W, 2048)):
        assert qc.predict_quantile(wt, 256, lin, 0, F64, F64, F64, None, 5, cols, 3)["family"] == "short"
        assert qc.predict_quantile(wt, 256, lin, 0, F64, F64, F64, None, 5, cols + 1, 3)["family"] == "radix"


def test_layout_rule():
    """choose_values: every stream has the sample dtype, unit column stride unless there is one column, and an element-aligned
    pointer; anything else gives up the fast family for every pass"""
    for layout, weighted in qc.LAYOUT_CASES:
        lay, wdt = qc.layout_streams(layout, weighted, 3, 4200)
        p = qc.predict_quantile(weighted, 256, qc._lin((100,)), 0, F64, F64, wdt, lay, 3, 4200, 2)
        assert p["window"] == p["digits"] == qc.LAYOUT_FAMILY[layout] + "/lds", (layout, p)
    assert not qc.streams_fast(F64, [F64, F64], [(1, 0), (1, 4)], 100) and qc.streams_fast(F32, [F32, F32], [(1, 0), (1, 4)], 100)
    assert qc.streams_fast(F64, [F64, F64], [(7, 0), (0, 0)], 1)


# ---------------------------------------------------------------------------------------------------------------------
# the GPU cases: what each prediction must show
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(qc.RADIX))
def test_radix_case_is_predicted_where_its_name_says(name):
    p = qc.radix_predict(name)
    assert p["family"] == "radix"
    qc.assert_expected(name, p)
    case = qc.RADIX[name]
    assert 4097 <= case["n_cols"] <= 6000 and case["n_cols"] > qc.SHORT_COLS[case["weighted"]]


def test_radix_cases_cover_the_closing_test():
    """the predictions alone reach what the closing test of the GPU module asks of the lines"""
    for wt in (U, W):
        ps = [(qc.radix_predict(n), c["n_q"]) for n, c in qc.RADIX.items() if c["weighted"] == wt]
        assert {qc.tier_of(p) for p, _ in ps} == {0, 1, 2}
        assert {p["d"] for p, _ in ps} == set(range(1, 9))
        assert any(p["groups"] > 1 and 0 < n_q - (p["groups"] - 1) * p["group"] < p["group"] for p, n_q in ps)
        assert any(p["chunks"] > 1 and p["groups"] > 1 for p, _ in ps)
    homes = {qc.homes_of(qc.radix_predict(n)) for n, c in qc.RADIX.items() if not c["weighted"]}
    assert homes >= {("lds", "lds", "lds"), ("lds", "lds", "global"), ("lds", "global", "global"), ("global", "global", "global")}


@pytest.mark.parametrize("name", list(qc.RADIX))
def test_radix_data_conditions(name):
    """every row: at least MIN_DISTINCT_BINS chosen bins with two or more distinct keys, each chosen bin with at least 40 values
    that are not NaN, a bin whose two keys (half of its values each, so that q = 0.5 reads one of each) differ only within the
    last digit, and a bin whose keys differ in the top bit.  float32 values have keys whose low 29 bits are zero: their closest
    pair differs in bit 29, which is within the last digit for no d, and is held to exactly that"""
    case = qc.RADIX[name]
    edges, cmp, xs, v, w, q, chosen = qc.radix_inputs(name)
    p = qc.radix_predict(name)
    last_bits = 64 - p["d"] * (p["passes"] - 1)
    assert 1 <= last_bits <= p["d"] and (p["d"] != 3 or last_bits == 1)
    assert 0.5 in q
    xc, ec = qc._cmp(xs, edges)
    nbs = [len(e) - 1 for e in edges]
    for r in range(case["n_rows"]):
        flat = np.zeros(case["n_cols"], np.int64)
        ok = np.ones(case["n_cols"], bool)
        for s, e, nb in zip(xc, ec, nbs):
            code = np.searchsorted(e, s[r], side="right")
            code = np.where(s[r] == e[-1], nb, code)
            ok &= (code >= 1) & (code <= nb) & (~np.isnan(s[r]) if s.dtype.kind == "f" else True)
            flat = flat * nb + np.clip(code - 1, 0, nb - 1)
        must = {0, int(np.prod(nbs)) - 1} | ({nbs[-1] - 1, nbs[-1]} if len(nbs) > 1 else set())
        assert must <= set(chosen[r]) and len(chosen[r]) == min(qc.N_CHOSEN, int(np.prod(nbs)))
        distinct = last_digit = top_bit = 0
        for b in chosen[r]:
            keys = np.sort(qc.keys_of(v[r][ok & (flat == b)]))
            assert len(keys) >= 40, (name, r, b, len(keys))
            u = np.unique(keys)
            distinct += len(u) >= 2
            top_bit += bool((u[0] ^ u[-1]) >> np.uint64(63))
            if len(u) == 2 and len(keys) % 2 == 0 and keys[len(keys) // 2 - 1] != keys[len(keys) // 2]:
                x = int(u[0] ^ u[1])
                last_digit += x < (1 << last_bits) if case["st"] == F64 else x == 1 << 29
        if len(chosen[r]) >= qc.N_CHOSEN:
            assert distinct >= MIN_DISTINCT_BINS, (name, r, distinct)
        else:  # (fewer bins than N_CHOSEN: every bin is chosen, the kinds rotate through them)
            assert distinct >= len(chosen[r]) // 2, (name, r, distinct)
        if len(chosen[r]) >= qc.N_KINDS:
            assert last_digit >= 1 and top_bit >= 1, (name, r, last_digit, top_bit)
    if case["weighted"]:
        assert set(np.unique(w)) <= set(range(8)) and (w == 0).any()


@pytest.mark.parametrize("weighted,n_rows,n_cols,nbs,n_q,st", qc.SHORT_CASES)
def test_short_cases_reach_their_shapes(weighted, n_rows, n_cols, nbs, n_q, st):
    R, N, last = qc.SHORT[weighted][(n_rows, n_cols, nbs, n_q, st)]
    p = qc.predict_quantile(weighted, 256, [np.zeros(nb + 1) for nb in nbs], 0, st, st, st, None, n_rows, n_cols, n_q)
    assert p["family"] == "short" and p["rows_per_wg"] == R and p["triples" if weighted else "pairs"] == N
    assert p["lds_bytes"] == N * (20 if weighted else 12) <= 48 * 1024
    assert n_rows - (-(-n_rows // R) - 1) * R == last
    assert R * int(np.prod(nbs)) < 100_000 and max(nbs) <= 100


def test_short_cases_cover_the_shapes():
    for wt, cols in ((U, 4096), (W, 2048)):
        ks = list(qc.SHORT[wt])
        got = {qc.SHORT[wt][k] for k in ks}
        assert {g[0] for g in got} >= {cols, 3, 2, 1}
        assert any(k[1] == 1 and k[0] % cols for k in ks)  # one column, a partial last workgroup
        assert any(k[0] < qc.SHORT[wt][k][0] for k in ks)  # one partial workgroup
        assert any(k[1] == cols for k in ks) and any(k[1] == cols // 2 + 1 for k in ks)  # no padding / almost half padding
        assert any(int(np.prod(k[2])) == 1 for k in ks)  # one bin
        assert {k[3] for k in ks} == {1, 8, 9, 17}


# ---------------------------------------------------------------------------------------------------------------------
# the small counts
# ---------------------------------------------------------------------------------------------------------------------
def test_small_count_data():
    for n_cols, n_used in ((2080, 64), (4200, 64), (2048, 63)):
        x, v = qc.small_count_data(n_cols, 1, n_used)
        assert x.shape == v.shape == (1, n_cols)
        inside = (x[0] >= 0) & (x[0] < 64)
        for b in range(64):
            vb = v[0][inside & (np.floor(x[0]) == b)]
            vb = vb[~np.isnan(vb)]
            assert len(vb) == len(np.unique(vb)) == (b + 1 if b < n_used else 0)
    w = qc.small_weights(x, v, 1)
    assert set(np.unique(w)) <= set(range(8)) and (w == 0).any()


def _classes(x):
    """where x = (n - 1) q falls: on a whole number, one ulp beside it, on a half, one ulp beside it"""
    out = set()
    r = np.rint(x)
    h = np.floor(x) + 0.5
    for name, at in (("whole", r), ("half", h)):
        out |= {name} if (x == at).any() else set()
        out |= {name + "-below"} if ((x == np.nextafter(at, -np.inf)) & (at > 0)).any() else set()
        out |= {name + "-above"} if (x == np.nextafter(at, np.inf)).any() else set()
    return out


def test_index_q_lands_on_and_beside_whole_numbers_and_halves():
    """over the (n, q) of the small-count test, numpy's own virtual index (n - 1) q, which every method starts from, falls
    exactly on a whole number, exactly on a half, and one ulp on either side of both; and each method's own index then differs
    between the neighbours where it should: floor / ceil / rint disagree across a whole number or a half"""
    q = qc.index_q()
    assert len(q) > 64 and q[0] == 0.0 and q[-1] == 1.0 and np.all(np.diff(q) > 0)
    seen = set()
    flips = {m: 0 for m in qc.METHODS}
    for n in range(1, qc.SMALL_BINS + 1):
        x = (n - 1) * q
        if n > 2:
            seen |= _classes(x[(x > 0.25) & (x < n - 1.25)])
        lo, hi = x[:-1], x[1:]
        near = (hi - lo) <= 4 * np.spacing(hi)  # neighbouring q values
        flips["lower"] += int((near & (np.floor(lo) != np.floor(hi))).sum())
        flips["higher"] += int((near & (np.ceil(lo) != np.ceil(hi))).sum())
        flips["nearest"] += int((near & (np.rint(lo) != np.rint(hi))).sum())
        flips["midpoint"] += int((near & (np.floor(lo) + np.ceil(lo) != np.floor(hi) + np.ceil(hi))).sum())
        g_lo, g_hi = lo - np.floor(lo), hi - np.floor(hi)
        flips["linear"] += int((near & ((g_lo >= 0.5) != (g_hi >= 0.5))).sum())  # (_lerp's other branch)
    assert seen == {"whole", "whole-below", "whole-above", "half", "half-below", "half-above"}, seen
    assert all(k >= 10 for k in flips.values()), flips


def test_weighted_step_q():
    x, v = qc.small_count_data(4200, 950 + 4200)
    w = qc.small_weights(x, v, 950 + 4200)
    q = qc.weighted_step_q(x, v, w)
    assert q[0] >= 0.0 and q[-1] == 1.0 and len(q) > 500 and np.all(np.diff(q) > 0)
    # every step of a bin and both of its neighbours are there
    inside = ~np.isnan(v[0]) & (np.floor(x[0]) == 10)
    o = np.argsort(v[0][inside], kind="stable")
    c = np.cumsum(w[0][inside][o].astype(F64))
    for s in (c / c[-1])[:-1]:
        for t in (s, np.nextafter(s, -1.0), np.nextafter(s, 2.0)):
            assert t in q or not 0.0 <= t <= 1.0
