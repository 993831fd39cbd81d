"""What tests/test_gpu_values_census_streams.py derives, spelled out where no GPU is needed: the restatement of the values
launcher's choice (choose_values / values_geometry of xhist_values.hip.h) with histogram_cov's slots of 24 and 56 bytes, the
row chunks of its largest case, and the conditions its data must meet for the checks to bite: every copies case has bins that
are checked bit for bit and bins that are checked against the float64 bound, and every element of a tile-edge case counts."""
import numpy as np
import pytest

import cov_exact as cx
import meanvar_oracle as mo
import test_gpu_values_census_streams as cs
from test_gpu_cov import _flat, predict_cov
from test_gpu_values_census import LDS_MAX, SLOTS, _last, predict, table_bytes

F64, F32 = np.float64, np.float32
CUS = 256  # (the segments per row depend on it; nothing asserted here does)


def _lin(nb):
    return [np.linspace(-4.0, 4.0, nb + 1)]


def test_cov_slots_are_registered():
    assert SLOTS["cov"] == ((24, 56), (24, 56))
    assert cs.SLOT_KEY == {"cov": "cov", "mean_var_w": "mean_var"}


def test_cov_copies_thresholds():
    """the last 1-D bin count of each number of copies, float64 samples: 56-byte slots within 24 KiB"""
    def copies(nb):
        return predict_cov(CUS, _lin(nb), 0, F64, F64, 1, 1)["copies"]
    assert [_last(lambda n: copies(n) >= c) for c in (16, 8, 4, 2)] == [27, 54, 109, 219]
    for (nbs, c) in cs.COV_COPIES:
        for st in (F64, F32):
            assert predict_cov(CUS, [_lin(nb)[0] for nb in nbs], 0, st, st, 1, 1)["copies"] == c
    for (nbs, c) in cs.W_COPIES:
        for st in (F64, F32):
            assert predict("mean_var", CUS, _lin(nbs[0]), 0, st, st, 1, 1)["copies"] == c


def _sides(stat, sdt, border):
    return [c[3] for c in cs.BORDERS if c[:3] == (stat, sdt, border)]


def test_cov_borders_sit_where_the_slots_say():
    assert _sides("cov", F64, "arith") == _sides("cov", F32, "arith") == [2925, 2926]  # 160 KiB / 56 B
    fine64 = _last(lambda n: table_bytes([np.zeros(n + 1)], "fine64") + n * 56 <= LDS_MAX)
    fine32 = _last(lambda n: table_bytes([np.zeros(n + 1)], "fine32") + n * 56 <= LDS_MAX)
    generic = _last(lambda n: table_bytes([np.zeros(n + 1)], "native") + n * 56 <= LDS_MAX)
    assert (fine64, fine32, generic) == (2303, 2457, 2303)
    assert _sides("cov", F64, "fine") == [fine64, fine64 + 1, fine64 + 1]
    assert _sides("cov", F32, "fine") == [fine32, fine32 + 1, fine32 + 1]
    assert _sides("cov", "gen", "generic_lds") == [generic, generic + 1]
    # the weighted slots have the unweighted sizes: the borders of test_gpu_values_census
    assert _sides("mean_var_w", F64, "arith") == [6826, 6827]  # 160 KiB / 24 B
    assert _sides("cov", "gen", "tables_in_lds") == _sides("mean_var_w", "gen", "tables_in_lds")


@pytest.mark.parametrize("i", range(len(cs.BORDERS)))
def test_border_sides_are_predicted_to_move(i):
    """each side of each border: the family and the home the GPU test asserts are what the restatement predicts"""
    stat, sdt, border, nb, kind, family = cs.BORDERS[i]
    want = cs.border_predict(i, CUS)[0]
    assert want["family"] == family
    if family == "fast":
        assert (want["scan"] == 5) == (kind == "lin")
    assert (want["slots"], want["tables_in_lds"]) == cs.border_home(stat, border, _sides(stat, sdt, border).index(nb), nb, family)


def test_third_stream_rule():
    """choose_values: the weights / b must have the sample dtype, unit column stride unless there is one column, and an
    element-aligned pointer; anything else gives up the fast family, whatever samples and values are"""
    assert cs.third_stream_fast(F64, F64, 1, 100) and cs.third_stream_fast(F32, F32, 7, 1) and cs.third_stream_fast(F32, F32, 0, 1)
    assert not cs.third_stream_fast(F64, F32, 1, 100)
    assert not cs.third_stream_fast(F64, F64, 3, 100) and not cs.third_stream_fast(F64, F64, 0, 2)
    assert not cs.third_stream_fast(F64, F64, 1, 100, x_ptr=4) and cs.third_stream_fast(F32, F32, 1, 100, x_ptr=4)
    e = _lin(30)
    assert predict_cov(CUS, e, 0, F64, F64, 2, 20_011, True, True, True)["family"] == "fast"
    assert predict_cov(CUS, e, 0, F64, F64, 2, 20_011, True, True, cs.third_stream_fast(F64, F64, 3, 20_011))["family"] == "generic"
    assert predict("mean_var", CUS, e, 0, F32, F32, 2, 20_011, True, True, cs.third_stream_fast(F32, F64, 1, 20_011))["family"] == "generic"


def test_row_chunks():
    assert cs.chunk_rows(256, 1) == 16_777_215 == (1 << 24) - 1
    assert cs.chunk_rows(512, 1) == 8_388_607 == (1 << 23) - 1
    assert cs.N_ROWS == 2 * 16_777_215 + 70_001
    assert (cs.chunk_count(256), cs.chunk_count(512)) == (3, 5)
    # two bins: a plane of the call is twice the row count apart, and a chunk's pointers advance by twice its rows
    assert len(cs.CHUNK_EDGES) - 1 == 2
    for stat in cs.STATS:
        for bt, family, block in ((F64, "fast", 256), (F32, "generic", 512)):
            pred = predict_cov if stat == "cov" else (lambda *p: predict("mean_var", *p))
            want = pred(CUS, [cs.CHUNK_EDGES], 0, F64, F64, cs.N_ROWS, 1, True, True, cs.third_stream_fast(F64, bt, 1, 1))
            assert (want["family"], want["block"], want["segs"]) == (family, block, 1)


CASES = [(stat, nbs, sdt) for stat, table in (("cov", cs.COV_COPIES), ("mean_var_w", cs.W_COPIES)) for nbs, _ in table
         for sdt in ("f64", "f32")]


@pytest.mark.parametrize("stat,nbs,sdt", CASES, ids=["%s-%s-%s" % (s, "x".join(map(str, n)), t) for s, n, t in CASES])
def test_copies_cases_check_both_ways(stat, nbs, sdt):
    """the oracle alone: bins whose moments are checked bit for bit (a power-of-two count from 2 to 2^9, W from 2 to 2^8) and
    non-empty bins checked against the bound"""
    assert (stat, nbs, sdt) in cs.COPIES_DATA and cs.COPIES_DATA[(stat, nbs, sdt)][0] <= 40_009
    bits, bound = cs.copies_split(stat, *cs.copies_data(stat, nbs, sdt))
    assert bits >= 1 and bound >= 1, (bits, bound)


@pytest.mark.parametrize("form", list(cs.TILE_FORMS))
def test_tile_edge_cases_count_every_element(form):
    st, D, tile, cols = cs.TILE_FORMS[form]
    vec = 16 // np.dtype(st).itemsize
    assert tile == 256 * vec * (4 if D == 1 else 8 // vec)  # (values_fast_body: blockDim x VEC x UNROLL)
    assert {c - tile for c in cols} >= {-1, 0, 1} and max(cols) > 2 * tile // (2 if D == 2 else 1)
    if form == "f64_D2":  # the halves of the weighted float64 pairs
        assert {c - tile // 2 for c in cols} >= {-1, 0, 1} and 3 * tile // 2 + 1 in cols
    for stat in cs.STATS:
        for n_rows in (1, 3):
            for n_cols in cols:
                edges, xs, a, b = cs.tile_data(stat, form, n_rows, n_cols)
                assert all(x.dtype == st and x.shape == (n_rows, n_cols) for x in xs) and a.dtype == b.dtype == st
                xc, ec = cs._cmp(xs, edges)
                ok, flat, _ = mo._flat_bins(xc, ec)
                assert ok.all() and not np.isnan(a).any() and not np.isnan(b).any()
                if stat == "cov":
                    ok, flat, size = _flat(xc, ec)
                    cnt = cx.expected(flat[ok], a[ok], b[ok], size)[0]
                    np.testing.assert_array_equal(cnt.reshape(n_rows, -1).sum(axis=1), n_cols)
                else:
                    assert b.min() >= 0 and b.max() <= 7 and np.array_equal(b, np.round(b))
