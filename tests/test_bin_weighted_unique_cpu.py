"""bin_weighted_unique and histogram_weighted_mode without a GPU: tests/weighted_unique_oracle.py held to a brute-force loop per
bin with np.unique (and to pandas where it is installed), the case tables of tests/weighted_unique_cases.py held to what they
claim, the restated describe() lines, and the Python and C surface with every refusal made before any device work."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import bin_unique_oracle as uo
import exact_weights as xw
import map_oracle as mo
import mode_oracle as mdo
import weighted_unique_cases as wc
import weighted_unique_oracle as wo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = wc.CUS


def _random_row(rng, c, nb, exact=True):
    idx = rng.integers(-1, nb, c)
    v = rng.integers(-3, 4, c).astype(np.float64)
    v[rng.random(c) < 0.1] = np.nan
    v[rng.random(c) < 0.1] = -0.0
    w = xw.f64(rng, c, "both") if exact else rng.standard_normal(c)
    return idx, v, w


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_oracle_against_a_loop_per_bin_with_np_unique():
    rng = np.random.default_rng(1)
    for c in (0, 1, 5, 64, 300):
        idx, v, w = _random_row(rng, c, 6)
        uniques, counts, sums, offsets, inverse = wo.wunique_row(idx, v, w, 6)
        bu, bc_, bs, bo_ = wo.brute_force(idx, v, w, 6)
        total = int(offsets[-1])
        assert total == len(bu) and np.array_equal(offsets, bo_)
        assert np.array_equal(uniques[:total], bu) and np.array_equal(counts[:total], bc_)  # (== : the zeros by value)
        wo.assert_sums(sums[:total], bs, "c=%d" % c)
        assert not counts[total:].any() and (wo.bits(sums[total:]) == 0).all() and (wo.bits(uniques[total:]) == wo.NAN_BITS).all()
        uo.assert_same((uniques, counts, offsets, inverse), uo.unique_row(idx, v, 6), "bin_unique's outputs")
        sel = inverse >= 0
        wo.assert_sums(np.bincount(inverse[sel], weights=w[sel], minlength=total)[:total] + 0.0, sums[:total] + 0.0, "bincount")


def test_oracle_against_pandas_groupby_sum():
    pd = pytest.importorskip("pandas")
    rng = np.random.default_rng(2)
    idx, v, w = _random_row(rng, 500, 5)
    keep = (idx >= 0) & ~np.isnan(v)
    g = pd.DataFrame({"b": idx[keep], "v": v[keep] + 0.0, "w": w[keep]}).groupby(["b", "v"])["w"].agg(["sum", "count"]).reset_index()
    uniques, counts, sums, offsets, _ = wo.wunique_row(idx, v, w, 5)
    total = int(offsets[-1])
    assert total == len(g) and np.array_equal(uniques[:total], g["v"].to_numpy()) and np.array_equal(counts[:total], g["count"].to_numpy())
    assert np.array_equal(sums[:total], g["sum"].to_numpy())  # (exactly summable weights: any order gives these bits)


def test_run_sum_rules():
    assert wo.run_sum([0.1] * 10) == math.fsum([0.1] * 10) == 1.0
    assert math.isnan(wo.run_sum([1.0, math.nan])) and math.isnan(wo.run_sum([math.inf, 1.0, -math.inf]))
    assert wo.run_sum([math.inf, 1.0]) == math.inf
    assert math.copysign(1, wo.run_sum([-0.0, -0.0])) == -1 and math.copysign(1, wo.run_sum([-0.0, 0.0])) == 1
    assert math.copysign(1, wo.run_sum([1.0, -1.0])) == 1


def test_weighted_mode_of_the_oracle():
    rng = np.random.default_rng(3)
    for _ in range(10):
        idx, v, w = _random_row(rng, 200, 7)
        count, nunique, mode, mode_weight = wo.wmode_row(idx, v, w, 7)
        uniques, counts, sums, offsets, _ = wo.wunique_row(idx, v, w, 7)
        c0, n0, _, _ = mdo.mode_row(idx, v, 7)
        assert np.array_equal(count, c0) and np.array_equal(nunique, n0)
        for b in range(7):
            seg = slice(offsets[b], offsets[b + 1])
            if count[b]:
                assert mode_weight[b] == sums[seg].max() and mode[b] == uniques[seg][sums[seg] == mode_weight[b]].min()
            else:
                assert wo.bits(mode[b:b + 1])[0] == wo.NAN_BITS and wo.bits(mode_weight[b:b + 1])[0] == 0
        ones = wo.wmode_row(idx, v, np.ones(200), 7)
        mdo.assert_same((ones[0], ones[1], ones[2], ones[3].astype(np.int64)), mdo.mode_row(idx, v, 7), "unit weights")
    # -0.0 against +0.0: equal, the smaller value wins; a NaN sum takes the bin; the heaviest is not the most frequent
    idx = np.zeros(6, np.int64)
    got = wo.wmode_row(idx, [1.0, 1.0, 2.0, 2.0, 3.0, 3.0], [1.0, -1.0, -0.0, -0.0, 0.0, 0.0], 1)
    assert got[2][0] == 1.0 and wo.bits(got[3])[0] == 0
    got = wo.wmode_row(idx, [2.0, 2.0, 1.0, 1.0, 3.0, 3.0], [-0.0, -0.0, 5.0, -5.0, 0.0, 0.0], 1)
    assert got[2][0] == 1.0
    got = wo.wmode_row(idx, [1.0, 1.0, 2.0, 2.0, 3.0, 3.0], [9.0, 9.0, np.nan, 1.0, 1.0, 1.0], 1)
    assert wo.bits(got[2])[0] == wo.bits(got[3])[0] == wo.NAN_BITS and got[0][0] == 6
    got = wo.wmode_row(idx, [1.0, 1.0, 1.0, 1.0, 2.0, 3.0], [0.5, 0.5, 0.5, 0.5, 7.0, 1.0], 1)
    assert got[2][0] == 2.0 and got[3][0] == 7.0 and mdo.mode_row(idx, [1.0, 1.0, 1.0, 1.0, 2.0, 3.0], 1)[2][0] == 1.0


def test_the_bound_is_the_projects():
    rng = np.random.default_rng(4)
    idx, v, w = (a[None] for a in _random_row(rng, 3000, 3, exact=False))
    sums = wo.wunique_rows(idx, v, w, 3)[2]
    wo.assert_within_bound(sums, idx, v, w, 3)
    off = sums.copy()
    off[0, 0] += abs(off[0, 0]) * 1e-9 + 1e-9
    with pytest.raises(AssertionError):
        wo.assert_within_bound(off, idx, v, w, 3)


# ---------------------------------------------------------------------------------------------------------------------
# the cases and the restated lines
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wc.gpu_cases(CUS), ids=lambda c: c["name"])
def test_cases_reach_what_they_claim(case):
    edges, idx, xs, v, w = wc.case_data(case, CUS)
    assert idx.shape == v.shape == w.shape == (case["n_rows"], case["n_cols"]) and v.dtype == case["vt"] and w.dtype == case["wt"]
    assert case["n_cols"] <= 140_105
    wc.check_claims(case, idx, v, w, CUS)
    np.testing.assert_array_equal(mo.index(xs, edges), idx)
    if case["layout"] and case["n_cols"] < 2000:  # the sums do not depend on the order of additions: exactly summable
        for r in range(case["n_rows"]):
            b, _, _, sums, _, _ = wo.runs_row(idx[r], v[r], w[r], int(np.prod(case["nbs"])))
            order = np.random.default_rng(r).permutation(case["n_cols"])
            wo.assert_sums(wo.runs_row(idx[r][order], v[r][order], w[r][order], int(np.prod(case["nbs"])))[3], sums, case["name"])


def test_the_case_table_covers_the_list():
    cases = wc.gpu_cases(CUS)
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    claimed = {cl for c in cases for cl in c["claims"]}
    assert claimed >= set(wc.CLAIMS) | {"a NaN value between two equal values' runs", "64 bins of one sample each in one word",
                                        "the same value on both sides of a bin border is two entries", "a bin of only NaNs has no entry",
                                        "dropped samples hold the row's longest run", "both zeros are one entry that reads -0.0",
                                        "every value distinct (U = c)", "one value only", "all dropped (U = 0)"}
    assert {c["n_cols"] for c in cases} >= {1, 63, 64, 65, 513} and {c["n_rows"] for c in cases} >= {1, 3}
    assert len({c["vt"] for c in cases}) == 7 and {c["wt"] for c in cases} == {np.dtype(t) for t in wc.WEIGHT_DTYPES}
    assert {int(np.prod(c["nbs"])) for c in cases} >= {1, 1023, 1024, 1025, 279 * 339}
    assert {c["inverse"] for c in cases} == {True, False}


def test_describe_lines_restated():
    want = wo.predict_unique(CUS, [np.linspace(0, 1, 101)], 0, np.float64, np.float32, 1, 4000, 4000, True)
    line = ("wunique size=4000 inverse=1 words=63 rows_per_launch=37449 | sort keys=fast value_passes=5 bin_passes=1 waves=4 "
            "block=256 chunks=7 chunk=576 slices=1 rows_per_launch=37449 D=1 cmp=0 vdtype=f32")
    assert wo.assert_variant(line, "wunique", want)["sort"]["keys"] == "fast"
    wo.assert_variant("wunique size=3 inverse=0 words=0 rows_per_launch=0 | none", "wunique",
                      wo.predict_unique(CUS, [np.linspace(0, 1, 4)], 0, np.float64, np.uint8, 5, 0, 3, False))
    mline = line.replace("wunique size=4000 inverse=1 ", "wmode ")
    wo.assert_variant(mline, "wmode", wo.predict_mode(CUS, [np.linspace(0, 1, 101)], 0, np.float64, np.float32, 1, 4000))
    wo.assert_variant("wmode words=0 rows_per_launch=0 | none", "wmode", wo.predict_mode(CUS, [np.linspace(0, 1, 4)], 0, np.float64, np.uint8, 5, 0))
    for old, new in (("words=63", "words=64"), ("wunique ", "unique "), ("size=4000", "size=4001"), ("inverse=1", "inverse=0")):
        with pytest.raises(AssertionError):
            wo.assert_variant(line.replace(old, new), "wunique", want)


# ---------------------------------------------------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------------------------------------------------
def _declared(name):
    text = open(os.path.join(ROOT, "include", "xhist_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int %s\(([^;]*)\);" % name, code)
    assert m, "the header does not declare %s(" % name
    return [a.strip() for a in " ".join(m.group(1).split()).split(",")]


def test_c_abi_surface():
    from xhistogram_amd import _native

    assert _declared("xhist_plan_execute_unique_weighted") == [
        "xhist_plan* plan", "const xhist_array* samples", "const xhist_array* values", "const xhist_array* weights", "int64_t n_rows",
        "int64_t n_cols", "int64_t size", "double* out_uniques", "int64_t* out_counts", "double* out_weight_sums", "int64_t* out_offsets",
        "int64_t* out_inverse", "int mem_kind", "void* stream"]
    assert _declared("xhist_plan_execute_mode_weighted") == [
        "xhist_plan* plan", "const xhist_array* samples", "const xhist_array* values", "const xhist_array* weights", "int64_t n_rows",
        "int64_t n_cols", "int64_t* out_count", "int64_t* out_nunique", "double* out_mode", "double* out_mode_weight", "int mem_kind",
        "void* stream"]
    # the unweighted entries are as they were
    assert len(_declared("xhist_plan_execute_unique")) == 12 and len(_declared("xhist_plan_execute_mode")) == 11
    for sym, meth, n in (("xhist_plan_execute_unique_weighted", "execute_unique_weighted", 14),
                         ("xhist_plan_execute_mode_weighted", "execute_mode_weighted", 12)):
        assert sym in _native.EXPORTS and hasattr(_native.Plan, meth)
        assert len(getattr(_native.load(), sym).argtypes) == n
    assert _native.ABI_VERSION == 11 and _native.load().xhist_abi_version() == 11
    text = open(os.path.join(ROOT, "include", "xhist_amd.h")).read()
    assert '"wunique size=.. inverse=0|1 words=.. rows_per_launch=.. | "' in text and '"wmode words=.. rows_per_launch=.. | "' in text


def test_public_surface():
    import xhistogram_amd
    from xhistogram_amd import core
    from xhistogram_amd import xarray as xhx

    for name in ("bin_weighted_unique", "histogram_weighted_mode"):
        assert name in core.__all__ and name in xhx.__all__ and name in xhistogram_amd.__all__
        assert getattr(xhistogram_amd, name) is getattr(core, name)
    assert list(inspect.signature(core.bin_weighted_unique).parameters) == [
        "args", "values", "weights", "bins", "range", "axis", "size", "return_inverse"]
    assert list(inspect.signature(core.histogram_weighted_mode).parameters) == ["args", "values", "weights", "bins", "range", "axis"]
    assert list(inspect.signature(xhx.bin_weighted_unique).parameters) == [
        "args", "values", "weights", "bins", "range", "dim", "size", "return_inverse"]
    for identity in ("math.fsum", "2 * gamma(n) * sum(abs(w))", "np.bincount(inverse[inverse >= 0], weights=w[inverse >= 0], minlength=U)",
                     "histogram(..., weights=w)", "weight_sums == counts"):
        assert identity in core.bin_weighted_unique.__doc__, identity
    # the unweighted calls refuse weights as they did
    with pytest.raises(NotImplementedError, match="histogram_mode does not take weights"):
        core.histogram_mode(np.zeros(3), values=np.zeros(3), weights=np.ones(3), bins=[np.linspace(0, 1, 3)])
    with pytest.raises(TypeError, match="unexpected keyword argument 'weights'"):
        core.bin_unique(np.zeros(3), values=np.zeros(3), weights=np.ones(3), bins=[np.linspace(0, 1, 3)])


def _no_device_work(monkeypatch, core):
    for fn in ("_upload_host", "_value_views", "_get_plan", "_value_rows", "_resident"):
        monkeypatch.setattr(core, fn, lambda *a, **k: pytest.fail("device work"))


class _Shaped:
    def __init__(self, shape, chunks=None):
        self.shape, self.ndim, self.chunks, self.dtype = shape, len(shape), chunks, np.dtype(np.float64)


def test_refusals_before_any_device_work(monkeypatch):
    from xhistogram_amd import core

    _no_device_work(monkeypatch, core)
    e = [np.linspace(0, 1, 3)]
    z = np.zeros(4)
    for fn, name in ((core.bin_weighted_unique, "bin_weighted_unique"), (core.histogram_weighted_mode, "histogram_weighted_mode")):
        with pytest.raises(TypeError, match="%s needs weights" % name):
            fn(z, values=z, weights=None, bins=e)
        with pytest.raises(TypeError, match="missing 1 required keyword-only argument: 'weights'"):
            fn(z, values=z, bins=e)
        with pytest.raises(TypeError, match="complex values have no order"):
            fn(z, values=z, weights=np.zeros(4, np.complex128), bins=e)
        with pytest.raises(TypeError, match="complex values have no order"):
            fn(z, values=np.zeros(4, np.complex64), weights=z, bins=e)
        with pytest.raises(TypeError, match="%s needs values" % name):
            fn(z, values=None, weights=z, bins=e)
        with pytest.raises(TypeError, match="unexpected keyword argument 'descending'"):
            fn(z, values=z, weights=z, descending=True, bins=e)
    for bad in (-1, True, 2.5, "3", (3,)):
        with pytest.raises(ValueError, match="size must be None or an integer >= 0"):
            core.bin_weighted_unique(z, values=z, weights=z, bins=e, size=bad)
    with pytest.raises(TypeError, match="return_inverse must be a bool"):
        core.bin_weighted_unique(z, values=z, weights=z, bins=e, return_inverse=1)

    class _Edges:
        def __len__(self):
            return (1 << 32) + 1

    calls = ((lambda a, **k: core.bin_weighted_unique(a, values=a, weights=a, bins=e, size=10, **k), "bin_weighted_unique"),
             (lambda a, **k: core.histogram_weighted_mode(a, values=a, weights=a, bins=e, **k), "histogram_weighted_mode"))
    for call, name in calls:
        for shape, axis, drop in (((3, 1 << 31), [1], (1,)), ((1 << 31,), None, (0,))):
            arr = _Shaped(shape)
            monkeypatch.setattr(core, "_values_call", lambda *a, arr=arr, axis=axis, drop=drop, **k: ("device", [arr] * 3, None, e, axis, drop))
            with pytest.raises(NotImplementedError, match=r"%s takes fewer than 2\^31 = 2147483648 samples per output row" % name):
                call(arr, axis=axis)
        arr = _Shaped((3, 5))
        monkeypatch.setattr(core, "_values_call", lambda *a, **k: ("device", [arr] * 3, None, [_Edges()], [1], (1,)))
        with pytest.raises(NotImplementedError, match=r"%s takes at most 2\^32 - 1 = 4294967295 bins, got 4294967296" % name):
            call(arr, axis=1)
        arr = _Shaped((4, 6), ((2, 2), (3, 3)))
        monkeypatch.setattr(core, "_values_call", lambda *a, **k: ("dask", [arr] * 3, None, e, [1], (1,)))
        with pytest.raises(ValueError, match="of several chunks cannot be merged: rechunk the reduced axes"):
            call(arr, axis=1)


def test_c_abi_refusals_without_a_device():
    """what the library refuses before it looks for a device: NULL plan aside, the shape checks need a plan, and a plan needs a
    GPU; so here only the symbols' own argument order is exercised with a NULL plan"""
    import ctypes as C

    from xhistogram_amd import _native

    lib = _native.load()
    view = _native.make_view(0, _native.F64, 4, 1)
    arr = (_native.XhistArray * 1)(view)
    null = C.c_void_p(0)
    assert lib.xhist_plan_execute_unique_weighted(None, arr, C.byref(view), C.byref(view), 1, 4, -1, null, null, null, null, null,
                                                  _native.MEM_DEVICE, null) == _native.ERR_INVALID
    assert b"bin_weighted_unique takes a size of 0 or more" in lib.xhist_last_error()
    assert lib.xhist_plan_execute_unique_weighted(None, arr, C.byref(view), None, 1, 4, 1, null, null, null, null, null,
                                                  _native.MEM_DEVICE, null) == _native.ERR_INVALID
    assert b"weights are required" in lib.xhist_last_error()
    assert lib.xhist_plan_execute_mode_weighted(None, arr, C.byref(view), None, 1, 4, null, null, null, null, _native.MEM_DEVICE,
                                                null) == _native.ERR_INVALID
    assert b"weights are required" in lib.xhist_last_error()
    assert lib.xhist_plan_execute_mode_weighted(None, arr, C.byref(view), C.byref(view), 1, 4, null, null, null, null, _native.MEM_DEVICE,
                                                null) == _native.ERR_INVALID
    assert b"plan is NULL" in lib.xhist_last_error()


def test_dask_with_a_cut_reduced_axis_is_refused_before_any_compute(monkeypatch):
    dsa = pytest.importorskip("dask.array")
    from xhistogram_amd import core

    _no_device_work(monkeypatch, core)
    x = dsa.zeros((4, 6), chunks=(2, 3))
    e = [np.linspace(0, 1, 3)]
    with pytest.raises(ValueError, match="distinct values of several chunks"):
        core.bin_weighted_unique(x, values=x, weights=x, bins=e, axis=1)
    y = x.rechunk((2, 6))
    uniques, counts, sums, offsets, inverse, _ = core.bin_weighted_unique(y, values=y, weights=y, bins=e, axis=1, size=4, return_inverse=True)
    assert uniques.shape == counts.shape == sums.shape == (4, 4) and offsets.shape == (4, 3) and inverse.shape == (4, 6)
    assert uniques.dtype == sums.dtype == np.float64 and counts.dtype == offsets.dtype == inverse.dtype == np.int64
