"""bin_rank where no GPU is needed: tests/bin_rank_oracle.py against a brute-force count of lt, eq, d and D, against
scipy.stats.rankdata and pandas groupby.rank where they are installed, and on the golden hot-path vectors' bin indices; every GPU
case of tests/bin_rank_cases.py held to the conditions it claims; the describe() line restated; the C-ABI surface; and the
Python front's refusals before any device work."""
import os
import re

import numpy as np
import pytest

import bin_rank_cases as rc
import bin_rank_oracle as ro
import bin_sort_oracle as so
import map_oracle as mo
from conftest import MANIFEST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = rc.CUS


def _random_row(rng, n, n_bins):
    idx = rng.integers(-1, max(n_bins, 1), n) if n_bins else np.full(n, -1)
    v = np.round(rng.standard_normal(n) * 2, 0)  # (many ties)
    kind = rng.random(n)
    v[kind < 0.10] = np.nan
    v[(kind >= 0.10) & (kind < 0.18)] = -0.0
    v[(kind >= 0.18) & (kind < 0.26)] = 0.0
    v[(kind >= 0.26) & (kind < 0.30)] = np.inf
    v[(kind >= 0.30) & (kind < 0.34)] = -np.inf
    return idx, v


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,descending,pct", rc.MODES, ids=lambda x: str(x))
def test_oracle_is_the_definition(method, descending, pct):
    rng = np.random.default_rng(ro.METHODS.index(method) * 4 + 2 * descending + pct)
    for n_bins, n in ((0, 5), (1, 0), (1, 1), (1, 40), (3, 17), (7, 120), (40, 90)):
        for _ in range(3):
            idx, v = _random_row(rng, n, n_bins)
            got = ro.rank_row(idx, v, n_bins, method, descending, pct)
            mo.assert_bits(got, ro.brute_force(idx, v, n_bins, method, descending, pct), "%s %d bins %d" % (method, n_bins, n))
            assert np.array_equal(np.isnan(got), (idx < 0) | np.isnan(v))


def test_oracle_on_a_case_small_enough_to_write_down():
    idx = np.array([0, 0, 0, 0, 1, 1, -1, 0, 1])
    v = np.array([2.0, 1.0, 2.0, np.nan, 2.0, -0.0, 1.0, 3.0, 0.0])
    n = np.nan
    want = {"average": [2.5, 1, 2.5, n, 3, 1.5, n, 4, 1.5], "min": [2, 1, 2, n, 3, 1, n, 4, 1], "max": [3, 1, 3, n, 3, 2, n, 4, 2],
            "dense": [2, 1, 2, n, 2, 1, n, 3, 1], "ordinal": [2, 1, 3, n, 3, 1, n, 4, 2]}
    for method, w in want.items():
        mo.assert_bits(ro.rank_row(idx, v, 2, method), np.array(w, np.float64), method)
    mo.assert_bits(ro.rank_row(idx, v, 2, "ordinal", descending=True), np.array([2, 4, 3, n, 1, 3, n, 1, 2], np.float64), "ordinal, descending")
    mo.assert_bits(ro.rank_row(idx, v, 2, "max", pct=True), np.array([3 / 4, 1 / 4, 3 / 4, n, 1, 2 / 3, n, 1, 2 / 3]), "the ECDF")
    mo.assert_bits(ro.rank_row(idx, v, 2, "dense", pct=True), np.array([2 / 3, 1 / 3, 2 / 3, n, 1, 1 / 2, n, 1, 1 / 2]), "dense pct")
    assert ro.rank_rows(idx.reshape(3, 3), v.reshape(3, 3), 2).shape == (3, 3)
    assert np.isnan(ro.rank_rows(np.zeros((2, 4), np.int64), np.ones((2, 4)), 0)).all()  # (no bins: nothing is counted)


@pytest.mark.parametrize("method", ["average", "min", "max", "dense", "ordinal"])
def test_oracle_is_scipys_rankdata_per_bin(method):
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(11)
    for _ in range(20):
        idx, v = _random_row(rng, 150, 6)
        if method == "ordinal":
            v = np.where(v == 0, 0.0, v)  # (scipy breaks ties by position alone; here -0.0 is placed before +0.0)
        got = ro.rank_row(idx, v, 6, method)
        for b in range(6):
            sel = idx == b
            if sel.any() and not np.isnan(v[sel]).all():
                mo.assert_bits(got[sel], np.asarray(stats.rankdata(v[sel], method=method, nan_policy="omit"), np.float64), method)


@pytest.mark.parametrize("method,descending,pct", rc.MODES, ids=lambda x: str(x))
def test_oracle_is_pandas_groupby_rank(method, descending, pct):
    pd = pytest.importorskip("pandas")
    rng = np.random.default_rng(12)
    for _ in range(15):
        idx, v = _random_row(rng, 150, 6)
        if method == "ordinal":
            v = np.where(v == 0, 0.0, v)  # (pandas "first" breaks ties by position alone)
        got = ro.rank_row(idx, v, 6, method, descending, pct)
        keep = idx >= 0
        want = pd.Series(v[keep]).groupby(idx[keep]).rank(method="first" if method == "ordinal" else method, ascending=not descending,
                                                          pct=pct, na_option="keep")
        mo.assert_bits(got[keep], want.to_numpy(np.float64), method)
        assert np.isnan(got[~keep]).all()


@pytest.mark.parametrize("name", sorted(MANIFEST["hotpath"]))
def test_on_the_golden_vectors_bin_indices(golden, name):
    """on the bin indices of the committed vectors: the largest max rank of a bin is its count of non-NaN values (the vector's
    own count where no value is NaN), min rank 1 marks the bin's minimum, and ordinal is the place in bin_sort's segment"""
    samples, edges, w, out = golden.hotpath_case(name)
    if w is not None:
        pytest.skip("a weighted vector: the counts are not in it")
    idx = mo.index(samples, edges)[:3]
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    v = np.round(np.random.default_rng(len(name)).standard_normal(idx.shape), 1)
    top = ro.rank_rows(idx, v, n_bins, "max")
    low = ro.rank_rows(idx, v, n_bins, "min")
    place = ro.rank_rows(idx, v, n_bins, "ordinal")
    order, offsets = so.order_offsets(idx, v, n_bins)
    counts = np.asarray(out).reshape(-1, n_bins)
    for r in range(idx.shape[0]):
        for b in np.unique(idx[r][idx[r] >= 0])[:50]:
            sel = idx[r] == b
            assert top[r][sel].max() == sel.sum() == counts[r, b]
            assert np.array_equal(low[r][sel] == 1, v[r][sel] == v[r][sel].min())
        i = np.arange(idx.shape[1])
        at = np.searchsorted(offsets[r], i, side="right") - 1
        counted = at < n_bins
        mo.assert_bits(place[r][order[r]][counted], (i - offsets[r][np.minimum(at, n_bins - 1)] + 1)[counted].astype(np.float64), name)


def test_identities_of_the_methods():
    rng = np.random.default_rng(13)
    idx, v = _random_row(rng, 400, 5)
    ok = (idx >= 0) & ~np.isnan(v)
    r = {(m, p): ro.rank_row(idx, v, 5, m, pct=p) for m in ro.METHODS for p in (False, True)}
    n = np.bincount(idx[ok], minlength=5)[np.maximum(idx, 0)].astype(np.float64)
    np.testing.assert_array_equal(r["average", False][ok] * 2, (r["min", False] + r["max", False])[ok])
    for m in ("average", "min", "max", "ordinal"):
        mo.assert_bits(r[m, True][ok], (r[m, False] / n)[ok], m)
    assert (r["min", False][ok] <= r["ordinal", False][ok]).all() and (r["ordinal", False][ok] <= r["max", False][ok]).all()
    for b in range(5):
        sel = ok & (idx == b)
        assert r["max", True][sel].max() == 1.0 and r["dense", True][sel].max() == 1.0
        assert sorted(r["ordinal", False][sel]) == list(range(1, sel.sum() + 1))
        assert r["dense", False][sel].max() == len(np.unique(v[sel] + 0.0))


# ---------------------------------------------------------------------------------------------------------------------
# the cases and the restated line
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
@pytest.mark.parametrize("case", rc.gpu_cases(CUS), ids=lambda c: c["name"])
def test_cases_reach_what_they_claim(case, descending):
    edges, idx, xs, v = rc.case_data(case, CUS, descending)
    assert idx.shape == v.shape == (case["n_rows"], case["n_cols"]) and v.dtype == case["vt"] and case["n_cols"] <= 70_000
    assert all(x.dtype == case["st"] for x in xs)
    rc.check_claims(case, idx, v, CUS, descending)
    np.testing.assert_array_equal(mo.index(xs, edges), idx)  # (the samples carry these bin indices)


def test_the_case_table_covers_the_list():
    cases = rc.gpu_cases(CUS)
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    assert {c["n_cols"] for c in cases} >= set(rc.SIZES) and {c["n_rows"] for c in cases} >= {1, 3}
    assert {c["vt"] for c in cases} >= {np.dtype(t) for t in rc.VALUE_DTYPES}
    assert {int(np.prod(c["nbs"])) for c in cases} >= {1, 100, 40960, 279 * 339}
    assert len(rc.MODES) == 20


def test_describe_line_restated():
    want = ro.predict(CUS, [np.linspace(0, 1, 101)], 0, np.float64, np.float32, 1, 4000, "dense", True, True)
    line = ("rank method=dense pct=1 descending=1 words=63 rows_per_launch=37449 | sort keys=fast value_passes=5 bin_passes=1 waves=4 "
            "block=256 chunks=7 chunk=576 slices=1 rows_per_launch=37449 D=1 cmp=0 vdtype=f32")
    assert ro.assert_variant(line, want)["sort"]["keys"] == "fast"
    none = ro.predict(CUS, [np.linspace(0, 1, 4)], 0, np.float64, np.uint8, 5, 0, "average", False, False)
    ro.assert_variant("rank method=average pct=0 descending=0 words=0 rows_per_launch=0 | none", none)
    with pytest.raises(AssertionError):
        ro.assert_variant(line.replace("words=63", "words=64"), want)
    with pytest.raises(AssertionError):
        ro.assert_variant(line.replace("chunks=7", "chunks=8"), want)


# ---------------------------------------------------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------------------------------------------------
def test_c_abi_surface():
    from xhistogram_amd import _native

    text = open(os.path.join(ROOT, "include", "xhist_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int xhist_plan_execute_rank\(([^;]*)\);", code)
    assert m, "the header does not declare xhist_plan_execute_rank("
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["xhist_plan* plan", "const xhist_array* samples", "const xhist_array* values", "int64_t n_rows", "int64_t n_cols",
                    "int method", "int descending", "int pct", "double* out", "int mem_kind", "void* stream"]
    enum = re.search(r"typedef enum \{([^}]*)\} xhist_rank_method;", code)
    names = [x.split("=")[0].strip() for x in enum.group(1).split(",")]
    assert names == ["XHIST_RANK_AVERAGE", "XHIST_RANK_MIN", "XHIST_RANK_MAX", "XHIST_RANK_DENSE", "XHIST_RANK_ORDINAL"]
    assert "XHIST_RANK_AVERAGE = 0" in enum.group(1)
    assert [getattr(_native, n[6:]) for n in names] == [0, 1, 2, 3, 4]
    assert _native.RANK_METHODS == dict(zip(ro.METHODS, range(5)))
    assert "xhist_plan_execute_rank" in _native.EXPORTS and hasattr(_native.Plan, "execute_rank")
    assert _native.ABI_VERSION == 11 and "#define XHIST_ABI_VERSION 11" in text
    lib = _native.load()
    assert lib.xhist_abi_version() == 11 and len(lib.xhist_plan_execute_rank.argtypes) == 11


def test_public_surface():
    import inspect

    from xhistogram_amd import core
    from xhistogram_amd import xarray as xhx

    assert "bin_rank" in core.__all__ and "bin_rank" in xhx.__all__
    params = inspect.signature(core.bin_rank).parameters
    assert list(params) == ["args", "values", "bins", "range", "axis", "method", "descending", "pct"]
    assert (params["method"].default, params["descending"].default, params["pct"].default) == ("average", False, False)
    assert list(inspect.signature(xhx.bin_rank).parameters) == ["args", "values", "bins", "range", "dim", "method", "descending", "pct"]
    with pytest.raises(TypeError, match="needs at least one array"):
        core.bin_rank(values=np.zeros(3), bins=[np.linspace(0, 1, 3)])
    with pytest.raises(TypeError):
        core.bin_rank(np.zeros(3), values=np.zeros(3), weights=np.ones(3), bins=[np.linspace(0, 1, 3)])


def _no_device_work(monkeypatch, core):
    for fn in ("_upload_host", "_value_views", "_get_plan", "_sample_block", "_launch_outputs", "_resident"):
        monkeypatch.setattr(core, fn, lambda *a, **k: pytest.fail("device work"))


class _Shaped:
    """just enough of an array for the front of the call: its shape, and its chunks along each axis"""
    def __init__(self, shape, chunks=None):
        self.shape, self.ndim, self.chunks, self.dtype = shape, len(shape), chunks, np.dtype(np.float64)


def test_refusals_before_any_device_work(monkeypatch):
    from xhistogram_amd import core

    _no_device_work(monkeypatch, core)
    e = [np.linspace(0, 1, 3)]
    with pytest.raises(TypeError, match="complex samples have no order"):
        core.bin_rank(np.zeros(4, np.complex128), values=np.zeros(4), bins=e)
    with pytest.raises(TypeError, match="complex values have no order"):
        core.bin_rank(np.zeros(4), values=np.zeros(4, np.complex64), bins=e)
    with pytest.raises(TypeError, match="bin_rank needs values"):
        core.bin_rank(np.zeros(4), values=None, bins=e)
    for bad in ("mean", "first", None, 0):
        with pytest.raises(ValueError, match="unknown rank method"):
            core.bin_rank(np.zeros(4), values=np.zeros(4), bins=e, method=bad)
    with pytest.raises(TypeError, match="descending must be a bool"):
        core.bin_rank(np.zeros(4), values=np.zeros(4), bins=e, descending=1)
    with pytest.raises(TypeError, match="pct must be a bool"):
        core.bin_rank(np.zeros(4), values=np.zeros(4), bins=e, pct=1)
    with pytest.raises(ValueError, match="bins must be provided"):
        core.bin_rank(np.zeros(4), values=np.zeros(4))
    for shape, axis, drop in (((3, 1 << 31), [1], (1,)), ((1 << 16, 2, 1 << 15), [0, 2], (0, 2)), ((1 << 31,), None, (0,))):
        arr = _Shaped(shape)
        monkeypatch.setattr(core, "_values_call", lambda *a, arr=arr, axis=axis, drop=drop, **k: ("device", [arr, arr], None, e, axis, drop))
        with pytest.raises(NotImplementedError, match=r"bin_rank takes fewer than 2\^31 = 2147483648 samples per output row"):
            core.bin_rank(arr, values=arr, bins=e, axis=axis)
    arr = _Shaped((3, (1 << 31) - 1))  # one sample fewer passes the check (and reaches the device work this test forbids)
    monkeypatch.setattr(core, "_values_call", lambda *a, **k: ("device", [arr, arr], None, e, [1], (1,)))
    with pytest.raises(pytest.fail.Exception, match="device work"):
        core.bin_rank(arr, values=arr, bins=e, axis=1)

    class _Edges:  # (2^32 bins without their 32 GiB of edges)
        def __len__(self):
            return (1 << 32) + 1

    arr = _Shaped((3, 5))
    monkeypatch.setattr(core, "_values_call", lambda *a, **k: ("device", [arr, arr], None, [_Edges()], [1], (1,)))
    with pytest.raises(NotImplementedError, match=r"bin_rank takes at most 2\^32 - 1 = 4294967295 bins, got 4294967296"):
        core.bin_rank(arr, values=arr, bins=e, axis=1)
    arr = _Shaped((4, 6), ((2, 2), (3, 3)))
    monkeypatch.setattr(core, "_values_call", lambda *a, **k: ("dask", [arr, arr], None, e, [1], (1,)))
    with pytest.raises(ValueError, match="ranks of several chunks cannot be merged: rechunk the reduced axes"):
        core.bin_rank(arr, values=arr, bins=e, axis=1)


def test_dask_with_a_cut_reduced_axis_is_refused_before_any_compute(monkeypatch):
    dsa = pytest.importorskip("dask.array")
    from xhistogram_amd import core

    _no_device_work(monkeypatch, core)
    x = dsa.zeros((4, 6), chunks=(2, 3))
    with pytest.raises(ValueError, match="ranks of several chunks"):
        core.bin_rank(x, values=x, bins=[np.linspace(0, 1, 3)], axis=1)
    with pytest.raises(TypeError, match="bins must be provided as numpy array"):
        core.bin_rank(x.rechunk((2, 6)), values=x.rechunk((2, 6)), bins=5, axis=1)
    rank, _ = core.bin_rank(x.rechunk((2, 6)), values=x.rechunk((2, 6)), bins=[np.linspace(0, 1, 3)], axis=1, pct=True)  # (lazy)
    assert rank.shape == (4, 6) and rank.dtype == np.float64 and rank.numblocks == (2, 1)
