"""histogram_mode where no GPU is needed: tests/mode_oracle.py against a brute-force count with Python's ==, against
scipy.stats.mode and pandas groupby where they are installed, and on the golden hot-path vectors' bin indices; every GPU case of
tests/mode_cases.py held to the conditions it claims; the describe() line restated; the "mode" entry of the statistics' table;
the C-ABI surface; and the Python front's refusals before any device work."""
import inspect
import os
import pickle
import re
from functools import partial

import numpy as np
import pytest

import map_oracle as mo
import mode_cases as mc
import mode_oracle as mdo
from conftest import MANIFEST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = mc.CUS


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
def test_oracle_is_the_definition():
    rng = np.random.default_rng(1)
    for n_bins, n in ((0, 5), (1, 0), (1, 1), (1, 40), (3, 17), (7, 120), (40, 90), (5, 400)):
        for _ in range(4):
            idx, v = _random_row(rng, n, n_bins)
            mdo.assert_same(mdo.mode_row(idx, v, n_bins), mdo.brute_force(idx, v, n_bins), "%d bins %d" % (n_bins, n))


def test_oracle_on_a_case_small_enough_to_write_down():
    idx = np.array([0, 0, 0, 0, 1, 1, -1, 0, 1, 0, 2, 2])
    v = np.array([2.0, 1.0, 2.0, np.nan, 0.0, -0.0, 1.0, 1.0, 5.0, 3.0, np.nan, np.nan])
    n = np.nan
    # bin 0: 1, 1, 2, 2, 3 (two runs of two: the smaller value); bin 1: a run of both zeros, and 5; bin 2: NaN only; bin 3: empty
    want = (np.array([5, 3, 0, 0]), np.array([3, 2, 0, 0]), np.array([1.0, -0.0, n, n]), np.array([2, 2, 0, 0]))
    mdo.assert_same(mdo.mode_row(idx, v, 4), want, "written down")
    with pytest.raises(AssertionError):  # (the sign of a zero is held)
        mdo.assert_same(mdo.mode_row(idx, v, 4), (want[0], want[1], np.array([1.0, 0.0, n, n]), want[3]))
    got = mdo.mode_rows(idx.reshape(2, 6), v.reshape(2, 6), 4)
    assert all(g.shape == (2, 4) for g in got) and got[2].dtype == np.float64 and got[0].dtype == np.int64
    assert mdo.mode_rows(np.zeros((2, 4), np.int64), np.ones((2, 4)), 0)[2].shape == (2, 0)
    empty = mdo.mode_rows(np.zeros((3, 0), np.int64), np.zeros((3, 0)), 5)
    assert (empty[0] == 0).all() and (empty[2].view(np.uint64) == mdo.NAN_BITS).all()


def test_oracle_is_scipys_mode_per_bin():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(11)
    for _ in range(20):
        idx, v = _random_row(rng, 150, 6)
        count, nunique, mode, mode_count = mdo.mode_row(idx, v, 6)
        for b in range(6):
            vals = v[(idx == b) & ~np.isnan(v)]
            assert count[b] == len(vals) and nunique[b] == len(np.unique(vals + 0.0))
            if len(vals):
                res = stats.mode(vals, nan_policy="omit")
                assert float(np.ravel(res.mode)[0]) == mode[b] and int(np.ravel(res.count)[0]) == mode_count[b]  # (zeros by value)
            else:
                assert np.isnan(mode[b]) and mode_count[b] == 0


def test_oracle_is_pandas_groupby():
    pd = pytest.importorskip("pandas")
    rng = np.random.default_rng(12)
    for _ in range(15):
        idx, v = _random_row(rng, 150, 6)
        count, nunique, mode, mode_count = mdo.mode_row(idx, v, 6)
        keep = idx >= 0
        grouped = pd.Series(v[keep] + 0.0).groupby(idx[keep])
        nun = grouped.nunique()
        cnt = grouped.count()
        top = grouped.agg(lambda s: s.mode()[0] if s.notna().any() else np.nan)
        for b in range(6):
            if b in nun.index:
                assert nunique[b] == nun[b] and count[b] == cnt[b]
                assert (np.isnan(mode[b]) and np.isnan(top[b])) or mode[b] == top[b]  # (zeros by value)
            else:
                assert count[b] == 0 and nunique[b] == 0 and mode_count[b] == 0


@pytest.mark.parametrize("name", sorted(MANIFEST["hotpath"]))
def test_on_the_golden_vectors_bin_indices(golden, name):
    """on the bin indices of the committed vectors, with values that never are NaN: count is the vector's own count; with every
    value distinct the mode is the bin's minimum, once; with one value it is that value, count times"""
    samples, edges, w, out = golden.hotpath_case(name)
    if w is not None:
        pytest.skip("a weighted vector: the counts are not in it")
    idx = mo.index(samples, edges)[:3]
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    counts = np.asarray(out).reshape(-1, n_bins)[:idx.shape[0]]
    rng = np.random.default_rng(len(name))
    alone = np.stack([rng.permutation(idx.shape[1]) for _ in range(idx.shape[0])]).astype(np.float64)
    count, nunique, mode, mode_count = mdo.mode_rows(idx, alone, n_bins)
    np.testing.assert_array_equal(count, counts)
    np.testing.assert_array_equal(nunique, counts)
    np.testing.assert_array_equal(mode_count, np.minimum(counts, 1))
    for r in range(idx.shape[0]):
        for b in np.unique(idx[r][idx[r] >= 0])[:50]:
            assert mode[r, b] == alone[r][idx[r] == b].min()
    count, nunique, mode, mode_count = mdo.mode_rows(idx, np.float32(2.5), n_bins)
    np.testing.assert_array_equal(count, counts)
    np.testing.assert_array_equal(mode_count, counts)
    np.testing.assert_array_equal(nunique, np.minimum(counts, 1))
    assert (mode[counts > 0] == 2.5).all() and np.isnan(mode[counts == 0]).all()
    ties = np.round(rng.standard_normal(idx.shape), 1)
    if n_bins <= 200:
        mdo.assert_same(mdo.mode_row(idx[0], ties[0], n_bins), mdo.brute_force(idx[0], ties[0], n_bins), name)


# ---------------------------------------------------------------------------------------------------------------------
# the cases and the restated line
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.gpu_cases(CUS), ids=lambda c: c["name"])
def test_cases_reach_what_they_claim(case):
    edges, idx, xs, v = mc.case_data(case, CUS)
    assert idx.shape == v.shape == (case["n_rows"], case["n_cols"]) and v.dtype == case["vt"] and case["n_cols"] <= 70_010
    assert all(x.dtype == case["st"] for x in xs)
    mc.check_claims(case, idx, v, CUS)
    np.testing.assert_array_equal(mo.index(xs, edges), idx)  # (the samples carry these bin indices)


def test_the_case_table_covers_the_list():
    cases = mc.gpu_cases(CUS)
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    assert {c["n_cols"] for c in cases} >= set(mc.SIZES) and {c["n_rows"] for c in cases} >= {1, 3}
    assert {c["vt"] for c in cases} >= {np.dtype(t) for t in mc.VALUE_DTYPES} and len(mc.VALUE_DTYPES) == 7
    assert {int(np.prod(c["nbs"])) for c in cases} >= {1, 50, 40960, 279 * 339}
    claimed = {cl for c in cases for cl in c["claims"]}
    assert claimed >= {cl for cls in mc.LAYOUTS.values() for cl in cls} | {"every value distinct", "one value only", "all dropped", "specials"}
    assert {c["vt"] for c in cases if "specials" in c["claims"]} == {np.dtype(t) for t in (np.float64, np.float32, np.float16)}


def test_describe_line_restated():
    want = mdo.predict(CUS, [np.linspace(0, 1, 101)], 0, np.float64, np.float32, 1, 4000)
    line = ("mode words=63 rows_per_launch=37449 | sort keys=fast value_passes=5 bin_passes=1 waves=4 "
            "block=256 chunks=7 chunk=576 slices=1 rows_per_launch=37449 D=1 cmp=0 vdtype=f32")
    assert mdo.assert_variant(line, want)["sort"]["keys"] == "fast"
    mdo.assert_variant("mode words=0 rows_per_launch=0 | none", mdo.predict(CUS, [np.linspace(0, 1, 4)], 0, np.float64, np.uint8, 5, 0))
    with pytest.raises(AssertionError):
        mdo.assert_variant(line.replace("words=63", "words=64"), want)
    with pytest.raises(AssertionError):
        mdo.assert_variant(line.replace("chunks=7", "chunks=8"), want)
    with pytest.raises(AssertionError):
        mdo.assert_variant(line.replace("mode ", "rank "), want)


# ---------------------------------------------------------------------------------------------------------------------
# the table entry and the surface
# ---------------------------------------------------------------------------------------------------------------------
def test_the_table_entry():
    from xhistogram_amd import core

    st = core._VALUE_STATS["mode"]
    assert (st.k, st.ints, st.method, st.ptrs, st.extras, st.reduce, st.tail, st.ordered, st.noun, st.max_cols, st.max_bins) == (
        4, (0, 1, 3), "execute_mode", (0, 1, 2, 3), 0, None, (), False, "modes", 1 << 31, (1 << 32) - 1)  # (bin_sort's two limits)
    assert pickle.loads(pickle.dumps(st)) == st
    block = pickle.loads(pickle.dumps(partial(core._value_block, stat="mode")))  # (what a dask task carries)
    assert block.keywords == {"stat": "mode"}


def test_c_abi_surface():
    from xhistogram_amd import _native

    text = open(os.path.join(ROOT, "include", "xhist_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int xhist_plan_execute_mode\(([^;]*)\);", code)
    assert m, "the header does not declare xhist_plan_execute_mode("
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["xhist_plan* plan", "const xhist_array* samples", "const xhist_array* values", "int64_t n_rows", "int64_t n_cols",
                    "int64_t* out_count", "int64_t* out_nunique", "double* out_mode", "int64_t* out_mode_count", "int mem_kind", "void* stream"]
    assert "xhist_plan_execute_mode" in _native.EXPORTS and hasattr(_native.Plan, "execute_mode")
    assert _native.ABI_VERSION == 11 and "#define XHIST_ABI_VERSION 11" in text
    lib = _native.load()
    assert lib.xhist_abi_version() == 11 and len(lib.xhist_plan_execute_mode.argtypes) == 11


def test_public_surface():
    from xhistogram_amd import core
    from xhistogram_amd import xarray as xhx

    assert "histogram_mode" in core.__all__ and "histogram_mode" in xhx.__all__
    params = inspect.signature(core.histogram_mode).parameters
    assert list(params)[:5] == ["args", "values", "bins", "range", "axis"] and "block_size" in params and "descending" not in params
    assert list(inspect.signature(xhx.histogram_mode).parameters) == ["args", "values", "bins", "range", "dim", "block_size", "keep_coords",
                                                                       "bin_dim_suffix"]
    with pytest.raises(TypeError, match="needs at least one array"):
        core.histogram_mode(values=np.zeros(3), bins=[np.linspace(0, 1, 3)])


def _no_device_work(monkeypatch, core):
    for fn in ("_upload_host", "_value_views", "_get_plan", "_value_rows", "_resident"):
        monkeypatch.setattr(core, fn, lambda *a, **k: pytest.fail("device work"))


class _Shaped:
    """just enough of an array for the front of the call: its shape, and its chunks along each axis"""
    def __init__(self, shape, chunks=None):
        self.shape, self.ndim, self.chunks, self.dtype = shape, len(shape), chunks, np.dtype(np.float64)


def test_refusals_before_any_device_work(monkeypatch):
    from xhistogram_amd import core

    _no_device_work(monkeypatch, core)
    e = [np.linspace(0, 1, 3)]
    with pytest.raises(NotImplementedError, match="histogram_mode does not take weights"):
        core.histogram_mode(np.zeros(4), values=np.zeros(4), weights=np.ones(4), bins=e)
    with pytest.raises(TypeError, match="complex values have no order"):
        core.histogram_mode(np.zeros(4), values=np.zeros(4, np.complex64), bins=e)
    with pytest.raises(TypeError, match="histogram_mode needs values"):
        core.histogram_mode(np.zeros(4), values=None, bins=e)
    for shape, axis, drop in (((3, 1 << 31), [1], (1,)), ((1 << 16, 2, 1 << 15), [0, 2], (0, 2)), ((1 << 31,), None, (0,))):
        arr = _Shaped(shape)
        monkeypatch.setattr(core, "_values_call", lambda *a, arr=arr, axis=axis, drop=drop, **k: ("device", [arr, arr], None, e, axis, drop))
        with pytest.raises(NotImplementedError, match=r"histogram_mode takes fewer than 2\^31 = 2147483648 samples per output row"):
            core.histogram_mode(arr, values=arr, bins=e, axis=axis)
    arr = _Shaped((3, (1 << 31) - 1))  # one sample fewer passes the check (and reaches the device work this test forbids)
    monkeypatch.setattr(core, "_values_call", lambda *a, **k: ("device", [arr, arr], None, e, [1], (1,)))
    with pytest.raises(pytest.fail.Exception, match="device work"):
        core.histogram_mode(arr, values=arr, bins=e, axis=1)

    class _Edges:  # (2^32 bins without their 32 GiB of edges)
        def __len__(self):
            return (1 << 32) + 1

    arr = _Shaped((3, 5))
    monkeypatch.setattr(core, "_values_call", lambda *a, **k: ("device", [arr, arr], None, [_Edges()], [1], (1,)))
    with pytest.raises(NotImplementedError, match=r"histogram_mode takes at most 2\^32 - 1 = 4294967295 bins, got 4294967296"):
        core.histogram_mode(arr, values=arr, bins=e, axis=1)
    arr = _Shaped((4, 6), ((2, 2), (3, 3)))
    monkeypatch.setattr(core, "_values_call", lambda *a, **k: ("dask", [arr, arr], None, e, [1], (1,)))
    with pytest.raises(ValueError, match="modes of several chunks cannot be merged: rechunk the reduced axes"):
        core.histogram_mode(arr, values=arr, bins=e, axis=1)


def test_dask_with_a_cut_reduced_axis_is_refused_before_any_compute(monkeypatch):
    dsa = pytest.importorskip("dask.array")
    from xhistogram_amd import core

    _no_device_work(monkeypatch, core)
    x = dsa.zeros((4, 6), chunks=(2, 3))
    with pytest.raises(ValueError, match="modes of several chunks"):
        core.histogram_mode(x, values=x, bins=[np.linspace(0, 1, 3)], axis=1)
    count, nunique, mode, mode_count, _ = core.histogram_mode(x.rechunk((2, 6)), values=x.rechunk((2, 6)), bins=[np.linspace(0, 1, 3)], axis=1)
    assert mode.shape == (4, 2) and mode.numblocks == (2, 1)  # (lazy)
