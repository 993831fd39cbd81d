"""bin_unique where no GPU is needed: tests/bin_unique_oracle.py against a brute-force restatement with Python lists and ==,
against np.unique(..., return_counts=True, return_inverse=True) per bin, against pandas groupby.value_counts where pandas is
installed and against tests/mode_oracle.py; every GPU case of tests/bin_unique_cases.py held to the conditions it claims; the
describe() line restated; the C-ABI surface; and the Python front's refusals before any device work."""
import inspect
import os
import re

import numpy as np
import pytest

import bin_unique_cases as uc
import bin_unique_oracle as uo
import map_oracle as mo
import mode_oracle as mdo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = uc.CUS


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
            total = int(uo.unique_row(idx, v, n_bins)[2][-1])
            for size in (None, 0, 1, max(total - 1, 0), total, total + 1, n + 7):
                uo.assert_same(uo.unique_row(idx, v, n_bins, size), uo.brute_force(idx, v, n_bins, size), "%d bins %d size %s" % (n_bins, n, size))


def test_oracle_on_a_case_small_enough_to_write_down():
    idx = np.array([0, 0, 0, 0, 1, 1, -1, 0, 1, 0, 2, 2])
    v = np.array([2.0, 1.0, 2.0, np.nan, 0.0, -0.0, 1.0, 1.0, 5.0, 3.0, np.nan, np.nan])
    p = uo.PAD
    # bin 0: 1, 1, 2, 2, 3; bin 1: both zeros as one entry, and 5; bin 2: NaN only; bin 3: empty; seven entries of padding
    want = (np.array([1.0, 2.0, 3.0, -0.0, 5.0] + [p] * 7), np.array([2, 2, 1, 2, 1] + [0] * 7), np.array([0, 3, 5, 5, 5]),
            np.array([1, 0, 1, -1, 3, 3, -1, 0, 4, 2, -1, -1]))
    uo.assert_same(uo.unique_row(idx, v, 4), want, "written down")
    with pytest.raises(AssertionError):  # (the sign of a zero is held)
        uo.assert_same(uo.unique_row(idx, v, 4), (np.abs(want[0]),) + want[1:])
    with pytest.raises(AssertionError):  # (and so are the bits of the padding)
        uo.assert_same(uo.unique_row(idx, v, 4), (np.where(np.isnan(want[0]), -np.nan, want[0]),) + want[1:])
    cut = uo.unique_row(idx, v, 4, size=2)  # the cut: two entries, the offsets and the inverse as they were
    uo.assert_same(cut, (want[0][:2], want[1][:2], want[2], want[3]), "size=2")
    got = uo.unique_rows(idx.reshape(2, 6), v.reshape(2, 6), 4, size=3)
    assert got[0].shape == got[1].shape == (2, 3) and got[2].shape == (2, 5) and got[3].shape == (2, 6)
    assert got[0].dtype == np.float64 and all(g.dtype == np.int64 for g in got[1:])
    none = uo.unique_rows(np.zeros((2, 4), np.int64), np.ones((2, 4)), 0)  # a plan without bins
    assert (none[2] == 0).all() and none[2].shape == (2, 1) and (none[3] == -1).all() and (none[0].view(np.uint64) == uo.NAN_BITS).all()
    empty = uo.unique_rows(np.zeros((3, 0), np.int64), np.zeros((3, 0)), 5, size=4)
    assert (empty[2] == 0).all() and (empty[0].view(np.uint64) == uo.NAN_BITS).all() and empty[3].shape == (3, 0) and not empty[1].any()


def test_oracle_is_numpys_unique_per_bin():
    rng = np.random.default_rng(11)
    for _ in range(20):
        idx, v = _random_row(rng, 150, 6)
        uniques, counts, offsets, inverse = uo.unique_row(idx, v, 6)
        for b in range(6):
            sel = np.flatnonzero((idx == b) & ~np.isnan(v))
            vals, inv, cnt = np.unique(v[sel], return_inverse=True, return_counts=True)
            seg = slice(offsets[b], offsets[b + 1])
            np.testing.assert_array_equal(uniques[seg], vals)  # (zeros by value)
            np.testing.assert_array_equal(counts[seg], cnt)
            np.testing.assert_array_equal(inverse[sel], offsets[b] + inv.reshape(-1))
        assert (inverse[(idx < 0) | np.isnan(v)] == -1).all()
        total = offsets[-1]
        assert (uniques[total:].view(np.uint64) == uo.NAN_BITS).all() and not counts[total:].any()
        np.testing.assert_array_equal(np.bincount(inverse[inverse >= 0], minlength=total), counts[:total])
        np.testing.assert_array_equal(uniques[inverse[inverse >= 0]], v[inverse >= 0])


def test_oracle_is_pandas_value_counts():
    pd = pytest.importorskip("pandas")
    rng = np.random.default_rng(12)
    for _ in range(15):
        idx, v = _random_row(rng, 150, 6)
        uniques, counts, offsets, _ = uo.unique_row(idx, v, 6)
        keep = idx >= 0
        vc = pd.Series(v[keep] + 0.0).groupby(idx[keep]).value_counts()  # (NaN values are left out)
        assert len(vc) == offsets[-1]
        for b in range(6):
            for u in range(offsets[b], offsets[b + 1]):
                assert vc[(b, uniques[u] + 0.0)] == counts[u]


def test_oracle_agrees_with_the_mode_oracle():
    rng = np.random.default_rng(13)
    for _ in range(20):
        idx, v = _random_row(rng, 200, 7)
        uniques, counts, offsets, _ = uo.unique_row(idx, v, 7)
        count, nunique, mode, mode_count = mdo.mode_row(idx, v, 7)
        np.testing.assert_array_equal(np.diff(offsets), nunique)
        for b in range(7):
            seg = slice(offsets[b], offsets[b + 1])
            assert counts[seg].sum() == count[b]
            if count[b]:
                assert counts[seg].max() == mode_count[b]
                first = offsets[b] + int(np.argmax(counts[seg]))
                assert uniques[first:first + 1].view(np.uint64)[0] == mode[b:b + 1].view(np.uint64)[0]


# ---------------------------------------------------------------------------------------------------------------------
# the cases and the restated line
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", uc.gpu_cases(CUS), ids=lambda c: c["name"])
def test_cases_reach_what_they_claim(case):
    edges, idx, xs, v = uc.case_data(case, CUS)
    assert idx.shape == v.shape == (case["n_rows"], case["n_cols"]) and v.dtype == case["vt"] and case["n_cols"] <= 70_010
    assert all(x.dtype == case["st"] for x in xs)
    uc.check_claims(case, idx, v, CUS)
    np.testing.assert_array_equal(mo.index(xs, edges), idx)  # (the samples carry these bin indices)


def test_the_case_table_covers_the_list():
    cases = uc.gpu_cases(CUS)
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    assert {c["n_cols"] for c in cases} >= set(uc.SIZES) and {c["n_rows"] for c in cases} >= {1, 3}
    assert {c["vt"] for c in cases} >= {np.dtype(t) for t in uc.VALUE_DTYPES} and len(uc.VALUE_DTYPES) == 7
    assert {int(np.prod(c["nbs"])) for c in cases} >= {1, 2, 257, 1025, uo.SCAN_TILE - 1, uo.SCAN_TILE, uo.SCAN_TILE + 1, 279 * 339}
    claimed = {cl for c in cases for cl in c["claims"]}
    assert claimed >= {cl for cls in uc.LAYOUTS.values() for cl in cls} | {"specials", "the scan carries over a tile", "several chunks"}
    assert len(uc.LAYOUTS) == 16
    assert {c["vt"] for c in cases if "specials" in c["claims"]} == {np.dtype(t) for t in (np.float64, np.float32, np.float16)}
    assert {c["inverse"] for c in cases} == {True, False}
    assert uc.sizes_for(5, 9) == [None, 0, 1, 4, 5, 6, 16]


def test_describe_line_restated():
    want = uo.predict(CUS, [np.linspace(0, 1, 101)], 0, np.float64, np.float32, 1, 4000, 4000, True)
    line = ("unique size=4000 inverse=1 words=63 rows_per_launch=37449 | sort keys=fast value_passes=5 bin_passes=1 waves=4 "
            "block=256 chunks=7 chunk=576 slices=1 rows_per_launch=37449 D=1 cmp=0 vdtype=f32")
    assert uo.assert_variant(line, want)["sort"]["keys"] == "fast"
    uo.assert_variant("unique size=3 inverse=0 words=0 rows_per_launch=0 | none",
                      uo.predict(CUS, [np.linspace(0, 1, 4)], 0, np.float64, np.uint8, 5, 0, 3, False))
    for old, new in (("words=63", "words=64"), ("chunks=7", "chunks=8"), ("unique ", "mode "), ("size=4000", "size=4001"),
                     ("inverse=1", "inverse=0")):
        with pytest.raises(AssertionError):
            uo.assert_variant(line.replace(old, new), want)


# ---------------------------------------------------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------------------------------------------------
def test_c_abi_surface():
    from xhistogram_amd import _native

    text = open(os.path.join(ROOT, "include", "xhist_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int xhist_plan_execute_unique\(([^;]*)\);", code)
    assert m, "the header does not declare xhist_plan_execute_unique("
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["xhist_plan* plan", "const xhist_array* samples", "const xhist_array* values", "int64_t n_rows", "int64_t n_cols",
                    "int64_t size", "double* out_uniques", "int64_t* out_counts", "int64_t* out_offsets", "int64_t* out_inverse",
                    "int mem_kind", "void* stream"]
    assert "xhist_plan_execute_unique" in _native.EXPORTS and hasattr(_native.Plan, "execute_unique")
    assert _native.ABI_VERSION == 11 and "#define XHIST_ABI_VERSION 11" in text
    lib = _native.load()
    assert lib.xhist_abi_version() == 11 and len(lib.xhist_plan_execute_unique.argtypes) == 12


def test_public_surface():
    from xhistogram_amd import core
    from xhistogram_amd import xarray as xhx

    assert "bin_unique" in core.__all__ and "bin_unique" in xhx.__all__
    assert list(inspect.signature(core.bin_unique).parameters) == ["args", "values", "bins", "range", "axis", "size", "return_inverse"]
    assert list(inspect.signature(xhx.bin_unique).parameters) == ["args", "values", "bins", "range", "dim", "size", "return_inverse"]
    for identity in ("np.diff(offsets)", "mode_count", "vmin", "vmax", 'bin_rank(method="dense")', "np.bincount(inverse[inverse >= 0], minlength=U)",
                     "uniques[inverse] == values"):
        assert identity in core.bin_unique.__doc__, identity
    with pytest.raises(TypeError, match="needs at least one array"):
        core.bin_unique(values=np.zeros(3), bins=[np.linspace(0, 1, 3)])


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
    for bad in (-1, True, False, 2.0, 2.5, "3", np.float64(3), np.bool_(True), (3,)):
        with pytest.raises(ValueError, match="size must be None or an integer >= 0"):
            core.bin_unique(np.zeros(4), values=np.zeros(4), bins=e, size=bad)
    with pytest.raises(TypeError, match="return_inverse must be a bool"):
        core.bin_unique(np.zeros(4), values=np.zeros(4), bins=e, return_inverse=1)
    with pytest.raises(TypeError, match="unexpected keyword argument 'weights'"):
        core.bin_unique(np.zeros(4), values=np.zeros(4), weights=np.ones(4), bins=e)
    with pytest.raises(TypeError, match="unexpected keyword argument 'descending'"):
        core.bin_unique(np.zeros(4), values=np.zeros(4), descending=True, bins=e)
    with pytest.raises(TypeError, match="complex values have no order"):
        core.bin_unique(np.zeros(4), values=np.zeros(4, np.complex64), bins=e)
    with pytest.raises(TypeError, match="bin_unique needs values"):
        core.bin_unique(np.zeros(4), values=None, bins=e)
    for shape, axis, drop in (((3, 1 << 31), [1], (1,)), ((1 << 16, 2, 1 << 15), [0, 2], (0, 2)), ((1 << 31,), None, (0,))):
        arr = _Shaped(shape)
        monkeypatch.setattr(core, "_values_call", lambda *a, arr=arr, axis=axis, drop=drop, **k: ("device", [arr, arr], None, e, axis, drop))
        with pytest.raises(NotImplementedError, match=r"bin_unique takes fewer than 2\^31 = 2147483648 samples per output row"):
            core.bin_unique(arr, values=arr, bins=e, axis=axis, size=10)
    arr = _Shaped((3, (1 << 31) - 1))  # one sample fewer passes the check (and reaches the device work this test forbids)
    monkeypatch.setattr(core, "_values_call", lambda *a, **k: ("device", [arr, arr], None, e, [1], (1,)))
    with pytest.raises(pytest.fail.Exception, match="device work"):
        core.bin_unique(arr, values=arr, bins=e, axis=1, size=np.int32(10))

    class _Edges:  # (2^32 bins without their 32 GiB of edges)
        def __len__(self):
            return (1 << 32) + 1

    arr = _Shaped((3, 5))
    monkeypatch.setattr(core, "_values_call", lambda *a, **k: ("device", [arr, arr], None, [_Edges()], [1], (1,)))
    with pytest.raises(NotImplementedError, match=r"bin_unique takes at most 2\^32 - 1 = 4294967295 bins, got 4294967296"):
        core.bin_unique(arr, values=arr, bins=e, axis=1)
    arr = _Shaped((4, 6), ((2, 2), (3, 3)))
    monkeypatch.setattr(core, "_values_call", lambda *a, **k: ("dask", [arr, arr], None, e, [1], (1,)))
    with pytest.raises(ValueError, match="distinct values of several chunks cannot be merged: rechunk the reduced axes"):
        core.bin_unique(arr, values=arr, bins=e, axis=1)


def test_dask_with_a_cut_reduced_axis_is_refused_before_any_compute(monkeypatch):
    dsa = pytest.importorskip("dask.array")
    from xhistogram_amd import core

    _no_device_work(monkeypatch, core)
    x = dsa.zeros((4, 6), chunks=(2, 3))
    with pytest.raises(ValueError, match="distinct values of several chunks"):
        core.bin_unique(x, values=x, bins=[np.linspace(0, 1, 3)], axis=1)
    y = x.rechunk((2, 6))
    uniques, counts, offsets, inverse, _ = core.bin_unique(y, values=y, bins=[np.linspace(0, 1, 3)], axis=1, size=4, return_inverse=True)
    assert uniques.shape == counts.shape == (4, 4) and offsets.shape == (4, 3) and inverse.shape == (4, 6)  # (lazy)
    assert uniques.dtype == np.float64 and counts.dtype == offsets.dtype == inverse.dtype == np.int64
