"""bin_order where no GPU is needed: tests/bin_order_oracle.py against a pure-Python bucket loop and against the golden
hot-path vectors, its restatement of the host's geometry at the borders, every GPU case table of tests/bin_order_cases.py held
to the conditions it claims, the C-ABI surface, and the Python front's refusals before any device work."""
import os
import re

import numpy as np
import pytest

import bin_order_cases as bc
import bin_order_oracle as bo
import map_oracle as mo
from conftest import MANIFEST, assert_hist_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = bc.CUS
LDS = bo.LDS_MAX


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins,n", [(1, 0), (1, 1), (3, 17), (7, 300), (64, 1000), (500, 257)])
def test_oracle_is_the_bucket_loop(n_bins, n):
    rng = np.random.default_rng(n_bins * 1000 + n)
    idx = rng.integers(-1, n_bins, (3, n))
    order, offsets = bo.order_offsets(idx, n_bins)
    assert order.shape == (3, n) and offsets.shape == (3, n_bins + 1) and order.dtype == offsets.dtype == np.int64
    for r in range(3):
        o, f = bo.bucket_loop(idx[r], n_bins)
        np.testing.assert_array_equal(order[r], o)
        np.testing.assert_array_equal(offsets[r], f)
        bo.assert_grouped(order[r], offsets[r], idx[r], n_bins)


def test_oracle_on_a_case_small_enough_to_write_down():
    idx = np.array([2, -1, 0, 2, 1, -1, 0])
    order, offsets = bo.order_offsets(idx, 3)
    np.testing.assert_array_equal(order, [2, 6, 4, 0, 3, 1, 5])
    np.testing.assert_array_equal(offsets, [0, 2, 3, 5])
    with pytest.raises(AssertionError):
        bo.assert_grouped([6, 2, 4, 0, 3, 1, 5], offsets, idx, 3)  # (not stable)
    with pytest.raises(AssertionError):
        bo.assert_grouped(order, [0, 2, 3, 4], idx, 3)
    # the many-rows form counts the definition at once: the same offsets
    many = np.random.default_rng(1).integers(-1, 2, ((1 << 16) + 3, 2))
    _, got = bo.order_offsets(many, 2)
    np.testing.assert_array_equal(got[:100], bo.order_offsets(many[:100], 2)[1])
    np.testing.assert_array_equal(np.diff(got, axis=1)[:, 0], (many == 0).sum(1))


def test_rows_of_puts_the_reduced_axes_last_in_ascending_order():
    a = np.arange(2 * 3 * 4).reshape(2, 3, 4)
    np.testing.assert_array_equal(bo.rows_of(a, None), a.reshape(-1))
    np.testing.assert_array_equal(bo.rows_of(a, [1]), np.moveaxis(a, 1, 2))
    np.testing.assert_array_equal(bo.rows_of(a, [2, 0]), bo.rows_of(a, [0, 2]))
    np.testing.assert_array_equal(bo.rows_of(a, [0, 2]), np.transpose(a, (1, 0, 2)).reshape(3, 8))


@pytest.mark.parametrize("name", sorted(MANIFEST["hotpath"]))
def test_differences_of_the_offsets_are_the_golden_histogram(golden, name):
    samples, edges, w, out = golden.hotpath_case(name)
    if w is not None:
        pytest.skip("a weighted vector: the counts are not in it")
    idx = mo.index(samples, edges)
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    order, offsets = bo.order_offsets(idx, n_bins)
    assert_hist_equal(np.diff(offsets, axis=-1).reshape(out.shape), out, False)
    for r in range(min(idx.shape[0], 4)):
        bo.assert_grouped(order[r], offsets[r], idx[r], n_bins, name)


# ---------------------------------------------------------------------------------------------------------------------
# the geometry, at its borders
# ---------------------------------------------------------------------------------------------------------------------
def test_lds_bound_and_the_waves_of_a_workgroup():
    assert bo.MAX_BINS == 40959
    g = bo.geometry(CUS, bo.MAX_BINS, 1, 1000)
    assert (g["waves"], g["lds_bytes"], g["block"], g["bits"]) == (1, LDS, 64, 16)
    with pytest.raises(AssertionError):
        bo.geometry(CUS, bo.MAX_BINS + 1, 1, 1000)
    assert bo.geometry(CUS, bo.MAX_BINS - 1, 1, 1000)["lds_bytes"] == LDS - 4
    for nb, waves in ((LDS // 16 - 1, 4), (LDS // 16, 2), (LDS // 8 - 1, 2), (LDS // 8, 1)):
        g = bo.geometry(CUS, nb, 1, 1000)
        assert g["waves"] == waves and g["block"] == 64 * waves and g["lds_bytes"] == waves * (nb + 1) * 4 <= LDS, (nb, g)
    for nb, bits in ((1, 1), (2, 2), (3, 2), (63, 6), (64, 7), (65, 7), (127, 7), (128, 8)):
        assert bo.geometry(CUS, nb, 1, 1000)["bits"] == bits


def test_chunks_of_a_row():
    nb1 = bc.SIZE_BINS + 1
    # one chunk until a row holds two chunks of 2 * (B + 1) positions
    assert bo.geometry(CUS, bc.SIZE_BINS, 1, 4 * nb1 - 1)["chunks"] == 1
    g = bo.geometry(CUS, bc.SIZE_BINS, 1, 4 * nb1)
    assert (g["chunks"], g["chunk"]) == (2, 256)
    # a chunk is whole steps of a wave, at least one
    for n in (1, 63, 64, 65, 1000, 4000, 10**6 + 1):
        for rows in (1, 3, 5000):
            g = bo.geometry(CUS, 3, rows, n)
            assert g["chunk"] % 64 == 0 and g["chunk"] >= 64 and (g["chunks"] - 1) * g["chunk"] < n <= g["chunks"] * g["chunk"], (n, rows, g)
    assert bo.geometry(CUS, 3, 1, 65)["chunks"] == 2 and bo.geometry(CUS, 3, 1, 64)["chunks"] == 1
    # a single row of a few thousand samples is cut; rows that fill the device alone are not
    assert bo.geometry(CUS, bc.SIZE_BINS, 1, bc.REF_COLS) == dict(bits=7, waves=4, block=256, chunks=16, chunk=256, lds_bytes=4 * nb1 * 4,
                                                                   rows_per_launch=((1 << 32) - 1) // 256 * 4 // 16)
    assert bo.geometry(CUS, 50, CUS * 32, 10**6)["chunks"] == 1
    assert bo.geometry(CUS, 50, CUS * 32 - 1, 10**6)["chunks"] == 2
    # few long rows fill the CUs: 32 waves a CU in few bins, what 160 KiB hold of them in many
    g = bo.geometry(CUS, 100, 1, 10**9)  # (whole steps: a few chunks fewer than waves asked for)
    assert g["chunk"] == -(-(-(-10**9 // (CUS * 32))) // 64) * 64 and CUS * 32 - 8 < g["chunks"] <= CUS * 32
    assert bo.geometry(CUS, 100, 456, 720 * 1440)["chunks"] == -(-CUS * 32 // 456)
    assert bo.geometry(CUS, LDS // 16 - 1, 1, 10**9)["chunks"] == CUS * 4


def test_the_counter_table_stays_at_a_quarter_of_the_keys():
    for nb in (1, 7, 100, 2500, 10239, 40959):
        for rows, n in ((1, 10**4), (1, 10**7), (3, 5 * 10**5), (1000, 365), (10**5, 70)):
            g = bo.geometry(CUS, nb, rows, n)
            if g["chunks"] > 1:
                assert bo.table_bytes(CUS, nb, rows, n) * 4 <= rows * n * 8 and g["chunk"] >= 2 * (nb + 1), (nb, rows, n, g)
    # the cap binds: one chunk more would pass it
    g = bo.geometry(CUS, 2500, 1, 10**5)
    assert g["chunks"] == 10**5 // (2 * 2501) == 19


def test_rows_per_launch_keep_the_grid_in_32_bits():
    for nb, rows, n in ((1, 1 << 25, 2), (100, 1 << 20, 365), (100, 1, 10**9), (40959, 7, 10**6)):
        g = bo.geometry(CUS, nb, rows, n)
        units = g["rows_per_launch"] * g["chunks"]
        blocks = -(-units // g["waves"])
        assert blocks < (1 << 31) and blocks * g["block"] < (1 << 32) and g["rows_per_launch"] * 256 < (1 << 32), (nb, rows, n, g)
    assert bo.geometry(CUS, 1, 1 << 25, 2)["rows_per_launch"] == (1 << 24) - 1


def test_slices_of_the_scan():
    assert bo.slice_units(CUS, 100, 1, 255) == (1, 0)  # one chunk: the row's counters are scanned as they are
    assert bo.slice_units(CUS, 100, 1, 404) == (1, 1)
    assert bo.slice_units(CUS, 3, 1, 64 * 64) == (1, 1) and bo.slice_units(CUS, 3, 1, 64 * 65) == (2, 2)
    assert bo.slice_units(CUS, 2500, 1, 2 * 10**8) == (64, 640)
    assert bo.slice_units(CUS, 1, bo.SLICE_GRID + 1, 100) == (1, bo.SLICE_GRID + 1)


def test_describe_line_restated():
    want = bo.predict(CUS, [np.linspace(0, 1, 101)], 0, np.float64, 1, 4000)
    line = ("group keys=fast bits=7 waves=4 block=256 chunks=16 chunk=256 lds_bytes=1616 rows_per_launch=4194303 D=1 cmp=0")
    assert bo.assert_variant(line, want)["keys"] == "fast"
    assert bo.predict(CUS, [np.linspace(0, 1, 4)] * 8, 0, np.float64, 1, 4000)["keys"] == "generic"
    assert bo.predict(CUS, [np.linspace(0, 1, 4)], 1, np.int64, 1, 4000)["keys"] == "generic"
    none = bo.predict(CUS, [np.linspace(0, 1, 4)], 0, np.float64, 5, 0)
    bo.assert_variant("group keys=none bits=0 waves=0 block=0 chunks=0 chunk=0 lds_bytes=0 rows_per_launch=0 D=1 cmp=0", none)
    with pytest.raises(AssertionError):
        bo.assert_variant(line.replace("chunks=16", "chunks=15"), want)


# ---------------------------------------------------------------------------------------------------------------------
# the GPU cases reach what they claim
# ---------------------------------------------------------------------------------------------------------------------
def test_size_list_surrounds_the_chunk():
    c = bc.base_chunk(CUS)
    assert c == 256 and bc.size_list(CUS) == [1, 63, 64, 65, 255, 256, 257, 785, 403, 404]
    assert [bo.geometry(CUS, bc.SIZE_BINS, 1, n)["chunks"] for n in bc.size_list(CUS)] == [1, 1, 1, 1, 1, 1, 1, 3, 1, 2]


@pytest.mark.parametrize("case", bc.gpu_cases(CUS), ids=lambda c: c["name"])
def test_gpu_case_reaches_what_it_claims(case):
    edges, idx, xs = bc.case_data(case, CUS)
    assert idx.shape == (case["n_rows"], case["n_cols"]) and all(x.dtype == case["st"] and x.shape == idx.shape for x in xs)
    bc.check_claims(case, idx, CUS)
    # the samples land in the bins they were emitted from
    sel = slice(None) if idx.size <= 20000 else slice(0, 20000)
    np.testing.assert_array_equal(mo.index([x[:, sel] for x in xs], edges), idx[:, sel])
    if case["pattern"] == "dropped":
        assert any(np.isnan(x).any() for x in xs)


def test_the_claims_are_all_made_by_some_case():
    made = {c for case in bc.gpu_cases(CUS) for c in case["claims"]}
    assert {"several chunks", "run crosses chunk borders", "every lane a distinct key", "one key only", "all dropped", "every sample alone",
            "more than 65535 of one key in one chunk", "lds full", "several slices", "units beyond the slice grid", "several tiles", "waves=4", "waves=2", "waves=1",
            "bits=1", "bits=2", "bits=6", "bits=7"} <= made


# ---------------------------------------------------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------------------------------------------------
def test_c_abi_surface():
    from xhistogram_amd import _native

    text = open(os.path.join(ROOT, "include", "xhist_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int xhist_plan_execute_group\(([^;]*)\);", code)
    assert m, "the header does not declare xhist_plan_execute_group("
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["xhist_plan* plan", "const xhist_array* samples", "int64_t n_rows", "int64_t n_cols", "int64_t* out_order",
                    "int64_t* out_offsets", "int mem_kind", "void* stream"]
    assert "xhist_plan_execute_group" in _native.EXPORTS and hasattr(_native.Plan, "execute_group")
    assert _native.ABI_VERSION == 11 and "#define XHIST_ABI_VERSION 11" in text
    lib = _native.load()
    assert lib.xhist_abi_version() == 11 and len(lib.xhist_plan_execute_group.argtypes) == 8


def test_public_surface():
    from xhistogram_amd import core
    from xhistogram_amd import xarray as xhx

    assert "bin_order" in core.__all__ and "bin_order" in xhx.__all__
    with pytest.raises(TypeError, match="needs at least one array"):
        core.bin_order(bins=[np.linspace(0, 1, 3)])


def _no_device_work(monkeypatch, core):
    for fn in ("_upload_host", "_value_views", "_get_plan", "_order_offsets_rows", "_launch_outputs"):
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
        core.bin_order(np.zeros(4, np.complex128), bins=e)
    with pytest.raises(ValueError, match="bins must be provided"):
        core.bin_order(np.zeros(4))
    for shape, axis, drop in (((3, 1 << 31), [1], (1,)), ((1 << 16, 2, 1 << 15), [0, 2], (0, 2)), ((1 << 31,), None, (0,))):
        arr = _Shaped(shape)
        monkeypatch.setattr(core, "_values_call", lambda *a, arr=arr, axis=axis, drop=drop, **k: ("device", [arr], None, e, axis, drop))
        with pytest.raises(NotImplementedError, match=r"fewer than 2\^31 = 2147483648 samples per output row"):
            core.bin_order(arr, bins=e, axis=axis)
    arr = _Shaped((3, (1 << 31) - 1))  # one sample fewer passes the check (and reaches the device work this test forbids)
    monkeypatch.setattr(core, "_values_call", lambda *a, **k: ("device", [arr], None, e, [1], (1,)))
    with pytest.raises(pytest.fail.Exception, match="device work"):
        core.bin_order(arr, bins=e, axis=1)
    arr = _Shaped((4, 6), ((2, 2), (3, 3)))
    monkeypatch.setattr(core, "_values_call", lambda *a, **k: ("dask", [arr], None, e, [1], (1,)))
    with pytest.raises(ValueError, match="group orders of several chunks cannot be merged: rechunk the reduced axes"):
        core.bin_order(arr, bins=e, axis=1)


@pytest.mark.parametrize("axis", [None, 2, 0, (0, 2), (2, 0), (1,)], ids=str)
def test_sample_shape_undoes_rows_of(monkeypatch, axis):
    """_value_views derives the kept and the reduced axes once; _sample_shape, fed those, puts a [rows, cols] block back where
    the oracle's rows_of took it from"""
    from xhistogram_amd import _native, core

    class _Plan:
        n_dims, n_bins, bins_shape = 1, 2, (2,)

    a = np.arange(3 * 4 * 5).reshape(3, 4, 5)
    like = type("_Like", (), dict(shape=a.shape, ndim=3, dtype=np.dtype(np.float64), device=0))()  # (a DeviceArray's face)

    def rows_cols(arr, ax, full):
        rows = bo.rows_of(a, ax)
        return rows.reshape(-1, rows.shape[-1])

    # no GPU: no device, no plan, no native views; every array takes the general route, a [rows, cols] block
    monkeypatch.setattr(_native, "require_device", lambda device: None)
    monkeypatch.setattr(_native, "make_view", lambda *v: v)
    monkeypatch.setattr(core, "_get_plan", lambda *a: _Plan())
    monkeypatch.setattr(core, "_collapse", lambda *a: None)
    monkeypatch.setattr(core, "_rows_cols", rows_cols)
    monkeypatch.setattr(core, "_strided_view", lambda block, backend: (block,))
    rec = core._value_views([like], None, core._normalise_axis(axis, 3), [np.linspace(0, 1, 3)], "device", ordered=True)
    red = list(range(3)) if axis is None else sorted(np.atleast_1d(axis).tolist())
    assert list(rec.red) == red and list(rec.kept) == [i for i in range(3) if i not in red]
    assert rec.kept_shape == tuple(1 if i in red else a.shape[i] for i in range(3))
    rows = bo.rows_of(a, axis)
    assert (rec.m, rec.c) == (rows.size // rows.shape[-1], rows.shape[-1]) and rec.backend == "device" and rec.like is like
    np.testing.assert_array_equal(core._sample_shape(rows.reshape(rec.m, rec.c), a.shape, rec.kept, rec.red, "device"), a)


def test_each_refusal_text_is_raised_from_one_function(monkeypatch):
    """the limit of 2^31 samples per output row and the refusal of cut reduced axes: one function each, which the per-bin
    statistics and the per-sample calls both go through"""
    from xhistogram_amd import core

    class Marker(Exception):
        pass

    def raise_marker(*a, **k):
        raise Marker()

    _no_device_work(monkeypatch, core)
    e = [np.linspace(0, 1, 3)]
    text = open(core.__file__).read()
    assert text.count("samples per output row, got") == 1 and text.count("of several chunks cannot be merged") == 1
    arr = _Shaped((3, 1 << 31))
    calls = (lambda: core.histogram_sum(arr, values=arr, bins=e, axis=1), lambda: core.bin_order(arr, bins=e, axis=1))
    for n_arrays, call in zip((2, 1), calls):
        monkeypatch.setattr(core, "_values_call", lambda *a, n=n_arrays, **k: ("device", [arr] * n, None, e, [1], (1,)))
        with pytest.raises(NotImplementedError, match=r"fewer than 2\^31 = 2147483648 samples per output row"):
            call()
    cut = _Shaped((4, 6), ((2, 2), (3, 3)))
    for n_arrays, call in zip((2, 1), (lambda: core.histogram_sum(cut, values=cut, bins=e, axis=1), lambda: core.bin_order(cut, bins=e, axis=1))):
        monkeypatch.setattr(core, "_values_call", lambda *a, n=n_arrays, **k: ("dask", [cut] * n, None, e, [1], (1,)))
        with pytest.raises(ValueError, match="of several chunks cannot be merged"):
            call()
    monkeypatch.setattr(core, "_check_one_chunk", raise_marker)
    for n_arrays, call in zip((2, 1), (lambda: core.histogram_sum(cut, values=cut, bins=e, axis=1), lambda: core.bin_order(cut, bins=e, axis=1))):
        monkeypatch.setattr(core, "_values_call", lambda *a, n=n_arrays, **k: ("dask", [cut] * n, None, e, [1], (1,)))
        with pytest.raises(Marker):
            call()
    monkeypatch.setattr(core, "_check_sizes", raise_marker)
    for n_arrays, call in zip((2, 1), calls):
        monkeypatch.setattr(core, "_values_call", lambda *a, n=n_arrays, **k: ("device", [arr] * n, None, e, [1], (1,)))
        with pytest.raises(Marker):
            call()


def test_dask_with_a_cut_reduced_axis_is_refused_before_any_compute(monkeypatch):
    dsa = pytest.importorskip("dask.array")
    from xhistogram_amd import core

    _no_device_work(monkeypatch, core)
    x = dsa.zeros((4, 6), chunks=(2, 3))
    with pytest.raises(ValueError, match="group orders of several chunks"):
        core.bin_order(x, bins=[np.linspace(0, 1, 3)], axis=1)
    with pytest.raises(TypeError, match="bins must be provided as numpy array"):
        core.bin_order(x.rechunk((2, 6)), bins=5, axis=1)
    order, offsets, _ = core.bin_order(x.rechunk((2, 6)), bins=[np.linspace(0, 1, 3)], axis=1)  # (lazy: nothing runs)
    assert order.shape == (4, 6) and offsets.shape == (4, 3) and order.dtype == offsets.dtype == np.int64
    assert order.numblocks == (2, 1) and offsets.numblocks == (2, 1)
