"""bin_sort where no GPU is needed: tests/bin_sort_oracle.py against Python's sorted on tuples and against the golden hot-path
vectors' bin indices, its restatement of the host's geometry at the borders, the table of value digits a dtype makes constant
held to numpy, every GPU case table of tests/bin_sort_cases.py held to the conditions it claims, the C-ABI surface, and the
Python front's refusals before any device work."""
import os
import re

import numpy as np
import pytest

import bin_order_oracle as bo
import bin_sort_cases as sc
import bin_sort_oracle as so
import map_oracle as mo
from conftest import MANIFEST, assert_hist_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = sc.CUS


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("n_bins,n", [(0, 5), (1, 0), (1, 1), (3, 17), (7, 300), (64, 1000), (500, 257)])
def test_oracle_is_sorted_on_tuples(n_bins, n, descending):
    rng = np.random.default_rng(n_bins * 1000 + n)
    idx = rng.integers(-1, max(n_bins, 1), (3, n)) if n_bins else np.full((3, n), -1)
    v = np.round(rng.standard_normal((3, n)) * 2, 0)  # (many ties, both zeros)
    v[rng.random((3, n)) < 0.1] = np.nan
    v[rng.random((3, n)) < 0.1] = -0.0
    order, offsets = so.order_offsets(idx, v, n_bins, descending)
    assert order.shape == (3, n) and offsets.shape == (3, n_bins + 1) and order.dtype == offsets.dtype == np.int64
    for r in range(3):
        o, f = so.brute_force(idx[r], v[r], n_bins, descending)
        np.testing.assert_array_equal(order[r], o)
        np.testing.assert_array_equal(offsets[r], f)
        so.assert_sorted(order[r], offsets[r], idx[r], v[r], n_bins, descending)
    np.testing.assert_array_equal(offsets, bo.order_offsets(idx, n_bins)[1])  # (bin_order's offsets)
    np.testing.assert_array_equal(np.sort(order[:, :0], -1), order[:, :0])


def test_oracle_on_a_case_small_enough_to_write_down():
    idx = np.array([0, 1, -1, 0, 1, 0, -1])
    v = np.array([3.0, np.nan, 1.0, -0.0, 2.0, 0.0, -np.inf])
    order, offsets = so.order_offsets(idx, v, 2)
    np.testing.assert_array_equal(order, [3, 5, 0, 4, 1, 6, 2])  # -0.0 < +0.0 < 3; 2 < NaN; the dropped ones by value too
    np.testing.assert_array_equal(offsets, [0, 3, 5])
    order, offsets = so.order_offsets(idx, v, 2, descending=True)
    np.testing.assert_array_equal(order, [0, 5, 3, 4, 1, 2, 6])  # NaN stays last in its bin
    np.testing.assert_array_equal(offsets, [0, 3, 5])
    with pytest.raises(AssertionError):
        so.assert_sorted([5, 3, 0, 4, 1, 6, 2], offsets, idx, v, 2)
    ties = so.order_offsets(np.zeros(5, np.int64), np.array([1.0, 0.0, 1.0, 0.0, 1.0]), 1)[0]
    np.testing.assert_array_equal(ties, [1, 3, 0, 2, 4])  # ties in ascending position
    ties = so.order_offsets(np.zeros(5, np.int64), np.array([1.0, 0.0, 1.0, 0.0, 1.0]), 1, True)[0]
    np.testing.assert_array_equal(ties, [0, 2, 4, 1, 3])  # ... in both directions


def test_value_keys_are_the_librarys_with_nan_last_both_ways():
    from xhistogram_amd import core

    v = np.array([-np.inf, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, np.inf])
    k = so.value_keys(v)
    np.testing.assert_array_equal(k, core.extrema_keys(v))
    assert (np.diff(k.astype(object)) > 0).all()
    assert (np.diff(so.value_keys(v, True).astype(object)) < 0).all()
    for desc in (False, True):
        kn = so.value_keys(np.array([np.nan, -np.nan, np.inf, -np.inf]), desc)
        assert int(kn[0]) == int(kn[1]) == 2**64 - 1 and int(kn[2]) < 2**64 - 1 and int(kn[3]) < 2**64 - 1


@pytest.mark.parametrize("name", sorted(MANIFEST["hotpath"]))
def test_on_the_golden_vectors_bin_indices(golden, name):
    samples, edges, w, out = golden.hotpath_case(name)
    if w is not None:
        pytest.skip("a weighted vector: the counts are not in it")
    idx = mo.index(samples, edges)
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    v = np.round(np.random.default_rng(len(name)).standard_normal(idx.shape), 1)
    order, offsets = so.order_offsets(idx, v, n_bins)
    assert_hist_equal(np.diff(offsets, axis=-1).reshape(out.shape), out, False)
    grouped = bo.order_offsets(idx, n_bins)
    np.testing.assert_array_equal(offsets, grouped[1])
    for r in range(min(idx.shape[0], 4)):
        so.assert_sorted(order[r], offsets[r], idx[r], v[r], n_bins, False, name)
        for b in range(min(n_bins, 50)):
            seg = slice(offsets[r][b], offsets[r][b + 1])
            np.testing.assert_array_equal(np.sort(order[r][seg]), grouped[0][r][seg])


# ---------------------------------------------------------------------------------------------------------------------
# the geometry, at its borders
# ---------------------------------------------------------------------------------------------------------------------
def test_chunks_of_a_row():
    # a chunk is whole steps of a wave and never shorter than 512 positions unless the row is
    for n in (1, 63, 64, 65, 511, 512, 1023, 1024, 1025, 4000, 40_000, 10**6 + 1):
        for rows in (1, 3, 5000):
            g = so.geometry(CUS, rows, n)
            assert g["chunk"] % 64 == 0 and (g["chunks"] - 1) * g["chunk"] < n <= g["chunks"] * g["chunk"], (n, rows, g)
            assert g["chunks"] == 1 or g["chunk"] >= 512, (n, rows, g)
            assert (g["waves"], g["block"]) == (4, 256)
    assert so.geometry(CUS, 1, 1023)["chunks"] == 1 and so.geometry(CUS, 1, 1024) == dict(
        waves=4, block=256, chunks=2, chunk=512, slices=1, rows_per_launch=(256 << 20) // 2048)
    assert so.geometry(CUS, 1, sc.REF_COLS)["chunks"] == 7 and so.geometry(CUS, 1, sc.REF_COLS)["chunk"] == 576
    # rows that fill the device alone are not cut; few long rows are cut until 32 waves a CU exist
    assert so.geometry(CUS, CUS * 32, 10**6)["chunks"] == 1
    assert so.geometry(CUS, CUS * 32 - 1, 10**6)["chunks"] == 2
    g = so.geometry(CUS, 1, 10**9)
    assert g["chunk"] == -(-(-(-10**9 // (CUS * 32))) // 64) * 64 and CUS * 32 - 8 < g["chunks"] <= CUS * 32
    # slices of 64 chunks
    assert so.geometry(CUS, 1, 64 * 512)["slices"] == 1 and so.geometry(CUS, 1, 65 * 512)["slices"] == 2
    g = so.geometry(CUS, 1, sc.TWO_SLICES)
    assert (g["chunks"], g["chunk"], g["slices"]) == (70, 576, 2)


def test_rows_per_launch_keep_the_grid_in_32_bits_and_the_counters_in_their_budget():
    for rows, n in ((1 << 25, 2), (1 << 20, 365), (1, 10**9), (7, 10**6), (1 << 22, 600)):
        g = so.geometry(CUS, rows, n)
        units = g["rows_per_launch"] * g["chunks"]
        blocks = -(-units // g["waves"])
        assert blocks < (1 << 31) and blocks * g["block"] < (1 << 32) and g["rows_per_launch"] * 256 < (1 << 32), (rows, n, g)
        assert g["rows_per_launch"] >= 1 and (units * 1024 <= so.COUNTER_BYTES or g["rows_per_launch"] == 1), (rows, n, g)
    assert so.geometry(CUS, 1 << 25, 2)["rows_per_launch"] == 1 << 18


def test_passes_of_the_bin_phase():
    want = {0: 0, 1: 1, 2: 1, 255: 1, 256: 2, 257: 2, 40959: 2, 40960: 2, 65535: 2, 65536: 3, 70000: 3, 279 * 339: 3, (1 << 24) - 1: 3,
            1 << 24: 4, (1 << 32) - 1: 4}
    assert {b: so.bin_passes(b) for b in want} == want


# ---------------------------------------------------------------------------------------------------------------------
# the digits of a value key that the dtype makes constant
# ---------------------------------------------------------------------------------------------------------------------
def _every_value(vt):
    """every value of a dtype of at most 16 bits; 2^20 drawn bit patterns and the extremes of a wider one"""
    vt = np.dtype(vt)
    rng = np.random.default_rng(vt.itemsize)
    if vt.kind == "b":
        return np.array([False, True])
    if vt.itemsize <= 2:
        return np.arange(1 << (8 * vt.itemsize), dtype=np.uint32).astype("u%d" % vt.itemsize).view(vt)
    bits = rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32)
    drawn = bits.view(vt) if vt.itemsize == 4 else rng.integers(0, 1 << 63, 1 << 20, dtype=np.uint64).view(vt)
    if vt.kind == "f":
        ends = np.array([0.0, -0.0, np.inf, -np.inf, np.finfo(vt).max, np.finfo(vt).min, np.finfo(vt).smallest_subnormal, np.nan], vt)
    else:
        ends = np.array([np.iinfo(vt).min, np.iinfo(vt).max, 0, 1], vt)
    return np.concatenate([drawn, ends])


@pytest.mark.parametrize("vt", sc.VALUE_DTYPES, ids=lambda t: np.dtype(t).name)
def test_skipped_digits_are_constant_up_to_the_sign(vt):
    """The OR of the keys of all values >= +0.0 shows the claimed zero bits, and the AND of the keys of all values below shows
    them all set (a negative value's key is the complement of its bits): the low digits are a function of the key's top bit,
    and order nothing the higher digits do not.  A NaN's key, all ones, shares its launched digits with no other key."""
    name = so.DTYPE_NAME[np.dtype(vt)]
    shift = so.VALUE_SHIFT[name]
    v = _every_value(vt)
    with np.errstate(invalid="ignore"):  # (signalling NaN patterns among the drawn bits)
        f = v.astype(np.float64)
    low = np.uint64((1 << shift) - 1)
    for desc in (False, True):
        k = so.value_keys(f, desc)
        finite_or_inf = ~np.isnan(f)
        top = (k >> np.uint64(63)) != 0
        up, down = k[finite_or_inf & top], k[finite_or_inf & ~top]  # (either direction: zeros below a set top bit)
        assert len(up) + len(down) == finite_or_inf.sum() and len(up if not desc else down), (name, desc)
        if len(up):  # (an unsigned dtype has no value on the other side of the sign)
            assert int(np.bitwise_or.reduce(up) & low) == 0, (name, desc)
        if len(down):
            assert int(np.bitwise_and.reduce(down) & low) == int(low), (name, desc)
        # what is launched, the digits from shift // 8 on, orders every pair as the whole key does
        launched = k >> np.uint64(8 * (shift // 8))
        order_all, order_launched = np.argsort(k, kind="stable"), np.argsort(launched, kind="stable")
        np.testing.assert_array_equal(order_all, order_launched)
        if np.isnan(f).any():
            assert not (launched[finite_or_inf] == launched[np.isnan(f)][0]).any()
    assert so.value_passes(name) == 8 - shift // 8
    # the claim is sharp for the digit count wherever a dtype has a value that needs its last bit
    if shift:
        k = so.value_keys(f)
        assert int(np.bitwise_or.reduce(k[(k >> np.uint64(63)) != 0]) >> np.uint64(8 * (shift // 8)) & np.uint64(0xFF)) != 0


def test_the_pass_table():
    got = {n: so.value_passes(n) for n in so.VALUE_SHIFT}
    assert got == dict(f64=8, f32=5, f16=3, i64=8, i32=6, i16=4, i8=3, u64=8, u32=6, u16=4, u8=3, bool=2)
    src = open(os.path.join(ROOT, "xhistogram_amd", "csrc", "xhist_sort.hip")).read()
    body = src[src.index("static int sort_value_shift"):src.index("static const char* sort_dtype_name")]
    table = {}
    for line in re.findall(r"((?:case XHIST_\w+:\s*)+)return (\d+);", body):
        for tag in re.findall(r"XHIST_(\w+)", line[0]):
            table[tag.lower()] = int(line[1])
    assert table == {n: s for n, s in so.VALUE_SHIFT.items() if s}, "the host's table and its restatement differ"


# ---------------------------------------------------------------------------------------------------------------------
# the GPU cases reach what they claim
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.gpu_cases(CUS), ids=lambda c: c["name"])
def test_gpu_case_reaches_what_it_claims(case):
    edges, idx, xs, v = sc.case_data(case, CUS)
    assert idx.shape == v.shape == (case["n_rows"], case["n_cols"]) and v.dtype == case["vt"]
    assert all(x.dtype == case["st"] and x.shape == idx.shape for x in xs)
    sc.check_claims(case, idx, v, CUS)
    sel = slice(None) if idx.size <= 20000 else slice(0, 20000)
    np.testing.assert_array_equal(mo.index([x[:, sel] for x in xs], edges), idx[:, sel])


def test_the_claims_are_all_made_by_some_case():
    cases = sc.gpu_cases(CUS)
    made = {c for case in cases for c in case["claims"]}
    want = {"chunks=1", "several chunks", "two slices", "all values equal", "specials", "tie run crosses chunk borders",
            "more than 65535 equal values in one bin", "every lane a distinct digit", "every sample alone", "one key only", "all dropped"}
    want |= {"differs only in digit %d" % k for k in range(8)} | {"value_passes=%d" % p for p in (2, 3, 4, 5, 6, 8)}
    want |= {"bin_passes=%d" % p for p in (1, 2, 3)}
    assert want <= made
    assert {c["n_cols"] for c in cases} >= set(sc.SIZES) and {c["n_rows"] for c in cases} >= {1, 3}
    assert {int(np.prod(c["nbs"])) for c in cases} >= set(sc.BINS_1D) | {279 * 339}
    assert {so.DTYPE_NAME[c["vt"]] for c in cases} == set(so.VALUE_SHIFT)
    assert len({c["name"] for c in cases}) == len(cases)


def test_describe_line_restated():
    want = so.predict(CUS, [np.linspace(0, 1, 101)], 0, np.float64, np.float32, 1, 4000)
    line = "sort keys=fast value_passes=5 bin_passes=1 waves=4 block=256 chunks=7 chunk=576 slices=1 rows_per_launch=37449 D=1 cmp=0 vdtype=f32"
    assert so.assert_variant(line, want)["keys"] == "fast"
    assert so.predict(CUS, [np.linspace(0, 1, 4)] * 8, 0, np.float64, np.float64, 1, 4000)["keys"] == "generic"
    assert so.predict(CUS, [np.array([0.5])], 0, np.float64, np.float64, 1, 4000)["keys"] == "none"
    none = so.predict(CUS, [np.linspace(0, 1, 4)], 0, np.float64, np.uint8, 5, 0)
    so.assert_variant("sort keys=none value_passes=0 bin_passes=0 waves=0 block=0 chunks=0 chunk=0 slices=0 rows_per_launch=0 D=1 cmp=0 "
                      "vdtype=u8", none)
    with pytest.raises(AssertionError):
        so.assert_variant(line.replace("chunks=7", "chunks=8"), want)


# ---------------------------------------------------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------------------------------------------------
def test_c_abi_surface():
    from xhistogram_amd import _native

    text = open(os.path.join(ROOT, "include", "xhist_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int xhist_plan_execute_sort\(([^;]*)\);", code)
    assert m, "the header does not declare xhist_plan_execute_sort("
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["xhist_plan* plan", "const xhist_array* samples", "const xhist_array* values", "int64_t n_rows", "int64_t n_cols",
                    "int descending", "int64_t* out_order", "int64_t* out_offsets", "int mem_kind", "void* stream"]
    assert "xhist_plan_execute_sort" in _native.EXPORTS and hasattr(_native.Plan, "execute_sort")
    assert _native.ABI_VERSION == 11 and "#define XHIST_ABI_VERSION 11" in text
    lib = _native.load()
    assert lib.xhist_abi_version() == 11 and len(lib.xhist_plan_execute_sort.argtypes) == 10


def test_public_surface():
    import inspect

    from xhistogram_amd import core
    from xhistogram_amd import xarray as xhx

    assert "bin_sort" in core.__all__ and "bin_sort" in xhx.__all__
    params = inspect.signature(core.bin_sort).parameters
    assert list(params) == ["args", "values", "bins", "range", "axis", "descending"] and "weights" not in params
    with pytest.raises(TypeError, match="needs at least one array"):
        core.bin_sort(values=np.zeros(3), bins=[np.linspace(0, 1, 3)])
    with pytest.raises(TypeError):
        core.bin_sort(np.zeros(3), values=np.zeros(3), weights=np.ones(3), bins=[np.linspace(0, 1, 3)])


def _no_device_work(monkeypatch, core):
    for fn in ("_upload_host", "_value_views", "_get_plan", "_order_offsets_rows", "_launch_outputs", "_resident"):
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
        core.bin_sort(np.zeros(4, np.complex128), values=np.zeros(4), bins=e)
    with pytest.raises(TypeError, match="complex values have no order"):
        core.bin_sort(np.zeros(4), values=np.zeros(4, np.complex64), bins=e)
    with pytest.raises(TypeError, match="bin_sort needs values"):
        core.bin_sort(np.zeros(4), values=None, bins=e)
    with pytest.raises(TypeError, match="descending must be a bool"):
        core.bin_sort(np.zeros(4), values=np.zeros(4), bins=e, descending=1)
    with pytest.raises(ValueError, match="bins must be provided"):
        core.bin_sort(np.zeros(4), values=np.zeros(4))
    for shape, axis, drop in (((3, 1 << 31), [1], (1,)), ((1 << 16, 2, 1 << 15), [0, 2], (0, 2)), ((1 << 31,), None, (0,))):
        arr = _Shaped(shape)
        monkeypatch.setattr(core, "_values_call", lambda *a, arr=arr, axis=axis, drop=drop, **k: ("device", [arr, arr], None, e, axis, drop))
        with pytest.raises(NotImplementedError, match=r"fewer than 2\^31 = 2147483648 samples per output row"):
            core.bin_sort(arr, values=arr, bins=e, axis=axis)
    arr = _Shaped((3, (1 << 31) - 1))  # one sample fewer passes the check (and reaches the device work this test forbids)
    monkeypatch.setattr(core, "_values_call", lambda *a, **k: ("device", [arr, arr], None, e, [1], (1,)))
    with pytest.raises(pytest.fail.Exception, match="device work"):
        core.bin_sort(arr, values=arr, bins=e, axis=1)

    class _Edges:  # (2^32 bins without their 32 GiB of edges)
        def __len__(self):
            return (1 << 32) + 1

    arr = _Shaped((3, 5))
    monkeypatch.setattr(core, "_values_call", lambda *a, **k: ("device", [arr, arr], None, [_Edges()], [1], (1,)))
    with pytest.raises(NotImplementedError, match=r"at most 2\^32 - 1 = 4294967295 bins, got 4294967296"):
        core.bin_sort(arr, values=arr, bins=e, axis=1)
    arr = _Shaped((4, 6), ((2, 2), (3, 3)))
    monkeypatch.setattr(core, "_values_call", lambda *a, **k: ("dask", [arr, arr], None, e, [1], (1,)))
    with pytest.raises(ValueError, match="sorted orders of several chunks cannot be merged: rechunk the reduced axes"):
        core.bin_sort(arr, values=arr, bins=e, axis=1)


def test_more_than_40959_bins_pass_the_front(monkeypatch):
    """bin_order's bound is not bin_sort's: 40 960 and 279 x 339 bins reach the device work"""
    from xhistogram_amd import core

    _no_device_work(monkeypatch, core)
    for bins in ([np.linspace(0, 1, 40962)], [np.linspace(0, 1, 280), np.linspace(0, 1, 340)]):
        xs = [np.zeros(10)] * len(bins)
        with pytest.raises(pytest.fail.Exception, match="device work"):
            core.bin_sort(*xs, values=np.zeros(10), bins=bins)


def test_dask_with_a_cut_reduced_axis_is_refused_before_any_compute(monkeypatch):
    dsa = pytest.importorskip("dask.array")
    from xhistogram_amd import core

    _no_device_work(monkeypatch, core)
    x = dsa.zeros((4, 6), chunks=(2, 3))
    with pytest.raises(ValueError, match="sorted orders of several chunks"):
        core.bin_sort(x, values=x, bins=[np.linspace(0, 1, 3)], axis=1)
    with pytest.raises(TypeError, match="bins must be provided as numpy array"):
        core.bin_sort(x.rechunk((2, 6)), values=x.rechunk((2, 6)), bins=5, axis=1)
    order, offsets, _ = core.bin_sort(x.rechunk((2, 6)), values=x.rechunk((2, 6)), bins=[np.linspace(0, 1, 3)], axis=1)  # (lazy)
    assert order.shape == (4, 6) and offsets.shape == (4, 3) and order.dtype == offsets.dtype == np.int64
    assert order.numblocks == (2, 1) and offsets.numblocks == (2, 1)
