"""histogram_sum without a GPU: the oracle (tests/sum_oracle.py, the definition in Python integers) against math.fsum, exact
rationals and permutations; the host restatement of xhist_sum.hip.h, reached through the library's two test-support entry
points, against the oracle; the C ABI's symbol, the stats table, and the refusals raised before any device work."""
import ctypes as C
import importlib
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

import sum_cases as sc
import sum_oracle as so
from xhistogram_amd import _native, core

try:
    import xarray as xr  # noqa: F401
except ImportError:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "doubles"))
    import xarray as xr  # the double

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20_241


def _sizes(rng, n):
    """bin sizes from 1 to 2 049, most of them small, the ends and the tile borders of the kernels among them"""
    s = np.minimum(2049, np.maximum(1, rng.geometric(0.02, n)))
    s[:6] = [1, 2, 3, 2047, 2048, 2049]
    return s


def narrow_bins(seed=SEED, n=400):
    """random bins whose smallest and largest magnitude lie within 2^42 of each other, over the binades -1070 .. +970"""
    rng = np.random.default_rng(seed)
    out = []
    for size in _sizes(rng, n):
        b = int(rng.integers(-1070, 971))
        v = np.ldexp(rng.uniform(1.0, 2.0, size), b - rng.integers(0, 42, size)) * rng.choice([-1.0, 1.0], size)
        v[0] = math.ldexp(1.5, b)  # (the largest magnitude sits in binade b)
        out.append(v)
    return out


def wide_bins(seed=SEED + 1, n=120):
    """random bins over magnitudes 2^600 apart"""
    rng = np.random.default_rng(seed)
    out = []
    for size in np.minimum(_sizes(rng, n), 600):
        b = int(rng.integers(-400, 971))
        out.append(np.ldexp(rng.uniform(1.0, 2.0, size), b - rng.integers(0, 600, size)) * rng.choice([-1.0, 1.0], size))
    return out


def _exact(v):
    return sum((Fraction(float(x)) for x in v), Fraction(0))


def _rn(fr):
    """a rational, correctly rounded to float64 (int / int is), +-inf on overflow"""
    try:
        return fr.numerator / fr.denominator
    except OverflowError:
        return math.inf if fr > 0 else -math.inf


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_oracle_equals_fsum_on_narrow_spans():
    for v in narrow_bins():
        cnt, tot = so.bin_sum(v)
        want = math.fsum(v)
        assert cnt == len(v) and tot == want and math.copysign(1.0, tot) == math.copysign(1.0, want if want else 0.0), (v[:4], tot, want)


def test_oracle_keeps_the_bound_on_wide_spans():
    truncated = 0
    for v in wide_bins():
        _, tot = so.bin_sum(v)
        exact = _exact(v)
        err = abs(Fraction(tot) - exact)
        assert err <= Fraction(math.ulp(tot)) / 2 + Fraction(so.bound(v)), (v[:4], tot, float(exact))
        truncated += tot != _rn(exact) or any(so.quantum(x, so.unit_exponent(float(np.max(np.abs(v)))))[1] == 0 for x in v.tolist())
    assert truncated > 50  # (the cases do truncate)


def test_oracle_is_permutation_invariant():
    rng = np.random.default_rng(SEED + 2)
    for v in narrow_bins(n=40) + wide_bins(n=40):
        want = so.bin_sum(v)
        for _ in range(3):
            assert so.bin_sum(rng.permutation(v)) == want
        assert so.bin_sum(v[::-1]) == want


def test_offset_data_is_where_a_plain_sum_fails():
    """the issue's example: 10^5 samples of 1e8 + 1e3 N(0, 1) — np.sum depends on the order, the definition does not"""
    v = 1e8 + 1e3 * np.random.default_rng(0).standard_normal(100_000)
    assert so.bin_sum(v)[1] == so.bin_sum(v[::-1])[1] == math.fsum(v)


@pytest.mark.parametrize("name", list(sc.CASES))
def test_directed_cases(name):
    v = sc.CASES[name]
    cnt, tot = so.bin_sum(v)
    if name in sc.EXPECT:
        want_cnt, want = sc.EXPECT[name]
        assert cnt == want_cnt
        sc.same_bits(tot, want, name)
        if want == 0:
            assert not math.copysign(1.0, tot) < 0  # +0.0
    if name in sc.NARROW:
        sc.same_bits(tot, math.fsum(v[~np.isnan(v)]), name + " vs fsum")
    if name == "wide":
        fin = v[~np.isnan(v)]
        assert abs(Fraction(tot) - _exact(fin)) <= Fraction(math.ulp(tot)) / 2 + Fraction(so.bound(fin))
        assert tot != math.fsum(fin) or so.bound(fin) > 0


def test_limb_cases_carry_and_go_negative():
    u = so.unit_exponent(float(np.max(np.abs(sc.CASES["limbs_pos"]))))
    assert u == -20
    quanta = sorted({so.quantum(x, u)[1] for x in sc.CASES["limbs_pos"][:3].tolist()})
    assert quanta == [0xFFFFFFFF, 0xFFFFFFFF << 32, 0xFFFFFFFF << 64]
    assert sc.REPEAT * 0xFFFFFFFF > 1 << 48


def test_round_scaled_against_exact_rationals():
    rng = np.random.default_rng(SEED + 3)
    for nbits in list(range(1, 128)) * 3:
        s = int(rng.integers(0, 1 << 62)) | (int(rng.integers(0, 1 << 62)) << 62) | (int(rng.integers(0, 8)) << 124)
        s = (s >> (127 - nbits)) | (1 << (nbits - 1))
        if rng.random() < 0.3:  # ties and near-ties
            s = (s >> max(0, nbits - 54)) << max(0, nbits - 54)
            s |= int(rng.integers(0, 2))
        for u in (-1074, -1073, -1074 + 60, -1022 - nbits // 2, -20, 0, 900, 1023 - nbits, 1024 - nbits, 1023):
            if u < -1074:
                continue
            for sign in (1, -1):
                want = _rn(Fraction(sign * s) * Fraction(2) ** u)
                assert so.round_scaled(sign * s, u) == want, (s, u, sign)
    assert so.round_scaled(0, 5) == 0.0 and math.copysign(1.0, so.round_scaled(0, 5)) == 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the host restatement of xhist_sum.hip.h
# ---------------------------------------------------------------------------------------------------------------------
def _host(v):
    v = np.ascontiguousarray(v, np.float64)
    cnt, tot = C.c_int64(-1), C.c_double(-1.0)
    rc = _native.load().xhist_debug_sum_host(v.ctypes.data_as(C.POINTER(C.c_double)), v.size, C.byref(cnt), C.byref(tot))
    assert rc == 0
    return cnt.value, tot.value


def _host_round(l0, l1, l2, u):
    out = C.c_double(-1.0)
    assert _native.load().xhist_debug_sum_round(l0, l1, l2, u, C.byref(out)) == 0
    return out.value


def test_host_restatement_equals_the_oracle():
    cases = narrow_bins(n=150) + wide_bins(n=60) + list(sc.CASES.values()) + [np.zeros(0)]
    for v in cases:
        cnt, tot = _host(v)
        want_cnt, want = so.bin_sum(v)
        assert cnt == want_cnt
        sc.same_bits(tot, want, repr(v[:4]))
        if want == 0:
            assert math.copysign(1.0, tot) == 1.0


def test_host_rounding_ties():
    assert _host([2.0 ** 53, 1.0])[1] == 2.0 ** 53
    assert _host([2.0 ** 53, 1.0, 2.0 ** -40])[1] == 2.0 ** 53 + 2.0
    assert _host([2.0 ** 53 + 2.0, 1.0])[1] == 2.0 ** 53 + 4.0
    assert _host([5e-324] * 3) == (3, 1.5e-323)
    assert _host([1.5e308] * 4) == (4, math.inf)
    assert _host([1.5e308, 1.5e308, -1.5e308]) == (3, 1.5e308)


def _split(s):
    """a signed integer below 2^127 in magnitude -> int64 (L0, L1, L2) with L0 + L1 2^32 + L2 2^64 == s"""
    l2 = s >> 64  # (floor)
    rest = s - (l2 << 64)  # 0 .. 2^64 - 1
    l1 = rest >> 32
    l0 = rest & 0xFFFFFFFF
    assert -(1 << 63) <= l2 < (1 << 63) and l0 + (l1 << 32) + (l2 << 64) == s
    return l0, l1, l2


def test_host_rounding_of_54_to_127_bits():
    """results of every length up to 127 bits, both signs, subnormal results and overflow, against the oracle's rounding"""
    rng = np.random.default_rng(SEED + 4)
    seen_sub = seen_inf = 0
    for nbits in list(range(1, 128)) * 2:
        s = int(rng.integers(0, 1 << 62)) | (int(rng.integers(0, 1 << 62)) << 62) | (int(rng.integers(0, 8)) << 124)
        s = (s >> (127 - nbits)) | (1 << (nbits - 1))
        if rng.random() < 0.4 and nbits > 54:  # exactly half way, and one unit to either side
            s = ((s >> (nbits - 53)) << (nbits - 53)) | (1 << (nbits - 54))
            s += int(rng.integers(-1, 2))
        for u in (-1074, -1074 + 30, -1022 - nbits // 2, -20, 0, 1023 - nbits, 1024 - nbits, 1023):
            if u < -1074:
                continue
            for sign in (1, -1):
                want = so.round_scaled(sign * s, u)
                got = _host_round(*_split(sign * s), u)
                assert got == want and math.copysign(1.0, got) == math.copysign(1.0, want), (s, u, sign, got, want)
                seen_sub += 0 < abs(want) < 2.2250738585072014e-308
                seen_inf += math.isinf(want)
    assert seen_sub > 20 and seen_inf > 20
    # accumulators whose limbs disagree in sign, as a bin of mixed signs leaves them
    for l0, l1, l2 in ((-5, 7, -1), (1 << 62, -(1 << 62), 3), (-(1 << 63), (1 << 63) - 1, -(1 << 63)), (0, 0, 0)):
        assert _host_round(l0, l1, l2, -30) == so.round_scaled(l0 + (l1 << 32) + (l2 << 64), -30)


# ---------------------------------------------------------------------------------------------------------------------
# the layers
# ---------------------------------------------------------------------------------------------------------------------
def test_symbol_and_abi_versions_agree():
    assert "xhist_plan_execute_sum" in _native.EXPORTS
    header = open(os.path.join(ROOT, "include", "xhist_amd.h")).read()
    assert "xhist_plan_execute_sum(" in header and "#define XHIST_ABI_VERSION %d" % _native.ABI_VERSION in header
    lib = _native.load()
    assert lib.xhist_abi_version() == _native.ABI_VERSION
    assert len(lib.xhist_plan_execute_sum.argtypes) == 9
    assert callable(getattr(_native.Plan, "execute_sum"))
    assert "xhist_sum" in open(os.path.join(ROOT, "xhistogram_amd", "csrc", "build.sh")).read()


def test_the_statistic_is_an_entry_of_the_stats_table():
    st = core._VALUE_STATS["sum"]
    assert (st.k, st.ints, st.method, st.ptrs, st.extras, st.reduce, st.noun) == (2, (0,), "execute_sum", (0, 1), 0, None, "reproducible sums")
    assert st.max_cols == 1 << 31 and st.max_bins is None and not st.ordered
    # the only entries with a limit: the sum's rows, and the mode's rows and bins (those of bin_sort)
    assert {n: (s.max_cols, s.max_bins) for n, s in core._VALUE_STATS.items() if s.max_cols is not None or s.max_bins is not None} == {
        "sum": (1 << 31, None), "mode": (1 << 31, (1 << 32) - 1)}
    assert "histogram_sum" in core.__all__ and not hasattr(core, "combine_sum")


def _no_device_work(monkeypatch):
    for fn in ("_upload_host", "_value_rows", "_values_blockwise", "_get_plan"):
        monkeypatch.setattr(core, fn, lambda *a, **k: pytest.fail("device work"))


def test_argument_errors_come_before_any_device_work(monkeypatch):
    _no_device_work(monkeypatch)
    x = np.linspace(0, 1, 10)
    e = np.linspace(0, 1, 5)
    with pytest.raises(TypeError, match="multiply them into values"):
        core.histogram_sum(x, values=x, bins=e, weights=x)
    with pytest.raises(TypeError):
        core.histogram_sum(x, bins=e)
    with pytest.raises(TypeError):
        core.histogram_sum(x, values=None, bins=e)
    with pytest.raises(TypeError, match="complex"):
        core.histogram_sum(x, values=x + 1j, bins=e)
    with pytest.raises(TypeError):
        core.histogram_sum(x, values=x.astype("datetime64[s]"), bins=e)
    with pytest.raises(TypeError):
        core.histogram_sum(x, values=x, bins=e, density=True)


class _Shaped:
    """just enough of an array for the front of the call: its shape, and its chunks along each axis"""
    def __init__(self, shape, chunks=None):
        self.shape, self.ndim, self.chunks, self.dtype = shape, len(shape), chunks, np.dtype(np.float64)


def test_rows_of_2_31_samples_are_refused_before_any_device_work(monkeypatch):
    _no_device_work(monkeypatch)
    e = [np.linspace(0, 1, 3)]
    for shape, axis, drop in (((3, 1 << 31), [1], (1,)), ((1 << 16, 2, 1 << 15), [0, 2], (0, 2)), ((1 << 31,), None, (0,))):
        arr = _Shaped(shape)
        monkeypatch.setattr(core, "_values_call", lambda *a, arr=arr, axis=axis, drop=drop, **k: ("device", [arr, arr], None, e, axis, drop))
        with pytest.raises(NotImplementedError, match=r"fewer than 2\^31 = 2147483648 samples per output row"):
            core.histogram_sum(arr, values=arr, bins=e, axis=axis)
    # one sample fewer passes the check (and reaches the device work this test forbids)
    arr = _Shaped((3, (1 << 31) - 1))
    monkeypatch.setattr(core, "_values_call", lambda *a, **k: ("device", [arr, arr], None, e, [1], (1,)))
    with pytest.raises(pytest.fail.Exception, match="device work"):
        core.histogram_sum(arr, values=arr, bins=e, axis=1)


def test_dask_with_a_chunked_reduced_axis_is_refused_before_any_compute(monkeypatch):
    _no_device_work(monkeypatch)
    arr = _Shaped((4, 6), ((2, 2), (3, 3)))
    monkeypatch.setattr(core, "_values_call", lambda *a, **k: ("dask", [arr, arr], None, [np.linspace(0, 1, 3)], [1], (1,)))
    with pytest.raises(ValueError, match="reproducible sums of several chunks cannot be merged: rechunk the reduced axes"):
        core.histogram_sum(arr, values=arr, bins=[np.linspace(0, 1, 3)], axis=1)


def test_host_entry_points_check_their_arguments():
    lib = _native.load()
    out, cnt = C.c_double(0), C.c_int64(0)
    assert lib.xhist_debug_sum_host(None, 3, C.byref(cnt), C.byref(out)) == _native.ERR_INVALID
    assert lib.xhist_debug_sum_host(None, 0, C.byref(cnt), None) == _native.ERR_INVALID
    assert lib.xhist_debug_sum_round(0, 0, 0, -1075, C.byref(out)) == _native.ERR_INVALID
    assert lib.xhist_debug_sum_host(None, 0, C.byref(cnt), C.byref(out)) == 0 and (cnt.value, out.value) == (0, 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# the xarray wrapper, on the test double (compute swapped for the oracle)
# ---------------------------------------------------------------------------------------------------------------------
xhx = importlib.import_module("xhistogram_amd.xarray")


def _oracle_sum(*args, values, bins=None, range=None, axis=None, block_size="auto"):
    bins = [bins] * len(args) if isinstance(bins, np.ndarray) else list(bins)
    return so.histogram_sum(*args, values=values, bins=bins, axis=axis) + (bins,)


def test_xarray_wrapper_names_and_labels(monkeypatch):
    monkeypatch.setattr(core, "histogram_sum", _oracle_sum)
    rng = np.random.default_rng(7)
    dims, shape = ("t", "y", "x"), (2, 3, 40)
    coords = {d: np.arange(n) * 1.0 for d, n in zip(dims, shape)}
    T = xr.DataArray(rng.uniform(0, 1, shape), dims=dims, coords=coords, name="T", attrs={"units": "K"})
    S = xr.DataArray(rng.uniform(0, 1, shape), dims=dims, coords=coords, name="S")
    V = xr.DataArray(1e8 + rng.standard_normal(shape), dims=dims, coords=coords, name="heat")
    bins = [np.linspace(0, 1, 5), np.linspace(0, 1, 4)]
    cnt, tot = xhx.histogram_sum(T, S, values=V, bins=bins, dim=("x", "y"))
    assert (cnt.name, tot.name) == ("heat_count", "heat_sum")
    for da in (cnt, tot):
        assert da.dims == ("t", "T_bin", "S_bin")
        np.testing.assert_array_equal(da["T_bin"].values, 0.5 * (bins[0][:-1] + bins[0][1:]))
    assert tot["T_bin"].attrs == {"units": "K"}
    want = so.histogram_sum(T.values, S.values, values=V.values, bins=bins, axis=(1, 2))
    np.testing.assert_array_equal(cnt.values, want[0])
    sc.same_bits(tot.values, want[1])
    W = xr.DataArray(rng.standard_normal(shape[1:]), dims=dims[1:])  # nameless, broadcast over a dim it lacks
    cnt, tot = xhx.histogram_sum(T, values=W, bins=[bins[0]])
    assert (cnt.name, tot.name) == ("values_count", "values_sum") and cnt.values.dtype == np.int64
    assert "histogram_sum" in xhx.__all__
    with pytest.raises(TypeError):
        xhx.histogram_sum(T, values=V.values, bins=[bins[0]])
    with pytest.raises(TypeError):
        xhx.histogram_sum(T, values=V, weights=V, bins=[bins[0]])
