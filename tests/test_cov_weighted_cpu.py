"""histogram_weighted_cov without a GPU: the oracle (tests/cov_weighted_oracle.py) against np.cov with fweights and aweights,
the exactness analysis of tests/cov_weighted_exact.py on the host, the host merge of dask partials (core.combine_weighted_cov)
against the scalar restatement of tests/test_chan_merge_cpu.py bit for bit, argument errors raised before any device work, the
new C symbol, the xarray wrapper's names (compute swapped for the oracle), and the data conditions of every case of
tests/test_gpu_cov_weighted.py: each exact case has at least one bin on the bit-for-bit path."""
import importlib
import os
import pickle
import sys

import numpy as np
import pytest

import cov_weighted_exact as cwx
import cov_weighted_oracle as cwo
import test_chan_merge_cpu as tcm
import test_gpu_cov_weighted as tg
import values_exact as vx
from test_gpu_cov import predict_cov
from xhistogram_amd import _native, core

try:
    import xarray as xr  # noqa: F401
except ImportError:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "doubles"))
    import xarray as xr  # the double

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32 = np.float64, np.float32
CUS = 256  # (the segments per row depend on it; nothing asserted here does)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle against numpy
# ---------------------------------------------------------------------------------------------------------------------
def _per_bin_cov(x, edges, a, b, w, **cov_kw):
    """np.cov over the pairwise-complete triples of each bin of one row (1-D edges): (W, mean_a, mean_b, var_a, var_b, cov_ab)"""
    nb = len(edges) - 1
    idx = np.searchsorted(edges, x, side="right") - 1
    idx[x == edges[-1]] = nb - 1
    ok = (x >= edges[0]) & (x <= edges[-1]) & ~np.isnan(a) & ~np.isnan(b)
    out = [np.zeros(nb)] + [np.full(nb, np.nan) for _ in range(5)]
    for k in range(nb):
        sel = ok & (idx == k)
        out[0][k] = w[sel].sum()
        if out[0][k] > 0:
            out[1][k], out[2][k] = np.average(a[sel], weights=w[sel]), np.average(b[sel], weights=w[sel])
            c = np.cov(a[sel], b[sel], **{key: (w[sel].astype(int) if key == "fweights" else w[sel]) for key in cov_kw if key != "ddof"},
                       **({"ddof": cov_kw["ddof"]} if "ddof" in cov_kw else {}))
            out[3][k], out[4][k], out[5][k] = c[0, 0], c[1, 1], c[0, 1]
    return out


def _random_case(seed, integer):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(40, 400))
    edges = np.sort(rng.uniform(-2, 2, int(rng.integers(3, 8))))
    x = rng.uniform(-2.5, 2.5, n)
    on_edge = rng.random(n) < 0.2
    x[on_edge] = edges[rng.integers(0, len(edges), int(on_edge.sum()))]
    x[rng.random(n) < 0.05] = np.nan
    a = rng.standard_normal(n) * 3 + 10
    b = (-0.5 if seed % 2 else 0.7) * a + rng.standard_normal(n) - 4
    a[rng.random(n) < 0.08] = np.nan
    b[rng.random(n) < 0.08] = np.nan
    w = rng.integers(1, 8, n).astype(F64) if integer else rng.uniform(0.1, 3.0, n)
    return edges, x, a, b, w


@pytest.mark.parametrize("seed", range(4))
def test_oracle_matches_np_cov_fweights(seed):
    """integer weights, ddof = 1: np.cov(a_bin, b_bin, fweights=w_bin), to the last digit or two"""
    edges, x, a, b, w = _random_case(seed, True)
    want = _per_bin_cov(x, edges, a, b, w, fweights=True)
    for exact in (False, True):
        got = cwo.histogram_weighted_cov(x, values=(a, b), weights=w, bins=[edges], ddof=1, exact=exact)
        np.testing.assert_array_equal(got[0], want[0])
        for g, v in zip(got[1:3], want[1:3]):
            np.testing.assert_allclose(g, v, rtol=1e-14, atol=0, equal_nan=True)
        for g, v in zip(got[3:], want[3:]):
            np.testing.assert_allclose(g, v, rtol=1e-12, atol=1e-300, equal_nan=True)


@pytest.mark.parametrize("seed", range(4))
def test_oracle_matches_np_cov_aweights(seed):
    """any weights, ddof = 0: np.cov(a_bin, b_bin, aweights=w_bin, ddof=0)"""
    edges, x, a, b, w = _random_case(10 + seed, False)
    want = _per_bin_cov(x, edges, a, b, w, aweights=True, ddof=0)
    for exact in (False, True):
        got = cwo.histogram_weighted_cov(x, values=(a, b), weights=w, bins=[edges], ddof=0, exact=exact)
        np.testing.assert_allclose(got[0], want[0], rtol=1e-14)
        for g, v in zip(got[1:3], want[1:3]):
            np.testing.assert_allclose(g, v, rtol=1e-14, atol=0, equal_nan=True)
        for g, v in zip(got[3:], want[3:]):
            np.testing.assert_allclose(g, v, rtol=1e-12, atol=1e-300, equal_nan=True)


def test_oracle_rules():
    """the NaN and zero rules of the GPU test's data, stated by the oracle in both modes as that test states them by hand"""
    edges, x, a, b, w = tg.special_data()
    for ddof in (0, 1):
        for exact in (False, True):
            got = cwo.histogram_weighted_cov(x, values=(a, b), weights=w, bins=edges, ddof=ddof, exact=exact)
            for g, e, name in zip(got, tg.special_expected(ddof), ("W", "mean_a", "mean_b", "var_a", "var_b", "cov_ab")):
                if not exact and name != "W":  # (the fsum mode gives no moments next to an infinity, and NaN for a NaN weight)
                    keep = [0, 2, 4, 5, 6]
                    np.testing.assert_array_equal(g[keep], np.asarray(e)[keep], err_msg=name)
                else:
                    np.testing.assert_array_equal(g, e, err_msg="%s exact=%s" % (name, exact))
    # w == 1: the unweighted oracle
    import cov_oracle as co
    rng = np.random.default_rng(5)
    x = rng.uniform(0, 7, 500)
    a, b = rng.standard_normal(500), rng.standard_normal(500)
    a[::11] = np.nan
    ref = co.histogram_cov(x, values=(a, b), bins=edges, ddof=1, exact=True)
    got = cwo.histogram_weighted_cov(x, values=(a, b), weights=np.ones(500), bins=edges, ddof=1, exact=True)
    np.testing.assert_array_equal(got[0], ref[0].astype(F64))
    for g, r in zip(got[1:], ref[1:]):
        np.testing.assert_array_equal(g, r)


# ---------------------------------------------------------------------------------------------------------------------
# cov_weighted_exact on the host
# ---------------------------------------------------------------------------------------------------------------------
def _kernel_moments(a, b, w, mean_a, mean_b, W, rng, acc=F64, pieces=1):
    """what a kernel does with one bin: the five sums of its terms in a random order (split into `pieces` partial sums, as lane
    copies and workgroups do, then those in another random order), accumulated in `acc`, and the finalize step: (M2_a, C_ab, M2_b)"""
    wda, wdb, pab = cwx.kernel_terms(a, b, w, mean_a, mean_b)
    paa = cwx.kernel_terms(a, a, w, mean_a, mean_a)[2]
    pbb = cwx.kernel_terms(b, b, w, mean_b, mean_b)[2]
    perm = rng.permutation(len(pab))
    terms = [t[perm].astype(acc) for t in (wda, wdb, paa, pab, pbb)]
    cuts = np.sort(rng.integers(0, len(pab) + 1, pieces - 1))
    parts = [[np.add.accumulate(q)[-1] if len(q) else acc(0) for q in np.split(t, cuts)] for t in terms]
    tot = [acc(0)] * 5
    for i in rng.permutation(pieces):
        tot = [acc(s + q[i]) for s, q in zip(tot, parts)]
    sda, sdb, saa, sab, sbb = (float(t) for t in tot)
    return max(0.0, saa - sda * sda / W), sab - sda * sdb / W, max(0.0, sbb - sdb * sdb / W)


def _bin(rng, n, target_w=None):
    """n triples on the grid with integer weights 0..7 (their sum forced to target_w, if given, by the last weights)"""
    a, b = vx.grid(rng, n), vx.grid(rng, n)
    w = rng.integers(0, 8, n).astype(F64)
    if target_w is not None:
        w[:] = 0
        left = target_w
        for i in rng.permutation(n):
            w[i] = min(7, left)
            left -= w[i]
        assert left == 0
        assert w.sum() == target_w
    return a, b, w


def test_power_of_two_sums_of_weights_are_bit_for_bit():
    """W = 2^j <= 2^8: all three moments identical in 20 random orders of summation, and equal to the oracle's exact mode"""
    rng = np.random.default_rng(2)
    for j in range(0, 9):
        W = 1 << j
        n = max(-(-W // 7), int(rng.integers(1, 2 * W + 2)))
        a, b, w = _bin(rng, n, W)
        Wx, (ma, mb), star, bounds, exact = cwx.expected(np.zeros(n, np.int64), a, b, w, 1)
        assert Wx[0] == W and exact[0] and all(bd[0] == 0.0 for bd in bounds)
        got = {_kernel_moments(a, b, w, ma[0], mb[0], W, rng, pieces=p) for p in (1, 4, 16, 64) for _ in range(5)}
        assert got == {(star[0][0], star[1][0], star[2][0])}, (W, got)
        o = cwo.cov_w_rows([np.full((1, n), 0.5)], [np.array([0.0, 1.0])], a[None], b[None], w[None], exact=True)
        assert (o[3][0, 0], o[5][0, 0], o[4][0, 0]) == (star[0][0], star[1][0], star[2][0])
    # 3 x 4099 samples in 60 bins wider than the sample range: identical on every power-of-two bin in 20 orders of summation
    n = 3 * 4099
    flat = rng.integers(0, 60, n)
    a, b, w = _bin(rng, n)
    Wx, (ma, mb), star, bounds, exact = cwx.expected(flat, a, b, w, 60)
    assert not exact.any()  # (about 700 a bin: far beyond 2^8)
    flat = rng.integers(0, 600, n)
    Wx, (ma, mb), star, bounds, exact = cwx.expected(flat, a, b, w, 600)
    assert exact.sum() >= 3
    for k in np.flatnonzero(exact):
        sel = flat == k
        got = {_kernel_moments(a[sel], b[sel], w[sel], ma[k], mb[k], Wx[k], rng, pieces=4) for _ in range(20)}
        assert got == {(star[0][k], star[1][k], star[2][k])}, (k, got)
    # 2^9 is beyond POW2_EXACT: such a bin takes the bound
    a, b, w = _bin(rng, 200, 512)
    assert not cwx.expected(np.zeros(200, np.int64), a, b, w, 1)[4][0]


@pytest.mark.parametrize("n", [3, 5, 7, 100, 999, 4097, 50_000])
def test_bound_holds_for_float64_sums_in_many_orders(n):
    rng = np.random.default_rng(n)
    for off_a, off_b, slope in ((0.0, 0.0, 0.0), (3.5, -3.0, 0.5), (-3.0, 3.5, -1.0)):  # means far from zero, either sign of C
        a = np.round((vx.grid(rng, n) * 0.01 + off_a) / vx.SCALE) * vx.SCALE
        b = np.round((slope * (a - off_a) + vx.grid(rng, n) * 0.01 + off_b) / vx.SCALE) * vx.SCALE
        w = rng.integers(0, 8, n).astype(F64)
        w[0] = 7.0
        if cwx.w_exact(w.sum()):
            w[0] = 6.0
        Wx, (ma, mb), star, bounds, exact = cwx.expected(np.zeros(n, np.int64), a, b, w, 1)
        assert not exact[0] and all(bd[0] > 0 for bd in bounds)
        for pieces in (1, 2, 16, 256):
            for _ in range(8):
                got = _kernel_moments(a, b, w, ma[0], mb[0], Wx[0], rng, pieces=pieces)
                for g, s, bd in zip(got, star, bounds):
                    assert abs(g - s[0]) <= bd[0], (n, slope, pieces, g, s[0], abs(g - s[0]), bd[0])
    assert n < 100 or star[1][0] < 0  # (the last case: a negative co-moment, not clamped; a few triples may land either side)


@pytest.mark.parametrize("n", [7, 100, 999, 50_000])
def test_bound_is_broken_by_float32_sums(n):
    """the terms summed in float32 (what an accumulator of 24 bits would give): beyond the bound, by orders of magnitude"""
    rng = np.random.default_rng(100 + n)
    a, b, w = _bin(rng, n)
    w[0] = 7.0
    if cwx.w_exact(w.sum()):
        w[0] = 6.0
    Wx, (ma, mb), star, bounds, exact = cwx.expected(np.zeros(n, np.int64), a, b, w, 1)
    assert not exact[0]
    errs = [abs(_kernel_moments(a, b, w, ma[0], mb[0], Wx[0], rng, acc=F32, pieces=4)[1] - star[1][0]) for _ in range(8)]
    assert max(errs) > 100 * bounds[1][0], (errs, bounds[1][0])
    # and the bound is a small multiple of u n P: what float64 sums may move, not a loose tolerance
    P = float(np.sum(np.abs(cwx.kernel_terms(a, b, w, ma[0], mb[0])[2])))
    assert bounds[1][0] <= 16 * n * vx.U * P, (bounds[1][0], P)


def test_expected_drops_incomplete_pairs_whatever_their_weight():
    rng = np.random.default_rng(3)
    size = 12
    flat = np.repeat(np.arange(size), rng.integers(0, 70, size))
    a, b, w = _bin(rng, flat.size)
    a[::17] = np.nan
    b[::13] = np.nan
    Wx, (ma, mb), star, bounds, exact = cwx.expected(flat, a, b, w, size)
    keep = ~np.isnan(a) & ~np.isnan(b)
    np.testing.assert_array_equal(Wx, np.bincount(flat[keep], weights=w[keep], minlength=size))
    for k in np.flatnonzero(Wx):
        sel = keep & (flat == k)
        assert ma[k] == np.sum(w[sel] * a[sel]) / Wx[k] and mb[k] == np.sum(w[sel] * b[sel]) / Wx[k]
    cwx.assert_moments(star, star, bounds, exact)
    bad = star[1].copy()
    j = int(np.flatnonzero(~exact & (Wx > 2))[0])
    bad[j] = star[1][j] - 4 * bounds[1][j]
    with pytest.raises(AssertionError, match="bound"):
        cwx.assert_moments((star[0], bad, star[2]), star, bounds, exact)
    with pytest.raises(AssertionError, match="integers"):
        cwx.expected(flat, a, b, w + 0.5, size)


# ---------------------------------------------------------------------------------------------------------------------
# combine_weighted_cov against the scalar restatement, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
COV_PAIRS = [(0, 0), (1, 1), (0, 1)]


@pytest.mark.parametrize("n_parts,empty", tcm.CASES)
def test_combine_weighted_cov_bit_for_bit(n_parts, empty):
    rng = np.random.default_rng(300 + 10 * n_parts + len(empty))
    w, (ma, mb), (qa, qb, cc) = tcm._partials(rng, n_parts, empty, 2, 3, weighted=True)
    got = core.combine_weighted_cov(w[:, None], ma[:, None], mb[:, None], qa[:, None], qb[:, None], cc[:, None], axis=0)
    assert all(g.shape == (1, 1, tcm.N_BINS) and g.dtype == F64 for g in got)
    want = tcm._merge(w, [ma, mb], [qa, qb, cc], COV_PAIRS, tcm._weighed)
    for g, v in zip(got, want):
        tcm._same_bits(g, v)
    if len(empty) < n_parts:
        assert (got[5][0, 0, :5] < 0).any() or (cc[~np.isnan(cc)] > 0).all()  # (negative co-moments stay negative)
    # through the dask step, whose blocks keep the library's order (W, mean_a, mean_b, M2_a, C_ab, M2_b), and its last step
    blocks = np.stack([w, ma, mb, qa, cc, qb])
    out = core._cov_w_reduce(blocks, axis=(1,), keepdims=False)
    for i, v in zip((0, 1, 2, 3, 5, 4), want):
        tcm._same_bits(out[i], v)
    last = core._cov_w_reduce(blocks, axis=(1,), keepdims=False, ddof=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i, v in zip((3, 5, 4), want[3:]):
            tcm._same_bits(last[i], np.where(want[0] > 1, v / (want[0] - 1), np.nan))


def test_combine_weighted_cov_nan_and_zero_partials():
    """a partial with W == 0 is skipped; a NaN partial (a NaN W) makes the bin NaN; every partial empty: W 0, the rest NaN"""
    nan = np.nan
    w = np.array([[2.0, 0.0, nan, 0.0], [2.0, 3.0, 1.0, 0.0]])
    m = np.array([[1.0, nan, nan, nan], [3.0, 5.0, 1.0, nan]])
    q = np.array([[0.5, nan, nan, nan], [0.5, 2.0, 1.0, nan]])
    got = core.combine_weighted_cov(w, m, m, q, q, -q, axis=0)
    np.testing.assert_array_equal(got[0][0], [4.0, 3.0, nan, 0.0])
    np.testing.assert_array_equal(got[1][0], [2.0, 5.0, nan, nan])
    np.testing.assert_array_equal(got[3][0], [0.5 + 0.5 + 4.0 * 2 * 2 / 4, 2.0, nan, nan])
    np.testing.assert_array_equal(got[5][0], [-0.5 - 0.5 + 4.0 * 2 * 2 / 4, -2.0, nan, nan])
    assert pickle.loads(pickle.dumps(core._cov_w_reduce)).keywords == core._cov_w_reduce.keywords
    assert core._cov_w_reduce.func is core._moment_reduce and core._cov_w_reduce.keywords["present"] is core._weighed


# ---------------------------------------------------------------------------------------------------------------------
# arguments and wiring
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_device_work():
    x = np.linspace(0, 1, 10)
    e = np.linspace(0, 1, 5)
    f = core.histogram_weighted_cov
    with pytest.raises(TypeError):
        f(x, weights=x, bins=e)  # values are required
    for bad in (None, x, (x,), (x, x, x), [x], "ab", (x, None)):
        with pytest.raises(TypeError, match="pair"):
            f(x, values=bad, weights=x, bins=e)
    with pytest.raises(TypeError):
        f(x, values=(x, x), bins=e)  # weights are required
    with pytest.raises(TypeError, match="needs weights"):
        f(x, values=(x, x), weights=None, bins=e)
    with pytest.raises(TypeError, match="complex"):
        f(x, values=(x, x), weights=x + 1j, bins=e)
    with pytest.raises(TypeError):
        f(x, values=(x, x), weights=x.astype("datetime64[s]"), bins=e)
    with pytest.raises(TypeError, match="complex"):
        f(x, values=(x, x + 1j), weights=x, bins=e)
    for bad in (-1, 1.0, 0.5, "1", None, True):
        with pytest.raises(ValueError, match="ddof"):
            f(x, values=(x, x), weights=x, bins=e, ddof=bad)
    with pytest.raises(TypeError, match="sample"):
        f(values=(x, x), weights=x, bins=e)  # no samples
    assert "histogram_weighted_cov" in core.__all__ and "combine_weighted_cov" in core.__all__
    st = core._VALUE_STATS["cov_w"]
    assert (st.k, st.ints, st.extras, st.method, st.ptrs) == (6, (), 2, "execute_cov_weighted", (0, 1, 3))
    st = core._VALUE_STATS["cov"]  # (as tests/test_cov_cpu.py asserts it)
    assert (st.k, st.ints, st.extras, st.method, st.ptrs) == (6, (0,), 1, "execute_cov", (0, 1, 3))
    assert "histogram_weighted_cov" in core.histogram_cov.__doc__ and "is not provided" not in core.histogram_cov.__doc__


def test_symbol_and_abi_version():
    assert _native.ABI_VERSION == 11
    assert "xhist_plan_execute_cov_weighted" in _native.EXPORTS
    header = open(os.path.join(ROOT, "include", "xhist_amd.h")).read()
    assert "#define XHIST_ABI_VERSION 11" in header and "xhist_plan_execute_cov_weighted(" in header
    lib = _native.load()
    assert lib.xhist_abi_version() == 11
    assert len(lib.xhist_plan_execute_cov_weighted.argtypes) == 12
    assert callable(getattr(_native.Plan, "execute_cov_weighted"))
    assert "xhist_cov_w" in open(os.path.join(ROOT, "xhistogram_amd", "csrc", "build.sh")).read()


xhx = importlib.import_module("xhistogram_amd.xarray")


def _oracle_cw(*args, values, weights, bins=None, range=None, axis=None, ddof=0, block_size="auto"):
    bins = [bins] * len(args) if isinstance(bins, np.ndarray) else list(bins)
    return cwo.histogram_weighted_cov(*args, values=values, weights=weights, bins=bins, axis=axis, ddof=ddof) + (bins,)


def test_xarray_wrapper_names(monkeypatch):
    monkeypatch.setattr(core, "histogram_weighted_cov", _oracle_cw)
    rng = np.random.default_rng(7)
    dims, shape = ("t", "y", "x"), (2, 3, 40)
    coords = {d: np.arange(n) * 1.0 for d, n in zip(dims, shape)}
    T = xr.DataArray(rng.uniform(0, 1, shape), dims=dims, coords=coords, name="T", attrs={"units": "K"})
    S = xr.DataArray(rng.uniform(0, 1, shape), dims=dims, coords=coords, name="S")
    A = xr.DataArray(rng.standard_normal(shape), dims=dims, coords=coords, name="o2")
    B = xr.DataArray(rng.standard_normal(shape), dims=dims, coords=coords, name="temp")
    Wt = xr.DataArray(rng.uniform(0.5, 2, shape[1:]), dims=dims[1:], name="dVol")  # broadcast over t
    bins = [np.linspace(0, 1, 5), np.linspace(0, 1, 4)]
    out = xhx.histogram_weighted_cov(T, S, values=(A, B), weights=Wt, bins=bins, dim=("y", "x"), ddof=1)
    assert list(out) == ["o2_temp_sum_of_weights", "o2_mean", "temp_mean", "o2_var", "temp_var", "o2_temp_cov"]
    assert all(v.name == k and tuple(v.dims) == ("t", "T_bin", "S_bin") for k, v in out.items())
    np.testing.assert_array_equal(out["o2_temp_cov"]["T_bin"].values, 0.5 * (bins[0][:-1] + bins[0][1:]))
    assert out["o2_mean"]["T_bin"].attrs == {"units": "K"}
    want = cwo.histogram_weighted_cov(T.values, S.values, values=(A.values, B.values), weights=Wt.values[None], bins=bins, axis=(1, 2), ddof=1)
    for got, w in zip(out.values(), want):
        np.testing.assert_array_equal(np.asarray(got.values), w)
    # nameless values, everything reduced
    out = xhx.histogram_weighted_cov(T, values=(xr.DataArray(A.values, dims=dims), xr.DataArray(B.values, dims=dims)), weights=Wt,
                                     bins=[bins[0]])
    assert list(out) == ["a_b_sum_of_weights", "a_mean", "b_mean", "a_var", "b_var", "a_b_cov"]
    assert tuple(out["a_b_cov"].dims) == ("T_bin",)
    with pytest.raises(TypeError):
        xhx.histogram_weighted_cov(T, values=A, weights=Wt, bins=[bins[0]])
    with pytest.raises(TypeError):
        xhx.histogram_weighted_cov(T, values=(A, B), weights=Wt.values, bins=[bins[0]])
    with pytest.raises(TypeError):
        xhx.histogram_weighted_cov(T, values=(A, B), weights=None, bins=[bins[0]])
    assert "histogram_weighted_cov" in xhx.__all__


# ---------------------------------------------------------------------------------------------------------------------
# the data conditions of tests/test_gpu_cov_weighted.py, shape by shape: what the oracle alone says of each case
# ---------------------------------------------------------------------------------------------------------------------
def _split(edges, xs, a, b, w, ddof=0):
    """(bins checked bit for bit, bins checked against the bound) of one case's data"""
    xc, ec = tg.cs._cmp(xs, edges)
    W, _, _, _, exact = tg.expected_of(xc, ec, a, b, w)
    return tg.split(W, exact, ddof)


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("sdt", ["f64", "f32"])
@pytest.mark.parametrize("form", tg.FORMS)
def test_fast_form_cases(form, sdt, D):
    """3 rows of 20 011 columns: the predicted form, and bins of both kinds"""
    edges, xs, a, b, w, fine, arith = tg.form_data(form, sdt, D)
    assert xs[0].shape == tg.FORM_SHAPE == (3, 20_011) and len(edges) == D
    want = predict_cov(CUS, edges, 0, xs[0].dtype, a.dtype, *tg.FORM_SHAPE, fine, arith)
    assert want["family"] == "fast" and (want["scan"] == 5) == (form == "arith"), want
    bits, bound = _split(edges, xs, a, b, w, ddof=D - 1)
    assert bits >= 1 and bound >= 1, (bits, bound)


@pytest.mark.parametrize("home", tg.HOMES)
@pytest.mark.parametrize("dom", tg.DOMS)
def test_generic_cases(dom, home):
    edges, xs, a, b, w, cmp = tg.generic_data(dom, home)
    assert xs[0].shape == (2, tg.GENERIC_COLS[home]) and xs[0].shape[1] > 512  # (more than one block of the generic family)
    want = predict_cov(CUS, edges, cmp, xs[0].dtype, a.dtype, *xs[0].shape, False)
    assert want["family"] == "generic" and want["slots"] == ("lds" if home == "lds" else "global") and want["cmp"] == cmp
    bits, bound = _split(edges, xs, a, b, w, ddof=1)
    assert bits >= 1 and bound >= 1, (bits, bound)


def test_tile_cases():
    """the tile of every form and the parts it is read in (values_fast_body: 256 x VEC x UNROLL elements, fast_halves of four or
    five streams within 192 bytes per lane), the row lengths around the tile's end and around every internal split point, and,
    for every shape, that every element counts and a bin is on the bit-for-bit path"""
    for form, (st, D, T, parts) in tg.TILE_FORMS.items():
        vec = 16 // np.dtype(st).itemsize
        unroll = 4 if D == 1 else 8 // vec
        assert T == 256 * vec * unroll
        tile_bytes = (D + 3) * 16 * unroll  # D inputs, a, b and the weights
        h = 1
        while tile_bytes // h > 192 and h < unroll:
            h *= 2
        assert parts == h, (form, parts, h)
        cols = tg.tile_cols(form)
        assert {T - 1, T + 1, 2 * T - 1} <= set(cols)
        for k in range(1, parts):
            assert {k * T // parts - 1, k * T // parts + 1} <= set(cols)
        assert len(cols) == 3 + 2 * (parts - 1)
        for n_rows in (1, 3):
            for n_cols in cols:
                edges, xs, a, b, w = tg.tile_data(form, n_rows, n_cols)
                assert all(x.dtype == st and x.shape == (n_rows, n_cols) for x in xs) and a.dtype == b.dtype == w.dtype == st
                xc, ec = tg.cs._cmp(xs, edges)
                ok, _, _ = tg.tgc._flat(xc, ec)
                assert ok.all() and not np.isnan(a).any() and not np.isnan(b).any()
                assert predict_cov(CUS, edges, 0, st, st, n_rows, n_cols)["family"] == "fast"
                bits, _ = _split(edges, xs, a, b, w)
                assert bits >= 1, (form, n_rows, n_cols)
    assert {f: p for f, (_, _, _, p) in tg.TILE_FORMS.items()} == {"f64_D1": 2, "f32_D1": 2, "f64_D2": 2, "f32_D2": 1}


@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_alignment_cases(sdt):
    for shape in tg.ALIGN_SHAPES:
        edges, xs, a, b, w = tg.align_data(sdt, shape)
        assert shape[1] % 2 == 1  # (odd rows: every other row starts off 16 bytes)
        assert predict_cov(CUS, edges, 0, xs[0].dtype, a.dtype, *shape)["family"] == "fast"
        assert _split(edges, xs, a, b, w)[0] >= 1, shape


@pytest.mark.parametrize("how", ["stride2", "dtype", "row0"])
@pytest.mark.parametrize("which", ["b", "w"])
@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_layout_cases(sdt, which, how):
    edges, xs, a, b, w = tg.layout_data(sdt, which, how)
    st = xs[0].dtype
    assert (b.dtype != st, w.dtype != st) == (how == "dtype" and which == "b", how == "dtype" and which == "w")
    assert (b.shape[0] == 1, w.shape[0] == 1) == (how == "row0" and which == "b", how == "row0" and which == "w")
    # either extra stream alone decides: the rule of choose_values, per stream
    n_cols = tg.LAYOUT_SHAPE[1]
    fast = tg.streams_fast(st, n_cols, (b.dtype, 2 if (how, which) == ("stride2", "b") else 1, 0),
                           (w.dtype, 2 if (how, which) == ("stride2", "w") else 1, 0))
    assert fast == (how == "row0")
    assert predict_cov(CUS, edges, 0, st, a.dtype, *tg.LAYOUT_SHAPE, True, False, fast)["family"] == ("fast" if fast else "generic")
    assert _split(edges, xs, a, b, w)[0] >= 1


@pytest.mark.parametrize("sdt", ["f64", "f32"])
@pytest.mark.parametrize("nbs,copies", tg.COPIES, ids=[str(n[0]) for n, _ in tg.COPIES])
def test_copies_cases(nbs, copies, sdt):
    edges, xs, a, b, w = tg.copies_data(nbs, sdt)
    want = predict_cov(CUS, edges, 0, xs[0].dtype, a.dtype, *xs[0].shape, True, True)
    assert want["family"] == "fast" and want["copies"] == copies
    bits, bound = _split(edges, xs, a, b, w)
    assert bits >= 1 and bound >= 1, (bits, bound)
    assert {c for _, c in tg.COPIES} == {1, 2, 4, 8, 16}


def test_border_cases():
    """160 KiB / 56 B: the last bin count whose slots fit without tables, arithmetic edges"""
    assert tg.BORDER == 2925
    for side, (family, slots) in enumerate((("fast", "lds"), ("generic", "global"))):
        edges, xs, a, b, w = tg.border_data(tg.BORDER + side)
        want = predict_cov(CUS, edges, 0, F64, F64, *tg.BORDER_SHAPE, True, True)
        assert (want["family"], want["slots"]) == (family, slots), want
        assert _split(edges, xs, a, b, w)[0] >= 1


def test_row_chunk_case():
    assert all(np.gcd(tg.P_W, p) == 1 for p in (tg.cs.P_S, tg.cs.P_A, tg.cs.P_B))
    for wt, family, block, chunks in ((F64, "fast", 256, 3), (F32, "generic", 512, 5)):
        want = predict_cov(CUS, [tg.cs.CHUNK_EDGES], 0, F64, F64, tg.cs.N_ROWS, 1, True, True, tg.streams_fast(F64, 1, (F64, 1, 0), (wt, 1, 0)))
        assert (want["family"], want["block"], want["segs"]) == (family, block, 1)
        assert tg.cs.chunk_count(block) == chunks
    assert len(tg.cs.CHUNK_EDGES) - 1 == 2  # (the plane distance, rows * 2, is not the row count)


def test_identity_backend_and_xarray_cases():
    edges, xs, a, b, w = tg.ident_data()
    assert _split(edges, xs, a, b, w)[0] >= 1 and _split(edges, xs, a, a, w)[0] >= 1
    assert _split(edges, xs, a, b, np.ones(tg.IDENT_SHAPE), ddof=1)[0] >= 1
    assert _split(edges, [xs[0][:1]], a[:1], b[:1], w[:1])[0] >= 1  # (the row of the repeated-samples case)
    edges, x, a, b, w = tg.backend_data()
    assert _split(edges, [x], a, b, w)[0] >= 1
    edges, T, o2, temp, area = tg.xarray_data()
    assert _split([edges], [T.reshape(4, 48)], o2.reshape(4, 48), temp.reshape(4, 48), np.broadcast_to(area, T.shape).reshape(4, 48))[0] >= 1
    # the special values: bins 0 and 2 have W = 4
    W = tg.special_expected(0)[0]
    assert W[0] == 4.0 and W[2] == 4.0
