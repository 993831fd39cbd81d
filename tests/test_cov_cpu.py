"""histogram_cov without a GPU: the oracle (tests/cov_oracle.py) against np.cov / np.nanmean per bin, the exactness analysis of
tests/cov_exact.py on the host, the host merge of dask partials (core.combine_cov) against the oracle, argument errors raised
before any device work, the new C symbol, and the xarray wrapper's names (compute swapped for the oracle)."""
import importlib
import os
import sys

import numpy as np
import pytest

import cov_exact as cx
import cov_oracle as co
import values_exact as vx
from xhistogram_amd import _native, core

try:
    import xarray as xr  # noqa: F401
except ImportError:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "doubles"))
    import xarray as xr  # the double

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------
# the oracle against numpy
# ---------------------------------------------------------------------------------------------------------------------
def _per_bin_loop(samples, edges, a, b, ddof):
    """np.nanmean / np.cov over the pairwise-complete pairs of each bin of one row, bins found by a loop"""
    nbs = [len(e) - 1 for e in edges]
    groups = {}
    for i in range(len(a)):
        idx = []
        for s, e in zip(samples, edges):
            x = s[i]
            if not (x >= e[0] and x <= e[-1]):
                idx = None
                break
            idx.append(next(k for k in range(len(e) - 1) if e[k] <= x and (x < e[k + 1] or k == len(e) - 2)))
        if idx is not None:
            groups.setdefault(tuple(idx), []).append((a[i], b[i]))
    cnt = np.zeros(nbs, np.int64)
    out = [np.full(nbs, np.nan) for _ in range(5)]  # mean_a, mean_b, var_a, var_b, cov_ab
    for k, pairs in groups.items():
        pairs = np.asarray(pairs)
        good = pairs[~np.isnan(pairs).any(axis=1)]
        cnt[k] = len(good)
        if len(good):
            out[0][k], out[1][k] = np.nanmean(good[:, 0]), np.nanmean(good[:, 1])
        if len(good) > ddof:
            c = np.cov(good[:, 0], good[:, 1], ddof=ddof)
            out[2][k], out[3][k], out[4][k] = c[0, 0], c[1, 1], c[0, 1]
    return (cnt,) + tuple(out)


@pytest.mark.parametrize("ddof", [0, 1])
@pytest.mark.parametrize("seed", range(4))
def test_oracle_matches_np_cov(seed, ddof):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 400))
    D = 1 + seed % 2
    edges = [np.sort(rng.uniform(-2, 2, int(rng.integers(2, 9)))) for _ in range(D)]
    samples = []
    for e in edges:
        x = rng.uniform(-2.5, 2.5, n)
        on_edge = rng.random(n) < 0.2
        x[on_edge] = e[rng.integers(0, len(e), int(on_edge.sum()))]
        x[rng.random(n) < 0.05] = np.nan
        samples.append(x)
    a = rng.standard_normal(n) * 3 + 10
    b = (-0.5 if seed % 2 else 0.7) * a + rng.standard_normal(n) - 4
    only_a, only_b, both = (rng.random(n) < 0.08 for _ in range(3))  # NaN in a, in b, in both
    a[only_a | both] = np.nan
    b[only_b | both] = np.nan
    want = _per_bin_loop(samples, edges, a, b, ddof)
    for exact in (False, True):
        cnt, ma, mb, qa, qb, cc = co.cov_rows([s[None, :] for s in samples], edges, a[None, :], b[None, :], exact=exact)
        np.testing.assert_array_equal(cnt[0], want[0])
        np.testing.assert_allclose(ma[0], want[1], rtol=1e-13, atol=0, equal_nan=True)
        np.testing.assert_allclose(mb[0], want[2], rtol=1e-13, atol=0, equal_nan=True)
        for got, w in ((qa, want[3]), (qb, want[4]), (cc, want[5])):
            np.testing.assert_allclose(co.var_of(cnt, got, ddof)[0], w, rtol=1e-11, atol=1e-300, equal_nan=True)
    # the N-D front of the oracle gives the same
    got = co.histogram_cov(*samples, values=(a, b), bins=edges, ddof=ddof)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_allclose(got[5], want[5], rtol=1e-11, atol=1e-300, equal_nan=True)
    # the count and the samples a NaN value dropped make up the histogram's count
    ok, flat, nbs = co._flat_bins([s[None, :] for s in samples], edges)
    dropped = np.bincount(flat[ok & (np.isnan(a) | np.isnan(b))[None, :]], minlength=int(np.prod(nbs)))
    hist = np.bincount(flat[ok], minlength=int(np.prod(nbs)))
    np.testing.assert_array_equal(want[0].reshape(-1) + dropped, hist)


def test_oracle_cancellation_shows_the_naive_formula_fails():
    """a at 1e8, b at -1e8, spreads of 1: the oracle keeps the covariance; sum(a b)/n - mean_a mean_b is off by O(1)"""
    rng = np.random.default_rng(2)
    t = rng.standard_normal(100_000)
    a = 1e8 + t
    b = -1e8 - 0.5 * t + 0.1 * rng.standard_normal(t.size)
    x = np.full(a.shape, 0.5)
    cnt, ma, mb, qa, qb, cc = co.cov_rows([x[None]], [np.array([0.0, 1.0])], a[None], b[None])
    cov = cc[0, 0] / cnt[0, 0]
    np.testing.assert_allclose(cov, np.cov(a - 1e8, b + 1e8, ddof=0)[0, 1], rtol=1e-9)
    assert cov < 0
    naive = np.mean(a * b) - np.mean(a) * np.mean(b)
    assert abs(naive - cov) > 0.01


# ---------------------------------------------------------------------------------------------------------------------
# cov_exact on the host
# ---------------------------------------------------------------------------------------------------------------------
def _kernel_c(avals, bvals, mean_a, mean_b, rng, acc=np.float64, pieces=1):
    """what a kernel does with one bin's co-moment: da, db and p in float64, their sums in a random order (split into `pieces`
    partial sums, as lane copies and workgroups do, then those in another random order), accumulated in `acc`"""
    da, db, p = cx.kernel_terms(avals, bvals, mean_a, mean_b)
    perm = rng.permutation(len(p))
    terms = [t[perm].astype(acc) for t in (da, db, p)]
    cuts = np.sort(rng.integers(0, len(p) + 1, pieces - 1))
    parts = [[np.add.accumulate(q)[-1] if len(q) else acc(0) for q in np.split(t, cuts)] for t in terms]
    order = rng.permutation(pieces)
    tot = [acc(0)] * 3
    for i in order:
        tot = [acc(s + q[i]) for s, q in zip(tot, parts)]
    sa, sb, c = (float(t) for t in tot)
    return c - sa * sb / len(avals)


def _pairs(rng, n, dtype=np.float64):
    a = vx.grid(rng, n, dtype)
    b = vx.grid(rng, n, dtype)
    return a, b


def test_power_of_two_counts_give_the_comoment_bit_for_bit():
    rng = np.random.default_rng(2)
    for dtype in (np.float64, np.float32, np.int32):
        for j in range(0, 10):
            n = 1 << j
            a, b = _pairs(rng, n, dtype)
            cnt, (ma, mb), (m2a, c, m2b), (ba, bc, bb), exact = cx.expected(np.zeros(n, np.int64), a, b, 1)
            assert exact[0] and bc[0] == 0.0 and ba[0] == 0.0 and bb[0] == 0.0
            got = {_kernel_c(a, b, ma[0], mb[0], rng, pieces=p) for p in (1, 4, 16) for _ in range(5)}
            assert got == {c[0]}, (n, got, c[0])
            # the exact mode of the oracle is the same statement
            o = co.cov_rows([np.full((1, n), 0.5)], [np.array([0.0, 1.0])], a[None], b[None], exact=True)
            assert (o[3][0, 0], o[4][0, 0], o[5][0, 0]) == (m2a[0], m2b[0], c[0])
    # from 2^10 pairs on the products' sums round: such a bin takes the bound, and the bound holds
    a, b = _pairs(rng, 1 << 12)
    cnt, (ma, mb), (_, c, _), (_, bc, _), exact = cx.expected(np.zeros(a.size, np.int64), a, b, 1)
    assert not exact[0] and bc[0] > 0
    assert all(abs(_kernel_c(a, b, ma[0], mb[0], rng, pieces=16) - c[0]) <= bc[0] for _ in range(8))


@pytest.mark.parametrize("n", [3, 5, 7, 100, 999, 4097, 50_000])
def test_bound_holds_in_many_orders(n):
    rng = np.random.default_rng(n)
    for off_a, off_b, slope in ((0.0, 0.0, 0.0), (3.5, -3.0, 0.5), (-3.0, 3.5, -1.0)):  # means far from zero, either sign of C
        a = np.round((vx.grid(rng, n) * 0.01 + off_a) / vx.SCALE) * vx.SCALE
        b = np.round((slope * (a - off_a) + vx.grid(rng, n) * 0.01 + off_b) / vx.SCALE) * vx.SCALE
        cnt, (ma, mb), (_, c, _), (_, bc, _), exact = cx.expected(np.zeros(n, np.int64), a, b, 1)
        assert not exact[0] and bc[0] > 0
        for pieces in (1, 2, 16, 256):
            for _ in range(8):
                got = _kernel_c(a, b, ma[0], mb[0], rng, pieces=pieces)
                assert abs(got - c[0]) <= bc[0], (n, slope, pieces, got, c[0], abs(got - c[0]), bc[0])
    assert c[0] < 0  # (the last case: a negative co-moment, not clamped)


@pytest.mark.parametrize("n", [7, 100, 999, 50_000])
def test_bound_is_broken_by_float32_products(n):
    """p summed in float32 (what an accumulator of 24 bits would give): beyond the bound for every such bin"""
    rng = np.random.default_rng(100 + n)
    a, b = _pairs(rng, n)
    cnt, (ma, mb), (_, c, _), (_, bc, _), exact = cx.expected(np.zeros(n, np.int64), a, b, 1)
    assert not exact[0]
    errs = [abs(_kernel_c(a, b, ma[0], mb[0], rng, acc=np.float32, pieces=4) - c[0]) for _ in range(8)]
    assert max(errs) > 100 * bc[0], (errs, bc[0])
    # and the bound is a small multiple of u n P: what float64 sums may move, not a loose tolerance
    P = float(np.sum(np.abs(cx.kernel_terms(a, b, ma[0], mb[0])[2])))
    assert bc[0] <= 16 * n * vx.U * P, (bc[0], P)


def test_expected_drops_incomplete_pairs():
    rng = np.random.default_rng(3)
    size = 12
    flat = np.repeat(np.arange(size), rng.integers(0, 70, size))
    a, b = _pairs(rng, flat.size)
    a[::17] = np.nan
    b[::13] = np.nan
    cnt, (ma, mb), (m2a, c, m2b), bounds, exact = cx.expected(flat, a, b, size)
    keep = ~np.isnan(a) & ~np.isnan(b)
    np.testing.assert_array_equal(cnt, np.bincount(flat[keep], minlength=size))
    for k in np.flatnonzero(cnt):
        sel = keep & (flat == k)
        assert ma[k] == np.sum(a[sel]) / sel.sum() and mb[k] == np.sum(b[sel]) / sel.sum()
    cx.assert_moments((m2a, c, m2b), (m2a, c, m2b), bounds, exact)
    bad = c.copy()
    j = int(np.flatnonzero(~exact & (cnt > 2))[0])
    bad[j] = c[j] - 4 * bounds[1][j]
    with pytest.raises(AssertionError, match="bound"):
        cx.assert_moments((m2a, bad, m2b), (m2a, c, m2b), bounds, exact)


# ---------------------------------------------------------------------------------------------------------------------
# combine_cov
# ---------------------------------------------------------------------------------------------------------------------
def _partials(rng, n_parts, empty):
    nb = 5
    edges = [np.linspace(-1, 1, nb + 1)]
    parts, allx, alla, allb = [], [], [], []
    for i in range(n_parts):
        k = 0 if i in empty else int(rng.integers(1, 300))
        x = rng.uniform(-1.2, 1.2, k)
        a = rng.standard_normal(k) * 2 + 50
        b = -0.6 * a + rng.standard_normal(k) + 7
        a[rng.random(k) < 0.1] = np.nan
        b[rng.random(k) < 0.1] = np.nan
        allx.append(x)
        alla.append(a)
        allb.append(b)
        parts.append(co.cov_rows([x[None]], edges, a[None], b[None]))
    want = co.cov_rows([np.concatenate(allx)[None]], edges, np.concatenate(alla)[None], np.concatenate(allb)[None])
    return parts, want


def _check_combined(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    for i in (1, 2):
        np.testing.assert_allclose(got[i], want[i], rtol=1e-13, equal_nan=True)
    for i in (3, 4, 5):
        np.testing.assert_allclose(got[i], want[i], rtol=1e-10, atol=1e-12, equal_nan=True)


@pytest.mark.parametrize("seed", range(5))
def test_combine_cov_against_the_oracle(seed):
    rng = np.random.default_rng(10 + seed)
    n_parts = int(rng.integers(1, 7))
    empty = set(rng.choice(n_parts, int(rng.integers(0, n_parts)), replace=False).tolist()) if n_parts > 1 else set()
    parts, want = _partials(rng, n_parts, empty)
    stacked = [np.stack([p[i] for p in parts]) for i in range(6)]  # (part, row of extent 1, bins)
    got = core.combine_cov(*stacked, axis=0)
    assert all(g.shape == (1, 1, 5) and g.dtype == np.float64 for g in got)
    _check_combined([g[0] for g in got], want)
    if n_parts % 2 == 0:  # the same partials on two reduced axes (C order)
        two = [a.reshape((2, n_parts // 2) + a.shape[1:]) for a in stacked]
        got2 = core.combine_cov(*two, axis=(0, 1))
        np.testing.assert_array_equal(got2[0].reshape(got[0].shape), got[0])
        np.testing.assert_allclose(got2[5].reshape(got[5].shape), got[5], rtol=1e-13, atol=1e-12, equal_nan=True)
    # through the dask reduction step, whose blocks keep the library's order (n, mean_a, mean_b, M2_a, C_ab, M2_b)
    n, ma, mb, qa, qb, cc = stacked
    out = core._cov_reduce(np.stack([n, ma, mb, qa, cc, qb]).astype(np.float64), axis=(1,), keepdims=False, ddof=1)
    np.testing.assert_array_equal(out[0], want[0])
    for i, w in ((3, want[3]), (4, want[5]), (5, want[4])):
        np.testing.assert_allclose(out[i], co.var_of(want[0], w, 1), rtol=1e-10, atol=1e-12, equal_nan=True)


def test_combine_cov_all_empty():
    z = np.zeros((3, 2))
    nan = np.full((3, 2), np.nan)
    got = core.combine_cov(z, nan, nan, nan, nan, nan, axis=0)
    assert (got[0] == 0).all() and all(np.isnan(g).all() for g in got[1:])


def test_combine_cov_one_side_of_a_bin_empty():
    """bin 0 only in the first partial, bin 1 only in the second, bin 2 in both, bin 3 in neither"""
    edges = [np.arange(5.0)]
    x1, a1, b1 = np.array([0.5, 0.5, 2.5, 2.5]), np.array([1.0, 3.0, 2.0, 4.0]), np.array([4.0, 0.0, 1.0, 2.0])
    x2, a2, b2 = np.array([1.5, 1.5, 1.5, 2.5]), np.array([1.0, 2.0, 6.0, 9.0]), np.array([2.0, 2.0, 5.0, -3.0])
    p1 = co.cov_rows([x1[None]], edges, a1[None], b1[None])
    p2 = co.cov_rows([x2[None]], edges, a2[None], b2[None])
    want = co.cov_rows([np.r_[x1, x2][None]], edges, np.r_[a1, a2][None], np.r_[b1, b2][None])
    got = core.combine_cov(*[np.stack([u, v]) for u, v in zip(p1, p2)], axis=0)
    np.testing.assert_array_equal(got[0][0, 0], [2, 3, 3, 0])
    for g, u, v in zip(got[1:], p1[1:], p2[1:]):  # a bin one side left empty is the other side's, bit for bit
        assert g[0, 0, 0] == u[0, 0] and g[0, 0, 1] == v[0, 1] and np.isnan(g[0, 0, 3])
    _check_combined([g[0] for g in got], want)
    assert got[5][0, 0, 0] < 0 and got[5][0, 0, 2] < 0  # negative co-moments stay negative


# ---------------------------------------------------------------------------------------------------------------------
# arguments and wiring
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_device_work():
    x = np.linspace(0, 1, 10)
    e = np.linspace(0, 1, 5)
    with pytest.raises(TypeError):
        core.histogram_cov(x, bins=e)  # values are required
    for bad in (None, x, (x,), (x, x, x), [x], "ab", (x, None)):
        with pytest.raises(TypeError, match="pair"):
            core.histogram_cov(x, values=bad, bins=e)
    with pytest.raises(TypeError, match="complex"):
        core.histogram_cov(x, values=(x, x + 1j), bins=e)
    with pytest.raises(TypeError, match="complex"):
        core.histogram_cov(x, values=(x + 1j, x), bins=e)
    with pytest.raises(TypeError):
        core.histogram_cov(x, values=(x, x.astype("datetime64[s]")), bins=e)
    for bad in (-1, 1.0, 0.5, "1", None, True):
        with pytest.raises(ValueError, match="ddof"):
            core.histogram_cov(x, values=(x, x), bins=e, ddof=bad)
    with pytest.raises(TypeError, match="sample"):
        core.histogram_cov(values=(x, x), bins=e)  # no samples
    with pytest.raises(TypeError):
        core.histogram_cov(x, values=(x, x), bins=e, weights=x)  # no weighted form
    assert "histogram_cov" in core.__all__
    st = core._VALUE_STATS["cov"]
    assert (st.k, st.ints, st.extras, st.method, st.ptrs) == (6, (0,), 1, "execute_cov", (0, 1, 3))


def test_symbol_and_abi_version():
    assert _native.ABI_VERSION == 11
    assert "xhist_plan_execute_cov" in _native.EXPORTS
    header = open(os.path.join(ROOT, "include", "xhist_amd.h")).read()
    assert "#define XHIST_ABI_VERSION 11" in header and "xhist_plan_execute_cov(" in header
    lib = _native.load()
    assert lib.xhist_abi_version() == 11
    assert len(lib.xhist_plan_execute_cov.argtypes) == 11
    assert callable(getattr(_native.Plan, "execute_cov"))
    assert "xhist_cov" in open(os.path.join(ROOT, "xhistogram_amd", "csrc", "build.sh")).read()


xhx = importlib.import_module("xhistogram_amd.xarray")


def _oracle_cov(*args, values, bins=None, range=None, axis=None, ddof=0, block_size="auto"):
    bins = [bins] * len(args) if isinstance(bins, np.ndarray) else list(bins)
    return co.histogram_cov(*args, values=values, bins=bins, axis=axis, ddof=ddof) + (bins,)


def test_xarray_wrapper_names(monkeypatch):
    monkeypatch.setattr(core, "histogram_cov", _oracle_cov)
    rng = np.random.default_rng(7)
    dims, shape = ("t", "y", "x"), (2, 3, 40)
    coords = {d: np.arange(n) * 1.0 for d, n in zip(dims, shape)}
    T = xr.DataArray(rng.uniform(0, 1, shape), dims=dims, coords=coords, name="T", attrs={"units": "K"})
    S = xr.DataArray(rng.uniform(0, 1, shape), dims=dims, coords=coords, name="S")
    A = xr.DataArray(rng.standard_normal(shape), dims=dims, coords=coords, name="o2")
    B = xr.DataArray(rng.standard_normal(shape[1:]), dims=dims[1:], name="w")  # broadcast over t
    bins = [np.linspace(0, 1, 5), np.linspace(0, 1, 4)]
    out = xhx.histogram_cov(T, S, values=(A, B), bins=bins, dim=("y", "x"), ddof=1)
    assert list(out) == ["o2_w_count", "o2_mean", "w_mean", "o2_var", "w_var", "o2_w_cov"]
    assert all(v.name == k and tuple(v.dims) == ("t", "T_bin", "S_bin") for k, v in out.items())
    np.testing.assert_array_equal(out["o2_w_cov"]["T_bin"].values, 0.5 * (bins[0][:-1] + bins[0][1:]))
    assert out["o2_mean"]["T_bin"].attrs == {"units": "K"}
    np.testing.assert_array_equal(out["w_var"]["t"].values, coords["t"])
    want = co.histogram_cov(T.values, S.values, values=(A.values, B.values[None]), bins=bins, axis=(1, 2), ddof=1)
    for got, w in zip(out.values(), want):
        np.testing.assert_array_equal(np.asarray(got.values), w)
    # nameless values, everything reduced
    out = xhx.histogram_cov(T, values=(xr.DataArray(A.values, dims=dims), xr.DataArray(B.values, dims=dims[1:])), bins=[bins[0]])
    assert list(out) == ["a_b_count", "a_mean", "b_mean", "a_var", "b_var", "a_b_cov"]
    assert tuple(out["a_b_cov"].dims) == ("T_bin",)
    with pytest.raises(TypeError):
        xhx.histogram_cov(T, values=A, bins=[bins[0]])
    with pytest.raises(TypeError):
        xhx.histogram_cov(T, values=(A, B.values), bins=[bins[0]])
    assert "histogram_cov" in xhx.__all__
