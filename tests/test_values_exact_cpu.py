"""tests/values_exact.py on the host: the grid's sums are exact in any order, the M2 bound holds for float64 sums in many orders,
and it is tight enough that a float32 accumulator of d^2 breaks it."""
import numpy as np
import pytest

import values_exact as vx


def _kernel_m2(vals, mean, rng, acc=np.float64, pieces=1):
    """what a kernel does with one bin: d and q in float64, their sums in a random order (split into `pieces` partial sums, as
    lane copies and workgroups do, then those in another random order), accumulated in `acc`"""
    d, q = vx.kernel_terms(vals, mean)
    perm = rng.permutation(len(d))
    d, q = d[perm].astype(acc), q[perm].astype(acc)
    cuts = np.sort(rng.integers(0, len(d) + 1, pieces - 1))
    sd = [np.add.accumulate(p)[-1] if len(p) else acc(0) for p in np.split(d, cuts)]
    sq = [np.add.accumulate(p)[-1] if len(p) else acc(0) for p in np.split(q, cuts)]
    order = rng.permutation(len(sd))
    a, b = acc(0), acc(0)
    for i in order:
        a = acc(a + sd[i])
        b = acc(b + sq[i])
    a, b = float(a), float(b)
    r = b - a * a / len(vals)
    return 0.0 if r <= 0 else r


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.int32])
def test_grid_sums_and_means_are_exact_in_any_order(dtype):
    rng = np.random.default_rng(1)
    for n in (1, 3, 7, 100, 1000, 12_345):
        v = vx.grid(rng, n, dtype)
        assert vx.on_grid(v)
        v64 = v.astype(np.float64)
        sums = {np.add.accumulate(v64[rng.permutation(n)])[-1].tobytes() for _ in range(20)}
        sums.add(np.float64(np.sum(v64)).tobytes())  # (numpy's pairwise order)
        assert len(sums) == 1
        s = np.frombuffer(sums.pop(), np.float64)[0]
        assert s == sum(int(k) for k in np.round(v64 / (vx.SCALE if np.dtype(dtype).kind == "f" else 1.0))) * \
            (vx.SCALE if np.dtype(dtype).kind == "f" else 1.0)
        cnt, mean, *_ = vx.expected(np.zeros(n, np.int64), v, 1)
        assert cnt[0] == n and mean[0] == s / n


def test_power_of_two_counts_give_m2_bit_for_bit():
    rng = np.random.default_rng(2)
    for dtype in (np.float64, np.float32, np.int32):
        for j in range(0, 10):
            n = 1 << j
            v = vx.grid(rng, n, dtype)
            cnt, mean, m2, bound, exact = vx.expected(np.zeros(n, np.int64), v, 1)
            assert exact[0] and bound[0] == 0.0
            got = {_kernel_m2(v, mean[0], rng, pieces=p) for p in (1, 4, 16) for _ in range(5)}
            assert got == {m2[0]}, (n, got, m2[0])
    # from 2^10 values on the squares' sums round: such a bin takes the bound, and the bound holds
    v = vx.grid(rng, 1 << 12)
    cnt, mean, m2, bound, exact = vx.expected(np.zeros(v.size, np.int64), v, 1)
    assert not exact[0] and bound[0] > 0
    assert len({_kernel_m2(v, mean[0], rng, pieces=16) for _ in range(8)}) > 1
    assert all(abs(_kernel_m2(v, mean[0], rng, pieces=16) - m2[0]) <= bound[0] for _ in range(8))


def test_off_grid_values_are_refused():
    with pytest.raises(AssertionError):
        vx.expected(np.zeros(2, np.int64), np.array([0.1, 0.2]), 1)
    assert not vx.on_grid([4096.0])
    assert vx.on_grid([4095 * 2.0**-10, -4095.0 * 2.0**-10, np.nan])


@pytest.mark.parametrize("n", [3, 5, 7, 100, 999, 4097, 50_000])
def test_bound_holds_in_many_orders(n):
    rng = np.random.default_rng(n)
    for offset in (0.0, 3.5, -3.0):  # a mean far from zero: d has full mantissas and the cancellation matters
        v = vx.grid(rng, n) * 0.01 + offset
        v = np.round(v / vx.SCALE) * vx.SCALE
        cnt, mean, m2, bound, exact = vx.expected(np.zeros(n, np.int64), v, 1)
        assert not exact[0] and bound[0] > 0
        worst = 0.0
        for pieces in (1, 2, 16, 256):
            for _ in range(8):
                got = _kernel_m2(v, mean[0], rng, pieces=pieces)
                err = abs(got - m2[0])
                assert err <= bound[0], (n, offset, pieces, got, m2[0], err, bound[0])
                worst = max(worst, err)
        for ddof in (0, 1):
            var, vb = vx.var_bound(cnt, m2, bound, ddof)
            assert abs(_kernel_m2(v, mean[0], rng, pieces=4) / (n - ddof) - var[0]) <= vb[0]


@pytest.mark.parametrize("n", [7, 100, 999, 50_000])
def test_bound_is_broken_by_float32_squares(n):
    """q summed in float32 (what an accumulator of 24 bits would give): beyond the bound for every such bin"""
    rng = np.random.default_rng(100 + n)
    v = vx.grid(rng, n)
    cnt, mean, m2, bound, exact = vx.expected(np.zeros(n, np.int64), v, 1)
    assert not exact[0]
    errs = [abs(_kernel_m2(v, mean[0], rng, acc=np.float32, pieces=4) - m2[0]) for _ in range(8)]
    assert max(errs) > 100 * bound[0], (errs, bound[0])
    # and the bound is a small multiple of u n M2: what float64 sums may move, not a loose tolerance
    assert bound[0] <= 16 * n * vx.U * m2[0], (bound[0], m2[0])


def test_expected_over_many_bins():
    """several bins at once: counts of every size, empty bins NaN, NaN values dropped, the check helpers"""
    rng = np.random.default_rng(3)
    size = 40
    reps = rng.integers(0, 70, size)
    reps[[3, 9]] = 0
    reps[[4, 5]] = [64, 1]
    flat = np.repeat(np.arange(size), reps)
    v = vx.grid(rng, flat.size)
    v[::17] = np.nan
    cnt, mean, m2, bound, exact = vx.expected(flat, v, size)
    keep = ~np.isnan(v)
    np.testing.assert_array_equal(cnt, np.bincount(flat[keep], minlength=size))
    assert np.isnan(mean[cnt == 0]).all() and np.isnan(m2[cnt == 0]).all()
    np.testing.assert_array_equal(exact, vx.is_pow2(cnt))
    for b in np.flatnonzero(cnt):
        vals = v[keep][flat[keep] == b]
        assert mean[b] == np.sum(vals) / len(vals)
    vx.assert_m2(m2, m2, bound, exact)
    got = m2.copy()
    i = int(np.flatnonzero(exact & (cnt > 1) & (m2 > 0))[0])
    got[i] = np.nextafter(got[i], np.inf)
    with pytest.raises(AssertionError, match="power-of-two"):
        vx.assert_m2(got, m2, bound, exact)
    got = m2.copy()
    j = int(np.flatnonzero(~exact & (cnt > 2))[0])
    got[j] = m2[j] + 4 * bound[j]
    with pytest.raises(AssertionError, match="bound"):
        vx.assert_m2(got, m2, bound, exact)
