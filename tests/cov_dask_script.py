"""histogram_cov's dask branch, run by tests/test_gpu_cov.py in the interpreter that has dask: chunked inputs give what the
unchunked call gives.

Bit for bit: grid data (tests/values_exact.py) laid out so that every block holds a power-of-two count 2^j of every bin and two
blocks meet per output row.  Then the blocks' means are exact, and in Chan's merge d = mean_2 - mean_1 is exact, n_2 / n is a
power of two and mean_1 + d n_2 / n fits 53 bits: only divisions by powers of two, so the count and both means equal the
unchunked call's bit for bit; the moments are held to the tolerance of tests/test_cov_cpu.py's merge test.

To rounding: random counts with NaNs in both value arrays, reductions over every axis, over chunked axes and over none of the
chunks, ddof 0 and 1, the second value array broadcast from a smaller one.  There the merge's divisions round, so the means are
compared at rtol 1e-12."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import dask  # noqa: E402
import dask.array as dsa  # noqa: E402

from xhistogram_amd import core  # noqa: E402


def close(got, want, rtol, atol=1e-12):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.allclose(got[ok], want[ok], rtol=rtol, atol=atol), np.max(np.abs(got[ok] - want[ok]))


def grid(rng, shape):
    return rng.integers(-4095, 4096, shape) * 2.0**-10


def power_of_two_blocks():
    """shape (4, 64, 32), bin j % 8 at [t, i, j]: a (2, 32, 32) block holds 2^7 samples of every bin per t, two blocks meet along
    axis 1; a (2, 64, 32) block holds 2 samples per output row of a reduction over axis 0, two blocks meet along axis 0"""
    rng = np.random.default_rng(9)
    shape = (4, 64, 32)
    x = np.broadcast_to((np.arange(32) % 8) + 0.5, shape).copy()
    a, b = grid(rng, shape), grid(rng, shape)
    edges = [np.arange(9.0)]
    for axis, c in (((1, 2), (2, 32, 32)), ((0,), (2, 64, 32))):
        want = core.histogram_cov(x, values=(a, b), bins=edges, axis=axis, ddof=1)
        got = core.histogram_cov(dsa.from_array(x, chunks=c), values=(dsa.from_array(a, chunks=c), dsa.from_array(b, chunks=c)),
                                 bins=edges, axis=axis, ddof=1)
        got = dask.compute(*got[:6])
        assert got[0].dtype == np.int64 and np.array_equal(got[0], want[0])
        for g, w in zip(got[1:3], want[1:3]):  # the means: bit for bit
            assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~np.isnan(w)].view(np.int64), w[~np.isnan(w)].view(np.int64))
        for g, w in zip(got[3:], want[3:6]):
            close(g, w, 1e-10)


def main():
    dask.config.set(scheduler="threads")
    power_of_two_blocks()
    rng = np.random.default_rng(4)
    x = rng.uniform(-1.2, 1.2, (6, 40, 50))
    y = rng.uniform(-1.2, 1.2, (6, 40, 50))
    a = grid(rng, (6, 40, 50))
    b = np.round((-0.5 * a + 0.5 * grid(rng, a.shape)) * 2.0**10) * 2.0**-10
    a[rng.random(a.shape) < 0.05] = np.nan
    b[rng.random(b.shape) < 0.05] = np.nan
    edges = [np.linspace(-1, 1, 11), np.sort(rng.uniform(-1, 1, 7))]
    c = (2, 15, 20)
    for axis, ddof in ((None, 0), ((1, 2), 1), ((0,), 0), ((2,), 1), ((0, 2), 0)):
        want = core.histogram_cov(x, y, values=(a, b), bins=edges, axis=axis, ddof=ddof)
        got = core.histogram_cov(dsa.from_array(x, chunks=c), dsa.from_array(y, chunks=c),
                                 values=(dsa.from_array(a, chunks=c), dsa.from_array(b, chunks=c)), bins=edges, axis=axis, ddof=ddof)
        assert all(isinstance(g, dsa.Array) for g in got[:6])
        n, ma, mb, va, vb, cab = dask.compute(*got[:6])
        assert n.dtype == np.int64 and np.array_equal(n, want[0])
        # the means: Chan's merge divides (d * n2 / n), so a merged mean is the unchunked one to rounding
        close(ma, want[1], 1e-12)
        close(mb, want[2], 1e-12)
        close(va, want[3], 1e-10)
        close(vb, want[4], 1e-10)
        close(cab, want[5], 1e-10)
    # a reduction over axes nothing chunks: no merge, so the count and the means are the unchunked call's bit for bit
    c1 = (2, 40, 50)
    want = core.histogram_cov(x, values=(a, b), bins=edges[:1], axis=(1, 2))
    got = core.histogram_cov(dsa.from_array(x, chunks=c1), values=(dsa.from_array(a, chunks=c1), dsa.from_array(b, chunks=c1)),
                             bins=edges[:1], axis=(1, 2))
    got = dask.compute(*got[:6])
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g, w, equal_nan=True)
    for g, w in zip(got[3:], want[3:6]):
        close(g, w, 1e-10)
    # b broadcast from a smaller array (one map over time)
    bmap = grid(rng, (1, 40, 50))
    want = core.histogram_cov(x, values=(a, bmap), bins=edges[:1], axis=(1, 2))
    got = core.histogram_cov(dsa.from_array(x, chunks=(3, 10, 25)), values=(dsa.from_array(a, chunks=(3, 10, 25)),
                             dsa.from_array(bmap, chunks=(1, 10, 25))), bins=edges[:1], axis=(1, 2))
    got = dask.compute(*got[:6])
    assert np.array_equal(got[0], want[0])
    close(got[1], want[1], 1e-12)
    close(got[2], want[2], 1e-12)
    for g, w in zip(got[3:], want[3:6]):
        close(g, w, 1e-10)
    print("COV-DASK-OK")


if __name__ == "__main__":
    main()
