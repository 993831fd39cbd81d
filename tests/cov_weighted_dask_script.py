"""histogram_weighted_cov's dask branch, run by tests/test_gpu_cov_weighted.py in the interpreter that has dask: chunked
inputs give what the unchunked call gives.

Bit for bit: grid data (tests/values_exact.py) with weights 1, 2 and 4 laid out so that every block holds a power-of-two sum
of weights 2^j of every bin and two blocks meet per output row.  Then the blocks' means are exact, and in Chan's merge
d = mean_2 - mean_1 is exact, W_2 / W is a power of two and mean_1 + d W_2 / W fits 53 bits: only divisions by powers of two, so
W and both means equal the unchunked call's bit for bit.  The moments are NOT bit for bit after a merge, even on these blocks:
each block's moments are exact, but the merge adds d_i * d_j * W_1 * W_2 / W, a product of two 22-bit deviations of the means
that is formed and added in float64 in the merge's own order, while the unchunked call sums w * da * db about the overall mean;
the two agree to rounding only.  So the moments are held to the tolerance of tests/test_cov_cpu.py's merge test (rtol 1e-10),
as histogram_cov's dask test holds them; that each block's own moments are bit for bit is tests/test_gpu_cov_weighted.py's
business (every case there), not this script's.

To rounding: random integer weights with NaNs in both value arrays, reductions over every axis, over chunked axes and over none
of the chunks, ddof 0 and 1, the weights broadcast from a (lat, lon) map.  There the merge's divisions round, so the means are
compared at rtol 1e-12 and the moments at the rtol histogram_cov's dask test uses, for the same reason."""
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


def da(arrays, chunks):
    return [dsa.from_array(a, chunks=tuple(min(c, s) for c, s in zip(chunks, a.shape))) for a in arrays]


def power_of_two_blocks():
    """shape (4, 64, 32), bin j % 8 at [t, i, j], weight 1, 2, 4 or 1 by (j // 8): the four samples of a bin in a row of 32 weigh
    8 together, so a (2, 32, 32) block holds W = 2^8 of every bin per t, two blocks meet along axis 1; a (2, 64, 32) block holds
    two samples of the same weight per output row of a reduction over axis 0 (W = 2, 4 or 8), two blocks meet along axis 0"""
    rng = np.random.default_rng(9)
    shape = (4, 64, 32)
    x = np.broadcast_to((np.arange(32) % 8) + 0.5, shape).copy()
    w = np.broadcast_to(np.array([1.0, 2.0, 4.0, 1.0])[np.arange(32) // 8], shape).copy()
    a, b = grid(rng, shape), grid(rng, shape)
    edges = [np.arange(9.0)]
    for axis, c in (((1, 2), (2, 32, 32)), ((0,), (2, 64, 32))):
        want = core.histogram_weighted_cov(x, values=(a, b), weights=w, bins=edges, axis=axis, ddof=1)
        xd, ad, bd, wd = da((x, a, b, w), c)
        got = dask.compute(*core.histogram_weighted_cov(xd, values=(ad, bd), weights=wd, bins=edges, axis=axis, ddof=1)[:6])
        lg = np.log2(want[0][want[0] > 0])
        assert np.all(lg == np.round(lg)) and want[0].max() <= 512  # (each block's W a power of two up to 2^8, or 0)
        assert got[0].dtype == np.float64 and np.array_equal(got[0], want[0])
        for g, v in zip(got[1:3], want[1:3]):  # the means: bit for bit
            assert np.array_equal(np.isnan(g), np.isnan(v)) and np.array_equal(g[~np.isnan(v)].view(np.int64), v[~np.isnan(v)].view(np.int64))
        for g, v in zip(got[3:], want[3:6]):
            close(g, v, 1e-10)


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
    w = rng.integers(0, 8, a.shape).astype(np.float64)
    edges = [np.linspace(-1, 1, 11), np.sort(rng.uniform(-1, 1, 7))]
    c = (2, 15, 20)
    for axis, ddof in ((None, 0), ((1, 2), 1), ((0,), 0), ((2,), 1), ((0, 2), 0)):
        want = core.histogram_weighted_cov(x, y, values=(a, b), weights=w, bins=edges, axis=axis, ddof=ddof)
        xd, yd, ad, bd, wd = da((x, y, a, b, w), c)
        got = core.histogram_weighted_cov(xd, yd, values=(ad, bd), weights=wd, bins=edges, axis=axis, ddof=ddof)
        assert all(isinstance(g, dsa.Array) for g in got[:6])
        W, ma, mb, va, vb, cab = dask.compute(*got[:6])
        assert W.dtype == np.float64 and np.array_equal(W, want[0])  # (sums of small integers: exact whatever the blocks)
        # the means: Chan's merge divides (d * W2 / W), so a merged mean is the unchunked one to rounding
        close(ma, want[1], 1e-12)
        close(mb, want[2], 1e-12)
        close(va, want[3], 1e-10)
        close(vb, want[4], 1e-10)
        close(cab, want[5], 1e-10)
    # a reduction over axes nothing chunks: no merge, so W and the means are the unchunked call's bit for bit
    c1 = (2, 40, 50)
    want = core.histogram_weighted_cov(x, values=(a, b), weights=w, bins=edges[:1], axis=(1, 2))
    xd, ad, bd, wd = da((x, a, b, w), c1)
    got = dask.compute(*core.histogram_weighted_cov(xd, values=(ad, bd), weights=wd, bins=edges[:1], axis=(1, 2))[:6])
    for g, v in zip(got[:3], want[:3]):
        assert np.array_equal(g, v, equal_nan=True)
    for g, v in zip(got[3:], want[3:6]):
        close(g, v, 1e-10)
    # the weights broadcast from a (lat, lon) map over time
    wmap = rng.integers(0, 8, (1, 40, 50)).astype(np.float64)
    want = core.histogram_weighted_cov(x, values=(a, b), weights=wmap, bins=edges[:1], axis=(1, 2))
    xd, ad, bd, wd = da((x, a, b, wmap), (3, 10, 25))
    got = dask.compute(*core.histogram_weighted_cov(xd, values=(ad, bd), weights=wd, bins=edges[:1], axis=(1, 2))[:6])
    assert np.array_equal(got[0], want[0])
    close(got[1], want[1], 1e-12)
    close(got[2], want[2], 1e-12)
    for g, v in zip(got[3:], want[3:6]):
        close(g, v, 1e-10)
    print("COV-WEIGHTED-DASK-OK")


if __name__ == "__main__":
    main()
