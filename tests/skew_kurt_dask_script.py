"""histogram_skew_kurt's dask branch, run by tests/test_gpu_skew_kurt.py in the interpreter that has dask: chunked inputs give
what the unchunked call gives, with and without weights.

Every reduction here splits over a reduced axis, so that blocks that share output rows meet in the merge
(core.combine_skew_kurt / combine_weighted_skew_kurt, Pébay's pairwise update).  The values are on the narrow grid of
tests/skew_kurt_exact.py (k 2^-4, |k| < 2^6) with NaNs, the weights small integers, so x (the count, or W) is exact whatever
the blocks and is compared bit for bit.  The merged mean divides (d * xb / x), so it is the unchunked one to rounding (rtol
1e-12, as the mean_var and cov scripts hold it); the merged M2 is combine_mean_var's, held to those scripts' rtol 1e-10 on var;
M3 and M4 add correction terms of products of up to four deviations of the blocks' means, each formed in float64 in the merge's
own order, and skew and kurt divide them by powers of m2: both are held to rtol 1e-9 with an absolute 1e-9, which covers a skew
near 0 (a bin's |skew| and |kurt| are O(1) here, the terms' roundings O(1e-15)).  A reduction over axes nothing chunks merges
nothing: every output is the unchunked call's bit for bit where the sums are exact, and to rounding elsewhere."""
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
    assert np.array_equal(np.isnan(got), np.isnan(want)), (np.isnan(got).sum(), np.isnan(want).sum())
    ok = ~np.isnan(want)
    assert np.allclose(got[ok], want[ok], rtol=rtol, atol=atol), np.max(np.abs(got[ok] - want[ok]))


def narrow(rng, shape):
    return rng.integers(-63, 64, shape) * 2.0**-4


def da(arrays, chunks):
    return [dsa.from_array(a, chunks=tuple(min(c, s) for c, s in zip(chunks, a.shape))) for a in arrays]


def main():
    dask.config.set(scheduler="threads")
    rng = np.random.default_rng(14)
    shape = (6, 40, 50)
    x = rng.uniform(-1.2, 1.2, shape)
    y = rng.uniform(-1.2, 1.2, shape)
    v = narrow(rng, shape) + np.where(rng.random(shape) < 0.3, 2.0, 0.0)  # (a second mode: skewed bins)
    v[rng.random(shape) < 0.05] = np.nan
    w = rng.integers(0, 8, shape).astype(np.float64)
    edges = [np.linspace(-1, 1, 11), np.sort(rng.uniform(-1, 1, 7))]
    c = (2, 15, 20)
    for wts in (None, w):
        for axis, kw in ((None, {}), ((1, 2), dict(ddof=1, bias=False)), ((0,), dict(fisher=False)), ((2,), dict(ddof=1)),
                         ((0, 2), dict(bias=False, fisher=False))):
            want = core.histogram_skew_kurt(x, y, values=v, weights=wts, bins=edges, axis=axis, **kw)
            arrays = da((x, y, v) + (() if wts is None else (wts,)), c)
            got = core.histogram_skew_kurt(arrays[0], arrays[1], values=arrays[2], weights=None if wts is None else arrays[3],
                                           bins=edges, axis=axis, **kw)
            assert all(isinstance(g, dsa.Array) for g in got[:5])
            first, mean, var, skew, kurt = dask.compute(*got[:5])
            assert first.dtype == (np.int64 if wts is None else np.float64) and np.array_equal(first, want[0])
            close(mean, want[1], 1e-12)
            close(var, want[2], 1e-10)
            close(skew, want[3], 1e-9, 1e-9)
            close(kurt, want[4], 1e-9, 1e-9)
            assert np.isfinite(want[4]).sum() > (want[4].size // 2 if axis is None else 0)  # (something to compare)
    # the merge on the host against the whole: the partials of two halves of one row
    xr, vr, wr = x.reshape(1, -1), v.reshape(1, -1), w.reshape(1, -1)
    half = xr.shape[1] // 2
    for wts, combine in ((None, core.combine_skew_kurt), (wr, core.combine_weighted_skew_kurt)):
        stat = "skew_kurt" if wts is None else "skew_kurt_w"
        parts = []
        for sl in (slice(0, half), slice(half, None)):
            _, outs, _, _ = core._value_stat(stat, [xr[:, sl]], vr[:, sl], edges[:1], None, (1,), "histogram_skew_kurt",
                                             weights=None if wts is None else wts[:, sl])
            parts.append(np.stack([np.asarray(o, np.float64) for o in outs]))
        _, whole, _, _ = core._value_stat(stat, [xr], vr, edges[:1], None, (1,), "histogram_skew_kurt", weights=wts)
        merged = combine(*np.stack(parts, axis=1), axis=0)
        assert np.array_equal(merged[0].reshape(-1), np.asarray(whole[0], np.float64).reshape(-1))
        close(merged[1].reshape(-1), np.asarray(whole[1]).reshape(-1), 1e-12)
        for k in (2, 3, 4):
            close(merged[k].reshape(-1), np.asarray(whole[k]).reshape(-1), 1e-9, 1e-9)
    # a reduction over axes nothing chunks: no merge
    c1 = (2, 40, 50)
    for wts in (None, w):
        want = core.histogram_skew_kurt(x, values=v, weights=wts, bins=edges[:1], axis=(1, 2))
        arrays = da((x, v) + (() if wts is None else (wts,)), c1)
        got = dask.compute(*core.histogram_skew_kurt(arrays[0], values=arrays[1], weights=None if wts is None else arrays[2],
                                                     bins=edges[:1], axis=(1, 2))[:5])
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1], equal_nan=True)
        close(got[2], want[2], 1e-10)
        close(got[3], want[3], 1e-9, 1e-9)
        close(got[4], want[4], 1e-9, 1e-9)
    print("SKEW-KURT-DASK-OK")


if __name__ == "__main__":
    main()
