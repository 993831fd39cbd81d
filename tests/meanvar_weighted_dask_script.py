"""histogram_mean_var's weighted dask branch, run by tests/test_gpu_meanvar_weighted.py in the interpreter that has dask:
chunked inputs give what the unchunked call gives (W exactly on integer weights; means and variances to rounding, since the
partials meet in the weighted Chan merge), for reductions over every axis, over chunked axes and over none of the chunks, for
ddof 0 and 1, with weights broadcast from a smaller array."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import dask  # noqa: E402
import dask.array as dsa  # noqa: E402

from xhistogram_amd import core  # noqa: E402


def close(got, want, rtol):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.allclose(got[ok], want[ok], rtol=rtol, atol=1e-12), np.max(np.abs(got[ok] - want[ok]))


def main():
    dask.config.set(scheduler="threads")
    rng = np.random.default_rng(4)
    x = rng.uniform(-1.2, 1.2, (6, 40, 50))
    y = rng.uniform(-1.2, 1.2, (6, 40, 50))
    v = 20.0 + rng.standard_normal((6, 40, 50))
    v[rng.random(v.shape) < 0.05] = np.nan
    w = rng.integers(0, 8, (6, 40, 50)).astype(np.float64)
    edges = [np.linspace(-1, 1, 11), np.sort(rng.uniform(-1, 1, 7))]
    for axis, ddof in ((None, 0), ((1, 2), 1), ((0,), 0), ((2,), 1), ((0, 2), 0)):
        want = core.histogram_mean_var(x, y, values=v, weights=w, bins=edges, axis=axis, ddof=ddof)
        c = (2, 15, 20)
        got = core.histogram_mean_var(dsa.from_array(x, chunks=c), dsa.from_array(y, chunks=c), values=dsa.from_array(v, chunks=c),
                                      weights=dsa.from_array(w, chunks=c), bins=edges, axis=axis, ddof=ddof)
        assert all(isinstance(a, dsa.Array) for a in got[:3])
        W, mean, var = dask.compute(*got[:3])
        assert W.dtype == np.float64 and np.array_equal(W, want[0])
        close(mean, want[1], 1e-12)
        close(var, want[2], 1e-9)
    # weights broadcast from a smaller array (a cell area over time)
    area = rng.uniform(1e6, 1e9, (1, 40, 50))
    want = core.histogram_mean_var(x, values=v, weights=area, bins=edges[:1], axis=(1, 2))
    got = core.histogram_mean_var(dsa.from_array(x, chunks=(3, 10, 25)), values=dsa.from_array(v, chunks=(3, 10, 25)),
                                  weights=dsa.from_array(area, chunks=(1, 10, 25)), bins=edges[:1], axis=(1, 2))
    close(got[0].compute(), want[0], 1e-12)
    close(got[1].compute(), want[1], 1e-12)
    close(got[2].compute(), want[2], 1e-9)
    print("MEANVAR-W-DASK-OK")


if __name__ == "__main__":
    main()
