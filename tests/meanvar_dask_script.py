"""histogram_mean_var's dask branch, run by tests/test_gpu_meanvar.py in the interpreter that has dask: chunked inputs give what
the unchunked call gives (counts exactly; means and variances to rounding, since the partials meet in Chan's merge), for
reductions over every axis, over chunked axes and over none of the chunks, and for ddof 0 and 1."""
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
    rng = np.random.default_rng(3)
    x = rng.uniform(-1.2, 1.2, (6, 40, 50))
    y = rng.uniform(-1.2, 1.2, (6, 40, 50))
    v = 20.0 + rng.standard_normal((6, 40, 50))
    v[rng.random(v.shape) < 0.05] = np.nan
    edges = [np.linspace(-1, 1, 11), np.sort(rng.uniform(-1, 1, 7))]
    for axis, ddof in ((None, 0), ((1, 2), 1), ((0,), 0), ((2,), 1), ((0, 2), 0)):
        want = core.histogram_mean_var(x, y, values=v, bins=edges, axis=axis, ddof=ddof)
        got = core.histogram_mean_var(dsa.from_array(x, chunks=(2, 15, 20)), dsa.from_array(y, chunks=(2, 15, 20)),
                                      values=dsa.from_array(v, chunks=(2, 15, 20)), bins=edges, axis=axis, ddof=ddof)
        assert all(isinstance(a, dsa.Array) for a in got[:3])
        cnt, mean, var = dask.compute(*got[:3])
        assert cnt.dtype == np.int64 and np.array_equal(cnt, want[0])
        close(mean, want[1], 1e-12)
        close(var, want[2], 1e-9)
    # values broadcast from a smaller array
    vb = rng.standard_normal((1, 40, 1))
    want = core.histogram_mean_var(x, values=vb, bins=edges[:1], axis=(1, 2))
    got = core.histogram_mean_var(dsa.from_array(x, chunks=(3, 10, 25)), values=dsa.from_array(vb, chunks=(1, 10, 1)), bins=edges[:1],
                                  axis=(1, 2))
    assert np.array_equal(got[0].compute(), want[0])
    close(got[1].compute(), want[1], 1e-12)
    close(got[2].compute(), want[2], 1e-9)
    print("MEANVAR-DASK-OK")


if __name__ == "__main__":
    main()
