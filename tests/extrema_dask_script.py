"""histogram_extrema's dask branch, run by tests/test_gpu_extrema.py in the interpreter that has dask: chunked inputs give
bit for bit what the unchunked call gives, for reductions over every axis, over chunked axes and over none of the chunks."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import dask  # noqa: E402
import dask.array as dsa  # noqa: E402

from xhistogram_amd import core  # noqa: E402


def same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    assert np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))


def main():
    dask.config.set(scheduler="threads")
    rng = np.random.default_rng(3)
    x = rng.uniform(-1.2, 1.2, (6, 40, 50))
    y = rng.uniform(-1.2, 1.2, (6, 40, 50))
    v = rng.standard_normal((6, 40, 50))
    v[rng.random(v.shape) < 0.05] = np.nan
    v[0, 0, :5] = [-0.0, 0.0, -0.0, 0.0, -0.0]
    edges = [np.linspace(-1, 1, 11), np.sort(rng.uniform(-1, 1, 7))]
    for axis in (None, (1, 2), (0,), (2,), (0, 2)):
        want = core.histogram_extrema(x, y, values=v, bins=edges, axis=axis)
        got = core.histogram_extrema(dsa.from_array(x, chunks=(2, 15, 20)), dsa.from_array(y, chunks=(2, 15, 20)),
                                     values=dsa.from_array(v, chunks=(2, 15, 20)), bins=edges, axis=axis)
        assert isinstance(got[0], dsa.Array)
        lo, hi = dask.compute(got[0], got[1])
        same(lo, want[0])
        same(hi, want[1])
    # values broadcast from a smaller array
    vb = rng.standard_normal((1, 40, 1))
    want = core.histogram_extrema(x, values=vb, bins=edges[:1], axis=(1, 2))
    got = core.histogram_extrema(dsa.from_array(x, chunks=(3, 10, 25)), values=dsa.from_array(vb, chunks=(1, 10, 1)), bins=edges[:1], axis=(1, 2))
    same(got[0].compute(), want[0])
    same(got[1].compute(), want[1])
    print("EXTREMA-DASK-OK")


if __name__ == "__main__":
    main()
