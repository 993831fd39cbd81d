"""histogram_argextrema's dask branch, run by tests/test_gpu_argextrema.py in the interpreter that has dask: inputs chunked
along the kept axes give exactly what the unchunked call gives (C4's call shape in miniature: float32 rows, 50 uniform bins,
one reduced axis in one chunk), the positions arrive as int64, and a chunked reduced axis is refused before any compute."""
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


def compare(got, want):
    assert all(isinstance(g, dsa.Array) for g in got[:4])
    assert got[0].dtype == np.int64 and got[1].dtype == np.int64 and got[2].dtype == np.float64
    amin, amax, vmin, vmax = dask.compute(*got[:4])
    assert amin.dtype == np.int64 and amax.dtype == np.int64
    assert np.array_equal(amin, want[0]) and np.array_equal(amax, want[1])
    same(vmin, want[2])
    same(vmax, want[3])
    return amin


def main():
    dask.config.set(scheduler="threads")
    rng = np.random.default_rng(3)
    # C4 in miniature: float32 rows, 50 uniform bins over [-4, 4], the row axis reduced; values with ties and NaN
    x = rng.standard_normal((24, 3_000)).astype(np.float32)
    v = rng.integers(-3, 4, x.shape).astype(np.float32)
    v[rng.random(v.shape) < 0.05] = np.nan
    v[0, :5] = [0.0, -0.0, 0.0, -0.0, 0.0]
    e50 = np.linspace(-4, 4, 51)
    want = core.histogram_argextrema(x, values=v, bins=e50, axis=1)
    got = core.histogram_argextrema(dsa.from_array(x, chunks=(5, -1)), values=dsa.from_array(v, chunks=(5, -1)), bins=e50, axis=1)
    amin = compare(got, want)
    assert (amin == -1).any() and (amin > 0).any()  # (empty bins in the tails, positions elsewhere)
    # two inputs, kept axes on both sides of the reduced one, values broadcast from a smaller array
    x3 = rng.uniform(-1.2, 1.2, (6, 40, 7))
    y3 = rng.uniform(-1.2, 1.2, (6, 40, 7))
    v3 = rng.integers(0, 3, (1, 40, 7)).astype(np.float64)
    edges = [np.linspace(-1, 1, 6), np.sort(rng.uniform(-1, 1, 5))]
    for axis, chunks in (((1,), (2, 40, 3)), ((2, 1), (4, 40, 7)), ((0, 1, 2), (6, 40, 7))):
        want = core.histogram_argextrema(x3, y3, values=v3, bins=edges, axis=axis)
        got = core.histogram_argextrema(dsa.from_array(x3, chunks=chunks), dsa.from_array(y3, chunks=chunks),
                                        values=dsa.from_array(v3, chunks=(1,) + chunks[1:]), bins=edges, axis=axis)
        compare(got, want)
    # a reduced axis in several chunks: refused where the graph is built, with histogram_quantile's wording
    try:
        core.histogram_argextrema(dsa.from_array(x, chunks=(5, 1_000)), values=dsa.from_array(v, chunks=(5, 1_000)), bins=e50, axis=1)
    except ValueError as e:
        assert "rechunk the reduced axes" in str(e)
    else:
        raise AssertionError("a chunked reduced axis was accepted")
    print("ARGEXTREMA-DASK-OK")


if __name__ == "__main__":
    main()
