"""histogram_sum's dask branch, run by tests/test_gpu_sum.py in the interpreter that has dask: inputs chunked along the kept
axes give exactly what the unchunked numpy call gives (every reduced axis in one chunk), the counts arrive as int64, and a
chunked reduced axis is refused before any compute."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import dask  # noqa: E402
import dask.array as dsa  # noqa: E402

from xhistogram_amd import core  # noqa: E402


def compare(got, want):
    assert all(isinstance(g, dsa.Array) for g in got[:2])
    assert got[0].dtype == np.int64 and got[1].dtype == np.float64
    cnt, tot = dask.compute(*got[:2])
    assert cnt.dtype == np.int64 and np.array_equal(cnt, want[0])
    assert tot.shape == want[1].shape and np.array_equal(tot.view(np.uint64), want[1].view(np.uint64))
    return cnt


def main():
    dask.config.set(scheduler="threads")
    rng = np.random.default_rng(3)
    x = rng.standard_normal((24, 3_000)).astype(np.float32)
    v = (1e8 + 1e3 * rng.standard_normal(x.shape)).astype(np.float64)
    v[rng.random(v.shape) < 0.05] = np.nan
    e50 = np.linspace(-4, 4, 51)
    want = core.histogram_sum(x, values=v, bins=e50, axis=1)
    got = core.histogram_sum(dsa.from_array(x, chunks=(5, -1)), values=dsa.from_array(v, chunks=(5, -1)), bins=e50, axis=1)
    cnt = compare(got, want)
    assert (cnt == 0).any() and (cnt > 0).any()
    # two inputs, kept axes on both sides of the reduced one, values broadcast from a smaller array
    x3 = rng.uniform(-1.2, 1.2, (6, 40, 7))
    y3 = rng.uniform(-1.2, 1.2, (6, 40, 7))
    v3 = rng.standard_normal((1, 40, 7)) * 1e6
    edges = [np.linspace(-1, 1, 6), np.sort(rng.uniform(-1, 1, 5))]
    for axis, chunks in (((1,), (2, 40, 3)), ((2, 1), (4, 40, 7)), ((0, 1, 2), (6, 40, 7))):
        want = core.histogram_sum(x3, y3, values=v3, bins=edges, axis=axis)
        got = core.histogram_sum(dsa.from_array(x3, chunks=chunks), dsa.from_array(y3, chunks=chunks),
                                 values=dsa.from_array(v3, chunks=(1,) + chunks[1:]), bins=edges, axis=axis)
        compare(got, want)
    # a reduced axis in two chunks: refused where the graph is built
    try:
        core.histogram_sum(dsa.from_array(x, chunks=(5, 1_500)), values=dsa.from_array(v, chunks=(5, 1_500)), bins=e50, axis=1)
    except ValueError as e:
        assert "reproducible sums of several chunks cannot be merged" in str(e) and "rechunk the reduced axes" in str(e)
    else:
        raise AssertionError("a chunked reduced axis was accepted")
    print("SUM-DASK-OK")


if __name__ == "__main__":
    main()
