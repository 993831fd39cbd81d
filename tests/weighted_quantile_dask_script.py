"""histogram_weighted_quantile's dask branch, run by tests/test_gpu_weighted_quantile.py in the interpreter that has dask: inputs
chunked only along kept axes give exactly what the unchunked call gives (one task per block, no merge), for reductions over one
axis and over two, with weights of full shape and weights broadcast over a kept axis; a reduced axis split into several chunks
is refused with the advice to rechunk."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dask  # noqa: E402
import dask.array as dsa  # noqa: E402

import exact_weights as xw  # noqa: E402
from xhistogram_amd import core  # noqa: E402


def main():
    dask.config.set(scheduler="threads")
    rng = np.random.default_rng(3)
    shape = (6, 40, 50)
    x = rng.uniform(-1.2, 1.2, shape)
    y = rng.uniform(-1.2, 1.2, shape)
    v = np.round(20.0 + rng.standard_normal(shape), 1)
    v[rng.random(shape) < 0.05] = np.nan
    w = np.where(rng.random(shape) < 0.3, 0.0, xw.f64(rng, shape))
    edges = [np.linspace(-1, 1, 11), np.sort(rng.uniform(-1, 1, 7))]
    for axis, chunks, q in (((1, 2), (2, 40, 50), [0.25, 0.5, 0.75]), ((0,), (6, 15, 20), 0.5), ((0, 2), (6, 10, 50), [0.1, 0.9])):
        want, _ = core.histogram_weighted_quantile(x, y, values=v, weights=w, q=q, bins=edges, axis=axis)
        got, _ = core.histogram_weighted_quantile(dsa.from_array(x, chunks=chunks), dsa.from_array(y, chunks=chunks),
                                                  values=dsa.from_array(v, chunks=chunks), weights=dsa.from_array(w, chunks=chunks),
                                                  q=q, bins=edges, axis=axis)
        assert isinstance(got, dsa.Array)
        g = got.compute()
        assert g.shape == want.shape, (g.shape, want.shape)
        np.testing.assert_array_equal(g, want)
    # weights of a cell area, broadcast over the leading axis (numpy weights next to dask samples)
    area = w[0]
    want, _ = core.histogram_weighted_quantile(x, values=v, weights=area, q=[0.5], bins=edges[:1], axis=(1, 2))
    got, _ = core.histogram_weighted_quantile(dsa.from_array(x, chunks=(2, 40, 50)), values=dsa.from_array(v, chunks=(2, 40, 50)),
                                              weights=area, q=[0.5], bins=edges[:1], axis=(1, 2))
    np.testing.assert_array_equal(got.compute(), want)
    try:
        core.histogram_weighted_quantile(dsa.from_array(x, chunks=(2, 40, 50)), values=dsa.from_array(v, chunks=(2, 40, 50)),
                                         weights=dsa.from_array(w, chunks=(2, 40, 50)), q=0.5, bins=edges[:1], axis=(0,))
    except ValueError as e:
        assert "rechunk" in str(e)
    else:
        raise AssertionError("a chunked reduced axis was accepted")
    print("WEIGHTED-QUANTILE-DASK-OK")


if __name__ == "__main__":
    main()
