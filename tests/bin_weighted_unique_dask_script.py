"""The dask branches of bin_weighted_unique and histogram_weighted_mode, run by tests/test_gpu_bin_weighted_unique.py in an
interpreter that has dask: inputs chunked along the kept axes (every reduced axis one chunk) give what the numpy call gives, bit
for bit, and that is the oracle's result; a cut reduced axis is refused."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dask  # noqa: E402
import dask.array as dsa  # noqa: E402

import bin_order_oracle as bo  # noqa: E402
import exact_weights as xw  # noqa: E402
import map_oracle as mo  # noqa: E402
import weighted_unique_oracle as wo  # noqa: E402
from xhistogram_amd import core  # noqa: E402

SHAPE = (4, 40, 50)
CHUNK = (2, 20, 25)


def main():
    dask.config.set(scheduler="threads")
    rng = np.random.default_rng(13)
    edges = [np.linspace(-1, 1, 9), np.sort(rng.uniform(-1, 1, 6))]
    x, y = rng.uniform(-1.2, 1.2, (2,) + SHAPE)
    v = rng.integers(-5, 6, SHAPE).astype(np.float32)
    v[rng.random(SHAPE) < 0.05] = np.nan
    w = xw.f64(rng, SHAPE, "both")
    idx = mo.index([x, y], edges)
    for axis in (None, (1, 2), (0,), (2,)):
        red = tuple(range(3)) if axis is None else axis
        chunks = tuple(SHAPE[i] if i in red else CHUNK[i] for i in range(3))
        dx, dy, dv, dw = (dsa.from_array(a, chunks=chunks) for a in (x, y, v, w))
        rows = (bo.rows_of(idx, axis), bo.rows_of(v, axis), bo.rows_of(w, axis))
        *got, e = core.bin_weighted_unique(dx, dy, values=dv, weights=dw, bins=edges, axis=axis, size=60)
        assert all(isinstance(g, dsa.Array) for g in got) and [g.dtype for g in got] == [np.float64, np.int64, np.float64, np.int64]
        want = wo.wunique_rows(*rows, 40, 60)[:4]
        wo.assert_same(dask.compute(*got), want, "dask axis=%s" % (axis,))
        wo.assert_same(core.bin_weighted_unique(x, y, values=v, weights=w, bins=edges, axis=axis, size=60)[:4], want, "numpy axis=%s" % (axis,))
        kept = tuple(SHAPE[i] for i in range(3) if i not in red)
        *got, e = core.histogram_weighted_mode(dx, dy, values=dv, weights=dw, bins=edges, axis=axis)
        assert all(isinstance(g, dsa.Array) and g.shape == kept + (8, 5) for g in got)
        assert [g.dtype for g in got] == [np.int64, np.int64, np.float64, np.float64]
        wo.assert_mode_same(dask.compute(*got), [a.reshape(kept + (8, 5)) for a in wo.wmode_rows(*rows, 40)], "dask mode axis=%s" % (axis,))
    for fn in (core.bin_weighted_unique, core.histogram_weighted_mode):
        try:
            fn(*(dsa.from_array(a, chunks=CHUNK) for a in (x, y)), values=dsa.from_array(v, chunks=CHUNK), weights=dsa.from_array(w, chunks=CHUNK),
               bins=edges, axis=(1,))
        except ValueError as err:
            assert "of several chunks cannot be merged" in str(err)
        else:
            raise AssertionError("a cut reduced axis was accepted")
    print("WUNIQUE-DASK-OK")


if __name__ == "__main__":
    main()
