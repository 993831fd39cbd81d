"""The dask branch of bin_sort, run by tests/test_gpu_bin_sort.py in an interpreter that has dask: inputs chunked along the
kept axes (every reduced axis one chunk) give what the numpy call gives, bit for bit, and that is the oracle's result; a cut
reduced axis is refused."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dask  # noqa: E402
import dask.array as dsa  # noqa: E402

import bin_order_oracle as bo  # noqa: E402
import bin_sort_oracle as so  # noqa: E402
import map_oracle as mo  # noqa: E402
from xhistogram_amd import core  # noqa: E402

SHAPE = (4, 40, 50)
CHUNK = (2, 20, 25)


def main():
    dask.config.set(scheduler="threads")
    rng = np.random.default_rng(13)
    edges = [np.linspace(-1, 1, 9), np.sort(rng.uniform(-1, 1, 6))]
    x, y = rng.uniform(-1.2, 1.2, (2,) + SHAPE)
    v = rng.integers(-5, 6, SHAPE).astype(np.float32)  # (many ties)
    v[rng.random(SHAPE) < 0.05] = np.nan
    idx = mo.index([x, y], edges)
    for axis, descending in ((None, False), ((1, 2), True), ((0,), False), ((2,), True), ((2, 0), False)):
        red = tuple(range(3)) if axis is None else axis
        chunks = tuple(SHAPE[i] if i in red else CHUNK[i] for i in range(3))
        dx, dy, dv = (dsa.from_array(a, chunks=chunks) for a in (x, y, v))
        order, offsets, e = core.bin_sort(dx, dy, values=dv, bins=edges, axis=axis, descending=descending)
        assert isinstance(order, dsa.Array) and isinstance(offsets, dsa.Array) and all(isinstance(b, np.ndarray) for b in e)
        want_order, want_offsets = so.order_offsets(bo.rows_of(idx, axis), bo.rows_of(v, axis), 40, descending)
        assert order.shape == want_order.shape and offsets.shape == want_offsets.shape, (axis, order.shape, offsets.shape)
        got_order, got_offsets = dask.compute(order, offsets)
        mo.assert_bits(got_order, want_order, "dask order axis=%s" % (axis,))
        mo.assert_bits(got_offsets, want_offsets, "dask offsets axis=%s" % (axis,))
        np_order, np_offsets, _ = core.bin_sort(x, y, values=v, bins=edges, axis=axis, descending=descending)
        mo.assert_bits(np_order, want_order, "numpy order axis=%s" % (axis,))
        mo.assert_bits(np_offsets, want_offsets, "numpy offsets axis=%s" % (axis,))
    try:
        core.bin_sort(dsa.from_array(x, chunks=CHUNK), dsa.from_array(y, chunks=CHUNK), values=dsa.from_array(v, chunks=CHUNK), bins=edges,
                      axis=(1,))
    except ValueError as err:
        assert "sorted orders of several chunks cannot be merged" in str(err)
    else:
        raise AssertionError("a cut reduced axis was accepted")
    print("BIN-SORT-DASK-OK")


if __name__ == "__main__":
    main()
