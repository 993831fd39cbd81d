"""The dask branch of bin_unique, run by tests/test_gpu_bin_unique.py in an interpreter that has dask: inputs chunked along the
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
import bin_unique_oracle as uo  # noqa: E402
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
    for axis in (None, (1, 2), (0,), (2,), (2, 0)):
        red = tuple(range(3)) if axis is None else tuple(sorted(axis))
        kept = [i for i in range(3) if i not in red]
        chunks = tuple(SHAPE[i] if i in red else CHUNK[i] for i in range(3))
        dx, dy, dv = (dsa.from_array(a, chunks=chunks) for a in (x, y, v))
        for size in (None, 30):
            *got, e = core.bin_unique(dx, dy, values=dv, bins=edges, axis=axis, size=size, return_inverse=True)
            assert all(isinstance(g, dsa.Array) for g in got) and all(isinstance(b, np.ndarray) for b in e)
            assert [g.dtype for g in got] == [np.float64, np.int64, np.int64, np.int64]
            uniques, counts, offsets, flat = uo.unique_rows(bo.rows_of(idx, axis), bo.rows_of(v, axis), 40, size)
            full = flat.reshape([SHAPE[i] for i in kept] + [SHAPE[i] for i in red])
            want = (uniques, counts, offsets, np.moveaxis(full, range(len(kept), 3), red) if kept else full)
            assert [g.shape for g in got] == [w.shape for w in want], ([g.shape for g in got], [w.shape for w in want])
            uo.assert_same(dask.compute(*got), want, "dask axis=%s size=%s" % (axis, size))
            uo.assert_same(core.bin_unique(x, y, values=v, bins=edges, axis=axis, size=size, return_inverse=True)[:4], want,
                           "numpy axis=%s size=%s" % (axis, size))
        assert len(core.bin_unique(dx, dy, values=dv, bins=edges, axis=axis)) == 4
    try:
        core.bin_unique(dsa.from_array(x, chunks=CHUNK), dsa.from_array(y, chunks=CHUNK), values=dsa.from_array(v, chunks=CHUNK),
                        bins=edges, axis=(1,))
    except ValueError as err:
        assert "distinct values of several chunks cannot be merged" in str(err)
    else:
        raise AssertionError("a cut reduced axis was accepted")
    print("BIN-UNIQUE-DASK-OK")


if __name__ == "__main__":
    main()
