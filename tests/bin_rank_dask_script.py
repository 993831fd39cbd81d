"""The dask branch of bin_rank, run by tests/test_gpu_bin_rank.py in an interpreter that has dask: inputs chunked along the
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
import bin_rank_oracle as ro  # noqa: E402
import map_oracle as mo  # noqa: E402
from xhistogram_amd import core  # noqa: E402

SHAPE = (4, 40, 50)
CHUNK = (2, 20, 25)


def want_of(idx, v, axis, *mode):
    """the oracle's ranks in the inputs' shape: rows over the kept axes, moved back"""
    flat = ro.rank_rows(bo.rows_of(idx, axis), bo.rows_of(v, axis), 40, *mode)
    if axis is None:
        return flat.reshape(idx.shape)
    red = sorted(axis)
    kept = [i for i in range(idx.ndim) if i not in red]
    full = flat.reshape([idx.shape[i] for i in kept] + [idx.shape[i] for i in red])
    return np.moveaxis(full, range(len(kept), idx.ndim), red)


def main():
    dask.config.set(scheduler="threads")
    rng = np.random.default_rng(13)
    edges = [np.linspace(-1, 1, 9), np.sort(rng.uniform(-1, 1, 6))]
    x, y = rng.uniform(-1.2, 1.2, (2,) + SHAPE)
    v = rng.integers(-5, 6, SHAPE).astype(np.float32)  # (many ties)
    v[rng.random(SHAPE) < 0.05] = np.nan
    idx = mo.index([x, y], edges)
    cases = ((None, ("average", False, False)), ((1, 2), ("max", True, True)), ((0,), ("dense", False, True)), ((2,), ("ordinal", True, False)),
             ((2, 0), ("min", False, True)))
    for axis, mode in cases:
        red = tuple(range(3)) if axis is None else axis
        chunks = tuple(SHAPE[i] if i in red else CHUNK[i] for i in range(3))
        dx, dy, dv = (dsa.from_array(a, chunks=chunks) for a in (x, y, v))
        kw = dict(bins=edges, axis=axis, method=mode[0], descending=mode[1], pct=mode[2])
        rank, e = core.bin_rank(dx, dy, values=dv, **kw)
        assert isinstance(rank, dsa.Array) and rank.shape == SHAPE and rank.dtype == np.float64 and all(isinstance(b, np.ndarray) for b in e)
        want = want_of(idx, v, axis, *mode)
        mo.assert_bits(rank.compute(), want, "dask axis=%s" % (axis,))
        mo.assert_bits(core.bin_rank(x, y, values=v, **kw)[0], want, "numpy axis=%s" % (axis,))
    try:
        core.bin_rank(dsa.from_array(x, chunks=CHUNK), dsa.from_array(y, chunks=CHUNK), values=dsa.from_array(v, chunks=CHUNK), bins=edges,
                      axis=(1,))
    except ValueError as err:
        assert "ranks of several chunks cannot be merged" in str(err)
    else:
        raise AssertionError("a cut reduced axis was accepted")
    print("BIN-RANK-DASK-OK")


if __name__ == "__main__":
    main()
