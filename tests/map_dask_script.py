"""The dask branches of bin_index, histogram_lookup and histogram_anomaly, run by tests/test_gpu_map.py in an interpreter that has
dask: chunked inputs, several chunks along kept and reduced axes, give what the numpy call gives bit for bit.

Index and lookup are per-sample work, so any chunking gives the same bits.  The anomaly goes through the lazy
histogram_mean_var, whose partials meet in Chan's merge, and its unchunked twin adds with float64 atomics in any order: both
repeat their bits only on data whose sums are exact.  So the anomaly's data are built per axis choice (map_cases.pow2_data): one
chunk whose bins, per output row, hold a power-of-two count of values on the grid of tests/values_exact.py, repeated 2 x 2 x 2
times.  Every partial of a bin then has the same count, mean and M2: the merge's correction d * nb / n is exactly 0, k * M2 is
exact, and mean, M2 and var of the merged result are the unchunked call's bit for bit (counts up to 16 * 8 = 128: within the
2^9 of values_exact).  Weights are a power of two that depends on the bin alone, so W, the weighted mean and M2 stay exact too."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dask  # noqa: E402
import dask.array as dsa  # noqa: E402

import map_cases as mc  # noqa: E402
import map_oracle as mo  # noqa: E402
import values_exact as vx  # noqa: E402
from xhistogram_amd import core  # noqa: E402

CHUNK = (2, 20, 25)
TILES = (2, 2, 2)


def index_and_lookup(rng):
    """two inputs, any data: every axis choice, a numpy table and a dask table whose bin axes come in two chunks"""
    edges = [np.linspace(-1, 1, 9), np.sort(rng.uniform(-1, 1, 6))]
    x, y = rng.uniform(-1.2, 1.2, (2,) + tuple(c * t for c, t in zip(CHUNK, TILES)))
    dx, dy = (dsa.from_array(a, chunks=CHUNK) for a in (x, y))
    want, _ = core.bin_index(x, y, bins=edges)
    got, e = core.bin_index(dx, dy, bins=edges)
    assert isinstance(got, dsa.Array) and got.chunks == dx.chunks and all(isinstance(b, np.ndarray) for b in e)
    mo.assert_bits(got.compute(), want, "dask bin_index")
    mo.assert_bits(want, mo.index([x, y], edges), "numpy bin_index")
    for axis in (None, (1, 2), (0,), (2,), (0, 2)):
        red = tuple(range(3)) if axis is None else axis
        kept = tuple(s for i, s in enumerate(x.shape) if i not in red)
        table = vx.grid(rng, kept + (8, 5))
        want, _ = core.histogram_lookup(x, y, table=table, bins=edges, axis=axis)
        mo.assert_bits(want, mo.lookup([x, y], edges, table, axis), "numpy lookup axis=%s" % (axis,))
        for t in (table, dsa.from_array(table, chunks=tuple(2 for _ in kept) + (4, 5))):
            got, _ = core.histogram_lookup(dx, dy, table=t, bins=edges, axis=axis)
            assert isinstance(got, dsa.Array) and got.chunks == dx.chunks
            mo.assert_bits(got.compute(), want, "dask lookup axis=%s" % (axis,))


def anomalies(rng):
    """plain and standardized, unweighted with ddof 0 and weighted with ddof 1: dask against the numpy call, and both against
    the composition of the numpy histogram_mean_var with the lookup"""
    edges = [np.linspace(-1.0, 1.0, 9)]
    for axis in (None, (1, 2), (0,), (2,), (0, 2)):
        bx, bv = mc.pow2_data(rng, CHUNK, edges[0], axis)
        x, v = np.tile(bx, TILES), np.tile(bv, TILES)
        w = 2.0 ** (np.maximum(mo.index([x], edges), 0) % 3)  # 1, 2 or 4, the same for every sample of a bin
        dx, dv, dw = (dsa.from_array(a, chunks=CHUNK) for a in (x, v, w))
        for weights, dweights, ddof in ((None, None, 0), (w, dw, 1)):
            what = "axis=%s weights=%s ddof=%d" % (axis, weights is not None, ddof)
            n, mean, var, _ = core.histogram_mean_var(x, values=v, bins=edges, axis=axis, weights=weights, ddof=ddof)
            assert (n > ddof).any() and np.isfinite(var).any(), what
            mo.assert_bits(mean.reshape(-1, 8), mo.exact_mean([x], edges, v, axis, weights), "mean " + what)
            centre = mo.lookup([x], edges, mean, axis)
            with np.errstate(invalid="ignore", divide="ignore"):
                parts = {False: v - centre, True: (v - centre) / mo.lookup([x], edges, np.sqrt(var), axis)}
            for standardize in (False, True):
                kw = dict(bins=edges, axis=axis, ddof=ddof, standardize=standardize)
                want, _ = core.histogram_anomaly(x, values=v, weights=weights, **kw)
                mo.assert_bits(want, parts[standardize], "numpy anomaly against its parts, z=%s %s" % (standardize, what))
                got, _ = core.histogram_anomaly(dx, values=dv, weights=dweights, **kw)
                assert isinstance(got, dsa.Array) and got.chunks == dx.chunks
                mo.assert_bits(got.compute(), want, "dask anomaly z=%s %s" % (standardize, what))
            # the z-scores are not all NaN or inf, so the check above bites (but over axis 0 alone: a row of a chunk is 2 samples
            # in 2 bins, the repeats bring equal values, every variance is 0 and every z-score 0 / 0)
            assert np.isfinite(parts[True]).any() or axis == (0,), what


def main():
    dask.config.set(scheduler="threads")
    rng = np.random.default_rng(11)
    index_and_lookup(rng)
    anomalies(rng)
    print("MAP-DASK-OK")


if __name__ == "__main__":
    main()
