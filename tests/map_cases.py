"""The case tables of tests/test_gpu_map.py, and the data whose statistics are exact: plain numpy, so that tests/test_map_cpu.py
holds every table to the restated choice of tests/map_oracle.py without a GPU (and without torch), as tests/values_cases.py serves
the statistics' tests."""
import numpy as np

import map_oracle as mo
import values_exact as vx

F64, F32 = np.float64, np.float32

# family x digitize form of the fast family: (edge kind, bins per input for D = 1, 2) per op class and sample type, and what the
# plan makes of them (fine, arith).  The arithmetic kernels run only where the fine tables and the table rows no longer fit LDS
# together: bin_index keeps no row, so its fine tables alone must pass 160 KiB (tests/test_map_cpu.py checks every entry).
ARITH_BINS = {  # (op class, sample type) -> bins per input for D = 1, 2
    ("index", F64): ((19_000,), (2, 19_000)), ("index", F32): ((37_000,), (2, 37_000)),
    ("table", F64): ((9_500,), (3, 6_000)), ("table", F32): ((12_500,), (3, 6_000)),
    ("scaled", F64): ((9_500,), (3, 3_000)), ("scaled", F32): ((9_000,), (3, 3_000)),
}
FAST_FORMS = {
    "k1": lambda cls, st: ("k1", ((300,), (24, 30)), 1, False),
    "k2": lambda cls, st: ("k2", ((300,), (24, 30)), 2, False),
    "arith": lambda cls, st: ("lin", ARITH_BINS[(cls, st)], 1, True),
}


def fast_form(form, op, st, D, scaled=False):
    """(edge kind, bins per input, fine, arith) of a fast case: `scaled`, an anomaly with a scale table"""
    cls = "index" if op == "index" else "scaled" if scaled else "table"
    kind, (nb1, nb2), fine, arith = FAST_FORMS[form](cls, st)
    return kind, (nb1 if D == 1 else nb2), fine, arith


def fast_shapes(st, D):
    """(rows, cols) around the fast tile: cols in {1, 3, tile - 1, tile, tile + 1, 2 tile + 5}, rows in {1, 3}"""
    t = mo.tile_of(st, D)
    return [(1, 1), (3, 3), (1, t - 1), (3, t), (1, t + 1), (3, 2 * t + 5)]


GENERIC_SHAPES = [(1, 511), (3, 512), (1, 513), (3, 1500)]  # around the generic block of 512

# the generic family's table homes: 1-D bins, whether a scale table comes with them
HOMES = {"lds": (200, False), "global_l2": (30_000, False), "global_scale": (12_000, True)}
# the (op, home) pairs that exist: only the anomaly takes a scale table
GENERIC_CASES = [(op, home) for op in mo.OPS for home, (_, scale) in HOMES.items() if op == "anomaly" or not scale]

AXES = [None, (2,), (1,), (0, 2), (0,)]


def pow2_data(rng, shape, edges, axis, dt=F64):
    """samples whose bins (per output row over `axis`) hold 1, 2, 4, 8 or 16 of them, the rest outside the range or NaN, and
    grid values: the mean and M2 of every bin are exact sums, so histogram_mean_var gives the same bits on every run"""
    nd = len(shape)
    red = list(range(nd)) if axis is None else sorted(np.atleast_1d(axis) % nd)
    kept = [i for i in range(nd) if i not in red]
    m = int(np.prod([shape[i] for i in kept], dtype=np.int64))
    c = int(np.prod([shape[i] for i in red]))
    mids = 0.5 * (edges[:-1] + edges[1:])
    rows = []
    for r in range(m):
        kmax = min(4, int(np.log2(max(1, c // len(mids)))))  # (the largest count that still fits a row of c samples)
        counts = 1 << rng.integers(0, kmax + 1, len(mids))
        x = np.repeat(mids, counts)[:c] if c < len(mids) else np.repeat(mids, counts)
        assert len(x) <= c, (len(x), c)
        pad = rng.choice([np.nan, edges[0] - 1.0, edges[-1] + 1.0, np.inf], c - len(x))
        rows.append(rng.permutation(np.concatenate([x, pad])))
    x = np.array(rows).reshape([shape[i] for i in kept] + [shape[i] for i in red])
    x = np.ascontiguousarray(np.transpose(x, np.argsort(kept + red))).astype(dt)
    return x, vx.grid(rng, shape, dt)
