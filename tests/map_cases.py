"""The case tables of tests/test_gpu_map.py, and the data whose statistics are exact: plain numpy, so that tests/test_map_cpu.py
holds every table to the restated choice of tests/map_oracle.py without a GPU (and without torch), as tests/values_cases.py serves
the statistics' tests.  Below them, what tests/test_gpu_map_properties.py runs: the table drawn for each replayed case of
tests/values_cases.py and what the maps must give on it, the periodic data, table formulas and closed form of the row-chunk
test, and the eight inputs whose joint bins pass 2^32."""
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


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_map_properties.py
# ---------------------------------------------------------------------------------------------------------------------
MAP_STATS = ("mean_var", "mean_var_w")  # the statistics of tests/values_cases.py whose drawn cases the maps replay

# (a) the table of histogram_lookup, drawn from a generator of its own: the case's seed plus a constant, so that the case's
# own stream (tests/values_cases.build) is untouched
TABLE_SEED = 77_003
TABLE_DTYPES = ("float64", "float32", "float16", "int32", "int64", "uint8", "bool")
TABLE_CONTAINERS = ("numpy", "list", "torch_gpu", "torch_cpu", "device")
TABLE_LAYOUTS = ("contiguous", "transposed", "sliced", "broadcast")


def table_shape(case):
    """the shape ``histogram`` gives for a case of tests/values_cases.py: kept axes, then bin axes"""
    ndim = len(case["shape"])
    red = set(range(ndim)) if case["axis"] is None else {a % ndim for a in case["axis"]}
    return tuple(n for i, n in enumerate(case["shape"]) if i not in red), tuple(len(e) - 1 for e in case["edges"])


def table_draw(case):
    """(spec, allocation, view, float64 image) of the case's table.  The values are values_exact.grid's at the table's dtype
    (float16 rounds them, uint8 wraps them, bool tells zero from the rest: the image is whatever the view holds, as float64).
    The view lies in the 1-D allocation as its layout says: contiguous, the transpose of a block stored with its axes
    reversed, every second element along every axis of a block twice the size, or read-only at stride 0 along a kept axis
    (np.broadcast_to; a table without kept axes is contiguous then).  spec: dtype, container, layout (as drawn) and
    `laid` (the layout the view has); a nested list has no layout and cannot say a shape with a leading 0, so a table whose
    list would lose its shape stays a numpy array (`container` says which it is)."""
    kept, bins = table_shape(case)
    shape = kept + bins
    rng = np.random.default_rng(case["seed"] + TABLE_SEED)
    dtype, container, layout = (TABLE_DTYPES[int(rng.integers(0, 7))], TABLE_CONTAINERS[int(rng.integers(0, 5))],
                                TABLE_LAYOUTS[int(rng.integers(0, 4))])
    laid = "contiguous" if layout == "broadcast" and not kept else layout
    ax = int(rng.integers(0, len(kept))) if kept else 0
    drawn = tuple(1 if laid == "broadcast" and i == ax else n for i, n in enumerate(shape))
    x = vx.grid(rng, drawn, np.float64 if dtype == "float16" else dtype)
    x = x.astype(dtype) if dtype == "float16" else x
    if laid == "transposed":
        buf = np.ascontiguousarray(x.T).reshape(-1)
        view = buf.reshape(drawn[::-1]).T
    elif laid == "sliced":
        big = np.resize(x.reshape(-1)[::-1], [2 * n for n in drawn]).astype(x.dtype) if x.size else np.zeros([2 * n for n in drawn], x.dtype)
        cut = tuple(slice(None, None, 2) for _ in drawn)
        big[cut] = x
        buf, view = big.reshape(-1), big[cut]
    else:
        buf = x.reshape(-1).copy()
        view = buf.reshape(drawn)
        if laid == "broadcast":
            view = np.broadcast_to(view, shape)
    if container == "list" and np.shape(view.tolist()) != shape:
        container = "numpy"
    image = np.ascontiguousarray(view).astype(np.float64)
    return dict(dtype=dtype, container=container, layout=layout, laid=laid), buf, view, image


def expectations(built):
    """what the maps must give on a built case of tests/values_cases.py (mean_var or mean_var_w), from the contiguous host
    copies: index; anomaly = float64(v) - the exact mean of the sample's bin (the case's weights included); var, bound: the
    sample's bin's var* and its bound at the case's ddof (map_oracle.variance_star), NaN where the sample is not counted"""
    case, d, edges, axis = built.case, built.d, built.edges, built.case["axis"]
    xs, v = built.host[:d], built.host[d]
    w = built.host[d + 1] if case["weights"] else None
    mean = mo.exact_mean(xs, edges, v, axis, w)
    var, b = mo.variance_star(xs, edges, v, axis, case["params"]["ddof"], w)
    return dict(index=mo.index(xs, edges), mean=mean, anomaly=mo.anomaly(xs, edges, v, mean, None, axis), var_table=var,
                var=mo.lookup(xs, edges, var, axis), bound=mo.lookup(xs, edges, b, axis))


# (d) more rows than one launch takes: rows are grouped views of small periodic arrays, the tables are formulas of the row
ROWS_COLS, ROWS_BINS = 3, 2  # (they differ, and neither is 1: a swapped or missing factor of the row advance shows)
P_S, P_V = 251, 127  # the periods of the samples and of the values, coprime
ROWS_EXTRA = 4099
ROW_CASES = [("fast", "index"), ("fast", "take"), ("fast", "anomaly"), ("generic", "index"), ("generic", "take"), ("generic", "anomaly")]
SCALE_LUT = np.array([2.0 ** k for k in range(-4, 4)])


def launch_rows(block, segs):
    """the rows of one launch (values_geometry): below 2^31 workgroups and 2^32 lanes"""
    return min((1 << 31) - 1, ((1 << 32) - 1) // block) // segs


def rows_data(family, op):
    """(edges, samples [P_S, 3], values [P_V, 3] or None) of a ROW_CASES case: float64 samples for the fast family (float64
    values) and for the generic anomaly (int32 values, another type than the samples'), int64 samples on int64 edges for
    the generic index and take.  About a third of the samples lie outside the edges; float ones are NaN now and then, and
    some lie on an edge."""
    rng = np.random.default_rng(900 + ROW_CASES.index((family, op)))
    if family == "generic" and op != "anomaly":
        edges = [np.array([0, 5, 10], np.int64)]
        xs = rng.integers(-3, 14, (P_S, ROWS_COLS)).astype(np.int64)
        xs.reshape(-1)[:3] = [0, 5, 10]
    else:
        edges = [np.array([0.0, 0.5, 1.0])]
        xs = rng.uniform(-0.25, 1.25, (P_S, ROWS_COLS))
        flat = xs.reshape(-1)
        flat[:5] = [0.0, 0.5, 1.0, -0.0, np.nan]
        flat[rng.integers(5, flat.size, 40)] = np.nan
    vs = None
    if op == "anomaly":
        vs = vx.grid(rng, (P_V, ROWS_COLS), np.float64 if family == "fast" else np.int32)
        if family == "fast":
            vs.reshape(-1)[rng.integers(0, vs.size, 20)] = np.nan
    return edges, xs, vs


def _f64(xp, a):
    return a.astype(np.float64) if xp is np else a.double()


def centre_of(xp, r, b):
    """centre[r, b]: a multiple of 2^-3 below 2^10 in magnitude that depends on the row and on the bin (r, b: integer arrays
    of numpy or tensors of torch, which broadcast)"""
    return _f64(xp, (r % 1021) * 3 + b * 1000 - 2000) * 0.125


def scale_of(xp, r, b, lut):
    """scale[r, b]: a power of two 2^-4 .. 2^3 that depends on both (lut: SCALE_LUT where r and b are)"""
    return lut[(r + 3 * b) % 8]


def rows_expected(xp, op, rows, bin_base, v_base, lut=None):
    """the closed form of the [len(rows), 3] block of the given rows: bin_base [P_S, 3] the bins of the periodic samples
    (map_oracle.index, -1: not counted), v_base [P_V, 3] the periodic values as float64, lut: SCALE_LUT for an anomaly with a
    scale table (None: none).  Row r reads samples row r mod P_S, values row r mod P_V and the table rows centre_of(r, .),
    scale_of(r, .).  Values on the grid minus a multiple of 2^-3 below 2^10 is exact, and so is a division by a power of
    two: the result does not depend on the instruction or the order that computes it."""
    b = bin_base[rows % P_S]
    if op == "index":
        return b
    ok = b >= 0
    at = xp.where(ok, b, b * 0)
    r = rows[:, None]
    val = centre_of(xp, r, at)
    if op == "anomaly":
        val = v_base[rows % P_V] - val
        if lut is not None:
            val = val / scale_of(xp, r, at, lut)
    return xp.where(ok, val, val + float("nan"))


# (e) joint bins beyond 32 bits
JOINT_D, JOINT_BINS, JOINT_N = 8, 17, 4099


def joint_inputs():
    """(edges, samples) of 8 float64 inputs of 4099 samples on 17 bins each: 17^8 = 6 975 757 441 joint bins.  Every input draws
    its bins uniformly, so the counted indices lie on both sides of 2^32 (the first input's bin decides: 17^7 * 10.47 = 2^32);
    samples 0 and 1 are the indices 2^32 - 1 and 2^32 themselves, 2 and 3 the first and the last bin of all; every input
    drops samples of its own (below, above, NaN), and on those no other input does"""
    rng = np.random.default_rng(1708)
    edges = [np.linspace(d, d + 8.5, JOINT_BINS + 1) for d in range(JOINT_D)]
    bins = rng.integers(0, JOINT_BINS, (JOINT_D, JOINT_N))
    for i, flat in enumerate(((1 << 32) - 1, 1 << 32, 0, JOINT_BINS ** JOINT_D - 1)):
        bins[:, i] = np.unravel_index(flat, (JOINT_BINS,) * JOINT_D)
    xs = []
    for d in range(JOINT_D):
        x = edges[d][bins[d]] + 0.25 * rng.uniform(0.0, 1.0, JOINT_N)  # (bins are 0.5 wide)
        own = 8 + 24 * d + np.arange(24)  # (this input's own dropped samples)
        x[own] = np.resize([edges[d][0] - 0.25, edges[d][-1] + 0.25, np.nan], 24)
        xs.append(x)
    return edges, xs
