"""Random cases for the ten per-bin statistics of values: one plain function of a numpy Generator per kind of decision
the Python front of those statistics takes (core._value_views and what it calls), `case_of`, which makes a case of them from
one seed, the one hypothesis strategy `cases(stat)`, which draws that seed, and one builder.  No GPU and no test functions here:
tests/test_values_cases_cpu.py holds the generator to its conditions and tests/test_gpu_values_properties.py runs the cases.

A case is a dict of plain values (its repr is the whole case), made by `case_of(stat, seed)`:
  - D = 1..3 sample arrays of ndim 1..4, leading extents 1..7, last extent 1..300, sometimes one extent 0; `axis` None or a
    non-empty subset of the axes in any order, some of them negative; rows x bins at most 4096 (rows: the kept extents);
  - a sample dtype per array; the four edge kinds of test_gpu_properties._edges, 1..12 bins per dimension;
  - what the values are made of (VALUE_KINDS: only what the statistic's exact check takes), the dtype of the weights;
  - a layout PER ARRAY (samples, values, second values, weights), a backend, the statistic's per-call parameters, a seed.
`build(case)` draws the data from the seed: samples relative to the edges (`edge_relative`), values and weights on the exactly
summable grids of tests/values_exact.py and tests/skew_kurt_exact.py, every array laid out as its layout says.  A laid-out
array equals its contiguous copy by value, only the strides differ; the oracles read the contiguous copies (`Built.host`),
the library reads `Built.inputs(backend)`."""
import numpy as np

import skew_kurt_exact as sx
import values_exact as vx

STATS = ("extrema", "argextrema", "mean_var", "mean_var_w", "cov", "cov_w", "skew_kurt", "skew_kurt_w", "quantile", "quantile_w")
WEIGHTED = ("mean_var_w", "cov_w", "skew_kurt_w", "quantile_w")
PAIRS = ("cov", "cov_w")
WITH_DDOF = ("mean_var", "mean_var_w", "cov", "cov_w", "skew_kurt", "skew_kurt_w")
NARROW = ("skew_kurt", "skew_kurt_w")  # values on skew_kurt_exact's narrow grid, a subset of values_exact's
SAMPLE_DTYPES = ("float64", "float32", "int32", "int64")
EDGE_KINDS = ("uniform", "random", "duplicates", "geometric")
LAYOUTS = ("contiguous", "permuted", "sliced_all", "sliced_one", "offset", "broadcast", "negative")  # negative: numpy only
BACKENDS = ("numpy", "torch", "device")
METHODS = ("linear", "lower", "higher", "midpoint", "nearest")
SMALL_INT_DTYPES = ("int8", "uint8", "int16", "int32", "int64", "float16", "bool")
WEIGHT_DTYPES = ("float64", "float32", "float16", "int8", "uint8", "int16", "int32", "int64")
_GRID = tuple("grid:" + d for d in ("float64", "float32")) + tuple("small:" + d for d in SMALL_INT_DTYPES)
# extrema and argextrema order anything: +-inf and +-0.0 among the values, and int64 near 2^62, which astype(float64) ties
_ANY = _GRID + ("special:float64", "special:float32", "big:int64")
VALUE_KINDS = {s: (_ANY if s in ("extrema", "argextrema") else _GRID) for s in STATS}
MAX_OUT = 4096  # rows x bins: keeps the per-bin Python loops of the oracles short
# Mixed into every case's seed.  60 independent cases hold an extent 0 (one case in twenty) with probability 0.95 and more
# than six cases that count nothing with probability 0.05, per statistic, so some values of the salt miss a condition of
# tests/test_values_cases_cpu.py for some statistic.  With this one, the first of 0..59 that leaves a margin everywhere, every
# enumerated choice is drawn at least twice per statistic and at most 5 of a statistic's 60 cases count nothing (6 allowed).
# Whatever changes the stream of choices (an edit to case_of or to a function it calls, another numpy Generator) moves the
# examples: if that CPU file then fails, look for the next salt that passes it (set SALT, run the file) and update the tallies
# in the docstring of tests/test_gpu_values_properties.py.
SALT = 49


def edge_relative(rng, shape, edges, dtype, specials=True):
    """samples that meet the edges whatever the edges are: uniform over the edge span (at least 1 wide, about the edges' middle)
    widened by a tenth on each side, a quarter of them (at least one) on an edge value; integer dtypes rounded; float ones with NaN, +-inf,
    +-0.0 and the first and last edge on about 1/17 of the positions (`specials`)"""
    e = np.asarray(edges, np.float64)
    dt = np.dtype(dtype)
    lo, hi = float(e[0]), float(e[-1])
    span = max(hi - lo, 1.0)
    mid = 0.5 * (lo + hi)
    x = rng.uniform(mid - 0.6 * span, mid + 0.6 * span, shape)
    flat = x.reshape(-1)
    if flat.size:  # (a quarter, and at least one: the one sample of a (1,) array meets an edge)
        on = rng.permutation(flat.size)[: max(1, (flat.size + 2) // 4)]
        flat[on] = rng.choice(e, on.size)
    if dt.kind != "f":
        return np.clip(np.rint(x), np.iinfo(dt).min, np.iinfo(dt).max).astype(dt)
    x = x.astype(dt)
    if specials:
        sprinkle(rng, x, 17, [np.nan, np.inf, -np.inf, 0.0, -0.0, lo, hi])
    return x


def sprinkle(rng, x, every, specials):
    """one of `specials` on about one position in `every` of the float array x, each position on its own: an array of one
    or two samples is not all special values"""
    at = rng.random(x.shape) < 1.0 / every
    x[at] = rng.choice(np.array(specials), int(at.sum())).astype(x.dtype)


# ---------------------------------------------------------------------------------------------------------------------
# one function per kind of decision, and the strategy that draws a case
#
# A case is decided by ONE drawn integer, the seed of the numpy generator the functions below read.  Hypothesis fills five
# examples in six of its generate phase with mutants of the example before (it copies one span of choices over another of the
# same label: engine.generate_mutations_from), so a strategy that draws every decision on its own gives, in 60 examples, about
# 18 independent cases and chains of near-copies: not every layout, dtype and method appears, and one empty case begets five.
# A single drawn integer leaves nothing to copy: every example is a case of its own.
# ---------------------------------------------------------------------------------------------------------------------
def pick(rng, options):
    return options[int(rng.integers(0, len(options)))]


def shape_of(rng):
    """ndim 1..4, leading extents 1..7, the last 1..300; about one in twenty has an extent 0"""
    ndim = int(rng.integers(1, 5))
    shape = [int(rng.integers(1, 8)) for _ in range(ndim - 1)] + [int(rng.integers(1, 301))]
    if rng.integers(0, 20) == 0:
        shape[int(rng.integers(0, ndim))] = 0
    return shape


def axis_of(rng, ndim):
    """None, or a non-empty subset of the axes in any order (permutations, not combinations), each as itself or negative"""
    if rng.integers(0, 6) == 0:
        return None
    order = rng.permutation(ndim)[: int(rng.integers(1, ndim + 1))]
    return tuple(int(a) - ndim if rng.integers(0, 2) else int(a) for a in order)


def edges_of(rng, kind, n):
    """n bins of one of the four kinds of test_gpu_properties._edges, restated for a numpy generator"""
    if kind == "uniform":
        lo = rng.uniform(-5, 0)
        return np.linspace(lo, lo + rng.uniform(0.5, 9), n + 1)
    if kind == "random":
        return np.sort(rng.uniform(-4, 4, n + 1).astype(np.float32).astype(np.float64))
    if kind == "duplicates":
        return np.sort(np.round(rng.uniform(-3, 3, n + 1), 0))
    # geometric: tiny and huge bins together
    return np.concatenate([[-4.0], -4.0 + np.cumsum(np.geomspace(1e-9, 4.0, n))])


def layout_of(rng, ndim, backend, samples=False):
    """how one array lies in memory; a negative stride only where the backend has them (numpy).  samples: a sample array is
    broadcast along some of its axes, never along all of them (one sample value for the whole array counts nothing too often)"""
    kind = pick(rng, LAYOUTS if backend == "numpy" else LAYOUTS[:-1])
    if samples and kind == "broadcast" and ndim == 1:
        kind = "contiguous"
    lay = {"kind": kind}
    if kind == "permuted":  # (Fortran order: the reversed axes)
        lay["perm"] = tuple(reversed(range(ndim))) if rng.integers(0, 2) else tuple(int(a) for a in rng.permutation(ndim))
    elif kind in ("sliced_one", "negative"):
        lay["ax"] = int(rng.integers(0, ndim))
    elif kind == "broadcast":  # stride 0 along these axes; `expanded`: handed over at full shape, else at extent 1 / lower rank
        lay["axes"] = tuple(sorted(int(a) for a in rng.permutation(ndim)[: int(rng.integers(1, ndim if samples else ndim + 1))]))
        lay["expanded"] = bool(rng.integers(0, 2))
    return lay


def quantile_levels_of(rng):
    """q: a scalar or a list of 1..3 numbers in [0, 1], 0 and 1 among them now and then"""
    def one():
        return pick(rng, (0.0, 1.0, 0.5)) if rng.integers(0, 3) == 0 else float(rng.random())
    return one() if rng.integers(0, 2) else [one() for _ in range(int(rng.integers(1, 4)))]


def params_of(rng, stat):
    """the statistic's per-call parameters"""
    p = {}
    if stat in WITH_DDOF:
        p["ddof"] = int(rng.integers(0, 3))
    if stat in NARROW:
        p["bias"] = bool(rng.integers(0, 2))
        p["fisher"] = bool(rng.integers(0, 2))
    if stat in ("quantile", "quantile_w"):
        p["q"] = quantile_levels_of(rng)
    if stat == "quantile":
        p["method"] = pick(rng, METHODS)
    return p


def kept_rows(shape, axis):
    ndim = len(shape)
    red = set(range(ndim)) if axis is None else {a % ndim for a in axis}
    return int(np.prod([shape[i] for i in range(ndim) if i not in red], dtype=np.int64))


def sample_dtype_of(rng, edges):
    """one of SAMPLE_DTYPES; an integer dtype only where an integer lies inside the edges (rounded samples would meet no bin)"""
    dt = pick(rng, SAMPLE_DTYPES)
    return dt if dt.startswith("float") or np.ceil(edges[0]) <= np.floor(edges[-1]) else "float64"


def case_of(stat, entropy):
    rng = np.random.default_rng([entropy, STATS.index(stat), SALT])
    backend = pick(rng, BACKENDS)
    d = int(rng.integers(1, 4))
    shape = shape_of(rng)
    ndim = len(shape)
    axis = axis_of(rng, ndim)
    kinds = tuple(pick(rng, EDGE_KINDS) for _ in range(d))
    edges = [edges_of(rng, k, int(rng.integers(1, 13))) for k in kinds]
    # rows x bins <= MAX_OUT: halve the largest kept extent, then the longest edge array, until it holds
    red = set(range(ndim)) if axis is None else {a % ndim for a in axis}
    while kept_rows(shape, axis) > MAX_OUT:
        i = max((i for i in range(ndim) if i not in red), key=lambda i: shape[i])
        shape[i] = (shape[i] + 1) // 2
    while kept_rows(shape, axis) * int(np.prod([len(e) - 1 for e in edges])) > MAX_OUT:
        j = max(range(d), key=lambda j: len(edges[j]))
        edges[j] = edges[j][: (len(edges[j]) + 2) // 2]
    n_arrays = d + (2 if stat in PAIRS else 1) + (1 if stat in WEIGHTED else 0)
    return {
        "stat": stat, "backend": backend, "shape": tuple(shape), "axis": axis,
        "sample_dtypes": tuple(sample_dtype_of(rng, e) for e in edges),
        "edge_kinds": kinds, "edges": [e.tolist() for e in edges],
        "values": tuple(pick(rng, VALUE_KINDS[stat]) for _ in range(2 if stat in PAIRS else 1)),
        "weights": pick(rng, WEIGHT_DTYPES) if stat in WEIGHTED else None,
        "layouts": [layout_of(rng, ndim, backend, samples=i < d) for i in range(n_arrays)],
        "params": params_of(rng, stat),
        "seed": int(rng.integers(0, 2**31 - 1)),
    }


def cases(stat):
    """the strategy of one statistic's cases.  The seed is drawn as eight bytes, not as an integer: hypothesis now and then
    hands out the integer constants it finds in whatever project modules happen to be imported, which made a few of the
    examples depend on the tests that ran before; it finds no eight-byte constants.  (hypothesis is imported here, not at
    the top: the test files that import this module keep their own importorskip.)"""
    import hypothesis.strategies as st

    return st.binary(min_size=8, max_size=8).map(lambda b: case_of(stat, int.from_bytes(b, "little")))


# ---------------------------------------------------------------------------------------------------------------------
# the builder
# ---------------------------------------------------------------------------------------------------------------------
def reduced_axes(case):
    ndim = len(case["shape"])
    return tuple(range(ndim)) if case["axis"] is None else tuple(a % ndim for a in case["axis"])


def _drawn_shape(shape, lay):
    """the shape the data of one array is drawn at: extent 1 along the axes its layout broadcasts"""
    if lay["kind"] != "broadcast":
        return tuple(shape)
    return tuple(1 if i in lay["axes"] else n for i, n in enumerate(shape))


def _filler(x, shape):
    """an array of `shape` and x's dtype holding x's values in another order: what a wrong stride would read"""
    return np.resize(x.reshape(-1)[::-1], shape).astype(x.dtype) if x.size else np.zeros(shape, x.dtype)


def lay_out(x, lay, shape, keep_rank=False):
    """(the 1-D allocation, the view of it that `lay` describes) for contiguous data x of _drawn_shape(shape, lay); the view
    equals x by value (and broadcasts to `shape`).  keep_rank: a broadcast array is always handed over at full shape."""
    kind = lay["kind"]
    if kind == "permuted":
        p = lay["perm"]
        buf = np.ascontiguousarray(x.transpose(p)).reshape(-1)
        return buf, buf.reshape([x.shape[i] for i in p]).transpose(np.argsort(p))
    if kind in ("sliced_all", "sliced_one"):
        which = range(x.ndim) if kind == "sliced_all" else (lay["ax"],)
        big = _filler(x, [2 * n if i in which else n for i, n in enumerate(x.shape)])
        cut = tuple(slice(None, None, 2) if i in which else slice(None) for i in range(x.ndim))
        big[cut] = x
        return big.reshape(-1), big[cut]
    if kind == "offset":  # one element off the allocation's start: misaligned row starts
        buf = np.concatenate([_filler(x, (1,)), x.reshape(-1)])
        return buf, buf[1:].reshape(x.shape)
    if kind == "negative":
        buf = np.ascontiguousarray(np.flip(x, lay["ax"])).reshape(-1)
        return buf, np.flip(buf.reshape(x.shape), lay["ax"])
    buf = x.reshape(-1).copy()
    a = buf.reshape(x.shape)
    if kind == "broadcast":
        if lay["expanded"] or keep_rank:
            return buf, np.broadcast_to(a, shape)
        while a.ndim > 1 and a.shape[0] == 1:  # a lower-rank array: the leading axes are the library's to add
            a = a[0]
    return buf, a


def _with_nans(rng, v, every=17):
    if v.dtype.kind == "f" and every:
        sprinkle(rng, v, every, [np.nan])
    return v


def draw_values(rng, shape, kind, narrow, nans=17):
    """values of one kind ("what:dtype") at `shape`: exactly summable for the moment statistics, any order for the extrema;
    NaN on about one position in `nans` of a float array (0: none)"""
    what, name = kind.split(":")
    dt = np.dtype(name)
    if what in ("grid", "special"):
        v = (sx.narrow if narrow else vx.grid)(rng, shape, dt)
        if what == "special":
            sprinkle(rng, v, 9, [np.inf, -np.inf, 0.0, -0.0])
        return _with_nans(rng, v, nans)
    if what == "big":  # float64 is 1024 apart here: neighbours tie once converted, and the first holder as float64 counts
        return (rng.choice(np.array([-1, 1]), shape) * ((1 << 62) + rng.integers(-3000, 3000, shape))).astype(np.int64)
    top = (sx.K_MAX if narrow else 1 << 7) - 1
    if dt.kind == "b":
        return rng.integers(0, 2, shape).astype(dt)
    k = rng.integers(0 if dt.kind == "u" else -top, top + 1, shape)
    return _with_nans(rng, k.astype(dt), nans)


class Built:
    """one case's arrays.  `host`: the contiguous copies at full shape, samples..., values[, second values][, weights] (what
    the oracles read); `views`: the same arrays laid out in host memory, each on `bufs`' allocation of its own; `edges`"""

    def __init__(self, case, edges, bufs, views, host):
        self.case, self.edges, self.bufs, self.views, self.host = case, edges, bufs, views, host
        self.d = len(case["sample_dtypes"])

    def inputs(self, backend=None):
        """the arrays as the backend's callers hold them: numpy views, torch tensors on the GPU, or DeviceArrays with the
        very strides (and offsets) of the host views"""
        backend = backend or self.case["backend"]
        if backend == "numpy":
            return list(self.views)
        out = []
        for buf, a in zip(self.bufs, self.views):
            item = a.dtype.itemsize
            off = (a.__array_interface__["data"][0] - buf.__array_interface__["data"][0]) // item if a.size else 0
            if backend == "torch":
                import torch

                t = torch.as_tensor(buf).cuda() if buf.size else torch.empty(0, dtype=torch.as_tensor(buf).dtype, device="cuda")
                out.append(t.as_strided(a.shape, [s // item for s in a.strides], off) if a.size else t.new_empty(a.shape))
            else:
                from xhistogram_amd.devicearray import DeviceArray

                dev = DeviceArray.from_numpy(buf if a.size else np.empty(a.shape, a.dtype))
                out.append(DeviceArray(dev.owner, dev.ptr + off * item, a.shape, a.strides, a.dtype, dev.device) if a.size else dev)
        return out

    def call_kwargs(self, arrays):
        """(sample arrays, keyword arguments) of the public call on `arrays` (inputs() or host)"""
        case, d = self.case, self.d
        rest = list(arrays[d:])
        kw = dict(bins=self.edges if d > 1 else self.edges[0], axis=case["axis"], **case["params"])
        if case["stat"] in WEIGHTED:
            kw["weights"] = rest.pop()
        kw["values"] = tuple(rest) if case["stat"] in PAIRS else rest[0]
        return list(arrays[:d]), kw


def plain(case):
    """the case with every array float64 and no NaN or infinity anywhere: what scipy's and numpy's own functions take"""
    return dict(case, sample_dtypes=("float64",) * len(case["sample_dtypes"]), values=("grid:float64",) * len(case["values"]),
                weights="float64" if case["weights"] else None, plain=True)


def build(case):
    rng = np.random.default_rng(case["seed"])
    stat, shape = case["stat"], case["shape"]
    edges = [np.asarray(e, np.float64) for e in case["edges"]]
    d = len(edges)
    drawn = []
    for lay, dt, e in zip(case["layouts"], case["sample_dtypes"], edges):
        drawn.append(edge_relative(rng, _drawn_shape(shape, lay), e, dt, specials=not case.get("plain")))
    for lay, kind in zip(case["layouts"][d:], case["values"]):
        drawn.append(draw_values(rng, _drawn_shape(shape, lay), kind, stat in NARROW, nans=0 if case.get("plain") else 17))
    if stat in WEIGHTED:  # the integers 0..7: every sum of weights and of w * v is exact in any order
        drawn.append(rng.integers(0, 8, _drawn_shape(shape, case["layouts"][-1])).astype(case["weights"]))
    bufs, views = [], []
    for i, (x, lay) in enumerate(zip(drawn, case["layouts"])):
        buf, a = lay_out(x, lay, shape, keep_rank=i < d)
        bufs.append(buf)
        views.append(a)
    host = [np.ascontiguousarray(np.broadcast_to(a, shape)) for a in views]
    return Built(case, edges, bufs, views, host)


# ---------------------------------------------------------------------------------------------------------------------
# the statistic's oracle (tests/*_oracle.py) on host arrays, with the public call's outputs in the public call's order
# ---------------------------------------------------------------------------------------------------------------------
def oracle(stat, arrays, edges, axis, params):
    """arrays: host samples..., values[, second values][, weights] (broadcastable).  The moment statistics run their oracle's
    exact mode: with the values and weights of build() every sum of theirs is exact, so counts, sums of weights and means
    are the library's bit for bit; what the library may round differently (M2 and beyond) is the business of the *_exact.py
    bounds the GPU tests apply."""
    import argextrema_oracle as ao
    import cov_oracle as co
    import cov_weighted_oracle as cwo
    import extrema_oracle as eo
    import meanvar_oracle as mo
    import meanvar_weighted_oracle as mwo
    import quantile_oracle as qo
    import skew_kurt_oracle as so
    import weighted_quantile_oracle as wqo

    d = len(edges)
    args, rest = list(arrays[:d]), list(arrays[d:])
    kw = dict(bins=[np.asarray(e) for e in edges], axis=axis, **params)
    if stat in WEIGHTED:
        kw["weights"] = rest.pop()
    kw["values"] = tuple(rest) if stat in PAIRS else rest[0]
    if stat == "extrema":
        return eo.histogram_extrema(*args, **kw)
    if stat == "argextrema":
        return ao.histogram_argextrema(*args, **kw)
    if stat == "mean_var":
        return mo.histogram_mean_var(*args, exact=True, **kw)
    if stat == "mean_var_w":
        return mwo.histogram_mean_var_w(*args, exact=True, **kw)
    if stat == "cov":
        return co.histogram_cov(*args, exact=True, **kw)
    if stat == "cov_w":
        return cwo.histogram_weighted_cov(*args, exact=True, **kw)
    if stat in NARROW:
        return so.histogram_skew_kurt(*args, **kw)
    if stat == "quantile":
        return (qo.histogram_quantile(*args, **kw),)
    return (wqo.histogram_weighted_quantile(*args, **kw),)
