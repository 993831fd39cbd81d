"""Property and concurrency tests of the ten per-bin statistics of values (histogram_extrema, _argextrema, _mean_var, _cov,
_weighted_cov, _skew_kurt, _quantile, _weighted_quantile and the weighted mean_var and skew_kurt) on an MI355X: what
tests/test_gpu_properties.py is to `histogram`.  The directed files build each case for one launch variant; these walk the
Python front that feeds the launcher (core._value_views, _value_rows, _value_block, _value_stat): which order of the reduced
axes walks memory as one stride, grouped rows, when a layout is copied, stride-0 values and weights, and argextrema's column
order, with samples, values and weights that each have a layout of their own.

(a) test_random_cases_match_oracle[stat]: 60 cases of tests/values_cases.py per statistic (derandomised: the very examples
    tests/test_values_cases_cpu.py replays without a GPU), the public call against the statistic's oracle on the contiguous
    host copies.  Exact outputs (extrema, positions, quantiles, counts, sums of weights, means) bit for bit; M2 and beyond
    through the directed files' own checks (bit for bit where values_exact / skew_kurt_exact say the sums are exact, their
    float64 bounds elsewhere).  No new tolerance.
(b) test_blocks_as_dask_hands_them[stat]: the reduced axes cut into 1..3 chunks, core._value_block on every block of host
    arrays as dask's tasks call it, each block against the oracle on that block; the exact partials (extrema, counts, sums
    of weights) merged as dask.array.reduction(concatenate=True) merges them, against the unchunked block, bit for bit.
(c) test_value_statistics_one_plan_many_threads: 8 threads, a stream and data each, one shared plan, all ten statistics.
(d) test_a_statistic_initialises_the_scratch_it_inherits: the two-pass statistics' `sd` block taken from the scratch cache
    full of set bits, left there by a call on the same and on another stream.

What the 60 examples per statistic of (a) hold (printed by tests/test_values_cases_cpu.py, which asserts that every enumerated
choice is drawn for every statistic; totals over the ten statistics' 600 cases, and the fewest .. most of one statistic):
  cases that count no sample 33 (2 .. 5), 32 of them through an extent 0 (2 .. 5); a bin with two or more counted values in
  539 (51 .. 56); backends numpy 194, torch 222, DeviceArray 184 (each 13 .. 24); ndim 1 / 2 / 3 / 4: 149 / 154 / 150 / 147
  (9 .. 22); D 1 / 2 / 3: 207 / 196 / 197; sample dtypes float64 314, float32 308, int32 287, int64 281 (22 .. 38);
  layouts over the 2150 arrays: contiguous 388, permuted 309, sliced_all 371, sliced_one 334, offset 359, broadcast 286,
  negative 103 (numpy only; 4 .. 20); axis None in 94 cases (6 .. 15), listed out of order in 161 (12 .. 20), with a negative
  number in 314 (25 .. 39); a stride-0 reduced axis of extent > 1 in 191 (11 .. 29); ddof 0 / 1 / 2: 111 / 124 / 125
  (13 .. 25); bias and fisher each way 26 .. 34 times; histogram_quantile's methods linear 14, lower 11, higher 9, midpoint
  13, nearest 13; q a scalar 31 and a list 29 times per quantile statistic, holding 0 or 1 in 25 .. 27 cases; every value
  kind 2 .. 19 times per statistic (+-inf / +-0.0 values 2 .. 6 and int64 near 2^62 3 .. 5 times for extrema and
  argextrema); every dtype of the weights 2 .. 13 times.
A drawn case that failed once stays below as a directed case (DIRECTED), whatever becomes of the strategy."""
import threading

import numpy as np
import pytest

import argextrema_oracle as ao
import values_cases as vc
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
hyp = pytest.importorskip("hypothesis")
from hypothesis import HealthCheck, Phase, given, settings  # noqa: E402

import test_gpu_cov as tgc  # noqa: E402
import test_gpu_cov_weighted as tcw  # noqa: E402
import test_gpu_meanvar_weighted as tmw  # noqa: E402
import test_gpu_skew_kurt as tsk  # noqa: E402
import test_gpu_values_census as tvc  # noqa: E402
from test_gpu_argextrema import assert_first_holder  # noqa: E402

EXAMPLES, BLOCK_EXAMPLES = 60, 30
INT_OUTPUTS = {"argextrema": (0, 1), "mean_var": (0,), "cov": (0,), "skew_kurt": (0,)}  # of the public call's outputs
N_OUTPUTS = {"extrema": 2, "argextrema": 4, "mean_var": 3, "mean_var_w": 3, "cov": 6, "cov_w": 6, "skew_kurt": 5,
             "skew_kurt_w": 5, "quantile": 1, "quantile_w": 1}


@pytest.fixture(scope="module")
def xh():
    from xhistogram_amd import _native, core

    assert _native.device_count() >= 1
    return core


def for_each_case(stat, max_examples, body):
    """body(case) on the first `max_examples` derandomised examples of values_cases.cases(stat): the same ones wherever this
    runs (the seed comes from `examples` below, not from the caller).  A failure carries the whole drawn case; nothing is
    shrunk (a shrink would run hundreds of further calls on the GPU)."""
    @settings(max_examples=max_examples, deadline=None, derandomize=True, database=None, suppress_health_check=list(HealthCheck),
              phases=(Phase.explicit, Phase.generate))
    @given(vc.cases(stat))
    def examples(case):
        try:
            body(case)
        except Exception as e:
            raise AssertionError("%s: %s\ncase = %r" % (type(e).__name__, e, case)) from e

    examples()


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def public(core, stat):
    name = {"mean_var_w": "mean_var", "skew_kurt_w": "skew_kurt", "cov_w": "weighted_cov", "quantile_w": "weighted_quantile"}.get(stat, stat)
    return getattr(core, "histogram_" + name)


# ---------------------------------------------------------------------------------------------------------------------
# the comparison: the library's outputs, as numpy arrays in the public call's order, against the oracles on host arrays
# ---------------------------------------------------------------------------------------------------------------------
def _rows(host, shape, axis):
    """[rows, columns] of broadcast host arrays: the kept axes in place, the reduced ones in ascending axis number"""
    ax = onp.normalise_axis(axis, len(shape))
    return [ao.rows_cols_sorted(np.broadcast_to(h, shape), ax) for h in host]


def compare(stat, host, edges, axis, params, got, want=None):
    """got: {"outs": the public outputs (without the edges)[, "ext": histogram_extrema's pair and "hist": histogram's counts on
    the same inputs (mean_var)][, "moms": (x, mean, M2, M3, M4) as core._value_stat gives them (skew_kurt)]}; host: the
    contiguous host arrays samples..., values[, second values][, weights]; want: the oracle's outputs, if already computed"""
    outs = [np.asarray(o) for o in got["outs"]]
    d = len(edges)
    shape = np.broadcast_shapes(*[h.shape for h in host])
    for i, o in enumerate(outs):
        assert o.dtype == (np.int64 if i in INT_OUTPUTS.get(stat, ()) else np.float64), (i, o.dtype)
    ddof = params.get("ddof", 0)
    if stat in ("extrema", "argextrema", "quantile", "quantile_w"):
        want = want if want is not None else vc.oracle(stat, host, edges, axis, params)
        assert len(outs) == len(want)
        for i, (g, w) in enumerate(zip(outs, want)):
            assert g.shape == np.shape(w), (i, g.shape, np.shape(w))
            if g.dtype == np.int64:
                np.testing.assert_array_equal(g, w, err_msg="%s output %d" % (stat, i))
            else:  # (the weighted quantiles too: the values of values_cases hold no -0.0, which numpy would leave unordered)
                tvc._bits(g, w, "%s output %d" % (stat, i))
        if stat == "argextrema":
            assert_first_holder([np.broadcast_to(h, shape) for h in host[:d]], np.broadcast_to(host[d], shape), edges, axis, *outs)
        return
    rows = _rows(host, shape, axis)
    xs, rest = rows[:d], rows[d:]
    if stat == "mean_var":
        tvc.check_results(xs, edges, rest[0], got["ext"], outs, got["hist"], ddof=ddof, what=stat)
    elif stat == "mean_var_w":
        tmw.check_exact(xs, edges, rest[0], rest[1], outs, ddof=ddof, what=stat)
    elif stat == "cov":
        tgc.check_exact(None, xs, edges, rest[0], rest[1], outs, ddof=ddof, what=stat)
    elif stat == "cov_w":
        tcw.check_exact(xs, edges, rest[0], rest[1], rest[2], outs, ddof=ddof, what=stat, need_exact=False)
    else:
        w = rest[1] if stat == "skew_kurt_w" else None
        tsk.check_results(None, xs, edges, rest[0], w, got["moms"], outs, ddof=ddof, bias=params["bias"], fisher=params["fisher"],
                          what=stat, need_exact=False)
    # counts, sums of weights and means once more against the N-D oracle: by value and bit for bit, in the public shape
    want = want if want is not None else vc.oracle(stat, host, edges, axis, params)
    n_means = 3 if stat in vc.PAIRS else 2
    for i in range(n_means):
        assert outs[i].shape == want[i].shape, (i, outs[i].shape, want[i].shape)
        if i == 0:
            np.testing.assert_array_equal(outs[0], want[0], err_msg=stat + " count / sum of weights")
        else:
            tvc._bits(outs[i], want[i], "%s mean %d" % (stat, i))


# ---------------------------------------------------------------------------------------------------------------------
# (a) the public call
# ---------------------------------------------------------------------------------------------------------------------
def kept_shape(case):
    red = vc.reduced_axes(case)
    return tuple(n for i, n in enumerate(case["shape"]) if i not in red)


def run_public(core, built, backend=None):
    """the public call on the built inputs: its outputs as numpy arrays (compare's `got`) and the edges it returned, after
    the checks of shape, dtype and container"""
    case = built.case
    stat, backend = case["stat"], backend or case["backend"]
    arrays = built.inputs(backend)
    args, kw = built.call_kwargs(arrays)
    *outs, edges = public(core, stat)(*args, **kw)
    edges = [_np(e) for e in edges]
    for e, mine in zip(edges, built.edges):
        np.testing.assert_array_equal(e, mine)
    shape = kept_shape(case) + tuple(len(e) - 1 for e in edges)
    q = case["params"].get("q")
    if q is not None and np.ndim(q):
        shape = (len(q),) + shape
    assert len(outs) == N_OUTPUTS[stat]
    for i, o in enumerate(outs):
        assert tuple(o.shape) == shape, (i, tuple(o.shape), shape)
        ints = i in INT_OUTPUTS.get(stat, ())
        if backend == "torch":  # torch in -> torch out on the same device
            assert isinstance(o, torch.Tensor) and o.device == arrays[0].device, (i, type(o))
            assert o.dtype == (torch.int64 if ints else torch.float64), (i, o.dtype)
        else:  # numpy in -> numpy out, DeviceArray in -> numpy out
            assert isinstance(o, np.ndarray), (i, type(o))
            assert o.dtype == (np.int64 if ints else np.float64), (i, o.dtype)
    got = {"outs": [_np(o) for o in outs]}
    if stat == "mean_var":
        vmin, vmax, _ = core.histogram_extrema(*args, values=kw["values"], bins=kw["bins"], axis=kw["axis"])
        # (arrays without elements: `histogram` gives zeros of the right shape for them on all three backends, but its
        # oracle, oracle_np.histogram, raises ValueError as the reference's reshape does, so there is nothing to hold it to
        # and it is not called here; the counts check_results needs are those of no samples, zeros)
        hist = np.zeros(shape, np.int64) if 0 in case["shape"] else _np(core.histogram(*args, bins=kw["bins"], axis=kw["axis"])[0])
        got.update(ext=(_np(vmin), _np(vmax)), hist=hist)
    if stat in vc.NARROW:
        _, moms, _, _ = core._value_stat(stat, args, kw["values"], kw["bins"], None, kw["axis"], "histogram_skew_kurt", weights=kw.get("weights"))
        got["moms"] = [_np(m) for m in moms]
    return got, edges


def check_case(core, case):
    built = vc.build(case)
    got, edges = run_public(core, built)
    compare(case["stat"], built.host, edges, case["axis"], case["params"], got)


@pytest.mark.parametrize("stat", vc.STATS)
def test_random_cases_match_oracle(xh, stat):
    for_each_case(stat, EXAMPLES, lambda case: check_case(xh, case))


# Drawn cases that failed once, kept as they were drawn.
DIRECTED = [
    # torch tensors with a kept axis of extent 0 whose layout takes the copying route: _rows_cols asked torch to infer the
    # number of columns of a [0, -1] reshape, which torch refuses (RuntimeError instead of an empty result)
    {'stat': 'cov_w', 'backend': 'torch', 'shape': (4, 0, 4, 28), 'axis': (-2,), 'sample_dtypes': ('float32',),
     'edge_kinds': ('duplicates',), 'edges': [[-2.0, -2.0, -1.0, -1.0, -1.0, 1.0, 1.0, 2.0, 2.0, 3.0, 3.0]],
     'values': ('small:int32', 'small:bool'), 'weights': 'float64',
     'layouts': [{'kind': 'sliced_one', 'ax': 1}, {'kind': 'contiguous'}, {'kind': 'contiguous'}, {'kind': 'contiguous'}],
     'params': {'ddof': 0}, 'seed': 1893265697},
]


@pytest.mark.parametrize("i", range(len(DIRECTED)))
def test_drawn_cases_that_failed_once(xh, i):
    check_case(xh, DIRECTED[i])


# ---------------------------------------------------------------------------------------------------------------------
# (b) the blocks of a chunked call, as dask's tasks hand them to core._value_block
# ---------------------------------------------------------------------------------------------------------------------
def block_params(core, stat, params):
    """the per-call parameters as the public functions hand them to _value_block"""
    from xhistogram_amd import _native

    if stat == "quantile":
        return dict(q=np.atleast_1d(np.asarray(params["q"], np.float64)), code=_native.QUANTILE_METHODS.index(params["method"]))
    if stat == "quantile_w":
        return dict(q=np.atleast_1d(np.asarray(params["q"], np.float64)))
    return {}


def block_to_public(core, stat, block, red, params):
    """a block's outputs [k, block axes (reduced ones of extent 1), bins...] in the order _VALUE_STATS documents -> compare's
    `got` with ddof = 0: merged counts are float64 by value, int64 outputs that are never merged the bits they are"""
    st = core._VALUE_STATS[stat]
    assert block.dtype == np.float64 and block.shape[0] == (st.k or len(np.atleast_1d(params["q"])))
    o = [block[i].squeeze(tuple(red)) for i in range(block.shape[0])]  # (red: the reduced axes, of extent 1 in a block)
    for i in st.ints:
        if st.reduce is not None:
            np.testing.assert_array_equal(o[i], np.rint(o[i]))
            o[i] = o[i].astype(np.int64)
        else:
            o[i] = np.ascontiguousarray(o[i]).view(np.int64)
    if stat == "extrema":
        return {"outs": o}
    if stat == "argextrema":
        return {"outs": [o[2], o[3], o[0], o[1]]}
    if stat in ("quantile", "quantile_w"):
        return {"outs": [np.stack(o) if np.ndim(params["q"]) else o[0]]}
    x = o[0]
    if stat in ("mean_var", "mean_var_w"):
        return {"outs": [x, o[1], core._var_of(x, o[2], 0)]}
    if stat in vc.PAIRS:  # (x, mean_a, mean_b, M2_a, C_ab, M2_b) -> (x, mean_a, mean_b, var_a, var_b, cov_ab)
        return {"outs": [x, o[1], o[2], core._var_of(x, o[3], 0), core._var_of(x, o[5], 0), core._var_of(x, o[4], 0)]}
    skew, kurt = core._skew_kurt_of(x, o[2], o[3], o[4], params["bias"], params["fisher"])
    return {"outs": [x, o[1], core._var_of(x, o[2], 0), skew, kurt], "moms": o}


def cuts_of(rng, n):
    """1..3 chunks of an axis of extent n: (start, stop) pairs, none empty unless the axis is"""
    k = min(int(rng.integers(1, 4)), max(n, 1))
    inner = np.sort(rng.choice(np.arange(1, n), k - 1, replace=False)) if k > 1 else []
    b = [0, *[int(c) for c in inner], n]
    return list(zip(b, b[1:]))


def check_blocks(core, case):
    built = vc.build(case)
    stat, shape, params = case["stat"], case["shape"], case["params"]
    st = core._VALUE_STATS[stat]
    rng = np.random.default_rng(case["seed"] + 1)
    red = sorted(vc.reduced_axes(case))
    axis = onp.normalise_axis(case["axis"], len(shape))  # (what _values_blockwise hands on)
    cuts = [cuts_of(rng, shape[a]) for a in red]
    full = [np.broadcast_to(a, shape) for a in built.views]  # (dask broadcasts its arrays before it cuts them)
    host = [np.broadcast_to(h, shape) for h in built.host]
    bp = block_params(core, stat, params)
    flat_params = dict(params, ddof=0) if "ddof" in params else params  # (a block holds M2: its variance is M2 / x)
    partials = {}
    for idx in np.ndindex(*[len(c) for c in cuts]):
        sl = [slice(None)] * len(shape)
        for a, c, j in zip(red, cuts, idx):
            sl[a] = slice(*c[j])
        sl = tuple(sl)
        blocks = [a[sl] for a in full]
        out = core._value_block(*blocks, stat=stat, axis=axis, bins=built.edges, **bp)
        got = block_to_public(core, stat, out, red, params)
        if stat == "mean_var":
            ext = core._value_block(*blocks, stat="extrema", axis=axis, bins=built.edges)
            hist = (np.zeros(got["outs"][0].shape, np.int64) if 0 in blocks[0].shape else
                    core.histogram(*blocks[:built.d], bins=built.edges if built.d > 1 else built.edges[0], axis=axis)[0])
            got.update(ext=(ext[0], ext[1]), hist=hist)
        compare(stat, [np.ascontiguousarray(h[sl]) for h in host], built.edges, axis, flat_params, got)
        partials[idx] = out
    if st.reduce is None:
        return
    # the merge of dask.array.reduction(..., concatenate=True): the step on every block, the partials concatenated along the
    # reduced axes, the step again (the aggregate of the exact statistics is the step itself)
    red1 = tuple(a + 1 for a in red)
    stepped = {idx: st.reduce(p, axis=red1, keepdims=True) for idx, p in partials.items()}

    def assemble(prefix):
        if len(prefix) == len(red):
            return stepped[tuple(prefix)]
        return np.concatenate([assemble(prefix + [j]) for j in range(len(cuts[len(prefix)]))], axis=red1[len(prefix)])

    merged = st.reduce(assemble([]), axis=red1, keepdims=True)
    whole = core._value_block(*full, stat=stat, axis=axis, bins=built.edges, **bp)
    exact = range(2) if stat == "extrema" else (0,)  # (extrema; the count or the sum of weights of the moment statistics)
    for i in exact:
        assert merged[i].shape == whole[i].shape
        tvc._bits(merged[i], whole[i], "%s merged output %d" % (stat, i))


@pytest.mark.parametrize("stat", vc.STATS)
def test_blocks_as_dask_hands_them(xh, stat):
    for_each_case(stat, BLOCK_EXAMPLES, lambda case: check_blocks(xh, case))


# Drawn cases whose blocks failed once, kept as they were drawn.
DIRECTED_BLOCKS = [
    # a kept axis of extent 0: core._merge_partials asked numpy to infer the number of partials of an array without elements
    # (ValueError in the dask step instead of an empty result); tests/test_values_cases_cpu.py holds the merge itself to it
    {'stat': 'skew_kurt',
     'backend': 'torch',
     'shape': (3, 7, 0, 25),
     'axis': (-3,),
     'sample_dtypes': ('int64', 'int32'),
     'edge_kinds': ('duplicates', 'uniform'),
     'edges': [[-3.0, -3.0, -2.0, 0.0, 0.0, -0.0, -0.0, 2.0, 2.0, 2.0, 3.0, 3.0],
               [-4.119456778066544, -3.963732303304493, -3.8080078285424412, -3.6522833537803896, -3.4965588790183384,
                -3.340834404256287, -3.1851099294942355, -3.029385454732184, -2.8736609799701327]],
     'values': ('small:int16',),
     'weights': None,
     'layouts': [{'kind': 'broadcast', 'axes': (1,), 'expanded': True}, {'kind': 'sliced_all'},
                 {'kind': 'permuted', 'perm': (2, 1, 3, 0)}],
     'params': {'ddof': 0, 'bias': True, 'fisher': False},
     'seed': 1563278315},
]


@pytest.mark.parametrize("i", range(len(DIRECTED_BLOCKS)))
def test_blocks_of_drawn_cases_that_failed_once(xh, i):
    check_blocks(xh, DIRECTED_BLOCKS[i])


# ---------------------------------------------------------------------------------------------------------------------
# (d) dirty scratch  (before (c): the threads leave megabytes of staging blocks in the cache)
# ---------------------------------------------------------------------------------------------------------------------
TWO_PASS = ("mean_var", "mean_var_w", "cov", "cov_w", "skew_kurt", "skew_kurt_w")
FIXED_PARAMS = {"mean_var": dict(ddof=1), "mean_var_w": dict(ddof=1), "cov": dict(ddof=1), "cov_w": dict(ddof=1),
                "skew_kurt": dict(ddof=1, bias=False, fisher=True), "skew_kurt_w": dict(ddof=1, bias=True, fisher=False),
                "quantile": dict(q=[0.25, 0.5], method="linear"), "quantile_w": dict(q=[0.25, 0.5]), "extrema": {}, "argextrema": {}}


def call_fixed(core, stat, arrays, edges, axis=1):
    """one public call of `stat` on (samples, values[, second values][, weights]) with FIXED_PARAMS: compare's `got`"""
    xs, rest = arrays[0], list(arrays[1:])
    kw = dict(bins=edges, axis=axis, **FIXED_PARAMS[stat])
    if stat in vc.WEIGHTED:
        kw["weights"] = rest.pop()
    kw["values"] = tuple(rest) if stat in vc.PAIRS else rest[0]
    *outs, _ = public(core, stat)(xs, **kw)
    got = {"outs": [_np(o) for o in outs]}
    if stat == "mean_var":
        vmin, vmax, _ = core.histogram_extrema(xs, values=kw["values"], bins=edges, axis=axis)
        got.update(ext=(_np(vmin), _np(vmax)), hist=_np(core.histogram(xs, bins=edges, axis=axis)[0]))
    if stat in vc.NARROW:
        _, moms, _, _ = core._value_stat(stat, [xs], kw["values"], edges, None, axis, "histogram_skew_kurt", weights=kw.get("weights"))
        got["moms"] = [_np(m) for m in moms]
    return got


def fixed_data(seed, shape, edges):
    """samples about the edges, two value arrays on the narrow grid with NaNs of their own, the integer weights 0..7"""
    import skew_kurt_exact as sx

    rng = np.random.default_rng(seed)
    return (vc.edge_relative(rng, shape, edges, np.float64), sx.narrow_nan(rng, shape), sx.narrow_nan(rng, shape),
            rng.integers(0, 8, shape).astype(np.float64))


def arrays_of(stat, data):
    xs, a, b, w = data
    return [xs, a] + ([b] if stat in vc.PAIRS else []) + ([w] if stat in vc.WEIGHTED else [])


def test_a_statistic_initialises_the_scratch_it_inherits(xh):
    """Every two-pass statistic takes its `sd` block (rows x bins doubles; two of them for the covariances) from the
    stream-ordered scratch cache.  Here that block comes back full of set bits: every cached block it could be given instead
    is held out of the cache, a call of the statistic makes the one block, a host-route histogram of samples whose bytes
    are all ones stages them into that very block on the same stream or on another one (it allocates nothing new either: its
    output takes a smallest block put there for it, its staging request the only block of that size left), and the statistic
    runs again on other data.  It allocates nothing new, so the block was reused, and its results are the oracle's.  The quantile calls take several blocks of sizes of their own: they inherit what a call of the same shape on
    other data left behind, on the same stream and on another one."""
    from xhistogram_amd import _native

    R, C, B = 13, 600, 127
    edges = np.linspace(-4.0, 4.0, B + 1)
    data = fixed_data(11, (R, C), edges)
    other = fixed_data(12, (R, C), edges)
    dev = [torch.as_tensor(a).cuda() for a in data]
    dev_other = [torch.as_tensor(a).cuda() for a in other]
    sd = R * B * 8
    dirty_plan = _native.Plan([np.array([0.0, 0.5, 1.0])], _native.CMP_F64, 0)
    side = torch.cuda.Stream()

    def total():
        s = _native.scratch_stats(0)
        return s["cached"] + s["live"]

    def dirty(nbytes, stream):
        ones = np.frombuffer(b"\xff" * nbytes, np.float64)  # (NaN samples: nothing is counted)
        out = np.empty(2, np.int64)
        dirty_plan.execute([_native.make_view(ones.ctypes.data, _native.F64, ones.size, 1)], None, 1, ones.size, out.ctypes.data,
                           False, _native.MEM_HOST, stream=stream)
        assert not out.any()

    torch.cuda.synchronize()
    held = []
    try:
        for size in (sd, 2 * sd):  # hold every cached block a request of this size could be given
            for _ in range(20_000):
                before = _native.scratch_stats(0)["cached"]
                held.append(_native.DeviceBuffer(0, size))
                if _native.scratch_stats(0)["cached"] == before:  # (a fresh allocation: the cache had nothing left for it)
                    break
            else:
                raise AssertionError("the scratch cache never ran out of blocks")
        for where in ("same stream", "another stream"):
            for stat in TWO_PASS:
                call_fixed(xh, stat, arrays_of(stat, dev_other), edges)  # makes the blocks of this shape, `sd` among them
                torch.cuda.synchronize()
                nbytes = 2 * sd if stat in vc.PAIRS else sd
                _native.DeviceBuffer(0, 16).close()  # (a smallest block for the histogram's own output: it is asked for first)
                before = total()
                dirty(nbytes, 0 if where == "same stream" else side.cuda_stream)
                torch.cuda.synchronize()
                assert total() == before, "the all-ones samples were staged into a fresh block, not into the cached one"
                got = call_fixed(xh, stat, arrays_of(stat, dev), edges)
                torch.cuda.synchronize()
                assert total() == before, "%s allocated scratch of its own (%s)" % (stat, where)
                compare(stat, arrays_of(stat, data), [edges], 1, FIXED_PARAMS[stat], got)
            for stat in ("quantile", "quantile_w"):
                if where == "same stream":
                    call_fixed(xh, stat, arrays_of(stat, dev_other), edges)
                else:
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        call_fixed(xh, stat, arrays_of(stat, dev_other), edges)
                torch.cuda.synchronize()
                before = total()
                got = call_fixed(xh, stat, arrays_of(stat, dev), edges)
                torch.cuda.synchronize()
                assert total() == before, "%s allocated scratch of its own (%s)" % (stat, where)
                compare(stat, arrays_of(stat, data), [edges], 1, FIXED_PARAMS[stat], got)
    finally:
        for h in held:
            h.close()
        dirty_plan.close()


# ---------------------------------------------------------------------------------------------------------------------
# (c) one plan, many threads
# ---------------------------------------------------------------------------------------------------------------------
def test_value_statistics_one_plan_many_threads(xh):
    """the twin of test_gpu_properties.test_one_plan_many_threads: 8 threads with a stream and data of their own share one
    edge array, so one cached plan, and run all ten statistics three times each, resident and numpy inputs taking turns (dask's
    threaded scheduler does this through _value_block).  Every round of every thread goes through the comparison of (a): exact
    outputs bit for bit against oracles computed beforehand, the moments through the directed files' checks."""
    edges = np.linspace(-4.0, 4.0, 11)
    datas = [fixed_data(100 + i, (3, 50_000 + 1_000 * i), edges) for i in range(8)]
    exact = ("extrema", "argextrema", "quantile", "quantile_w")
    want = [{stat: vc.oracle(stat, arrays_of(stat, d), [edges], 1, FIXED_PARAMS[stat]) for stat in exact} for d in datas]
    results = [[] for _ in datas]
    errors = []

    def work(i):
        try:
            s = torch.cuda.Stream()
            for rnd in range(3):
                with torch.cuda.stream(s):
                    src = [torch.as_tensor(a).cuda() for a in datas[i]] if (rnd + i) % 2 == 0 else datas[i]
                    results[i].append({stat: call_fixed(xh, stat, arrays_of(stat, src), edges) for stat in vc.STATS})
                s.synchronize()
        except Exception as e:  # pragma: no cover
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(datas))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i, d in enumerate(datas):
        for stat in vc.STATS:
            for rnd in results[i]:  # (every round: resident and numpy inputs took turns)
                compare(stat, arrays_of(stat, d), [edges], 1, FIXED_PARAMS[stat], rnd[stat], want=want[i].get(stat))
