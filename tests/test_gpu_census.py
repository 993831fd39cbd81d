"""Every kernel instantiation the library can dispatch is compared with the oracle (VERDICT r5 "next" #2).

The dispatch surface of libxhist_amd.so is a cross product — sample dtype x weight dtype x inputs x digitize form x histogram
home x row shape — of which the other GPU tests, written around BASELINE's configs and the reference's known answers, select a
third.  This module walks that product on purpose: for every (dtype, weights, inputs) it builds the smallest inputs that make
the pickers of xhist_exec_device.hip.h choose each digitize form (through the EDGES: one, two, three, four or many edges per
bucket of the plan's grid, np.linspace edges, geometric edges) and each histogram home (through the BIN COUNT and the documented
plan parameters that the C ABI exposes: force_global, partition, fused, slices, lanes, flat_rows, pack, arith, route_spl), runs
the call through the C ABI on resident data and compares with oracle_np.bincount_rows — what the reference computes with
searchsorted + ravel_multi_index + bincount (/root/reference/xhistogram/core.py:163-183, :73-83).  Samples sit on edges, next to
edges, outside the range and on NaN; the column count leaves a ragged last tile.

With XHIST_AMD_KERNEL_LOG set (tests/conftest.py sets it for `-m gpu` runs) the library logs the symbol of every kernel it
picks; tests/test_zz_gpu_census_total.py (the last-sorted module) then holds the session's log against the host stubs of the
shared object: an instantiation that nothing selected fails the run — it has to be given a case here or leave the library.
The product of the float families (`_cases`, ~9 200 cases) is run in full only in discovery mode; the suite runs the set cover of
it that tests/golden/census_cases.json names (tools/census_cover.py), plus the special families below, which are always complete.
"""
import os

import numpy as np
import pytest

import exact_weights as ew
# the edges, samples, homes and family inputs, in plain numpy (the modules that import them from here keep doing so)
from census_inputs import (F32, F64, FORM_PARAMS, HOMES, KINDS, _MIN_NB, _ST, _WT, _cases, _key, _split_bins, _uniform,  # noqa: F401
                           edges_of, generic_integer_domains_inputs, int64_domain_inputs, mixed_dtypes_inputs, samples_for,
                           small_samples_inputs, two_weights_inputs)
from conftest import assert_hist_equal
from oracle import oracle_np as onp
from test_gpu_parity import _dev, xh  # noqa: F401  (xh: the module fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_KNOBS = ("block_threads", "grid_blocks", "force_global", "force_generic", "fused", "records48", "exchange", "route_spl", "flat_rows",
          "min_parts", "route_pool_pct", "partition", "lanes", "slices", "route_grid", "acc_grid", "pack", "arith", "arith32", "lds_copies",
          "exchange_budget_ms", "exchange_arrive_us", "exchange_min_pct")


def _fresh(plan):
    """every tuning key back to its default: plans are cached by their edges, and np.linspace / geometric edges are shared with
    other tests of the session — what a case selects must not depend on what ran before it"""
    for k in _KNOBS:
        plan.set_param(k, 0)
    return plan


def _dev_lead(a):
    """[rows, cols] on the GPU with the ROWS as the contiguous direction (strides (1, rows)): what a reduction over a leading
    axis of a C-ordered array hands to the hot path"""
    import torch

    return torch.as_tensor(np.ascontiguousarray(a.T)).cuda().T


def _bound_check(xs, edges, w, got, want, desc):
    """beside assert_hist_equal for full-mantissa weights: the float64 bound of tests/exact_weights.py (the oracle's |w| histogram
    and counts over the samples `xs` as the oracle takes them; 2^-37 per weight more where the description shows packed records)"""
    ew.assert_within_f64_bound(got, want, onp.bincount_rows(xs, edges, np.abs(w.astype(F64))), onp.bincount_rows(xs, edges, None),
                               ew.records_rounding(desc), desc)


def _run_case(core, st, wt, D, case, seed, make_w=None):
    """make_w: None (weights U[0.25, 2), compared within 1e-6 and the float64 bound) or a factory (rng, shape) -> weights of
    exactly summable values (tests/exact_weights.py), compared bit for bit"""
    import torch

    edges = [edges_of(case["kind"], nb, seed=seed + d) for d, nb in enumerate(case["nbs"])]
    n_rows, n_cols = case["shape"]
    xs = samples_for(edges, n_rows, n_cols, st, seed)
    rng = np.random.default_rng(seed + 99)
    if wt is None or make_w is None:
        w = None if wt is None else rng.uniform(0.25, 2.0, (n_rows, n_cols)).astype(wt)
    else:
        w = make_w(rng, (n_rows, n_cols))
        assert w.dtype == wt
        ew.assert_summable(n_cols, wt)
    # the oracle compares in float64 against float64 edges (numpy's promotion); float32 weights are added as float64
    want = onp.bincount_rows([x.astype(F64) for x in xs], edges, None if w is None else w.astype(F64))
    put = _dev_lead if case.get("lead") else _dev
    xd = [put(x) for x in xs]
    wd = None if w is None else put(w)
    dts = [core._np_dtype_of(s) for s in xd]
    cmp_domain, conv, _ = core._compare_domain(dts, edges)
    plan = _fresh(core._get_plan(conv, cmp_domain, 0))
    for k, v in case["params"].items():
        plan.set_param(k, v)
    try:
        got = core._bincount_2d_vectorized(*xd, bins=edges, weights=wd)
        torch.cuda.synchronize()
        desc = plan.describe()
    finally:
        for k in case["params"]:
            plan.set_param(k, 0)
    got = got.cpu().numpy()
    if make_w is not None and wt is not None:
        ew.assert_bits_equal(got, want, desc)
        return desc
    assert_hist_equal(got, want, weighted=wt is not None), (case, desc)
    if wt is not None:
        _bound_check([x.astype(F64) for x in xs], edges, w, got, want, desc)
    return desc



# Which of the ~3900 cases of the product are RUN: the smallest set that still selects every kernel the whole product selects
# (greedy set cover over a discovery run: XHIST_CENSUS_DISCOVER=<file> XHIST_AMD_KERNEL_LOG_ALL=1 runs them all and writes which
# case picked which kernels; tools/census_cover.py reduces that to tests/golden/census_cases.json).  Without the file: all of them.
_COVER = os.path.join(ROOT, "tests", "golden", "census_cases.json")


def _selected_keys():
    if os.environ.get("XHIST_CENSUS_DISCOVER") or not os.path.exists(_COVER):
        return None
    import json

    return set(json.load(open(_COVER))["cases"])


def _log_lines():
    path = os.environ.get("XHIST_AMD_KERNEL_LOG")
    if not path or not os.path.exists(path):
        return []
    with open(path) as f:
        return f.read().splitlines()


@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("wt", ["none", "f32", "f64"])
@pytest.mark.parametrize("st", ["f64", "f32"])
def test_dispatch_surface_float_samples(xh, st, wt, D):
    """float64 / float32 samples x {counts, float32 weights, float64 weights} x 1-3 inputs: every digitize form in every
    histogram home, each result against the oracle"""
    keep = _selected_keys()
    discover = os.environ.get("XHIST_CENSUS_DISCOVER")
    n = 0
    for i, case in enumerate(_cases(_ST[st], _WT[wt], D)):
        key = _key(st, wt, D, case)
        if keep is not None and key not in keep:
            continue
        before = len(_log_lines()) if discover else 0
        _run_case(xh, _ST[st], _WT[wt], D, case, seed=1000 * D + 17 * i)
        if discover:
            import json

            with open(discover, "a") as f:
                f.write(json.dumps({"case": key, "kernels": sorted(set(_log_lines()[before:]))}) + "\n")
        n += 1
    assert n > 0


# ---------------------------------------------------------------------------------------------------------------------
# the other kernel families: small integer / half samples, the exact int64 domain, dtype mixtures, two weights, generic
# ---------------------------------------------------------------------------------------------------------------------
def _run_general(core, samples, edges, w, params, weighted, lead=False, exact=False):
    """samples: list of [rows, cols] numpy arrays (any dtype); compares with the oracle in float64 / exact int64 — weighted results
    also within the float64 bound, or (exact=True: `w` exactly summable, tests/exact_weights.py) bit for bit"""
    import torch

    put = _dev_lead if lead else _dev
    xd = [put(x) for x in samples]
    wd = None if w is None else put(w)
    dts = [core._np_dtype_of(t) for t in xd]
    cmp_domain, conv, _ = core._compare_domain(dts, edges)
    plan = _fresh(core._get_plan(conv, cmp_domain, 0))
    for k, v in params.items():
        plan.set_param(k, v)
    try:
        got = core._bincount_2d_vectorized(*xd, bins=edges, weights=wd)
        torch.cuda.synchronize()
        desc = plan.describe()
    finally:
        for k in params:
            plan.set_param(k, 0)
    want = onp.bincount_rows(samples, edges, w)
    got = got.cpu().numpy()
    if exact and w is not None:
        ew.assert_summable(samples[0].shape[1], w.dtype)
        ew.assert_bits_equal(got, want, desc)
        return
    assert_hist_equal(got, want, weighted)
    if w is not None:
        _bound_check(samples, edges, w, got, want, desc)


@pytest.mark.parametrize("dtype", ["int32", "int64", "int16", "uint8", "float16"])
def test_dispatch_surface_small_samples(xh, dtype):
    """one input of a small integer / half dtype (compared in float64 like numpy does): counts or float64 weights, histogram in
    LDS or behind memory-side atomics, one edge per bucket or a binary search; rows streamed or one row per lane"""
    _small_samples(xh, dtype)


# The bodies of the families below take an optional weights factory (rng, shape) -> weights: None draws today's full-mantissa
# weights; an exactly summable one (tests/exact_weights.py, from test_gpu_weighted_exact.py) makes every weighted result bitwise.
# Their inputs come from the generators of tests/census_inputs.py, one case at a time.
def _run_family(xh, cases, exact):
    for c in cases:
        _run_general(xh, c["samples"], c["edges"], c["w"], c["params"], c["weighted"], lead=c["lead"], exact=exact)


def _small_samples(xh, dtype, make_w=None):
    _run_family(xh, small_samples_inputs(dtype, make_w), make_w is not None)


def test_dispatch_surface_int64_domain(xh):
    """int64 samples against INTEGER edges: compared exactly in int64 (values beyond 2^53 included)"""
    _int64_domain(xh)


def _int64_domain(xh, make_w=None):
    _run_family(xh, int64_domain_inputs(make_w), make_w is not None)


def test_dispatch_surface_generic_integer_domains(xh):
    """the generic family's exact-integer variants: TWO int64 inputs against integer edges (compared in int64), an int64 input
    next to a float64 one (a compare domain per input), edge arrays too long for LDS; histogram in LDS or behind memory-side atomics"""
    _generic_integer_domains(xh)


def _generic_integer_domains(xh, make_w=None):
    _run_family(xh, generic_integer_domains_inputs(make_w), make_w is not None)


@pytest.mark.parametrize("D", [1, 2, 3])
def test_dispatch_surface_mixed_dtypes(xh, D):
    """inputs of different dtypes / integer weights (consumed as float64 by the MIXED vector kernels; the generic family where
    those have no variant): every digitize form they take, weighted and not"""
    _mixed_dtypes(xh, D)


def _mixed_dtypes(xh, D, make_w=None):
    _run_family(xh, mixed_dtypes_inputs(D, make_w), make_w is not None)


def test_dispatch_surface_odds_and_ends(xh):
    """what the products above do not reach by construction: ONE input of a dtype that has no vector kernel of its own (uint16:
    the MIXED kernels take it, unweighted, as float64) on every digitize form, and the three-pass partitioned mode with more than
    128 partitions and float32 weights (records in groups of four)"""
    rng = np.random.default_rng(12)
    shape = (3, 20_011)
    x16 = rng.integers(0, 1200, shape).astype(np.uint16)
    x8 = rng.integers(-128, 128, shape).astype(np.int8)
    xb = rng.integers(0, 2, shape).astype(np.bool_)
    for kind in ("lin", "k1", "k2", "crowd"):
        for x, lo, hi in ((x16, 100.0, 1100.0), (x8, -100.0, 100.0), (xb, -0.5, 1.5)):
            e = edges_of(kind, 96 if x is not xb else 12, lo=lo, hi=hi, seed=2)
            for params in ({}, {"arith": 1}, {"arith": -1}):
                _run_general(xh, [x], [e], None, params, False)
            # the same from HOST memory (numpy in, numpy out: the dtype reaches the library as it is — torch has no uint16 /
            # uint32 arithmetic to hand it over resident), plus uint32
            for xin in ((x, x.astype(np.uint32)) if x is x16 else (x,)):
                got = xh._bincount_2d_vectorized(xin, bins=[e], weights=None)
                assert_hist_equal(got, onp.bincount_rows([xin], [e], None), False)
    nb = 1_600  # 1600 x 1600 float64 sums = 157 partitions of 2^14 bins
    edges = [np.linspace(-4, 4, nb + 1), edges_of("k1", nb, seed=5)]
    xs = samples_for(edges, 1, 40_013, F32, 3)
    w = rng.uniform(0.5, 1.5, (1, 40_013)).astype(F32)
    _run_general(xh, [x.astype(F64) for x in xs], edges, w.astype(F64), {"partition": 1}, True)          # float64: groups of four as well
    xd32 = [x for x in xs]
    import torch

    dts = [np.dtype(F32)] * 2
    cmp_domain, conv, _ = xh._compare_domain(dts, edges)
    plan = xh._get_plan(conv, cmp_domain, 0)
    plan.set_param("partition", 1)
    try:
        got = xh._bincount_2d_vectorized(*[_dev(x) for x in xd32], bins=edges, weights=_dev(w))
        torch.cuda.synchronize()
    finally:
        plan.set_param("partition", 0)
    assert_hist_equal(got.cpu().numpy(), onp.bincount_rows([x.astype(F64) for x in xs], edges, w.astype(F64)), True)
    # counts with more than 128 partitions (2100 x 2100 bins = 135 partitions of 2^15): three passes, records in groups of four
    nb = 2_100
    edges = [np.linspace(-4, 4, nb + 1), edges_of("k1", nb, seed=6)]
    xs = samples_for(edges, 1, 40_013, F64, 4)
    _run_general(xh, xs, edges, None, {"partition": 1}, False)
    # ONE column taken out of a wider array (a [rows, 1] view with a column stride): no vector kernel of the homogeneous family
    # takes a strided column, the MIXED one does (n_cols == 1) — unweighted, on a binary search, one and two edges per bucket
    base = torch.as_tensor(rng.uniform(-4.4, 4.4, (6_007, 3))).cuda()
    col = base[:, 1:2]
    assert col.stride() == (3, 1) and col.shape == (6_007, 1)
    for kind in ("k1", "k2", "crowd", "lin"):
        e = edges_of(kind, 96, seed=9)
        got = xh._bincount_2d_vectorized(col, bins=[e], weights=None)
        torch.cuda.synchronize()
        assert_hist_equal(got.cpu().numpy(), onp.bincount_rows([col.cpu().numpy()], [e], None), False)


@pytest.mark.parametrize("weighted", [False, True])
def test_padded_layout_at_the_lds_capacity_border(xh, weighted):
    """one float32 input on np.linspace edges takes the float32 arithmetic digitize with a PADDED LDS layout (32 slots in
    front, 32 behind).  Within 64 bins of the LDS capacity the padded histogram does not fit while the unpadded one would: the
    picker must not hand the padded kernel an unpadded allocation there (it now keeps the digitize it had).  Bin counts on both
    sides of both borders, against the oracle."""
    rng = np.random.default_rng(13)
    cap = (160 * 1024) // (8 if weighted else 4)
    x = rng.uniform(-4.2, 4.2, (1, 300_007)).astype(F32)
    x[0, ::211] = np.nan
    w = rng.uniform(0.5, 1.5, x.shape).astype(F32) if weighted else None
    for nb in (cap - 80, cap - 64, cap - 50, cap - 33, cap - 32, cap - 20, cap - 1):
        e = np.linspace(-4.0, 4.0, nb + 1)
        for params in ({}, {"arith32": 1}):
            _run_general(xh, [x], [e], w, params, weighted)


def test_dispatch_surface_one_long_float64_row(xh):
    """one float64 row of >= 2^29 samples without weights takes tiles twice as long (the headline's 8 B/sample variant; one or two
    edges per bucket).  Too long for the oracle in a test: the whole row must equal the sum of its two halves — which are short
    enough for the ordinary kernels the rest of this module holds to the oracle — and the total the in-range count torch finds."""
    import torch

    n = (1 << 29) + 4_099
    g = torch.Generator(device="cuda")
    g.manual_seed(77)
    x = torch.empty((1, n), dtype=torch.float64, device="cuda").normal_(generator=g)
    x[0, ::1_000_003] = float("nan")
    for kind in ("k1", "k2"):
        e = edges_of(kind, 100, seed=3)
        x[0, 5::2_000_003] = float(e[17])  # on an edge
        x[0, 7::3_000_017] = float(e[-1])  # the right edge counts
        whole = xh._bincount_2d_vectorized(x, bins=[e], weights=None)
        h = n // 2
        a = xh._bincount_2d_vectorized(x[:, :h], bins=[e], weights=None)
        b = xh._bincount_2d_vectorized(x[:, h:], bins=[e], weights=None)
        torch.cuda.synchronize()
        assert torch.equal(whole, a + b)
        inside = int(((x >= float(e[0])) & (x <= float(e[-1]))).sum().item())
        assert int(whole.sum().item()) == inside


@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("wt", ["f32", "f64"])
@pytest.mark.parametrize("st", ["f64", "f32"])
def test_dispatch_surface_two_weights(xh, st, wt, D):
    """two weight arrays in one pass (histogram_two_weights: the TODO at /root/reference/xhistogram/xarray.py:106): each of the
    pair equals the oracle's single-weight histogram, for one and two edges per bucket"""
    _two_weights(xh, st, wt, D)


def _two_weights(xh, st, wt, D, make_w=None):
    import torch

    for c in two_weights_inputs(st, wt, D, make_w):
        xs, edges, wa, wb, params = c["samples"], c["edges"], c["w"], c["w2"], c["params"]
        xd = [_dev(x) for x in xs]
        dts = [xh._np_dtype_of(t) for t in xd]
        cmp_domain, conv, _ = xh._compare_domain(dts, edges)
        plan = xh._get_plan(conv, cmp_domain, 0)
        for k, v in params.items():
            plan.set_param(k, v)
        try:
            ha, hb, _ = xh.histogram_two_weights(*xd, bins=edges, axis=1, weights=(_dev(wa), _dev(wb)))
            torch.cuda.synchronize()
        finally:
            for k in params:
                plan.set_param(k, 0)
        x64 = [x.astype(F64) for x in xs]
        for h, wx in ((ha, wa), (hb, wb)):
            want = onp.bincount_rows(x64, edges, wx.astype(F64))
            if make_w is not None:
                ew.assert_bits_equal(h.cpu().numpy(), want, "histogram_two_weights")
            else:
                assert_hist_equal(h.cpu().numpy(), want, True)
