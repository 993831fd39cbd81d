"""xhist_plan_execute, xhist_plan_execute_two_weights and xhist_bincount_rows held to their output contract in every histogram
home: what they write, where, and what accumulate = 1 adds to.

The census (tests/test_gpu_census.py, test_gpu_weighted_exact.py) reaches every home through core._bincount_2d_vectorized, which
hands the library a torch.empty output and accumulate = 0: a missed zeroing shows only when the allocator returns dirty memory, a
write past the last bin lands in somebody else's tensor, and a flush that stores where it should add is right on a buffer that was
just zeroed (the host route's).  Here every case of tests/output_contract_cases.py is binned three times on the device:

  (a) as the census does it: its result and its describe() line are the baseline;
  (b) accumulate = 0 into an [n_rows, n_bins] block inside a DeviceBuffer of sentinels (`guarded` of test_gpu_dense_front.py; the
      block starts 8 bytes off 16-byte alignment in every second case): the sentinel intact around it and between the pair of a
      two-weights call, gone from every element of it; int64 by value, float64 by bits (an empty bin holds +0.0); describe() = (a)'s;
  (c) accumulate = 1 into the block uploaded as the prefill P: the block holds P + H exactly (the prefill of counts carries out of
      the low 32 bits, exactly summable weights make P + H exact in any order); describe() = (a)'s but for direct_store, which is 0.

The views are made as _bincount_2d_vectorized makes them (core._strided_view, _native.make_view), the plan is the cached one,
every tuning key reset before each leg (what an earlier leg taught the plan — weights of both signs — must not pick the next one's
kernels) and after the case.  Every second case runs on a side stream.  The exchange mode's lines carry four notes of EARLIER
calls of the plan (exchange_*_before, exchange_aborts, exchange_arrival_misses): those are no property of the call and are masked.

Then: the calls on host memory (MEM_HOST between numpy guard bands: the host-side add; MEM_HOST_TO_DEVICE into the guarded device
block), calls without columns, without rows and without bins, and xhist_bincount_rows.

No d1_* rung is dropped: the ladder's cases are the smallest of the table."""
import ctypes as C
import itertools
import re

import numpy as np
import pytest

import exact_weights as ew
import output_contract_cases as occ
from test_gpu_census import _dev, _dev_lead, _fresh, xh  # noqa: F401  (xh: the module fixture)
from test_gpu_dense_front import CASE_NO, GAP, SENTINEL, guarded

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

assert SENTINEL == occ.SENTINEL
RAN = itertools.count()
HISTORY = re.compile(r"exchange_(window_ppm_before|aborts|busiest_owner_ppm_before|arrival_misses)=\d+")
DIRECT = re.compile(r"direct_store=\d")


def masked(line, direct=False):
    line = HISTORY.sub(lambda m: m.group(0).split("=")[0] + "=*", line)
    return DIRECT.sub("direct_store=*", line) if direct else line


def start_parity(odd):
    """the next `guarded` call puts its first block 8 bytes off 16-byte alignment (odd) or on it"""
    if (next(CASE_NO) + 1) % 2 != int(odd):
        next(CASE_NO)


def upload(native, ptr, host):
    """host -> device address, final on return"""
    host = np.ascontiguousarray(host)
    native.check(native.load().xhist_buffer_copy(0, C.c_void_p(ptr), C.c_void_p(host.ctypes.data), host.nbytes, 0, None))


def view_of(core, native, a, backend):
    ptr, tag, rs, cs, ir, os_, keep = core._strided_view(a, backend)
    return native.make_view(ptr, tag, rs, cs, ir, os_), keep


def plan_of(core, arrays, edges):
    cmp_domain, conv, _ = core._compare_domain([core._np_dtype_of(a) for a in arrays], edges)
    return core._get_plan(conv, cmp_domain, 0)


def with_params(plan, params, fn):
    """fn() on the plan made fresh, with the case's parameters -> (what fn returned, the describe() line)"""
    torch.cuda.synchronize()  # (what the GPU notes for the plan arrives with the end of the call before)
    _fresh(plan)
    for k, v in params.items():
        plan.set_param(k, v)
    try:
        result = fn()
        torch.cuda.synchronize()
        return result, plan.describe()
    finally:
        for k in params:
            plan.set_param(k, 0)


def assert_block(case, k, block, want, what):
    """one [n_rows, n_bins] block as int64 against the expectation: counts by value, sums by bits"""
    assert not (block == np.int64(SENTINEL)).any(), "%s: %d elements were never written" % (what, (block == np.int64(SENTINEL)).sum())
    if case.weighted:
        ew.assert_bits_equal(block.view(np.float64).reshape(want.shape), want, what)
    else:
        np.testing.assert_array_equal(block.reshape(want.shape), want, err_msg=what)


def run_case(core, case):
    """the three legs of one case -> its three describe() lines"""
    from xhistogram_amd import _native as native

    k = next(RAN)
    put = _dev_lead if case.lead else _dev
    xd = [put(x) for x in case.samples]
    wd = [put(np.asarray(w)) for w in case.weights()]
    plan = plan_of(core, xd, case.edges)
    assert plan.n_bins == case.n_bins
    stream = torch.cuda.Stream() if k % 2 else torch.cuda.current_stream()
    views = [view_of(core, native, t, "torch") for t in xd + wd]
    sv, wv = [v for v, _ in views[:len(xd)]], [v for v, _ in views[len(xd):]]
    n = case.n_rows * case.n_bins
    wants = [case.want(j) for j in range(max(1, len(wd)))]
    torch.cuda.synchronize()

    def baseline():
        with torch.cuda.stream(stream):
            if case.w2 is not None:
                return list(core.histogram_two_weights(*xd, bins=case.edges, axis=1, weights=tuple(wd))[:2])
            return [core._bincount_2d_vectorized(*xd, bins=case.edges, weights=wd[0] if wd else None)]

    def execute(accumulate):
        def call(ptrs):
            if accumulate:
                for j, p in enumerate(ptrs):
                    upload(native, p, case.prefill(j))
                torch.cuda.synchronize()
            if case.w2 is not None:
                plan.execute_two_weights(sv, wv[0], wv[1], case.n_rows, case.n_cols, ptrs[0], ptrs[1], native.MEM_DEVICE,
                                         accumulate=accumulate, stream=stream.cuda_stream)
            else:
                plan.execute(sv, wv[0] if wv else None, case.n_rows, case.n_cols, ptrs[0], case.weighted, native.MEM_DEVICE,
                             accumulate=accumulate, stream=stream.cuda_stream)
        return lambda: guarded(native, [n] * len(wants), call)[1]

    try:
        got, line_a = with_params(plan, case.params, baseline)
        for j, want in enumerate(wants):
            g = got[j].cpu().numpy().reshape(want.shape)
            assert_block(case, j, np.ascontiguousarray(g).view(np.int64), want, "%s (a) %s" % (case.name, line_a))
        for token in case.expect:
            assert token in line_a, (case.name, token, line_a)
        start_parity(k % 2)
        blocks, line_b = with_params(plan, case.params, execute(False))
        for j, want in enumerate(wants):
            assert_block(case, j, blocks[j], want, "%s (b) accumulate=0 %s" % (case.name, line_b))
        assert masked(line_b) == masked(line_a), case.name
        blocks, line_c = with_params(plan, case.params, execute(True))
        for j, want in enumerate(wants):
            assert_block(case, j, blocks[j], case.prefill(j) + want, "%s (c) accumulate=1 %s" % (case.name, line_c))
        assert masked(line_c, True) == masked(line_a, True) and "direct_store=1" not in line_c, (case.name, line_a, line_c)
    finally:
        torch.cuda.synchronize()
        _fresh(plan)  # (forgets "both signs": later modules still select the packed kernels)
    print("output contract: %s | %s" % (case.name, line_b))
    return line_a, line_b, line_c


class Ledger:
    """the lines of every group of cases that has run, each group once"""

    def __init__(self):
        self.lines = {}

    def run(self, core, key, cases):
        if key not in self.lines:
            self.lines[key] = [run_case(core, c) for c in cases()]
            assert self.lines[key], key
        return self.lines[key]


@pytest.fixture(scope="module")
def ledger():
    return Ledger()


GROUPS = {}
for _st in occ.STS:
    for _wt in occ.WTS:
        for _D in occ.DS:
            GROUPS["float", _st, _wt, _D] = lambda st=_st, wt=_wt, D=_D: occ.float_cases(st, wt, D)
for _dt in occ.SMALL_DTYPES:
    GROUPS["small", _dt] = lambda dt=_dt: occ.small_sample_cases(dt)
GROUPS["int64",] = occ.int64_domain_cases
GROUPS["generic",] = occ.generic_integer_cases
for _D in occ.DS:
    GROUPS["mixed", _D] = lambda D=_D: occ.mixed_dtype_cases(D)
for _st in occ.STS:
    for _wt in ("f32", "f64"):
        for _D in occ.DS:
            GROUPS["two", _st, _wt, _D] = lambda st=_st, wt=_wt, D=_D: occ.two_weight_cases(st, wt, D)
GROUPS["table",] = occ.table_column_cases
for _n in occ.EXCHANGE_N:
    GROUPS["exchange", _n] = lambda n=_n: occ.exchange_cases(n)


@pytest.mark.parametrize("D", occ.DS)
@pytest.mark.parametrize("wt", occ.WTS)
@pytest.mark.parametrize("st", occ.STS)
def test_float_samples(xh, ledger, st, wt, D):
    """every histogram home the census has for (st, wt, D), the d1_* ladder included"""
    ledger.run(xh, ("float", st, wt, D), GROUPS["float", st, wt, D])


@pytest.mark.parametrize("dtype", occ.SMALL_DTYPES)
def test_small_samples(xh, ledger, dtype):
    ledger.run(xh, ("small", dtype), GROUPS["small", dtype])


def test_int64_domain(xh, ledger):
    ledger.run(xh, ("int64",), GROUPS["int64",])


def test_generic_integer_domains(xh, ledger):
    ledger.run(xh, ("generic",), GROUPS["generic",])


@pytest.mark.parametrize("D", occ.DS)
def test_mixed_dtypes(xh, ledger, D):
    ledger.run(xh, ("mixed", D), GROUPS["mixed", D])


@pytest.mark.parametrize("D", occ.DS)
@pytest.mark.parametrize("wt", ["f32", "f64"])
@pytest.mark.parametrize("st", occ.STS)
def test_two_weights(xh, ledger, st, wt, D):
    """the pair of outputs as two blocks with a gap of sentinels between them"""
    ledger.run(xh, ("two", st, wt, D), GROUPS["two", st, wt, D])


def test_table_columns(xh, ledger):
    ledger.run(xh, ("table",), GROUPS["table",])


@pytest.mark.parametrize("n", occ.EXCHANGE_N)
def test_exchange_mode_forced(xh, ledger, n):
    """C5's edges: packed8 records, exact12 records, the packed attempt discarded inside the call, no budget (the classic passes
    take the call), and the classic routing home with both signs"""
    ledger.run(xh, ("exchange", n), GROUPS["exchange", n])


def test_zz_across_the_module(xh, ledger):
    """over the whole table (groups that have not run yet run now): the plain-store flush of every streaming and lanes family was
    under the sentinel test, and every hist= and route= value of the baseline was reached with accumulate = 0 and 1 as well"""
    lines = [t for key, cases in GROUPS.items() for t in ledger.run(xh, key, cases)]
    for family in ("family=fast ", "family=flat_rows ", "family=lanes "):
        assert any(family in b and "direct_store=1" in b for _, b, _ in lines), "no case of %sstored its block directly" % family
    rows1 = [b for _, b, _ in lines if "transpose=fused" in b]
    assert rows1 and any("direct_store=1" in b for b in rows1)
    for field in ("hist", "route"):
        reached = [{m for line in leg for m in re.findall(r"\b%s=(\S+)" % field, line)} for leg in zip(*lines)]
        assert reached[0] and reached[0] <= reached[1] and reached[0] <= reached[2], (field, reached)
    print("output contract: hist= %s route= %s" % tuple(sorted({m for _, _, c in lines for m in re.findall(r"\b%s=(\S+)" % f, c)})
                                                        for f in ("hist", "route")))


# ---------------------------------------------------------------------------------------------------------------------
# host memory
# ---------------------------------------------------------------------------------------------------------------------
def host_call(core, native, case, mem, accumulate, ptr):
    views = [view_of(core, native, np.asarray(a), "numpy") for a in case.samples + case.weights()]
    plan = plan_of(core, case.samples, case.edges)
    sv = [v for v, _ in views[:len(case.samples)]]
    return with_params(plan, case.params, lambda: plan.execute(sv, views[-1][0] if case.weighted else None, case.n_rows, case.n_cols, ptr,
                                                               case.weighted, mem, accumulate=accumulate))[1]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("home", ["lds", "global", "lanes", "route"])
def test_host_routes(xh, home, weighted):
    """MEM_HOST: a numpy block between numpy guard bands (accumulate = 1: the host-side add, int64 and float64);
    MEM_HOST_TO_DEVICE: the guarded device block; each with accumulate = 0 over the sentinel and accumulate = 1 over P"""
    from xhistogram_amd import _native as native

    case, = [c for c in occ.host_route_cases() if c.home == home and c.weighted == weighted]
    want, P, n = case.want(), case.prefill(), case.n_rows * case.n_bins
    try:
        for accumulate in (False, True):
            expected = P + want if accumulate else want
            lead = 64 + int(accumulate)
            host = np.full(lead + n + GAP, SENTINEL, np.uint64).view(np.int64)
            if accumulate:
                host[lead:lead + n] = P.reshape(-1).view(np.int64)
            line = host_call(xh, native, case, native.MEM_HOST, accumulate, host.ctypes.data + 8 * lead)
            assert occ.HOST_ROUTE_LINES[home] in line + " ", line
            assert (host[:lead] == np.int64(SENTINEL)).all() and (host[lead + n:] == np.int64(SENTINEL)).all(), "the guard bands were written"
            assert_block(case, 0, host[lead:lead + n], expected, "%s MEM_HOST accumulate=%d %s" % (case.name, accumulate, line))

            def call(ptrs):
                if accumulate:
                    upload(native, ptrs[0], P)
                return host_call(xh, native, case, native.MEM_HOST_TO_DEVICE, accumulate, ptrs[0])
            line, blocks, _ = guarded(native, [n], call)
            assert occ.HOST_ROUTE_LINES[home] in line + " ", line
            assert_block(case, 0, blocks[0], expected, "%s MEM_HOST_TO_DEVICE accumulate=%d %s" % (case.name, accumulate, line))
    finally:
        torch.cuda.synchronize()
        _fresh(plan_of(xh, case.samples, case.edges))


# ---------------------------------------------------------------------------------------------------------------------
# calls without columns, rows or bins
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("mem", ["device", "host", "host_to_device"])
def test_degenerate_shapes(xh, mem, weighted):
    """n_cols == 0: zeros with accumulate = 0, P untouched with accumulate = 1; n_rows == 0 and a plan without bins: nothing in
    the buffer changes"""
    from xhistogram_amd import _native as native

    rng = np.random.default_rng(71)
    x, w = rng.uniform(-1.2, 1.2, (3, 65)), ew.f64(rng, (3, 65), "both")
    kind = {"device": native.MEM_DEVICE, "host": native.MEM_HOST, "host_to_device": native.MEM_HOST_TO_DEVICE}[mem]
    keep = [_dev(x), _dev(w)] if mem == "device" else [x, w]
    backend = "torch" if mem == "device" else "numpy"
    (sv, _), (wv, _) = (view_of(xh, native, a, backend) for a in keep)
    edges = {"four_bins": np.linspace(-1.0, 1.0, 5), "no_bins": np.array([0.25])}
    P = (occ.from_units(occ.weighted_prefill_units(5, 3, 4)) if weighted else occ.count_prefill(3, 4)).reshape(-1).view(np.int64)

    def run(plan, n_rows, n_cols, accumulate, n, fill=None):
        """-> (the block, whether anything in the buffer changed)"""
        def execute(ptr):
            plan.execute([sv], wv if weighted else None, n_rows, n_cols, ptr, weighted, kind, accumulate=accumulate)
        if mem == "host":
            host = np.full(64 + n + GAP, SENTINEL, np.uint64).view(np.int64)
            if fill is not None:
                host[64:64 + n] = fill
            before = host.copy()
            execute(host.ctypes.data + 8 * 64)
            assert (host[:64] == before[:64]).all() and (host[64 + n:] == before[64 + n:]).all(), "the guard bands were written"
            return host[64:64 + n], bool((host != before).any())

        def call(ptrs):
            if fill is not None:
                upload(native, ptrs[0], fill)
            execute(ptrs[0])
        _, blocks, changed = guarded(native, [n], call)
        return blocks[0], changed

    plan = plan_of(xh, [keep[0]], [edges["four_bins"]])
    block, _ = run(plan, 3, 0, False, 12)
    assert (block == 0).all(), "no columns, accumulate=0: all zeros (+0.0)"
    block, _ = run(plan, 3, 0, True, 12, fill=P)
    np.testing.assert_array_equal(block, P, err_msg="no columns, accumulate=1: P untouched")
    for accumulate in (False, True):
        for n_cols in (0, 65):
            assert not run(plan, 0, n_cols, accumulate, 12)[1], "no rows: nothing is written"
        assert not run(plan_of(xh, [keep[0]], [edges["no_bins"]]), 3, 65, accumulate, 12)[1], "no bins: nothing is written"


# ---------------------------------------------------------------------------------------------------------------------
# the one-shot entry point
# ---------------------------------------------------------------------------------------------------------------------
def test_bincount_rows_accumulates(xh):
    """xhist_bincount_rows through ctypes (its own plan cache), accumulate = 1 over P, counts and float64 weights"""
    from xhistogram_amd import _native as native

    lib = native.load()
    for case in occ.host_route_cases():
        if case.home != "lds":
            continue
        xd, wd = [_dev(x) for x in case.samples], [_dev(w) for w in case.weights()]
        views = [view_of(xh, native, t, "torch")[0] for t in xd + wd]
        D = len(xd)
        edges = [np.ascontiguousarray(e, np.float64) for e in case.edges]
        eptr = (C.c_void_p * D)(*[e.ctypes.data for e in edges])
        elen = (C.c_int64 * D)(*[e.size for e in edges])
        torch.cuda.synchronize()

        def call(ptrs):
            upload(native, ptrs[0], case.prefill())
            return lib.xhist_bincount_rows(0, D, (native.XhistArray * D)(*views[:D]), C.byref(views[D]) if case.weighted else None, case.n_rows,
                                           case.n_cols, eptr, elen, native.CMP_F64, C.c_void_p(ptrs[0]), native.F64 if case.weighted else native.I64,
                                           native.MEM_DEVICE, 1, None)
        start_parity(case.weighted)
        rc, blocks, _ = guarded(native, [case.n_rows * case.n_bins], call)
        assert rc == native.OK, (rc, lib.xhist_last_error())
        assert_block(case, 0, blocks[0], case.prefill() + case.want(), "%s xhist_bincount_rows accumulate=1" % case.name)
