"""The argument checks the ten xhist_plan_execute_* entry points of the per-bin statistics share, through the C ABI itself
(_native.load() and a plan's handle): the Python front checks its arguments before it calls, so nothing else reaches them.

One plan of 4 bins and 1 row x 8 float64 columns on the device.  Every rejected call returns before any launch; each asserts
the status code and the whole xhist_last_error() text.  n_rows = 0 is no error: XHIST_OK, and the plan's describe() stays.
After them one valid call of the same entry point still gives the oracle's result and the describe() line of its launch.

The data make every sum exact: small integer values, and in every bin a count and a sum of integer weights that are powers of
two, so counts, sums of weights, means and the sums of powers of deviations are dyadic numbers of a few bits whatever the order
of additions.  They are held to the oracles bit for bit, as are extrema, positions and quantiles.  Skewness and kurtosis are
the library's public conversion (core._skew_kurt_of) of those exact sums and the oracle's own: each a dozen correctly rounded
float64 operations (2^-53 each, the power 3/2 among them) on the same exact inputs, held to 1e-13 relative."""
import ctypes as C

import numpy as np
import pytest

import values_cases as vc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EDGES = np.array([0.0, 1.0, 2.0, 3.0, 4.0])
X = np.array([[0.5, 1.5, 0.5, 2.5, 0.5, 3.5, 1.5, 0.5]])  # bins 0 1 0 2 0 3 1 0: 4, 2, 1 and 1 samples
A = np.array([[1.0, 3.0, 2.0, -2.0, 4.0, 6.0, 5.0, 7.0]])
B = np.array([[2.0, -1.0, 0.0, 3.0, 5.0, 1.0, 4.0, -3.0]])
W = np.array([[1.0, 1.0, 3.0, 2.0, 2.0, 4.0, 3.0, 2.0]])  # per bin 8, 4, 2 and 4
Q = np.array([0.25, 0.5])
N_BINS, N_COLS = 4, 8

# symbol -> the statistic of tests/values_cases.py, its value (and weight) views in the call's order, its outputs (name, planes
# of [1, 4] elements, dtype)
STATS = {
    "xhist_plan_execute_extrema": ("extrema", ("values",), (("out_min", 1, "f8"), ("out_max", 1, "f8"))),
    "xhist_plan_execute_argextrema": ("argextrema", ("values",), (("out_values", 2, "f8"), ("out_index", 2, "i8"))),
    "xhist_plan_execute_mean_var": ("mean_var", ("values",), (("out_count", 1, "i8"), ("out_mean", 1, "f8"), ("out_m2", 1, "f8"))),
    "xhist_plan_execute_mean_var_weighted": ("mean_var_w", ("values", "weights"),
        (("out_wsum", 1, "f8"), ("out_mean", 1, "f8"), ("out_m2", 1, "f8"))),
    "xhist_plan_execute_skew_kurt": ("skew_kurt", ("values",),
        (("out_count", 1, "i8"), ("out_mean", 1, "f8"), ("out_moments", 3, "f8"))),
    "xhist_plan_execute_skew_kurt_weighted": ("skew_kurt_w", ("values", "weights"),
        (("out_wsum", 1, "f8"), ("out_mean", 1, "f8"), ("out_moments", 3, "f8"))),
    "xhist_plan_execute_cov": ("cov", ("values", "values_b"),
        (("out_count", 1, "i8"), ("out_mean", 2, "f8"), ("out_comoment", 3, "f8"))),
    "xhist_plan_execute_cov_weighted": ("cov_w", ("values", "values_b", "weights"),
        (("out_wsum", 1, "f8"), ("out_mean", 2, "f8"), ("out_comoment", 3, "f8"))),
    "xhist_plan_execute_quantile": ("quantile", ("values",), (("out", 2, "f8"),)),
    "xhist_plan_execute_quantile_weighted": ("quantile_w", ("values", "weights"), (("out", 2, "f8"),)),
}
# the plan's describe() after the valid call
DESCRIBE = {
    "extrema": "extrema family=fast slots=lds scan=1 block=256 segs=1 lds_bytes=272 tables_in_lds=1 D=1 cmp=0",
    "argextrema": "argextrema pass1=extrema_fast slots=lds pass2=argext_fast slots=lds scan=1 block=256 segs=1/1 lds_bytes=272/336 "
                  "tables_in_lds=1 D=1 cmp=0",
    "mean_var": "mean_var pass1=mv_sum_fast slots=lds pass2=mv_dev_fast slots=lds scan=1 copies=16 block=256 segs=1 "
                "lds_bytes=1232/1744 tables_in_lds=1 D=1 cmp=0",
    "mean_var_w": "mean_var_w pass1=mvw_sum_fast slots=lds pass2=mvw_dev_fast slots=lds scan=1 copies=16 block=256 segs=1 "
                  "lds_bytes=1232/1744 tables_in_lds=1 D=1 cmp=0",
    "skew_kurt": "skew_kurt pass1=mv_sum_fast slots=lds pass2=sk_dev_fast slots=lds scan=1 copies=16 block=256 segs=1 "
                 "lds_bytes=1232/2768 tables_in_lds=1 D=1 cmp=0",
    "skew_kurt_w": "skew_kurt_w pass1=mvw_sum_fast slots=lds pass2=skw_dev_fast slots=lds scan=1 copies=16 block=256 segs=1 "
                   "lds_bytes=1232/2768 tables_in_lds=1 D=1 cmp=0",
    "cov": "cov pass1=cov_sum_fast slots=lds pass2=cov_dev_fast slots=lds scan=1 copies=16 block=256 segs=1 lds_bytes=1744/3792 "
           "tables_in_lds=1 D=1 cmp=0",
    "cov_w": "cov_w pass1=covw_sum_fast slots=lds pass2=covw_dev_fast slots=lds scan=1 copies=16 block=256 segs=1 "
             "lds_bytes=1744/3792 tables_in_lds=1 D=1 cmp=0",
    "quantile": "quantile family=short rows_per_wg=512 pairs=4096 lds_bytes=49152 groups=1 block=256 D=1 cmp=0",
    "quantile_w": "weighted_quantile family=short rows_per_wg=256 triples=2048 lds_bytes=40960 groups=1 block=256 D=1 cmp=0",
}
PARAMS = {"extrema": {}, "argextrema": {}, "mean_var": dict(ddof=0), "mean_var_w": dict(ddof=0), "cov": dict(ddof=0),
          "cov_w": dict(ddof=0), "skew_kurt": dict(ddof=0, bias=True, fisher=False),
          "skew_kurt_w": dict(ddof=0, bias=True, fisher=False), "quantile": dict(q=Q.tolist(), method="linear"),
          "quantile_w": dict(q=Q.tolist())}  # the oracles' per-call parameters
# what an output that is NULL is answered with, where it is not "out is NULL" (the output validate_arrays is handed)
OUTS_MISSING = {
    ("extrema", "out_max"): "out_max is NULL", ("argextrema", "out_index"): "out_index is NULL",
    ("mean_var", "out_count"): "out_count / out_m2 is NULL", ("mean_var", "out_m2"): "out_count / out_m2 is NULL",
    ("mean_var_w", "out_m2"): "out_m2 is NULL",
    ("skew_kurt", "out_count"): "out_count / out_moments is NULL", ("skew_kurt", "out_moments"): "out_count / out_moments is NULL",
    ("skew_kurt_w", "out_moments"): "out_moments is NULL",
    ("cov", "out_count"): "out_count / out_comoment is NULL", ("cov", "out_comoment"): "out_count / out_comoment is NULL",
    ("cov_w", "out_comoment"): "out_comoment is NULL",
}


@pytest.fixture(scope="module")
def env():
    from xhistogram_amd import _native

    assert _native.device_count() >= 1
    dev = {name: torch.as_tensor(a).cuda() for name, a in (("samples", X), ("values", A), ("values_b", B), ("weights", W))}
    torch.cuda.synchronize()
    plan = _native.Plan([EDGES], _native.CMP_F64, 0)
    yield _native, plan, dev
    plan.close()


def arguments(native, plan, dev, symbol):
    """the valid call's arguments by name, in the entry point's order; the device tensors of its outputs"""
    stat, views, outs = STATS[symbol]
    view = lambda name: native.make_view(dev[name].data_ptr(), native.F64, N_COLS, 1)  # noqa: E731
    args = {"plan": plan._h, "samples": (native.XhistArray * 1)(view("samples"))}
    for name in views:
        args[name] = C.pointer(view(name))
    args.update(n_rows=1, n_cols=N_COLS)
    if stat in ("quantile", "quantile_w"):
        args.update(q=Q.ctypes.data_as(C.POINTER(C.c_double)), n_q=len(Q))
    if stat == "quantile":
        args["method"] = 0  # XHIST_Q_LINEAR
    tensors = {}
    for name, planes, dt in outs:
        tensors[name] = torch.full((planes, 1, N_BINS), -7, dtype=torch.float64 if dt == "f8" else torch.int64, device="cuda")
        args[name] = C.c_void_p(tensors[name].data_ptr())
    args["mem_kind"] = native.MEM_DEVICE
    if stat == "extrema":
        args["accumulate"] = 0
    args["stream"] = C.c_void_p(0)
    return args, tensors


def rejected(native, symbol, args, message, **changed):
    """the call with `changed` arguments returns XHIST_ERR_INVALID and leaves `message`"""
    rc = getattr(native.load(), symbol)(*dict(args, **changed).values())
    text = native.load().xhist_last_error().decode()
    print("%s %r -> %d %r" % (symbol, sorted(changed), rc, text))
    assert (rc, text) == (native.ERR_INVALID, message), (symbol, changed)


def check_valid(core, stat, tensors):
    """the outputs of the valid call against the statistic's oracle on the host arrays"""
    torch.cuda.synchronize()
    raw = [t.cpu().numpy() for t in tensors.values()]
    host = [X, A] + ([B] if stat in vc.PAIRS else []) + ([W] if stat in vc.WEIGHTED else [])
    want = [np.asarray(w) for w in vc.oracle(stat, host, [EDGES], 1, PARAMS[stat])]
    if stat == "extrema":
        got = [raw[0][0], raw[1][0]]
    elif stat == "argextrema":
        got = [raw[1][0], raw[1][1], raw[0][0], raw[0][1]]  # (the public order: the positions first)
    elif stat in ("quantile", "quantile_w"):
        got = [raw[0]]
    else:  # (x, means..., the sums of powers of deviations...) -> the public outputs, as core does
        x, mean, m = raw[0][0], raw[1], raw[2]
        if stat in vc.PAIRS:
            got = [x, mean[0], mean[1], core._var_of(x, m[0], 0), core._var_of(x, m[2], 0), core._var_of(x, m[1], 0)]
        elif stat in vc.NARROW:
            got = [x, mean[0], core._var_of(x, m[0], 0), *core._skew_kurt_of(x, m[0], m[1], m[2], True, False)]
        else:
            got = [x, mean[0], core._var_of(x, m[0], 0)]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (stat, i, g.shape, w.shape, g.dtype, w.dtype)
        if stat in vc.NARROW and i >= 3:
            np.testing.assert_allclose(g, w, rtol=1e-13, atol=0, equal_nan=True, err_msg="%s output %d" % (stat, i))
        else:
            np.testing.assert_array_equal(g.view(np.int64), w.view(np.int64), err_msg="%s output %d" % (stat, i))


@pytest.mark.parametrize("symbol", list(STATS))
def test_bad_calls_are_rejected_and_a_valid_call_still_runs(env, symbol):
    from xhistogram_amd import core

    native, plan, dev = env
    stat, views, outs = STATS[symbol]
    args, tensors = arguments(native, plan, dev, symbol)
    null = C.POINTER(native.XhistArray)()
    before = plan.describe()

    rejected(native, symbol, args, "values are required", values=null)
    rejected(native, symbol, args, "%s takes DEVICE arrays (mem_kind XHIST_MEM_DEVICE); upload host data first" % symbol,
             mem_kind=native.MEM_HOST)
    for name, _, _ in outs:
        rejected(native, symbol, args, OUTS_MISSING.get((stat, name), "out is NULL"), **{name: C.c_void_p(0)})
    if "weights" in views:
        rejected(native, symbol, args, "weights are required", weights=null)
        rejected(native, symbol, args, "weights are required", weights=null, values=null)
    if "values_b" in views:
        rejected(native, symbol, args, "values_b are required", values_b=null)
    if "q" in args:
        rejected(native, symbol, args, "q is NULL or n_q < 1", n_q=0)
        rejected(native, symbol, args, "q is NULL or n_q < 1", q=C.POINTER(C.c_double)())
    if "method" in args:
        rejected(native, symbol, args, "unknown quantile method 9", method=9)

    fn = getattr(native.load(), symbol)
    assert fn(*dict(args, n_rows=0).values()) == native.OK
    torch.cuda.synchronize()
    assert plan.describe() == before
    for t in tensors.values():  # (nothing ran)
        assert bool((t == -7).all())

    assert fn(*args.values()) == native.OK, native.load().xhist_last_error()
    print("%s describe() %r" % (symbol, plan.describe()))
    check_valid(core, stat, tensors)
    assert plan.describe() == DESCRIBE[stat]
