"""histogram_skew_kurt on an MI355X: the 36 + 2 kernels it adds (sk_dev_* of xhist_meanvar.hip, skw_dev_* of
xhist_meanvar_w.hip, moments_finalize4 of both) against tests/skew_kurt_exact.py and tests/skew_kurt_oracle.py.

Every case runs the unweighted and the weighted call on the narrow grid of skew_kurt_exact (values k 2^-4, |k| < 2^6, NaNs of
their own; integer weights 0..7) and checks two things:
  - the whole describe() line against `predict_sk`, test_gpu_values_census.predict with the slot sizes of the two passes (16 and
    40 bytes, copies) registered in that module's tables from here; the second pass's LDS bytes are restated here as
    test_gpu_cov.predict_cov restates them;
  - the results: x (the count, or W) and the mean bit for bit in every bin; M2, M3, M4 (read through core._value_stat, the
    public function's own path before it forms its outputs) bit for bit where x is 2, 4, 8, 16 or 32 and within
    skew_kurt_exact's bounds elsewhere, at least one bin on the bit-for-bit path per case; var, skew and kurt of the public
    call within the bounds propagated from those; x and mean bit-equal to histogram_mean_var's on the same inputs.
    histogram_mean_var's var is compared bit for bit where its sums are exact in every order (x = 1 and the bit-for-bit path):
    everywhere else both calls add rounded terms with float64 atomics in an order of their own, so neither repeats even its
    own last bits from run to run, and the two are held to the sum of their bounds about the same M2*.
The shapes are small (rows of a few hundred to a few thousand samples) and are listed by cases(), which
tests/test_skew_kurt_cpu.py walks without a GPU: every case has a bin on the bit-for-bit path, weighted and unweighted, and
in every such bin the terms and their sums are exact in rational arithmetic."""
import os
import subprocess
import sys

import numpy as np
import pytest

import meanvar_oracle as mo
import skew_kurt_exact as sx
import skew_kurt_oracle as so
import test_gpu_values_census as tvc
import test_gpu_values_census_streams as cs
import values_exact as vx
from test_gpu_census import edges_of
from test_gpu_meanvar_weighted import int_weights
from test_gpu_parity import _plan_for, xh  # noqa: F401  (xh: the module fixture)
from test_gpu_values_census import FORM_EDGES, HOME_BINS, LDS_MAX, _cus, _domain_edges, _last, float_samples, int_samples, table_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F64, F32 = np.float64, np.float32
PY39 = "/opt/conda/bin/python3.9"
SCRIPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "skew_kurt_dask_script.py")
SLOT1, SLOT2 = 16, 40  # a bin's LDS slot in the two passes (MomentSumSlot<1, .>, Moment4Slot of xhist_moments.hip.h)
tvc.SLOTS.setdefault("skew_kurt", ((SLOT1, SLOT2), (SLOT1, SLOT2)))
tvc.COPIES.setdefault("skew_kurt", True)


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _st(sdt):
    return F64 if sdt == "f64" else F32


# ---------------------------------------------------------------------------------------------------------------------
# the launcher's choice and the describe() line
# ---------------------------------------------------------------------------------------------------------------------
def predict_sk(cus, edges, cmp, sdt, vdt, n_rows, n_cols, fine=True, arith=False, layout_fast=True):
    """test_gpu_values_census.predict for the skew_kurt slots; that function reports one pass's LDS bytes for statistics it
    does not know to have two, so the second pass's are restated here: the same tables and copies, 40-byte slots"""
    want = tvc.predict("skew_kurt", cus, edges, cmp, sdt, vdt, n_rows, n_cols, fine, arith, layout_fast)
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    first = want["lds_bytes"][0]
    in_lds = want["slots"] == "lds"
    want["lds_bytes"] = [first, first + (n_bins * (SLOT2 - SLOT1) * want["copies"] if in_lds else 0) if first else 0]
    return want


def assert_sk_variant(desc, want, weighted):
    """a skew_kurt describe() line in the mean_var line's words, for test_gpu_values_census.assert_variant: pass 1 must be
    mean_var's own kernel family, pass 2 the new one"""
    if weighted:
        assert desc.startswith("skew_kurt_w pass1=mvw_sum_") and " pass2=skw_dev_" in desc, desc
        line = desc.replace("skew_kurt_w pass1=mvw_sum_", "mean_var pass1=mv_sum_").replace(" pass2=skw_dev_", " pass2=mv_dev_")
    else:
        assert desc.startswith("skew_kurt pass1=mv_sum_") and " pass2=sk_dev_" in desc, desc
        line = desc.replace("skew_kurt pass1=", "mean_var pass1=").replace(" pass2=sk_dev_", " pass2=mv_dev_")
    return tvc.assert_variant(line, want)


# ---------------------------------------------------------------------------------------------------------------------
# one case: both calls, the describe() lines and the results
# ---------------------------------------------------------------------------------------------------------------------
def flat_of(xs, edges):
    """(counted mask, flat bin index over rows, rows * bins) of [R, C] host samples in the domain they are compared in"""
    xc, ec = cs._cmp(xs, edges)
    ok, flat, nbs = mo._flat_bins(xc, ec)
    m, n_bins = xs[0].shape[0], int(np.prod(nbs))
    return ok, flat + (np.arange(m, dtype=np.int64) * n_bins)[:, None], m * n_bins


def expected_of(xs, edges, v, w=None):
    """skew_kurt_exact.expected of one case's host arrays (v, w broadcastable to the samples)"""
    ok, flat, size = flat_of(xs, edges)
    v = np.broadcast_to(np.asarray(v), ok.shape)
    w = None if w is None else np.broadcast_to(np.asarray(w), ok.shape)[ok]
    return sx.expected(flat[ok], v[ok], size, w)


def run_sk(core, xs, v, w, edges, axis=1, **kw):
    out = core.histogram_skew_kurt(*xs, values=v, weights=w, bins=edges, axis=axis, **kw)[:5]
    torch.cuda.synchronize()
    return tuple(_np(o) for o in out)


def run_moments(core, xs, v, w, edges, axis=1):
    """(x, mean, M2, M3, M4) as the public function receives them from the library"""
    stat = "skew_kurt" if w is None else "skew_kurt_w"
    _, outs, _, _ = core._value_stat(stat, list(xs), v, edges, None, axis, "histogram_skew_kurt", weights=w)
    torch.cuda.synchronize()
    return tuple(_np(o) for o in outs)


def check_results(core, xs, edges, v, w, moms, outs, dev=None, ddof=0, bias=True, fisher=True, what="", need_exact=True):
    """moms = (x, mean, M2, M3, M4), outs = (x, mean, var, skew, kurt) of the library against skew_kurt_exact; then
    histogram_mean_var on the same device arrays dev = (samples, values, weights or None).  Returns (x, exact mask).
    need_exact=False: random cases, which may have no bin on the bit-for-bit path."""
    x, mean, moments, bounds, exact = expected_of(xs, edges, v, w)
    for got in (moms, outs):
        gx = np.asarray(got[0]).reshape(-1)
        assert gx.dtype == (np.int64 if w is None else F64), gx.dtype
        np.testing.assert_array_equal(gx, x, err_msg="x " + what)
        tvc._bits(got[1], mean, "mean " + what)
    assert exact.any() or not need_exact, "no bin on the bit-for-bit path (%s)" % what
    for k, name in enumerate(("M2", "M3", "M4")):
        sx.assert_within(moms[2 + k], moments[k], bounds[k], exact, "%s %s" % (name, what))
    want, wb = sx.expected_outputs(x, moments, bounds, ddof, bias, fisher)
    for k, name in enumerate(("var", "skew", "kurt")):
        sx.assert_within(outs[2 + k], want[k], wb[k], None, "%s %s" % (name, what))
    # histogram_mean_var on the same inputs
    if dev is not None:
        xs_dev, v_dev, w_dev = dev
        mx, mm, mvar, _ = core.histogram_mean_var(*xs_dev, values=v_dev, weights=w_dev, bins=edges, axis=1, ddof=ddof)
        mx, mm, mvar = _np(mx).reshape(-1), _np(mm), _np(mvar).reshape(-1)
        assert mx.dtype == np.asarray(outs[0]).dtype
        np.testing.assert_array_equal(mx, np.asarray(outs[0]).reshape(-1), err_msg="x against histogram_mean_var " + what)
        tvc._bits(mm, outs[1], "mean against histogram_mean_var " + what)
        var = np.asarray(outs[2]).reshape(-1)
        same = (exact | (x == 1)) & (x > ddof)
        np.testing.assert_array_equal(var[same], mvar[same], err_msg="var against histogram_mean_var " + what)
        np.testing.assert_array_equal(np.isnan(var), np.isnan(mvar))
        rest = ~np.isnan(var) & ~same
        assert np.all(np.abs(var - mvar)[rest] <= 2.0 * wb[0][rest]), "var against histogram_mean_var beyond both bounds " + what
    return x, exact


def case(core, edges, xs, v, w, *, cmp=0, fine=True, arith=False, layout_fast=True, w_fast=True, dev=None, ddof=0, bias=True,
         fisher=True, what=""):
    """the unweighted and the weighted call on one case's data.  xs, v, w: the logical host arrays [R, C] (v, w broadcastable
    to it); dev: the (samples, values, weights) tensors to hand over (default: device copies); layout_fast: samples and values
    qualify for the fast family; w_fast: so do the weights.  Returns the two parsed describe() lines."""
    n_rows, n_cols = xs[0].shape
    xs_dev, v_dev, w_dev = dev if dev is not None else ([_dev(x) for x in xs], _dev(v), _dev(w))
    sdt, vdt = xs[0].dtype, np.asarray(v).dtype
    hits = []
    for weighted in (False, True):
        wd, wh = (w_dev, w) if weighted else (None, None)
        lf = layout_fast and (w_fast or not weighted)
        want = predict_sk(_cus(), edges, cmp, sdt, vdt, n_rows, n_cols, fine, arith, lf)
        outs = run_sk(core, xs_dev, v_dev, wd, edges, ddof=ddof, bias=bias, fisher=fisher)
        plan = _plan_for(core, xs_dev, edges)
        hits.append(assert_sk_variant(plan.describe(), want, weighted))
        moms = run_moments(core, xs_dev, v_dev, wd, edges)
        assert_sk_variant(plan.describe(), want, weighted)
        check_results(core, xs, edges, v, wh, moms, outs, (xs_dev, v_dev, wd), ddof, bias, fisher,
                      "%s %s" % (what, "weighted" if weighted else "unweighted"))
    return hits


def _values_and_weights(seed, shape, vdt, wdt):
    rng = np.random.default_rng(seed)
    return sx.narrow_nan(rng, shape, vdt), int_weights(rng, shape, wdt)


# ---------------------------------------------------------------------------------------------------------------------
# the cases' data (pure numpy: tests/test_skew_kurt_cpu.py walks CASES)
# ---------------------------------------------------------------------------------------------------------------------
FORMS = ("k1", "k2", "arith")
FORM_SHAPE = (3, 4_507)  # more than two tiles of every fast form, odd
# arithmetic edges: the fine tables and the 40-byte slots together exceed 160 KiB while the slots alone fit (n_bins <= 4096)
ARITH_BINS = ((3_600,), (3, 1_300))


def form_data(form, sdt, D):
    (kind, nb1, nb2), fine, arith = FORM_EDGES[form]
    if form == "arith":
        nb1, nb2 = ARITH_BINS
    st = _st(sdt)
    seed = 2_100 + 10 * FORMS.index(form) + 2 * D + (st == F32)
    edges = [edges_of(kind, nb, seed=seed + d) for d, nb in enumerate(nb1 if D == 1 else nb2)]
    xs = float_samples(edges, *FORM_SHAPE, st, seed)
    v, w = _values_and_weights(seed, FORM_SHAPE, st, st)
    return edges, xs, v, w, fine, arith


DOMS = ("f64", "i64", "mixed")
HOMES = ("lds", "global_tables_lds")
GENERIC_SHAPE = {"lds": (2, 1_531), "global_tables_lds": (2, 6_011)}  # (three and twelve blocks of 512 per row)


def generic_data(dom, home):
    rng = np.random.default_rng(2_300 + 3 * DOMS.index(dom) + HOMES.index(home))
    nb = HOME_BINS[home] if dom != "mixed" else max(2, HOME_BINS[home] // 6)
    edges = _domain_edges(dom, nb, rng)
    n_rows, n_cols = GENERIC_SHAPE[home]
    xs = []
    for d, e in enumerate(edges):
        if np.asarray(e).dtype.kind == "f":
            xs += float_samples([e], n_rows, n_cols, F64, 37 + d)
        else:
            xs += int_samples([e], n_rows, n_cols, None, 37 + d)
    # f64: float64 samples with values of another dtype; i64: integer values and weights
    v = sx.narrow_nan(rng, (n_rows, n_cols), F32 if dom == "f64" else F64)
    w = int_weights(rng, (n_rows, n_cols), F64)
    if dom == "i64":
        v, w = sx.narrow(rng, (n_rows, n_cols), np.int32), int_weights(rng, (n_rows, n_cols), np.int16)
    return edges, xs, v, w, {"f64": 0, "i64": 1, "mixed": 3}[dom]


TILE_FORMS = {"f64_D1": (F64, 1, 2_048), "f32_D1": (F32, 1, 4_096), "f64_D2": (F64, 2, 2_048), "f32_D2": (F32, 2, 2_048)}


def tile_cols(form):
    T = TILE_FORMS[form][2]
    return (T - 1, T, T + 1)


def tile_data(form, n_rows, n_cols):
    st, D, T = TILE_FORMS[form]
    seed = 2_500 + n_cols + 7 * n_rows
    edges = [edges_of("k1", nb, seed=seed + d) for d, nb in enumerate((300,) if D == 1 else (24, 12))]
    rng = np.random.default_rng(seed)
    xs = [rng.uniform(-3.9, 3.9, (n_rows, n_cols)).astype(st) for _ in edges]  # every element counts: the last one too
    v, w = sx.narrow(rng, (n_rows, n_cols), st), int_weights(rng, (n_rows, n_cols), st)
    return edges, xs, v, w


LAYOUT_SHAPE = (4, 3_001)
LAYOUTS = [(which, how) for which in ("v", "w") for how in ("offset", "stride2", "dtype", "row0")]


def layout_data(sdt, which, how):
    st = _st(sdt)
    seed = 2_700 + 10 * LAYOUTS.index((which, how)) + (st == F32)
    edges = [edges_of("k2", 250, seed=seed)]
    xs = float_samples(edges, *LAYOUT_SHAPE, st, seed)
    other = F32 if st == F64 else F64
    shape = {w_: ((1, LAYOUT_SHAPE[1]) if (which, how) == (w_, "row0") else LAYOUT_SHAPE) for w_ in ("v", "w")}
    rng = np.random.default_rng(seed)
    v = sx.narrow_nan(rng, shape["v"], other if (which, how) == ("v", "dtype") else st)
    w = int_weights(rng, shape["w"], other if (which, how) == ("w", "dtype") else st)
    return edges, xs, v, w


def layout_device(a, how, shape):
    """the device tensor of logical `a` in the layout `how`: one element off a 16-byte boundary in every row, at column stride
    2, or broadcast over the rows at row stride 0"""
    if how == "offset":
        t = _dev(np.concatenate([np.zeros((a.shape[0], 1), a.dtype), a], axis=1))[:, 1:]
        assert t.data_ptr() % 16
        return t
    if how == "stride2":
        t = _dev(np.repeat(a, 2, axis=1))[:, ::2]
        assert t.stride(1) == 2
        return t
    if how == "row0":
        t = _dev(a).expand(*shape)
        assert t.stride(0) == 0
        return t
    return _dev(a)


COPIES = [(30, 16), (50, 8), (100, 4), (200, 2), (400, 1)]  # (C4's 50 bins get 8 copies of the 40-byte slot, C2's 100 get 4)


def copies_data(nb, sdt):
    st = _st(sdt)
    edges = [edges_of("lin", nb, seed=nb)]
    shape = (8, 9 * nb + 1)
    xs = float_samples(edges, *shape, st, 2_900 + nb)
    v, w = _values_and_weights(2_900 + nb + (st == F32), shape, st, st)
    return edges, xs, v, w


def border_cases():
    """(border, bins, edge kind, values of another dtype, expected family, home) on both sides of every border the 40-byte slot
    moves: the fine tables next to the slots, the slots alone (arithmetic edges), the generic family's slots next to its tables"""
    fine = _last(lambda n: table_bytes([np.zeros(n + 1)], "fine64") + n * SLOT2 <= LDS_MAX)
    arith = LDS_MAX // SLOT2
    gen = _last(lambda n: table_bytes([np.zeros(n + 1)], "native") + n * SLOT2 <= LDS_MAX)
    return [("fine", fine, "k1", False, "fast", "lds"), ("fine", fine + 1, "k1", False, "generic", "global"),
            ("fine", fine + 1, "lin", False, "fast", "lds"),
            ("arith", arith, "lin", False, "fast", "lds"), ("arith", arith + 1, "lin", False, "generic", "global"),
            ("generic_lds", gen, "k1", True, "generic", "lds"), ("generic_lds", gen + 1, "k1", True, "generic", "global")]


BORDERS = border_cases()
BORDER_SHAPE = (1, 9_001)


def border_data(i):
    border, nb, kind, other, _, _ = BORDERS[i]
    edges = [edges_of(kind, nb, seed=3_100 + i)]
    xs = float_samples(edges, *BORDER_SHAPE, F64, 3_100 + i)
    v, w = _values_and_weights(3_100 + i, BORDER_SHAPE, F32 if other else F64, F64)
    return edges, xs, v, w


def rules_data():
    rng = np.random.default_rng(3_300)
    edges = [edges_of("k1", 120, seed=33)]
    xs = float_samples(edges, 2, 1_201, F64, 33)
    return edges, xs, sx.narrow_nan(rng, xs[0].shape, F64), int_weights(rng, xs[0].shape, F64)


def cases():
    """every shape of this module: name -> (edges, samples, values, weights)"""
    out = {}
    for form in FORMS:
        for sdt in ("f64", "f32"):
            for D in (1, 2):
                out["form-%s-%s-%d" % (form, sdt, D)] = form_data(form, sdt, D)[:4]
    for dom in DOMS:
        for home in HOMES:
            out["generic-%s-%s" % (dom, home)] = generic_data(dom, home)[:4]
    for form in TILE_FORMS:
        for n_cols in tile_cols(form):
            out["tile-%s-%d" % (form, n_cols)] = tile_data(form, 2, n_cols)
    for sdt in ("f64", "f32"):
        for which, how in LAYOUTS:
            out["layout-%s-%s-%s" % (sdt, which, how)] = layout_data(sdt, which, how)
        for nb, _ in COPIES:
            out["copies-%s-%d" % (sdt, nb)] = copies_data(nb, sdt)
    for i in range(len(BORDERS)):
        out["border-%d" % i] = border_data(i)
    out["rules"] = rules_data()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# every fast form: f32 / f64 x D 1 / 2 x SCAN 1 / 2 / arith  (24 of the binning kernels, both finalize kernels)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("sdt", ["f64", "f32"])
@pytest.mark.parametrize("form", FORMS)
def test_fast_forms(xh, form, sdt, D):
    edges, xs, v, w, fine, arith = form_data(form, sdt, D)
    want = predict_sk(_cus(), edges, 0, xs[0].dtype, v.dtype, *FORM_SHAPE, fine, arith)
    assert want["family"] == "fast" and (want["scan"] == 5) == (form == "arith"), want
    hits = case(xh, edges, xs, v, w, fine=fine, arith=arith, ddof=D - 1, bias=D == 1, fisher=sdt == "f64",
                what="%s %s D=%d" % (form, sdt, D))
    for hit in hits:
        assert hit["family"] == "fast" and hit["D"] == D and (hit["scan"] == 5) == (form == "arith")
        assert hit["lds_bytes"][1] > hit["lds_bytes"][0] > 0


# ---------------------------------------------------------------------------------------------------------------------
# the generic family: CMP 0 / 1 / 3, slots in LDS or sums in global memory  (12 of the binning kernels)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("home", HOMES)
@pytest.mark.parametrize("dom", DOMS)
def test_generic_domain_and_home(xh, dom, home):
    edges, xs, v, w, cmp = generic_data(dom, home)
    for hit in case(xh, edges, xs, v, w, cmp=cmp, fine=False, ddof=1, what="%s %s" % (dom, home)):
        assert hit["family"] == "generic" and hit["slots"] == ("lds" if home == "lds" else "global") and hit["cmp"] == cmp


# ---------------------------------------------------------------------------------------------------------------------
# ragged tiles, alignment and layouts per stream
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(TILE_FORMS))
def test_ragged_last_tile(xh, form):
    """rows one element short of the fast body's tile, exactly one tile, and one element past it: every element counts, the
    last one too"""
    for n_cols in tile_cols(form):
        edges, xs, v, w = tile_data(form, 2, n_cols)
        ok, _, _ = flat_of(xs, edges)
        assert ok.all()
        for hit in case(xh, edges, xs, v, w, what="tile %s %d" % (form, n_cols)):
            assert hit["family"] == "fast"


@pytest.mark.parametrize("which,how", LAYOUTS, ids=["%s-%s" % c for c in LAYOUTS])
@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_layout_per_stream(xh, sdt, which, how):
    """the values (v) or the weights (w) alone one element off the 16-byte boundary (fast: element alignment is enough), at a
    column stride or of another dtype (either sends the call to the generic family; the weights' only the weighted call), or
    broadcast over the rows at row stride 0 (fast)"""
    edges, xs, v, w = layout_data(sdt, which, how)
    dev = ([_dev(x) for x in xs], layout_device(v, how if which == "v" else "plain", LAYOUT_SHAPE),
           layout_device(w, how if which == "w" else "plain", LAYOUT_SHAPE))
    generic = how in ("stride2", "dtype")
    hits = case(xh, edges, xs, v, w, fine=2, layout_fast=not (generic and which == "v"), w_fast=not (generic and which == "w"),
                dev=dev, what="%s %s %s" % (sdt, which, how))
    assert hits[0]["family"] == ("generic" if generic and which == "v" else "fast")
    assert hits[1]["family"] == ("generic" if generic else "fast")


# ---------------------------------------------------------------------------------------------------------------------
# copies of the 40-byte slot, and the LDS borders it moves
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,copies", COPIES, ids=[str(n) for n, _ in COPIES])
@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_copies(xh, nb, copies, sdt):
    edges, xs, v, w = copies_data(nb, sdt)
    for hit in case(xh, edges, xs, v, w, arith=True, what="copies %d" % copies):
        assert hit["family"] == "fast" and hit["copies"] == copies
    assert {c for _, c in COPIES} == {1, 2, 4, 8, 16}


@pytest.mark.parametrize("i", range(len(BORDERS)), ids=["%s-%d-%s" % b[:3] for b in BORDERS])
def test_lds_border(xh, i):
    """both sides of the three borders of the 40-byte slot (mean_var's 24-byte slot puts them elsewhere: its tests do not touch
    these)"""
    border, nb, kind, other, family, home = BORDERS[i]
    edges, xs, v, w = border_data(i)
    for hit in case(xh, edges, xs, v, w, arith=kind == "lin", what="border %s %d" % (border, nb)):
        assert (hit["family"], hit["slots"]) == (family, home), hit


def test_borders_sit_where_the_slot_says():
    assert [b[1] for b in BORDERS if b[0] == "arith"] == [4096, 4097]  # 160 KiB / 40 B
    assert [b[1] for b in BORDERS if b[0] == "fine"] == [3071, 3072, 3072]
    assert [b[1] for b in BORDERS if b[0] == "generic_lds"] == [3071, 3072]


# ---------------------------------------------------------------------------------------------------------------------
# more than one row chunk, through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["sk", "skw"])
def test_more_than_one_row_chunk(xh, weighted):
    """test_gpu_values_census_streams' N_ROWS rows of one column through grouped views of periodic arrays: every row holds one
    sample or none, so every plane is known bit for bit (x, the mean = the value, moments 0 where x != 0 and NaN elsewhere).  The
    three moment planes are N_ROWS * 2 elements apart whatever the chunk, while the pointers advance by the chunk's rows.
    Weighted: float32 weights, the generic family (five chunks); unweighted: the fast family (three)."""
    from xhistogram_amd import _native

    N = cs.N_ROWS
    tvc._need(N * 2 * 8 * 7)
    xs, a, wts = cs._periodic("mean_var_w")
    xs_t, a_t, w_t = _dev(xs), _dev(a), _dev(wts.astype(F32))
    sv = [_native.make_view(xs_t.data_ptr(), _native.F64, 1, 1, inner_rows=cs.P_S, outer_stride=0)]
    vv = _native.make_view(a_t.data_ptr(), _native.F64, 1, 1, inner_rows=cs.P_A, outer_stride=0)
    wv = _native.make_view(w_t.data_ptr(), _native.F32, 1, 1, inner_rows=cs.P_B, outer_stride=0)
    plan = cs._abi_plan(xh, [cs.CHUNK_EDGES])
    first = torch.empty((N, 2), dtype=torch.float64 if weighted else torch.int64, device="cuda")
    mean = torch.empty((N, 2), dtype=torch.float64, device="cuda")
    mom = torch.empty((3, N, 2), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if weighted:
        plan.execute_skew_kurt_weighted(sv, vv, wv, N, 1, first.data_ptr(), mean.data_ptr(), mom.data_ptr(), stream=stream)
    else:
        plan.execute_skew_kurt(sv, vv, N, 1, first.data_ptr(), mean.data_ptr(), mom.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    want = predict_sk(_cus(), [cs.CHUNK_EDGES], 0, F64, F64, N, 1, True, True, not weighted)
    got = assert_sk_variant(plan.describe(), want, weighted)
    assert got["family"] == ("generic" if weighted else "fast") and got["segs"] == 1
    chunk = cs.chunk_rows(got["block"], got["segs"])
    assert -(-N // chunk) == (5 if weighted else 3)
    dev = mean.device
    bounds = [torch.arange(max(0, c - 32), min(N, c + 32)) for c in range(0, N + 1, chunk)]
    g = torch.Generator(device="cpu")
    g.manual_seed(7)
    rows = torch.cat(bounds + [torch.arange(N - 4096, N), torch.randint(0, N, (8192,), generator=g)]).to(dev)

    def planes_expected(rows):
        x, v, w = xs_t[rows % cs.P_S], a_t[rows % cs.P_A], w_t[rows % cs.P_B].to(torch.float64)
        counted = (x >= 0.0) & (x <= 1.0) & ~torch.isnan(v)
        here = counted[:, None] & ((x >= 0.5).to(torch.int64)[:, None] == torch.arange(2, device=dev)[None, :])
        nan = torch.full(here.shape, float("nan"), dtype=torch.float64, device=dev)
        zero = torch.zeros_like(nan)
        if weighted:
            W = torch.where(here, w[:, None], zero)
            return W, torch.where(W > 0, v[:, None].expand_as(W), nan), torch.where(W > 0, zero, nan)
        return here.to(torch.int64), torch.where(here, v[:, None], nan), torch.where(here, zero, nan)

    e_first, e_mean, e_mom = planes_expected(rows)
    torch.testing.assert_close(first[rows], e_first, rtol=0, atol=0)
    torch.testing.assert_close(mean[rows], e_mean, rtol=0, atol=0, equal_nan=True)
    for k in range(3):
        torch.testing.assert_close(mom[k][rows], e_mom, rtol=0, atol=0, equal_nan=True, msg=lambda m, k=k: "M%d: %s" % (k + 2, m))
    # whole planes: where the moments are 0 and where NaN, and nothing else
    n_zero = torch.zeros(2, dtype=torch.int64, device=dev)
    got_zero = [torch.zeros(2, dtype=torch.int64, device=dev) for _ in range(3)]
    got_nan = [torch.zeros(2, dtype=torch.int64, device=dev) for _ in range(3)]
    for r0 in range(0, N, 1 << 23):
        r = torch.arange(r0, min(N, r0 + (1 << 23)), device=dev)
        n_zero += (planes_expected(r)[2] == 0).sum(0)
        for k in range(3):
            part = mom[k][r0: r0 + (1 << 23)]
            got_zero[k] += (part == 0).sum(0)
            got_nan[k] += torch.isnan(part).sum(0)
    assert int(n_zero.min()) > N // 8
    for k in range(3):
        assert torch.equal(got_zero[k], n_zero) and torch.equal(got_nan[k], N - n_zero), k


# ---------------------------------------------------------------------------------------------------------------------
# the rules
# ---------------------------------------------------------------------------------------------------------------------
def test_rules_on_the_grid(xh):
    """w == 1 equals the unweighted call; integer weights equal repeated samples; zero weights add nothing; fisher and bias"""
    edges, xs, v, w = rules_data()
    xd, vd = [_dev(x) for x in xs], _dev(v)
    un = run_sk(xh, xd, vd, None, edges)
    ones = run_sk(xh, xd, vd, _dev(np.ones_like(w)), edges)
    x, mean, moments, bounds, exact = expected_of(xs, edges, v)
    want, wb = sx.expected_outputs(x, moments, bounds)
    np.testing.assert_array_equal(ones[0], un[0].astype(F64))
    tvc._bits(ones[1], un[1], "mean, w == 1")
    for k in range(3):  # both calls within the same bound of the same M*; bit for bit where the sums are exact
        g, u = ones[2 + k].reshape(-1), un[2 + k].reshape(-1)
        sx.assert_within(g, want[k], wb[k], None, "w == 1, output %d" % k)
        np.testing.assert_array_equal(g[exact], u[exact])
    # integer weights == the unweighted call on repeated samples, row by row (the rows get different lengths: one at a time)
    for r in range(xs[0].shape[0]):
        rep = w[r].astype(np.int64)
        xr, vr = np.repeat(xs[0][r], rep)[None], np.repeat(v[r], rep)[None]
        got_w = run_sk(xh, [_dev(xs[0][r:r + 1])], _dev(v[r:r + 1]), _dev(w[r:r + 1]), edges, ddof=1, bias=False)
        got_r = run_sk(xh, [_dev(xr)], _dev(vr), None, edges, ddof=1, bias=False)
        xw, _, mw, bw, ew = expected_of([xs[0][r:r + 1]], edges, v[r:r + 1], w[r:r + 1])
        xr_, _, mr, br, er = expected_of([xr], edges, vr)
        np.testing.assert_array_equal(got_w[0].reshape(-1), got_r[0].reshape(-1).astype(F64))
        tvc._bits(got_w[1], got_r[1], "mean, repeated samples")
        ww, wwb = sx.expected_outputs(xw, mw, bw, 1, False, True)
        wr, wrb = sx.expected_outputs(xr_, mr, br, 1, False, True)
        assert ew.any() and np.array_equal(ew, er)
        for k in range(3):  # each within its own bound; the two M* agree to the terms' roundings (w d d against d d, w times)
            sx.assert_within(got_w[2 + k], ww[k], wwb[k], None, "weighted, output %d" % k)
            sx.assert_within(got_r[2 + k], wr[k], wrb[k], None, "repeated, output %d" % k)
            np.testing.assert_array_equal(got_w[2 + k].reshape(-1)[ew], got_r[2 + k].reshape(-1)[ew])
    # zero weights: samples of weight 0 change nothing, whatever their value
    w0 = w.copy()
    zero = np.random.default_rng(1).random(w.shape) < 0.3
    w0[zero] = 0
    v_moved = np.where(zero & ~np.isnan(v), -v, v)
    a = run_sk(xh, xd, vd, _dev(w0), edges)
    b = run_sk(xh, xd, _dev(v_moved), _dev(w0), edges)
    xz, _, mz, bz, ez = expected_of(xs, edges, v, w0)
    wz, wzb = sx.expected_outputs(xz, mz, bz)
    np.testing.assert_array_equal(a[0], b[0])
    tvc._bits(a[1], b[1], "mean, zero weights")
    for k in range(3):
        sx.assert_within(a[2 + k], wz[k], wzb[k], None, "zero weights, output %d" % k)
        sx.assert_within(b[2 + k], wz[k], wzb[k], None, "zero weights moved, output %d" % k)
    # fisher=False adds 3 to the same g2 (the subtraction is the last step)
    kf = run_sk(xh, xd, vd, None, edges, fisher=False)
    wf, wfb = sx.expected_outputs(x, moments, bounds, 0, True, False)
    sx.assert_within(kf[4], wf[2], wfb[2], None, "fisher=False")
    ok = ~np.isnan(want[2])
    np.testing.assert_allclose((wf[2] - want[2])[ok], 3.0, rtol=0, atol=1e-12)


def test_special_values(xh):
    nan = np.nan
    edges = [np.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0])]
    #             bin 0: NaN values only | bin 1: n = 1 | bin 2: constant | bin 3: n = 2 | bin 4: n = 4, symmetric | bin 5: empty
    x = np.array([0.5, 0.5, 1.5, 1.5, 2.5, 2.5, 2.5, 3.5, 3.5, 4.5, 4.5, 4.5, 4.5, 9.0])
    v = np.array([nan, nan, 2.0, nan, 7.0, 7.0, 7.0, 1.0, 3.0, 0.0, 1.0, 3.0, 4.0, 1.0])
    n, mean, var, skew, kurt, _ = xh.histogram_skew_kurt(x, values=v, bins=edges)
    assert n.dtype == np.int64
    np.testing.assert_array_equal(n, [0, 1, 3, 2, 4, 0])
    np.testing.assert_array_equal(mean, [nan, 2.0, 7.0, 2.0, 2.0, nan])
    np.testing.assert_array_equal(var, [nan, 0.0, 0.0, 1.0, 2.5, nan])
    # constant bins (n = 1 and 7, 7, 7) are 0 / 0: NaN; n = 2: skew 0, g2 = 1; the symmetric bin: m4 = (16 + 1 + 1 + 16) / 4
    np.testing.assert_array_equal(skew, [nan, nan, nan, 0.0, 0.0, nan])
    np.testing.assert_array_equal(kurt, [nan, nan, nan, 1.0 - 3.0, 8.5 / 6.25 - 3.0, nan])
    assert not np.signbit(skew[3])
    np.testing.assert_array_equal(xh.histogram_skew_kurt(x, values=v, bins=edges, fisher=False)[4], [nan, nan, nan, 1.0, 8.5 / 6.25, nan])
    # bias=False: the small-count NaNs (scipy keeps the biased value there); ddof likewise
    n, mean, var, skew, kurt, _ = xh.histogram_skew_kurt(x, values=v, bins=edges, bias=False, ddof=2)
    np.testing.assert_array_equal(var, [nan, nan, 0.0, nan, 5.0, nan])
    np.testing.assert_array_equal(np.isnan(skew), [True, True, True, True, False, True])  # x <= 2
    np.testing.assert_array_equal(np.isnan(kurt), [True, True, True, True, False, True])  # x <= 3
    G2 = 3.0 / (2.0 * 1.0) * (5.0 * (8.5 / 6.25) - 3.0 * 3.0) + 3.0
    np.testing.assert_allclose(kurt[4], G2 - 3.0, rtol=4 * vx.U, atol=0)
    assert skew[4] == 0.0
    # weights: a NaN weight makes its own bin NaN and no other; weights that sum to 0 give W == 0 and NaN moments
    w = np.array([1.0, 1.0, 2.0, 1.0, nan, 1.0, 1.0, 2.0, 2.0, 0.0, 1.0, 1.0, 0.0, 1.0])
    W, mean, var, skew, kurt, _ = xh.histogram_skew_kurt(x, values=v, weights=w, bins=edges)
    assert W.dtype == F64
    np.testing.assert_array_equal(W, [0.0, 2.0, nan, 4.0, 2.0, 0.0])
    np.testing.assert_array_equal(mean, [nan, 2.0, nan, 2.0, 2.0, nan])
    np.testing.assert_array_equal(var, [nan, 0.0, nan, 1.0, 1.0, nan])
    np.testing.assert_array_equal(skew, [nan, nan, nan, 0.0, 0.0, nan])
    np.testing.assert_array_equal(kurt, [nan, nan, nan, -2.0, -2.0, nan])
    # n_cols == 0, and inputs with no counted sample
    for xe in (np.zeros(0), np.full(5, 9.0)):
        for wts in (None, np.ones(xe.shape)):
            out = xh.histogram_skew_kurt(xe, values=np.ones(xe.shape), weights=wts, bins=edges)
            assert not out[0].any() and out[0].dtype == (np.int64 if wts is None else F64)
            assert all(np.isnan(o).all() and o.shape == out[0].shape for o in out[1:5])


@pytest.mark.parametrize("weighted", [False, True], ids=["sk", "skw"])
def test_no_columns_through_the_c_abi(xh, weighted):
    """three rows of no columns: no binning launch, the outputs still overwritten (x 0, the mean and the moments NaN)"""
    from xhistogram_amd import _native

    plan = cs._abi_plan(xh, [np.linspace(0.0, 1.0, 6)])
    one = torch.zeros(4, dtype=torch.float64, device="cuda")
    view = _native.make_view(one.data_ptr(), _native.F64, 0, 1)
    first = torch.full((3, 5), 7, dtype=torch.float64 if weighted else torch.int64, device="cuda")
    mean = torch.full((3, 5), 7.0, dtype=torch.float64, device="cuda")
    mom = torch.full((3, 3, 5), 7.0, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if weighted:
        plan.execute_skew_kurt_weighted([view], view, view, 3, 0, first.data_ptr(), mean.data_ptr(), mom.data_ptr(), stream=stream)
    else:
        plan.execute_skew_kurt([view], view, 3, 0, first.data_ptr(), mean.data_ptr(), mom.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert not first.any() and bool(torch.isnan(mean).all()) and bool(torch.isnan(mom).all())
    desc = plan.describe()
    assert desc.startswith("skew_kurt_w pass1=mvw_sum_none " if weighted else "skew_kurt pass1=mv_sum_none "), desc
    assert (" pass2=skw_dev_none " if weighted else " pass2=sk_dev_none ") in desc, desc


# ---------------------------------------------------------------------------------------------------------------------
# accuracy of the design
# ---------------------------------------------------------------------------------------------------------------------
def _terms_allowance(vals, mean, x, w=None):
    """skew_kurt_exact's bound with the roundings of the terms themselves added to each sum: S_k also stands for the sum of the
    exactly formed terms then (d, w d and the k - 1 products each within u relative: g(2 k + 2) A_k), so the finalized values
    bound the kernel's distance AND the truth's distance from the host's evaluation"""
    sums = sx.kernel_sums(vals, mean, w)
    terms = sx.kernel_terms(vals, mean, w)
    import math

    sums = [sx.Err(s.val, s.err + vx.gamma(2 * k + 4) * math.fsum(np.abs(t))) for k, (s, t) in enumerate(zip(sums, terms))]
    return sx.finalize(x, *sums)


def test_accuracy_at_large_offset(xh):
    """values at 10^8 + N(0, 1): var, skew and kurt stay within their bound (below 1e-9 absolute in every bin) of the oracle,
    the exact central moments of the raw values; the raw-moment formula evaluated in float64 is off by O(1) or worse"""
    rng = np.random.default_rng(61)
    edges = [np.linspace(-3, 3, 9)]
    x = rng.standard_normal((1, 6_001))
    v = 1e8 + rng.standard_normal(x.shape)
    n, mean, var, skew, kurt = run_sk(xh, [_dev(x)], _dev(v), None, edges)
    want = so.histogram_skew_kurt(x, values=v, bins=edges, axis=1)
    np.testing.assert_array_equal(n, want[0])
    ok, flat, size = flat_of([x], edges)
    worst = 0.0
    for k in range(size):
        vals = v[ok & (flat == k)]
        m2, m3, m4 = _terms_allowance(vals, mean.reshape(-1)[k], float(len(vals)))
        outs = sx.outputs(float(len(vals)), m2, m3, m4)
        for got, w_, o in ((var, want[2], outs[0]), (skew, want[3], outs[1]), (kurt, want[4], outs[2])):
            err = abs(got.reshape(-1)[k] - w_.reshape(-1)[k])
            assert np.isfinite(o.err) and o.err < 1e-9 and err <= 2.0 * o.err, (k, err, float(o.err))
        # the raw moments in float64
        nk = len(vals)
        r1, r2, r3, r4 = (np.sum(vals ** j) / nk for j in (1, 2, 3, 4))
        c2 = r2 - r1 * r1
        c4 = r4 - 4 * r1 * r3 + 6 * r1 * r1 * r2 - 3 * r1 ** 4
        with np.errstate(all="ignore"):
            naive = c4 / (c2 * c2) - 3.0
        worst = max(worst, abs(naive - want[4].reshape(-1)[k]) if np.isfinite(naive) else np.inf)
    assert worst > 1.0, worst


# ---------------------------------------------------------------------------------------------------------------------
# backends
# ---------------------------------------------------------------------------------------------------------------------
def backend_data():
    rng = np.random.default_rng(71)
    edges = [np.linspace(-3, 3, 25)]
    x = rng.standard_normal((5, 1_500))
    return edges, x, sx.narrow_nan(rng, x.shape, F64), int_weights(rng, (1, 1_500), F64)


def test_backends(xh):
    from xhistogram_amd.devicearray import DeviceArray

    edges, x, v, w = backend_data()
    for wts in (None, w):
        xe, mean, moments, bounds, exact = expected_of([x], edges, v, wts)
        want, wb = sx.expected_outputs(xe, moments, bounds, 1, False, True)
        kw = dict(bins=edges, axis=1, ddof=1, bias=False)
        got_np = xh.histogram_skew_kurt(x, values=v, weights=wts, **kw)
        assert all(isinstance(g, np.ndarray) for g in got_np[:5]) and got_np[0].dtype == (np.int64 if wts is None else F64)
        assert np.array_equal(got_np[5][0], edges[0])
        xd, vd = _dev(x), _dev(v)
        wd = None if wts is None else _dev(wts).expand(*x.shape)
        got_t = xh.histogram_skew_kurt(xd, values=vd, weights=wd, **kw)
        assert all(t.device.type == "cuda" for t in got_t[:5]) and got_t[0].dtype == (torch.int64 if wts is None else torch.float64)
        DA = DeviceArray.from_numpy
        got_d = xh.histogram_skew_kurt(DA(x, 0), values=DA(v, 0), weights=None if wts is None else DA(wts, 0), **kw)
        assert all(isinstance(g, np.ndarray) for g in got_d[:5])
        for got in (got_np, got_t, got_d):
            np.testing.assert_array_equal(_np(got[0]).reshape(-1), xe)
            tvc._bits(_np(got[1]), mean, "mean")
            for k in range(3):
                sx.assert_within(_np(got[2 + k]), want[k], wb[k], None, "output %d" % k)
        # a reduction over everything and over a leading axis, against the oracle from the raw values
        for axis in (None, (0,)):
            got = xh.histogram_skew_kurt(xd, values=vd, weights=wd, bins=edges, axis=axis)
            ref = so.histogram_skew_kurt(x, values=v, weights=wts, bins=edges, axis=axis)
            np.testing.assert_array_equal(_np(got[0]), ref[0])
            for g, r in zip(got[1:5], ref[1:]):
                np.testing.assert_allclose(_np(g), r, rtol=1e-11, atol=1e-11, equal_nan=True)


def test_xarray(xh):
    try:
        import xarray as xr
    except ImportError:  # the small double of tests/doubles, as tests/test_xarray_wrapper.py uses it
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "doubles"))
        import xarray as xr
    from xhistogram_amd import xarray as xhx

    rng = np.random.default_rng(81)
    coords = {"time": np.arange(4), "lat": np.arange(6) * 1.5, "lon": np.arange(8) * 2.0}
    T = xr.DataArray(rng.uniform(0, 10, (4, 6, 8)), dims=("time", "lat", "lon"), name="T", coords=coords)
    o2 = xr.DataArray(sx.narrow_nan(rng, (4, 6, 8), F64), dims=("time", "lat", "lon"), name="o2", coords=coords)
    area = xr.DataArray(int_weights(rng, (6, 8), F64), dims=("lat", "lon"), name="area", coords={"lat": coords["lat"], "lon": coords["lon"]})
    edges = np.linspace(0, 10, 6)
    for wts, first in ((None, "o2_count"), (area, "o2_sum_of_weights")):
        out = xhx.histogram_skew_kurt(T, values=o2, weights=wts, bins=[edges], dim=["lat", "lon"], keep_coords=True)
        assert [o.name for o in out] == [first, "o2_mean", "o2_var", "o2_skew", "o2_kurt"]
        assert all(tuple(o.dims) == ("time", "T_bin") for o in out)
        np.testing.assert_array_equal(np.asarray(out[0].coords["T_bin"].values), 0.5 * (edges[:-1] + edges[1:]))
        wh = None if wts is None else np.broadcast_to(wts.values, (4, 6, 8)).reshape(4, 48)
        xe, mean, moments, bounds, _ = expected_of([T.values.reshape(4, 48)], [edges], o2.values.reshape(4, 48), wh)
        want, wb = sx.expected_outputs(xe, moments, bounds)
        np.testing.assert_array_equal(np.asarray(out[0].values).reshape(-1), xe)
        for k in range(3):
            sx.assert_within(np.asarray(out[2 + k].values), want[k], wb[k], None, "xarray output %d" % k)


def test_dask_chunked_equals_unchunked():
    env = dict(os.environ)
    sys_cxx = "/usr/lib/x86_64-linux-gnu/libstdc++.so.6"  # (as tests/test_dask_branch.py: conda's libstdc++ is older)
    if os.path.exists(sys_cxx):
        env["LD_PRELOAD"] = (sys_cxx + ":" + env["LD_PRELOAD"]) if env.get("LD_PRELOAD") else sys_cxx
    r = subprocess.run([PY39, "-W", "ignore", SCRIPT], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "SKEW-KURT-DASK-OK" in r.stdout
