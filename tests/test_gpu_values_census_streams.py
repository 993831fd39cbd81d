"""A directed census of the launch variants of histogram_cov and of histogram_mean_var with weights: the statistics of
xhist_values.hip.h that read a THIRD input stream (the weights, or b of cov) with a layout of its own, and, for cov, write
blocks of output planes and keep slots of 24 and 56 bytes.

tests/test_gpu_values_census.py does this for the two statistics of one value array; the cases here are built for what only
a third stream or cov's slots and planes reach: the copies of the 24 / 56-byte slots, every LDS border with those slots, the
generic family's domains and homes, more than two sample arrays (all four statistics), ragged tiles in the halved form of
the weighted float64 pairs, each stream misaligned on its own, a row layout per stream through the C ABI (the per-lane element
index of the generic body included), and more than one row chunk, where cov's plane distance and the per-chunk advance of its
output pointers differ.  Every case asserts
  - its whole describe() line against test_gpu_cov.predict_cov / test_gpu_values_census.predict("mean_var", ...), with the
    fast family given up when the third stream alone disqualifies it (`third_stream_fast`, restated from choose_values);
  - cov: count, both means bit for bit, var_a, var_b, cov_ab bit for bit on power-of-two counts up to 2^9 and within the
    bounds of tests/cov_exact.py elsewhere (test_gpu_cov.check_exact);
  - weighted mean_var: W and the mean bit for bit, the variance bit for bit where W is a power of two up to 2^8 and within
    meanvar_weighted_oracle.m2_bound elsewhere (test_gpu_meanvar_weighted.check_exact).
Samples come from float_samples / int_samples of the first census, values are on values_exact.grid with NaNs put
independently into a and b, weights are the integers 0..7.  What needs no GPU of all this (the borders, the chunk counts,
the data conditions of the copies and tile cases) is spelled out in tests/test_values_census_cpu.py."""
import numpy as np
import pytest

import meanvar_oracle as mo
import meanvar_weighted_oracle as mwo
import test_gpu_cov as tgc
import test_gpu_meanvar_weighted as tgw
import test_gpu_values_census as tvc
import values_exact as vx
from test_gpu_census import edges_of
from test_gpu_cov import assert_cov_variant, nan_grid, predict_cov, run_cov
from test_gpu_meanvar_weighted import as_unweighted_line, int_weights
from test_gpu_parity import _plan_for, xh  # noqa: F401  (xh: the module fixture)
from test_gpu_values_census import (HOME_BINS, LDS_MAX, SLOTS, _cus, _domain_edges, _last, _need, _tag, assert_variant,
                                    case_public, float_samples, int_samples, predict, table_bytes)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F64, F32 = np.float64, np.float32
STATS = ("cov", "mean_var_w")
HITS = []  # (stat, parsed describe) of every case_cov / case_weighted: the variants reached, for the closing test


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _st(sdt):
    return F64 if sdt == "f64" else F32


# ---------------------------------------------------------------------------------------------------------------------
# the launcher's choice for a third stream, restated (choose_values of xhist_values.hip.h)
# ---------------------------------------------------------------------------------------------------------------------
def third_stream_fast(sdt, xdt, x_cs, n_cols, x_ptr=0):
    """whether the weights (b of cov) leave the fast family to samples and values that qualify for it: the sample dtype, unit
    column stride (or one column), an element-aligned pointer"""
    sdt = np.dtype(sdt)
    return np.dtype(xdt) == sdt and (x_cs == 1 or n_cols == 1) and x_ptr % sdt.itemsize == 0


def chunk_rows(block, segs):
    """the rows of one launch (values_geometry): the grid below 2^31 workgroups and 2^32 lanes"""
    return min((1 << 31) - 1, ((1 << 32) - 1) // block) // segs


def _cmp(samples, edges):
    """samples and edges in the domain they are compared in: float64 if either side is a float (numpy's promotion), the
    integers otherwise, datetimes as the int64 they are"""
    cs, ce = [], []
    for s, e in zip(samples, edges):
        s, e = np.asarray(s), np.asarray(e)
        if s.dtype.kind == "M":
            s, e = s.view(np.int64), e.astype(s.dtype).view(np.int64)
        elif s.dtype.kind == "f" or e.dtype.kind == "f":
            s, e = s.astype(F64), e.astype(F64)
        cs.append(s)
        ce.append(e)
    return cs, ce


# ---------------------------------------------------------------------------------------------------------------------
# one case of each statistic
# ---------------------------------------------------------------------------------------------------------------------
def _abi_plan(core, edges):
    from xhistogram_amd import _native

    return core._get_plan([np.asarray(e, F64) for e in edges], _native.CMP_F64, 0)


def abi_cov(core, edges, views, n_rows, n_cols):
    """histogram_cov on C ABI views (sample views, a view, b view): (plan, count [R, B], means [2, R, B], moments [3, R, B])"""
    plan = _abi_plan(core, edges)
    sv, av, bv = views
    cnt = torch.empty((n_rows, plan.n_bins), dtype=torch.int64, device="cuda")
    mean = torch.empty((2, n_rows, plan.n_bins), dtype=torch.float64, device="cuda")
    co = torch.empty((3, n_rows, plan.n_bins), dtype=torch.float64, device="cuda")
    plan.execute_cov(sv, av, bv, n_rows, n_cols, cnt.data_ptr(), mean.data_ptr(), co.data_ptr(),
                     stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return plan, cnt, mean, co


def abi_weighted(core, edges, views, n_rows, n_cols):
    """weighted histogram_mean_var on C ABI views (sample views, value view, weight view): (plan, W, mean, M2), [R, B] each"""
    plan = _abi_plan(core, edges)
    sv, vv, wv = views
    outs = [torch.empty((n_rows, plan.n_bins), dtype=torch.float64, device="cuda") for _ in range(3)]
    plan.execute_mean_var_weighted(sv, vv, wv, n_rows, n_cols, *[o.data_ptr() for o in outs],
                                   stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (plan,) + tuple(outs)


def case_cov(core, cus, edges, xs, a, b, *, cmp=0, fine=True, arith=False, layout_fast=True, third=None, ddof=0, dev=None,
             views=None, hist=True, what=""):
    """xs, a, b: the logical host arrays [R, C] (a, b broadcastable to it); dev: the (samples, a, b) to hand to the public API
    (default: device copies of the host arrays); views: C ABI views (sample views, a view, b view) to run instead;
    third: (dtype, column stride, pointer) of b as the launcher sees it (default: b's dtype, stride 1)"""
    n_rows, n_cols = xs[0].shape
    sdt, vdt = xs[0].dtype, np.asarray(a).dtype
    xdt, x_cs, x_ptr = third if third is not None else (np.asarray(b).dtype, 1, 0)
    lf = layout_fast and third_stream_fast(sdt, xdt, x_cs, n_cols, x_ptr)
    want = predict_cov(cus, edges, cmp, sdt, vdt, n_rows, n_cols, fine, arith, lf)
    xc, ec = _cmp(xs, edges)
    if views is not None:
        plan, cnt, mean, co = abi_cov(core, edges, views, n_rows, n_cols)
        cnt, mean, co = _np(cnt), _np(mean), _np(co)
        got = (cnt, mean[0], mean[1], mo.var_of(cnt, co[0], ddof), mo.var_of(cnt, co[2], ddof), mo.var_of(cnt, co[1], ddof))
        xs_dev = None
    else:
        xs_dev, a_dev, b_dev = dev if dev is not None else ([_dev(x) for x in xs], _dev(a), _dev(b))
        got = run_cov(core, xs_dev, a_dev, b_dev, edges, ddof=ddof)
        plan = _plan_for(core, xs_dev, edges)
    hit = assert_cov_variant(plan.describe(), want)
    HITS.append(("cov", hit))
    cnt, exact = tgc.check_exact(core, xc, ec, a, b, got, xs_dev=xs_dev if hist else None, ddof=ddof, what=what)
    return hit, cnt, exact


def case_weighted(core, cus, edges, xs, v, w, *, cmp=0, fine=True, arith=False, layout_fast=True, third=None, ddof=0, dev=None,
                  views=None, what=""):
    """case_cov's arguments, for histogram_mean_var with weights: v the values, w the weights"""
    n_rows, n_cols = xs[0].shape
    sdt, vdt = xs[0].dtype, np.asarray(v).dtype
    xdt, x_cs, x_ptr = third if third is not None else (np.asarray(w).dtype, 1, 0)
    lf = layout_fast and third_stream_fast(sdt, xdt, x_cs, n_cols, x_ptr)
    want = predict("mean_var", cus, edges, cmp, sdt, vdt, n_rows, n_cols, fine, arith, lf)
    xc, ec = _cmp(xs, edges)
    if views is not None:
        plan, W, mean, m2 = abi_weighted(core, edges, views, n_rows, n_cols)
        W, mean, m2 = _np(W), _np(mean), _np(m2)
        got = (W, mean, mwo.var_of(W, m2, ddof))
    else:
        xs_dev, v_dev, w_dev = dev if dev is not None else ([_dev(x) for x in xs], _dev(v), _dev(w))
        got = tgw.run_w(core, xs_dev, v_dev, w_dev, edges, ddof=ddof)
        plan = _plan_for(core, xs_dev, edges)
    hit = assert_variant(as_unweighted_line(plan.describe()), want)
    HITS.append(("mean_var_w", hit))
    shape = xs[0].shape
    W = tgw.check_exact(xc, ec, np.broadcast_to(np.asarray(v), shape), np.broadcast_to(np.asarray(w), shape), got, ddof=ddof,
                        what=what)
    return hit, W


def case_stat(stat, core, cus, edges, xs, a, b, **kw):
    """one case of `stat`: (a, b) are cov's two value arrays, or the values and the weights; returns the parsed describe()"""
    return (case_cov if stat == "cov" else case_weighted)(core, cus, edges, xs, a, b, **kw)[0]


def third_of(stat, rng, shape, dt):
    """the third stream on exactly summable data: cov's b (grid values with NaNs of their own) or integer weights 0..7"""
    return nan_grid(rng, shape, dt) if stat == "cov" else int_weights(rng, shape, dt)


def split_cov(cnt, exact, ddof=0):
    """(bins checked bit for bit, non-empty bins checked against the bound) of a cov check; a count of 1 is not counted among
    the former, its moments being 0 whatever the kernel adds"""
    cnt, exact = np.asarray(cnt).reshape(-1), np.asarray(exact).reshape(-1)
    return int((exact & (cnt > max(1, ddof))).sum()), int((~exact & (cnt > ddof)).sum())


def split_weighted(W, ddof=0):
    """the same of a weighted check: W a power of two from 2 to 2^8 / any other W > ddof"""
    W = np.asarray(W).reshape(-1)
    lg = np.log2(np.where(W > 0, W, 1))
    pow2 = (W > ddof) & (W <= mwo.POW2_EXACT) & (lg == np.round(lg))
    return int((pow2 & (W > 1)).sum()), int(((W > ddof) & ~pow2).sum())


# ---------------------------------------------------------------------------------------------------------------------
# 1. copies of the slots
# ---------------------------------------------------------------------------------------------------------------------
COV_COPIES = [((20,), 16), ((40,), 8), ((80,), 4), ((160,), 2), ((300,), 1), ((4, 5), 16)]
W_COPIES = [((50,), 16), ((100,), 8), ((200,), 4), ((400,), 2), ((600,), 1)]
# (columns, seed) of each copies case, two rows each.  With 40 009 columns no bin of 20 or 40 has a power-of-two count up to 2^9
# (nor a W up to 2^8 among 50 to 200 bins), and the bit-for-bit path of the check would go unused, so the cases of few bins take
# fewer columns: those at which the oracle alone has bins of both kinds (tests/test_values_census_cpu.py holds every entry to
# that)
COPIES_DATA = {
    ("cov", (20,), "f64"): (11_377, 1020), ("cov", (20,), "f32"): (11_377, 1026),
    ("cov", (40,), "f64"): (22_755, 1040), ("cov", (40,), "f32"): (22_755, 1040),
    ("cov", (80,), "f64"): (22_755, 1080), ("cov", (80,), "f32"): (40_009, 1080),
    ("cov", (160,), "f64"): (40_009, 1161), ("cov", (160,), "f32"): (40_009, 1160),
    ("cov", (300,), "f64"): (40_009, 1300), ("cov", (300,), "f32"): (40_009, 1300),
    ("cov", (4, 5), "f64"): (5_689, 1011), ("cov", (4, 5), "f32"): (11_377, 1011),
    ("mean_var_w", (50,), "f64"): (4_055, 1051), ("mean_var_w", (50,), "f32"): (4_055, 1051),
    ("mean_var_w", (100,), "f64"): (8_111, 1100), ("mean_var_w", (100,), "f32"): (8_111, 1100),
    ("mean_var_w", (200,), "f64"): (16_223, 1200), ("mean_var_w", (200,), "f32"): (16_223, 1200),
    ("mean_var_w", (400,), "f64"): (40_009, 1400), ("mean_var_w", (400,), "f32"): (40_009, 1400),
    ("mean_var_w", (600,), "f64"): (40_009, 1600), ("mean_var_w", (600,), "f32"): (40_009, 1600),
}


def copies_data(stat, nbs, sdt, data=None):
    """(edges, samples [2, C], a / values, b / weights) of one copies case; data: (columns, seed) other than COPIES_DATA's"""
    st = _st(sdt)
    n_cols, seed = data or COPIES_DATA[(stat, nbs, sdt)]
    edges = [edges_of("lin", nb, seed=seed + d) for d, nb in enumerate(nbs)]
    xs = float_samples(edges, 2, n_cols, st, seed)
    rng = np.random.default_rng(seed)
    return edges, xs, nan_grid(rng, xs[0].shape, st), third_of(stat, rng, xs[0].shape, st)


def copies_split(stat, edges, xs, a, b):
    """what the oracle alone says of a copies case: (bins to check bit for bit, bins to check against the bound)"""
    xc, ec = _cmp(xs, edges)
    if stat == "cov":
        ok, flat, size = tgc._flat(xc, ec)
        cnt, _, _, _, exact = tgc.cx.expected(flat[ok], a[ok], b[ok], size)
        return split_cov(cnt, exact)
    return split_weighted(mwo.mean_var_w_rows(xc, ec, a, b, exact=True)[0])


@pytest.mark.parametrize("sdt", ["f64", "f32"])
@pytest.mark.parametrize("nbs,copies", COV_COPIES, ids=["x".join(map(str, n)) for n, _ in COV_COPIES])
def test_cov_copies(xh, nbs, copies, sdt):
    edges, xs, a, b = copies_data("cov", nbs, sdt)
    assert predict_cov(_cus(), edges, 0, xs[0].dtype, a.dtype, 1, 1)["copies"] == copies
    hit, cnt, exact = case_cov(xh, _cus(), edges, xs, a, b, arith=True, what="cov copies %d" % copies)
    assert hit["family"] == "fast" and hit["copies"] == copies and hit["D"] == len(nbs)
    bits, bound = split_cov(cnt, exact)
    assert bits >= 1 and bound >= 1, (bits, bound)


@pytest.mark.parametrize("sdt", ["f64", "f32"])
@pytest.mark.parametrize("nbs,copies", W_COPIES, ids=[str(n[0]) for n, _ in W_COPIES])
def test_weighted_copies(xh, nbs, copies, sdt):
    edges, xs, v, w = copies_data("mean_var_w", nbs, sdt)
    assert predict("mean_var", _cus(), edges, 0, xs[0].dtype, v.dtype, 1, 1)["copies"] == copies
    hit, W = case_weighted(xh, _cus(), edges, xs, v, w, arith=True, what="weighted copies %d" % copies)
    assert hit["family"] == "fast" and hit["copies"] == copies
    bits, bound = split_weighted(W)
    assert bits >= 1 and bound >= 1, (bits, bound)


# ---------------------------------------------------------------------------------------------------------------------
# 2. LDS borders: the last bin count a family or home takes, and the next one, which must move
# ---------------------------------------------------------------------------------------------------------------------
SLOT_KEY = {"cov": "cov", "mean_var_w": "mean_var"}  # (the weighted slots have the unweighted sizes)


def border_cases():
    """(stat, sample dtype or "gen", border, bins, edge kind, the family expected) for both sides of every border of both
    statistics, by the logic of test_gpu_values_census.border_cases on SLOTS["cov"] / SLOTS["mean_var"]"""
    out = []
    for stat in STATS:
        slots = SLOTS[SLOT_KEY[stat]]
        for sdt in (F64, F32):
            slot = max(slots[1 if sdt == F32 else 0])
            fine_t = "fine32" if sdt == F32 else "fine64"
            n = _last(lambda n: table_bytes([np.zeros(n + 1)], fine_t) + n * slot <= LDS_MAX)
            # the fine tables no longer fit next to the slots: the generic family, or the table-free arithmetic form
            out += [(stat, sdt, "fine", n, "k1", "fast"), (stat, sdt, "fine", n + 1, "k1", "generic"),
                    (stat, sdt, "fine", n + 1, "lin", "fast")]
            n = LDS_MAX // slot
            out += [(stat, sdt, "arith", n, "lin", "fast"), (stat, sdt, "arith", n + 1, "lin", "generic")]
        slot = max(slots[0])
        n = _last(lambda n: table_bytes([np.zeros(n + 1)], "native") + n * slot <= LDS_MAX)
        out += [(stat, "gen", "generic_lds", n, "k1", "generic"), (stat, "gen", "generic_lds", n + 1, "k1", "generic")]
        n = _last(lambda n: table_bytes([np.zeros(n + 1)], "native") + 1024 <= LDS_MAX)
        out += [(stat, "gen", "tables_in_lds", n, "k1", "generic"), (stat, "gen", "tables_in_lds", n + 1, "k1", "generic")]
    return out


BORDERS = border_cases()


def border_home(stat, border, side, nb, family):
    """(slots, tables_in_lds) a border's side must show; side 0: the last bin count that fits.  The generic family beyond a
    border of the fast one keeps its slots in LDS while the native tables and its largest slot of every bin fit there"""
    if border == "generic_lds":
        return ("lds", 1) if side == 0 else ("global", 1)
    if border == "tables_in_lds":
        return ("global", 1) if side == 0 else ("global", 0)
    if family == "fast":
        return ("lds", 1)
    fits = table_bytes([np.zeros(nb + 1)], "native") + nb * max(SLOTS[SLOT_KEY[stat]][0]) <= LDS_MAX
    return ("lds", 1) if fits else ("global", 1)


def border_predict(i, cus=256):
    """the prediction of BORDERS[i], the dtypes of its samples and of its values"""
    stat, sdt, border, nb, kind, family = BORDERS[i]
    st = F64 if sdt in ("gen", F64) else F32
    vdt = F32 if sdt == "gen" else st  # (values of another dtype: the generic family)
    edges = [edges_of(kind, nb, seed=700 + i)]
    pred = predict_cov if stat == "cov" else (lambda *a: predict("mean_var", *a))
    return pred(cus, edges, 0, st, vdt, 1, 30_011, True, kind == "lin"), edges, st, vdt


@pytest.mark.parametrize("i", range(len(BORDERS)),
                         ids=["%s-%s-%s-%d-%s" % (s, getattr(t, "__name__", t), b, n, k) for s, t, b, n, k, _ in BORDERS])
def test_lds_border(xh, i):
    stat, sdt, border, nb, kind, family = BORDERS[i]
    _, edges, st, vdt = border_predict(i)
    seed = 700 + i
    xs = float_samples(edges, 1, 30_011, st, seed)
    rng = np.random.default_rng(seed)
    a = nan_grid(rng, xs[0].shape, vdt)
    b = third_of(stat, rng, xs[0].shape, vdt)
    hit = case_stat(stat, xh, _cus(), edges, xs, a, b, arith=kind == "lin", what="border %s %s %d" % (stat, border, nb))
    assert hit["family"] == family, hit
    if family == "fast":
        assert hit["slots"] == "lds" and (hit["scan"] == 5) == (kind == "lin"), hit  # (lin: only past the fine border here)
    side = [c[3] for c in BORDERS if c[:3] == (stat, sdt, border)].index(nb)
    assert (hit["slots"], hit["tables_in_lds"]) == border_home(stat, border, side, nb, family), hit


# ---------------------------------------------------------------------------------------------------------------------
# 3. generic domains x homes, completed: what tests/test_gpu_cov.py and tests/test_gpu_meanvar_weighted.py do not run
#    (datetime64 and uint64 above 2^63 in every home, every domain with its tables read through L2), and the int64 input next
#    to a float64 one in every home, for the closing test
# ---------------------------------------------------------------------------------------------------------------------
DOMAIN_HOMES = [(d, h) for d in ("dt", "u64", "mixed") for h in HOME_BINS] + [("f64", "global_tables_l2"), ("i64", "global_tables_l2")]


@pytest.mark.parametrize("stat", STATS)
@pytest.mark.parametrize("dom,home", DOMAIN_HOMES, ids=["%s-%s" % c for c in DOMAIN_HOMES])
def test_generic_domain_and_home(xh, dom, home, stat):
    rng = np.random.default_rng(400 + DOMAIN_HOMES.index((dom, home)))
    nb = HOME_BINS[home] if dom != "mixed" else max(2, HOME_BINS[home] // 6)
    if dom == "mixed" and home == "global_tables_l2":
        nb = 21_000  # (the int64 input's edges alone must leave LDS)
    edges = _domain_edges(dom, nb, rng)
    n_rows, n_cols = 2, 20_011
    cmp = {"f64": 0, "i64": 1, "dt": 1, "u64": 1, "mixed": 3}[dom]
    xs = []
    for d, e in enumerate(edges):
        if np.asarray(e).dtype.kind == "f":
            xs += float_samples([e], n_rows, n_cols, F64, 37 + d)
        else:
            xs += int_samples([e], n_rows, n_cols, None, 37 + d)
    # f64: float64 samples with values of another dtype; i64: an integer a (integer weights) next to float64 values
    vdt = F32 if dom == "f64" else F64
    a = nan_grid(rng, (n_rows, n_cols), vdt)
    b = third_of(stat, rng, (n_rows, n_cols), vdt)
    if dom == "i64":
        if stat == "cov":
            a = vx.grid(rng, (n_rows, n_cols), np.int32)
        else:
            b = b.astype(np.int32)
    host = dom in ("dt", "u64")  # (torch holds neither datetime64 nor these uint64 samples: numpy inputs, uploaded by the call)
    hit = case_stat(stat, xh, _cus(), edges, xs, a, b, cmp=cmp, fine=False, ddof=1, dev=(xs, a, b) if host else None,
                    what="%s %s %s" % (stat, dom, home), **({"hist": not host} if stat == "cov" else {}))
    assert hit["family"] == "generic" and hit["cmp"] == cmp
    assert hit["slots"] == ("lds" if home == "lds" else "global")
    assert hit["tables_in_lds"] == (0 if home == "global_tables_l2" else 1)


# ---------------------------------------------------------------------------------------------------------------------
# 4. more than two sample arrays: the generic body takes up to eight (all four statistics)
# ---------------------------------------------------------------------------------------------------------------------
def many_inputs(which):
    """(edges, samples [2, 20 011] per input) of the cases of 3 and 8 inputs"""
    n_rows, n_cols = 2, 20_011
    if which == "D3_dtypes":  # float64, float32 and int32 samples against float edges: 5 x 4 x 3 bins
        edges = [edges_of("k1", 5, seed=41), edges_of("k2", 4, seed=42), edges_of("lin", 3, seed=43)]
        xs = float_samples(edges[:1], n_rows, n_cols, F64, 41) + float_samples(edges[1:2], n_rows, n_cols, F32, 42)
        xs.append(np.random.default_rng(43).integers(-5, 6, (n_rows, n_cols)).astype(np.int32))  # (-4 and 4 are edges)
    elif which == "D3_global":  # 40 x 40 x 40 bins: no statistic's slots fit in LDS
        edges = [edges_of("k1", 40, seed=44), edges_of("k2", 40, seed=45), edges_of("lin", 40, seed=46)]
        xs = float_samples(edges, n_rows, n_cols, F64, 44)
    else:  # eight inputs of two bins each: 256 bins, slots in LDS
        edges = [edges_of("lin", 2, lo=-4.0 - d, hi=4.0 + d) for d in range(8)]
        xs = float_samples(edges, n_rows, n_cols, F64, 47)
    return edges, xs


@pytest.mark.parametrize("which", ["D3_dtypes", "D3_global", "D8"])
def test_more_than_two_inputs(xh, which):
    edges, xs = many_inputs(which)
    D = len(edges)
    rng = np.random.default_rng(D)
    a = nan_grid(rng, xs[0].shape, F64)
    theirs, tvc.HITS = tvc.HITS, []  # (case_public records into its module's list: a list of this test's for the call)
    try:
        case_public(xh, _cus(), edges, xs, a, what=which)
        hits = [h for _, h in tvc.HITS]
    finally:
        tvc.HITS = theirs
    assert len(hits) == 2
    for stat in STATS:
        hits.append(case_stat(stat, xh, _cus(), edges, xs, a, third_of(stat, rng, xs[0].shape, F64), ddof=1,
                              what="%s %s" % (stat, which)))
    for h in hits:
        assert h["family"] == "generic" and h["D"] == D and h["cmp"] == 0, h
        assert h["slots"] == ("global" if which == "D3_global" else "lds"), h


# ---------------------------------------------------------------------------------------------------------------------
# 5. tiles and segments
# ---------------------------------------------------------------------------------------------------------------------
# the shapes of test_gpu_values_census.test_geometry_segments: (rows, columns (None: one past the fast tile of one input), the
# family, whether a row is one segment).  fast: rows that fill the device over two tiles each / segments per row (twice) / below
# one tile; generic (values and third stream of another dtype) with its slots in LDS: 512-thread blocks, three tiles a row,
# rows that fill the device at cus * 4
SEG_SHAPES = {"rows_fill": (2_048, None, "fast", True), "segments": (64, 20_000, "fast", False), "long_rows": (2, 200_003, "fast", False),
              "below_a_tile": (5, 700, "fast", True), "generic_rows_fill": (1_100, 1_100, "generic", True)}


@pytest.mark.parametrize("stat", STATS)
@pytest.mark.parametrize("shape", list(SEG_SHAPES))
@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_geometry_segments(xh, sdt, shape, stat):
    """12 bins, so that the oracle of 2 048 rows stays quick"""
    st = _st(sdt)
    n_rows, n_cols, family, one = SEG_SHAPES[shape]
    n_cols = n_cols or 256 * 4 * (4 if st == F32 else 2) + 1
    vt = st if family == "fast" else (F64 if st == F32 else F32)
    edges = [edges_of("k1", 12, seed=1)]
    rng = np.random.default_rng(61 + n_rows)
    xs = float_samples(edges, n_rows, n_cols, st, n_rows)
    a = nan_grid(rng, xs[0].shape, vt)
    hit = case_stat(stat, xh, _cus(), edges, xs, a, third_of(stat, rng, xs[0].shape, vt), what="%s rows %d cols %d" % (stat, n_rows, n_cols))
    assert hit["family"] == family and (hit["segs"] == 1) == one, (n_rows, n_cols, hit)


TILE_FORMS = {  # sample dtype, inputs, the fast body's tile in elements, the row lengths around its edges (and its halves')
    "f64_D2": (F64, 2, 2_048, (1_023, 1_024, 1_025, 2_047, 2_048, 2_049, 3_073)),
    "f32_D1": (F32, 1, 4_096, (4_095, 4_096, 4_097, 8_193)),
}


def tile_data(stat, form, n_rows, n_cols):
    """(edges, samples, a / values, b / weights) of one tile-edge case: every sample inside the bins, no NaN anywhere, so
    every element of a row counts"""
    st, D, _, cols = TILE_FORMS[form]
    seed = 800 + 10 * cols.index(n_cols) + n_rows
    edges = [edges_of("k2", 12, seed=3), edges_of("k1", 5, seed=4)][:D]
    rng = np.random.default_rng(seed)
    xs = [rng.uniform(e[0], e[-1], (n_rows, n_cols)).astype(st) for e in edges]
    for x, e in zip(xs, edges):  # (float32 rounding may leave the range: back onto the outer edges' float32 neighbours inside)
        lo = tvc.f32_neighbours(e[:1])[1][0] if st == F32 else e[0]
        hi = tvc.f32_neighbours(e[-1:])[0][0] if st == F32 else e[-1]
        np.clip(x, lo, hi, out=x)
        x[:, 0], x[:, -1] = lo, hi
    a = vx.grid(rng, (n_rows, n_cols), st)
    b = vx.grid(rng, (n_rows, n_cols), st) if stat == "cov" else int_weights(rng, (n_rows, n_cols), st)
    return edges, xs, a, b


@pytest.mark.parametrize("stat", STATS)
@pytest.mark.parametrize("n_rows", [1, 3])
@pytest.mark.parametrize("form", list(TILE_FORMS))
def test_ragged_last_tile(xh, form, n_rows, stat):
    """row lengths one below, at and one above the tile and, for the weighted float64 pairs of two inputs, its halves: the
    second half of a tile, the ragged tile in either half, a full tile followed by a ragged one"""
    st, D, tile, cols = TILE_FORMS[form]
    assert tile == 256 * (16 // np.dtype(st).itemsize) * (4 if D == 1 else 8 // (16 // np.dtype(st).itemsize))
    for n_cols in cols:
        edges, xs, a, b = tile_data(stat, form, n_rows, n_cols)
        what = "%s %s rows %d cols %d" % (stat, form, n_rows, n_cols)
        if stat == "cov":
            hit, cnt, _ = case_cov(xh, _cus(), edges, xs, a, b, what=what)
            np.testing.assert_array_equal(cnt.reshape(n_rows, -1).sum(axis=1), np.full(n_rows, n_cols), err_msg=what)
        else:
            hit, W = case_weighted(xh, _cus(), edges, xs, a, b, what=what)
            np.testing.assert_array_equal(W.reshape(n_rows, -1).sum(axis=1), b.astype(F64).sum(axis=1), err_msg=what)
        assert hit["family"] == "fast" and hit["D"] == D, hit


# ---------------------------------------------------------------------------------------------------------------------
# 6. alignment, one stream at a time
# ---------------------------------------------------------------------------------------------------------------------
def _offset(a, k):
    """a contiguous [R, C] device tensor of `a` that starts k elements past a 16-byte boundary"""
    flat = torch.empty(a.size + k, dtype=torch.as_tensor(a[:0]).dtype, device="cuda")
    assert flat.data_ptr() % 16 == 0
    t = flat[k:].view(a.shape)
    t.copy_(torch.as_tensor(np.ascontiguousarray(a)))
    assert t.data_ptr() % 16 == (k * a.itemsize) % 16
    return t


@pytest.mark.parametrize("stat", STATS)
@pytest.mark.parametrize("stream", ["samples", "a", "b"])
@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_alignment_one_stream(xh, sdt, stream, stat):
    """unit column stride; one of samples / a (values) / b (weights) starts 1 (float32: 1, 2, 3) elements past a 16-byte
    boundary while the other two are aligned; odd row lengths, so that every other row starts off 16 bytes in all three"""
    st = _st(sdt)
    edges = [edges_of("k2", 60, seed=2), edges_of("k1", 7, seed=3)][: 2 if st == F64 else 1]
    rng = np.random.default_rng(71)
    for shape in ((3, 20_011), (65, 301)):
        xs = float_samples(edges, shape[0], shape[1], st, shape[1])
        a = nan_grid(rng, shape, st)
        b = third_of(stat, rng, shape, st)
        for k in ((1,) if st == F64 else (1, 2, 3)):
            dev = ([_offset(x, k if stream == "samples" else 0) for x in xs], _offset(a, k if stream == "a" else 0),
                   _offset(b, k if stream == "b" else 0))
            off = [t.data_ptr() % 16 != 0 for t in dev[0]] + [dev[1].data_ptr() % 16 != 0, dev[2].data_ptr() % 16 != 0]
            assert off == [stream == "samples"] * len(xs) + [stream == "a", stream == "b"]
            hit = case_stat(stat, xh, _cus(), edges, xs, a, b, dev=dev, what="%s offset %d, %s" % (stream, k, shape))
            assert hit["family"] == "fast", hit


# ---------------------------------------------------------------------------------------------------------------------
# 7. the C ABI's row shapes, a layout per stream
# ---------------------------------------------------------------------------------------------------------------------
def _view(t, st, **kw):
    from xhistogram_amd import _native

    return _native.make_view(t.data_ptr(), _tag(st), **kw)


def _views_case(stat, core, edges, xs, a, b, sviews, aview, bview, third, keep, what, layout_fast=True):
    """a case on C ABI views; `keep` holds the device tensors behind them"""
    hit = case_stat(stat, core, _cus(), edges, xs, a, b, views=(sviews, aview, bview), third=third, layout_fast=layout_fast, what=what)
    del keep
    return hit


@pytest.mark.parametrize("stat", STATS)
@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_grouped_rows_fast(xh, sdt, stat):
    """G groups of I rows: samples and a as [G, I + 1, C] with the last row of each group skipped; b / the weights a dense
    [I, C] slab every group shares (outer stride 0): cell areas over (lat, lon) for fields over (time, lat, lon)"""
    st = _st(sdt)
    G, I, C = 5, 7, 3_001
    edges = [edges_of("k1", 30, seed=5), edges_of("lin", 9, seed=6)]
    xs = float_samples(edges, G * I, C, st, 81)
    rng = np.random.default_rng(81)
    a = nan_grid(rng, (G * I, C), st)
    slab = third_of(stat, rng, (I, C), st)

    def lay(t):  # [G*I, C] -> [G, I + 1, C], the logical rows at [g, i, :]
        big = np.full((G, I + 1, C), np.nan, t.dtype)
        big[:, :I, :] = t.reshape(G, I, C)
        return _dev(big)
    kw = dict(row_stride=C, col_stride=1, inner_rows=I, outer_stride=(I + 1) * C)
    xd, ad, bd = [lay(x) for x in xs], lay(a), _dev(slab)
    hit = _views_case(stat, xh, edges, xs, a, np.tile(slab, (G, 1)), [_view(t, st, **kw) for t in xd], _view(ad, st, **kw),
                      _view(bd, st, row_stride=C, col_stride=1, inner_rows=I, outer_stride=0), (st, 1, bd.data_ptr()), (xd, ad, bd),
                      "%s grouped rows, shared slab" % stat)
    assert hit["family"] == "fast", hit


@pytest.mark.parametrize("stat", STATS)
@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_row_stride_zero_per_stream(xh, sdt, stat):
    """one of a / b (values / weights) broadcast across the rows at row stride 0 while the other is dense: the fast family"""
    st = _st(sdt)
    R, C = 6, 12_007
    edges = [edges_of("k1", 80, seed=4)]
    xs = float_samples(edges, R, C, st, 83)
    rng = np.random.default_rng(83)
    for bcast in ("a", "b"):
        a = vx.grid(rng, (1, C), st) if bcast == "a" else nan_grid(rng, (R, C), st)
        b = third_of(stat, rng, (1, C) if bcast == "b" else (R, C), st)
        xd, ad, bd = [_dev(x) for x in xs], _dev(a), _dev(b)
        dense, row0 = dict(row_stride=C, col_stride=1), dict(row_stride=0, col_stride=1)
        hit = _views_case(stat, xh, edges, xs, np.broadcast_to(a, (R, C)), np.broadcast_to(b, (R, C)), [_view(xd[0], st, **dense)],
                          _view(ad, st, **(row0 if bcast == "a" else dense)), _view(bd, st, **(row0 if bcast == "b" else dense)),
                          (st, 1, bd.data_ptr()), (xd, ad, bd), "%s %s at row stride 0" % (stat, bcast))
        assert hit["family"] == "fast", hit


@pytest.mark.parametrize("stat", STATS)
@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_grouped_rows_generic(xh, sdt, stat):
    """samples and a as [G, C, I], the rows the contiguous direction (column stride I); b / the weights one [C] array for every
    row (row stride 0, column stride 1)"""
    st = _st(sdt)
    G, I, C = 5, 7, 3_001
    edges = [edges_of("k1", 30, seed=5), edges_of("lin", 9, seed=6)]
    xs = float_samples(edges, G * I, C, st, 85)
    rng = np.random.default_rng(85)
    a = nan_grid(rng, (G * I, C), st)
    b = third_of(stat, rng, (1, C), st)

    def lay(t):  # [G*I, C] -> [G, C, I]
        return _dev(t.reshape(G, I, C).transpose(0, 2, 1))
    kw = dict(row_stride=1, col_stride=I, inner_rows=I, outer_stride=C * I)
    xd, ad, bd = [lay(x) for x in xs], lay(a), _dev(b)
    hit = _views_case(stat, xh, edges, xs, a, np.broadcast_to(b, (G * I, C)), [_view(t, st, **kw) for t in xd], _view(ad, st, **kw),
                      _view(bd, st, row_stride=0, col_stride=1), (st, 1, bd.data_ptr()), (xd, ad, bd), "%s grouped generic" % stat,
                      layout_fast=False)
    assert hit["family"] == "generic", hit


@pytest.mark.parametrize("stat", STATS)
@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_third_stream_column_stride(xh, sdt, stat):
    """dense samples and a; b / the weights at column stride 3, then 0 (one per row): the third stream alone gives up the fast
    family, and with several segments per row each lane walks its own element index of it (xi, xstep of the generic body)"""
    st = _st(sdt)
    R, C = 2, 20_011
    edges = [edges_of("k1", 30, seed=7)]
    xs = float_samples(edges, R, C, st, 87)
    rng = np.random.default_rng(87)
    a = nan_grid(rng, (R, C), st)
    xd, ad = [_dev(x) for x in xs], _dev(a)
    dense = dict(row_stride=C, col_stride=1)
    for cs in (3, 0):
        b = third_of(stat, rng, (R, C if cs else 1), st)
        if cs:
            wide = third_of(stat, rng, (R, 3 * C), st)  # (the elements between: other numbers, NaNs among them for cov)
            wide[:, ::3] = b
            bd, bview = _dev(wide), dict(row_stride=3 * C, col_stride=3)
        else:
            bd, bview = _dev(b), dict(row_stride=1, col_stride=0)
        hit = _views_case(stat, xh, edges, xs, a, np.broadcast_to(b, (R, C)), [_view(xd[0], st, **dense)], _view(ad, st, **dense),
                          _view(bd, st, **bview), (st, cs, bd.data_ptr()), (xd, ad, bd), "%s third stream at column stride %d" % (stat, cs))
        assert hit["family"] == "generic" and hit["segs"] > 1, hit


@pytest.mark.parametrize("stat", STATS)
@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_one_column_at_column_strides(xh, sdt, stat):
    """n_cols == 1: samples and a at column stride 7 with b / the weights at 0, then the reverse; the fast family takes it (no
    vector load crosses a column)"""
    st = _st(sdt)
    R = 3_000
    edges = [edges_of("k2", 20, seed=8)]
    x = float_samples(edges, R, 1, st, 89)[0]
    rng = np.random.default_rng(89)
    a = nan_grid(rng, (R, 1), st)
    b = third_of(stat, rng, (R, 1), st)

    def lay(t):  # [R, 1] -> the first column of [R, 3]
        big = np.zeros((R, 3), st)
        big[:, 0] = t[:, 0]
        return _dev(big)
    xd, ad, bd = lay(x), lay(a), lay(b)
    for cs_sa, cs_b in ((7, 0), (0, 7)):
        hit = _views_case(stat, xh, edges, [x], a, b, [_view(xd, st, row_stride=3, col_stride=cs_sa)],
                          _view(ad, st, row_stride=3, col_stride=cs_sa), _view(bd, st, row_stride=3, col_stride=cs_b),
                          (st, cs_b, bd.data_ptr()), (xd, ad, bd), "%s one column, strides %d / %d" % (stat, cs_sa, cs_b))
        assert hit["family"] == "fast", hit


# ---------------------------------------------------------------------------------------------------------------------
# 8. row chunks: more rows than one launch takes
# ---------------------------------------------------------------------------------------------------------------------
N_ROWS = 2 * ((1 << 24) - 1) + 70_001  # two full chunks of the fast family and a remainder; four and one of the generic family
P_S, P_A, P_B = 1021, 1031, 1033  # the periods of samples, a and b / weights: pairwise coprime
CHUNK_EDGES = np.array([0.0, 0.5, 1.0])  # two bins: the plane distance (rows * 2) is not the row count


def _periodic(stat):
    rng = np.random.default_rng(91)
    xs = rng.uniform(-0.25, 1.25, P_S)  # about a third outside the edges
    xs[:5] = [0.0, 1.0, np.nan, -0.0, 0.5]
    xs[rng.integers(5, P_S, 20)] = np.nan
    a = vx.grid(rng, P_A)
    a[rng.integers(0, P_A, 60)] = np.nan
    if stat == "cov":
        b = vx.grid(rng, P_B)
        b[rng.integers(0, P_B, 60)] = np.nan
    else:
        b = int_weights(rng, P_B, F64)
    return xs, a, b


def _rows_expected(stat, rows, xs_t, a_t, b_t):
    """(the bin of each of the given rows (int64 tensor), whether its pair counts, a, b as float64)"""
    x, a, b = xs_t[rows % P_S], a_t[rows % P_A], b_t[rows % P_B].to(torch.float64)
    counted = (x >= 0.0) & (x <= 1.0) & ~torch.isnan(a)
    if stat == "cov":
        counted &= ~torch.isnan(b)
    return (x >= 0.5).to(torch.int64), counted, a, b


def _planes_expected(stat, rows, xs_t, a_t, b_t):
    """every output plane of the given rows, [len(rows), 2] each, in the order of `_run_chunks`' planes"""
    bin_, counted, a, b = _rows_expected(stat, rows, xs_t, a_t, b_t)
    here = counted[:, None] & (bin_[:, None] == torch.arange(2, device=rows.device)[None, :])
    nan = torch.full(here.shape, float("nan"), dtype=torch.float64, device=rows.device)
    zero = torch.zeros_like(nan)
    if stat == "cov":  # count, mean_a, mean_b, M2_a, C_ab, M2_b
        moment = torch.where(here, zero, nan)
        return [here.to(torch.int64), torch.where(here, a[:, None], nan), torch.where(here, b[:, None], nan), moment, moment, moment]
    W = torch.where(here, b[:, None], zero)  # W, mean, M2: NaN where W == 0
    return [W, torch.where(W > 0, a[:, None].expand_as(W), nan), torch.where(W > 0, zero, nan)]


def _run_chunks(stat, core, views):
    """the statistic over N_ROWS rows of one column: (plan, output planes [N_ROWS, 2] each)"""
    if stat == "cov":
        plan, cnt, mean, co = abi_cov(core, [CHUNK_EDGES], views, N_ROWS, 1)
        return plan, [cnt, mean[0], mean[1], co[0], co[1], co[2]]
    plan, W, mean, m2 = abi_weighted(core, [CHUNK_EDGES], views, N_ROWS, 1)
    return plan, [W, mean, m2]


def chunk_count(block, segs=1):
    return -(-N_ROWS // chunk_rows(block, segs))


@pytest.mark.parametrize("family", ["fast", "generic"])
@pytest.mark.parametrize("stat", STATS)
def test_more_than_one_row_chunk(xh, stat, family):
    """N_ROWS rows of one column through grouped views of three periodic arrays (row r reads element r mod P of each).  The
    rows go out in chunks (values_geometry); cov's planes are N_ROWS * 2 elements apart whatever the chunk, while its pointers
    advance by the chunk's rows.  Every row holds one pair or none, so every plane is known bit for bit: the rows on both sides
    of every chunk boundary, the last rows, random rows, and whole-plane sums.  generic: b / the weights are float32"""
    from xhistogram_amd import _native

    _need(N_ROWS * 2 * 8 * (8 if stat == "cov" else 4))
    xs, a, b = _periodic(stat)
    bt = F64 if family == "fast" else F32
    xs_t, a_t, b_t = _dev(xs), _dev(a), _dev(b.astype(bt))
    views = ([_native.make_view(xs_t.data_ptr(), _native.F64, 1, 1, inner_rows=P_S, outer_stride=0)],
             _native.make_view(a_t.data_ptr(), _native.F64, 1, 1, inner_rows=P_A, outer_stride=0),
             _native.make_view(b_t.data_ptr(), _tag(bt), 1, 1, inner_rows=P_B, outer_stride=0))
    plan, planes = _run_chunks(stat, xh, views)
    desc = plan.describe()
    pred = predict_cov if stat == "cov" else (lambda *p: predict("mean_var", *p))
    want = pred(_cus(), [CHUNK_EDGES], 0, F64, F64, N_ROWS, 1, True, True, third_stream_fast(F64, bt, 1, 1))
    got = assert_cov_variant(desc, want) if stat == "cov" else assert_variant(as_unweighted_line(desc), want)
    assert got["family"] == family and got["segs"] == 1, desc
    chunk = chunk_rows(got["block"], got["segs"])
    n_chunks = -(-N_ROWS // chunk)
    assert n_chunks > 2 and n_chunks == (3 if family == "fast" else 5), (chunk, n_chunks)
    dev = planes[0].device
    bounds = [torch.arange(max(0, c - 32), min(N_ROWS, c + 32)) for c in range(0, N_ROWS + 1, chunk)]
    g = torch.Generator(device="cpu")
    g.manual_seed(5)
    row_sets = {"chunk boundaries and last rows": torch.cat(bounds + [torch.arange(N_ROWS - 4096, N_ROWS)]).to(dev),
                "random rows": torch.randint(0, N_ROWS, (8192,), generator=g).to(dev)}
    for name, rows in row_sets.items():
        for k, (o, w) in enumerate(zip(planes, _planes_expected(stat, rows, xs_t, a_t, b_t))):
            torch.testing.assert_close(o[rows], w, rtol=0, atol=0, equal_nan=True, msg=lambda m, k=k, name=name: "plane %d, %s: %s" % (k, name, m))
    # whole planes, from the periodic arrays: per bin, the counted rows, the exact sums of their a and b (multiples of 2^-10
    # below 2^37 in any order), and where the moments are 0 and where NaN
    want_n = torch.zeros(2, dtype=torch.int64, device=dev)
    want_s = [torch.zeros(2, dtype=torch.float64, device=dev) for _ in range(2)]
    got_nan = [torch.zeros(2, dtype=torch.int64, device=dev) for _ in planes]
    got_sum = [torch.zeros(2, dtype=torch.float64, device=dev) for _ in planes]
    for r0 in range(0, N_ROWS, 1 << 23):
        rows = torch.arange(r0, min(N_ROWS, r0 + (1 << 23)), device=dev)
        exp = _planes_expected(stat, rows, xs_t, a_t, b_t)
        want_n += (exp[0] != 0).sum(0)
        for s, e in zip(want_s, exp[1:3] if stat == "cov" else (exp[0], exp[1])):
            s += torch.nan_to_num(e, nan=0.0).sum(0)
        for k, o in enumerate(planes):
            part = o[r0: r0 + (1 << 23)]
            got_nan[k] += torch.isnan(part).sum(0) if part.dtype == torch.float64 else (part == 0).sum(0)
            got_sum[k] += torch.nan_to_num(part.to(torch.float64), nan=0.0).sum(0)
    assert int(want_n.min()) > N_ROWS // 8  # (both bins take a good part of the rows)
    if stat == "cov":
        assert torch.equal(got_sum[0], want_n.to(torch.float64))
        assert torch.equal(got_sum[1], want_s[0]) and torch.equal(got_sum[2], want_s[1])
        for k in range(6):
            assert torch.equal(got_nan[k], N_ROWS - want_n), k
        for k in (3, 4, 5):
            assert torch.equal(got_sum[k], torch.zeros_like(got_sum[k])), k
    else:
        assert torch.equal(got_sum[0], want_s[0])  # (the weights of the counted rows)
        assert torch.equal(got_sum[1], want_s[1])
        assert torch.equal(got_nan[0], torch.zeros_like(got_nan[0]))
        assert torch.equal(got_nan[1], N_ROWS - want_n) and torch.equal(got_nan[2], N_ROWS - want_n)
        assert torch.equal(got_sum[2], torch.zeros_like(got_sum[2]))


# ---------------------------------------------------------------------------------------------------------------------
# what the sweep reached
# ---------------------------------------------------------------------------------------------------------------------
# the cases the tests above record when all of them run: copies, borders, domains, inputs, segments, tiles, alignment, layouts
N_CASES = (2 * (len(COV_COPIES) + len(W_COPIES)) + len(BORDERS) + 2 * len(DOMAIN_HOMES) + 2 * 3 + 2 * 2 * 5
           + 2 * 2 * sum(len(f[3]) for f in TILE_FORMS.values()) + 2 * 3 * 2 * (1 + 3) + 2 * 2 * (1 + 2 + 1 + 2 + 2))


def test_zz_variants_reached():
    """every row of the variant table reached by some case of this module, for each of the two statistics (a partial run
    checks only what it ran)"""
    if len(HITS) < N_CASES:
        pytest.skip("only part of the module ran (%d of %d cases)" % (len(HITS), N_CASES))
    for stat in STATS:
        hs = [h for s, h in HITS if s == stat]
        fast = [h for h in hs if h["family"] == "fast"]
        gen = [h for h in hs if h["family"] == "generic"]
        assert {h["copies"] for h in fast} >= {1, 2, 4, 8, 16}, stat
        assert {h["scan"] for h in fast} >= {1, 2, 5}, stat
        assert {h["D"] for h in fast} == {1, 2}, stat
        homes = {(h["cmp"], h["slots"], h["tables_in_lds"]) for h in gen}
        for cmp in (0, 1, 3):
            assert {(cmp, "lds", 1), (cmp, "global", 1), (cmp, "global", 0)} <= homes, (stat, cmp, sorted(homes))
        assert {h["D"] for h in gen} >= {3, 8}, stat
        assert {h["segs"] == 1 for h in hs} == {True, False}, stat
