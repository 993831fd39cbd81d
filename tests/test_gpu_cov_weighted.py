"""histogram_weighted_cov on an MI355X: the kernels of xhist_cov_w.hip against tests/cov_weighted_exact.py and
tests/cov_weighted_oracle.py.

On exactly summable data (both value arrays on values_exact.grid, NaNs put independently into each, integer weights 0..7) W
and both means are checked bit for bit in every bin, and M2_a, C_ab, M2_b bit for bit where W is a power of two up to 2^8 and
within cov_weighted_exact's float64 bounds elsewhere; every such case also asserts that at least one of its bins took the
bit-for-bit path (W from 2 to 2^8: tests/test_cov_weighted_cpu.py holds the data of every shape used here to that without a GPU).
Every case checks its whole describe() line against test_gpu_values_census.predict with cov's slot sizes (24 and 56 bytes,
copies): the weighted line is put into cov's words by `as_cov_line`, as test_gpu_meanvar_weighted.as_unweighted_line does for
mean_var, and the fast family is given up when b or the weights alone disqualify it (`streams_fast`, restated from
choose_values).

The cases: every fast form, every generic kernel (between them all 36 binning kernels of xhist_cov_w.hip plus its moments_mean and
moments_finalize, which tests/test_zz_gpu_census_total.py holds the session to), ragged tiles around the tile's end and around the split point of every
form that reads its tile in halves, each of the four streams misaligned on its own, b and the weights each alone
at a column stride or of another dtype, row stride 0 for either, every number of copies, one LDS border from both sides, more
than one row chunk through the C ABI, the NaN and zero rules, w == 1 and repeated samples against histogram_cov, b = a against
the weighted histogram_mean_var, the backends and dask."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cov_weighted_exact as cwx
import cov_weighted_oracle as cwo
import meanvar_weighted_oracle as mwo
import test_gpu_cov as tgc
import test_gpu_values_census as tvc
import test_gpu_values_census_streams as cs
import values_exact as vx
from test_gpu_census import edges_of
from test_gpu_meanvar_weighted import int_weights
from test_gpu_parity import _plan_for, xh  # noqa: F401  (xh: the module fixture)
from test_gpu_values_census import FORM_EDGES, HOME_BINS, _cus, _domain_edges, _need, _tag, float_samples, int_samples

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F64, F32 = np.float64, np.float32
PY39 = "/opt/conda/bin/python3.9"
SCRIPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cov_weighted_dask_script.py")


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _st(sdt):
    return F64 if sdt == "f64" else F32


def run_cw(core, xs, a, b, w, edges, axis=1, ddof=0):
    out = core.histogram_weighted_cov(*xs, values=(a, b), weights=w, bins=edges, axis=axis, ddof=ddof)[:6]
    torch.cuda.synchronize()
    return tuple(_np(o) for o in out)


# ---------------------------------------------------------------------------------------------------------------------
# the launcher's choice and the describe() line
# ---------------------------------------------------------------------------------------------------------------------
def streams_fast(sdt, n_cols, *streams):
    """whether b and the weights, each given as (dtype, column stride, pointer), leave the fast family to samples and values
    that qualify for it: each must pass choose_values' rule for an extra stream on its own"""
    return all(cs.third_stream_fast(sdt, dt, x_cs, n_cols, ptr) for dt, x_cs, ptr in streams)


def as_cov_line(desc):
    """a weighted cov describe() line in the cov line's words, for test_gpu_cov.assert_cov_variant"""
    assert desc.startswith("cov_w pass1=covw_sum_"), desc
    assert " pass2=covw_dev_" in desc, desc
    return desc.replace("cov_w ", "cov ").replace("covw_", "cov_")


def split(W, exact, ddof=0):
    """(bins checked bit for bit, bins with W > ddof checked against the bound); W <= 1 is not counted among the former, its
    moments being 0 whatever the kernel adds"""
    W, exact = np.asarray(W).reshape(-1), np.asarray(exact).reshape(-1)
    return int((exact & (W > max(1, ddof))).sum()), int((~exact & (W > ddof)).sum())


def expected_of(xs_host, edges, a, b, w):
    """cov_weighted_exact.expected of [R, C] host samples in their compare domain and values / weights broadcastable to them"""
    ok, flat, size = tgc._flat(xs_host, edges)
    a, b, w = (np.broadcast_to(np.asarray(t), ok.shape) for t in (a, b, w))
    return cwx.expected(flat[ok], a[ok], b[ok], w[ok], size)


def check_exact(xs_host, edges, a, b, w, got, ddof=0, what="", need_exact=True):
    """got = (W, mean_a, mean_b, var_a, var_b, cov_ab); returns (W, exact) after asserting that a bin took the bit-for-bit path
    (need_exact=False: random cases, which may have no such bin)"""
    W, (ma, mb), moments, bounds, exact = expected_of(xs_host, edges, a, b, w)
    assert np.asarray(got[0]).dtype == F64
    tvc._bits(got[0], W, "W " + what)
    tvc._bits(got[1], ma, "mean_a " + what)
    tvc._bits(got[2], mb, "mean_b " + what)
    cwx.assert_moments((got[3], got[5], got[4]), moments, bounds, exact, W=W, ddof=ddof, what=what)
    assert not need_exact or split(W, exact, ddof)[0] >= 1, "no bin on the bit-for-bit path (%s)" % what
    return W, exact


def abi_cw(core, edges, views, n_rows, n_cols):
    """histogram_weighted_cov on C ABI views (sample views, a view, b view, weight view): (plan, W [R, B], means [2, R, B],
    moments [3, R, B])"""
    plan = cs._abi_plan(core, edges)
    sv, av, bv, wv = views
    W = torch.empty((n_rows, plan.n_bins), dtype=torch.float64, device="cuda")
    mean = torch.empty((2, n_rows, plan.n_bins), dtype=torch.float64, device="cuda")
    co = torch.empty((3, n_rows, plan.n_bins), dtype=torch.float64, device="cuda")
    plan.execute_cov_weighted(sv, av, bv, wv, n_rows, n_cols, W.data_ptr(), mean.data_ptr(), co.data_ptr(),
                              stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return plan, W, mean, co


def case(core, edges, xs, a, b, w, *, cmp=0, fine=True, arith=False, extra=None, ddof=0, dev=None, views=None, what=""):
    """xs, a, b, w: the logical host arrays [R, C] (a, b, w broadcastable to it); dev: the (samples, a, b, w) to hand to the
    public API (default: device copies of the host arrays); views: C ABI views (sample views, a, b, w views) to run instead;
    extra: ((dtype, column stride, pointer) of b, the same of w) as the launcher sees them (default: their dtypes, stride 1).
    Returns (the parsed describe(), W, exact)."""
    n_rows, n_cols = xs[0].shape
    sdt, vdt = xs[0].dtype, np.asarray(a).dtype
    extra = extra if extra is not None else ((np.asarray(b).dtype, 1, 0), (np.asarray(w).dtype, 1, 0))
    want = tgc.predict_cov(_cus(), edges, cmp, sdt, vdt, n_rows, n_cols, fine, arith, streams_fast(sdt, n_cols, *extra))
    xc, ec = cs._cmp(xs, edges)
    if views is not None:
        plan, W, mean, co = abi_cw(core, edges, views, n_rows, n_cols)
        W, mean, co = _np(W), _np(mean), _np(co)
        got = (W, mean[0], mean[1], mwo.var_of(W, co[0], ddof), mwo.var_of(W, co[2], ddof), mwo.var_of(W, co[1], ddof))
    else:
        xs_dev, a_dev, b_dev, w_dev = dev if dev is not None else ([_dev(x) for x in xs], _dev(a), _dev(b), _dev(w))
        got = run_cw(core, xs_dev, a_dev, b_dev, w_dev, edges, ddof=ddof)
        plan = _plan_for(core, xs_dev, edges)
    hit = tgc.assert_cov_variant(as_cov_line(plan.describe()), want)
    W, exact = check_exact(xc, ec, a, b, w, got, ddof=ddof, what=what)
    return hit, W, exact


# ---------------------------------------------------------------------------------------------------------------------
# every fast form: f32 / f64 x D 1 / 2 x SCAN 1 / 2 / arith
# ---------------------------------------------------------------------------------------------------------------------
FORMS = ("k1", "k2", "arith")
FORM_SHAPE = (3, 20_011)


def form_data(form, sdt, D):
    """(edges, samples, a, b, w, fine, arith) of one fast-form case; the bins are those of test_gpu_cov.test_fast_forms"""
    (kind, nb1, nb2), fine, arith = FORM_EDGES[form]
    if form == "arith":
        nb1, nb2 = tgc.ARITH_BINS
    st = _st(sdt)
    seed = 1_900 + 10 * FORMS.index(form) + 2 * D + (st == F32)
    edges = [edges_of(kind, nb, seed=seed + d) for d, nb in enumerate(nb1 if D == 1 else nb2)]
    rng = np.random.default_rng(seed)
    xs = float_samples(edges, *FORM_SHAPE, st, seed)
    a, b = tgc.nan_grid(rng, xs[0].shape, st), tgc.nan_grid(rng, xs[0].shape, st)
    return edges, xs, a, b, int_weights(rng, xs[0].shape, st), fine, arith


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("sdt", ["f64", "f32"])
@pytest.mark.parametrize("form", FORMS)
def test_fast_forms(xh, form, sdt, D):
    edges, xs, a, b, w, fine, arith = form_data(form, sdt, D)
    hit, _, _ = case(xh, edges, xs, a, b, w, fine=fine, arith=arith, ddof=D - 1, what="%s %s D=%d" % (form, sdt, D))
    assert hit["family"] == "fast" and (hit["scan"] == 5) == (form == "arith") and hit["D"] == D, hit


# ---------------------------------------------------------------------------------------------------------------------
# the generic family: CMP 0 / 1 / 3, slots in LDS or sums in global memory
# ---------------------------------------------------------------------------------------------------------------------
DOMS = ("f64", "i64", "mixed")
HOMES = ("lds", "global_tables_lds")
GENERIC_ROWS = 2
GENERIC_COLS = {"lds": 4_001, "global_tables_lds": 20_011}  # (200 bins in LDS: 20 samples a bin, so that W meets powers of two up to 2^8)


def generic_data(dom, home):
    """(edges, samples, a, b, w, cmp) of one generic case.  f64: float64 samples with values and weights of another dtype; i64:
    an integer a next to a float64 b and int32 weights; mixed: an int64 input next to a float64 one"""
    rng = np.random.default_rng(2_120 + 3 * DOMS.index(dom) + HOMES.index(home))
    nb = HOME_BINS[home] if dom != "mixed" else max(2, HOME_BINS[home] // 6)
    edges = _domain_edges(dom, nb, rng)
    shape = (GENERIC_ROWS, GENERIC_COLS[home])
    xs = []
    for d, e in enumerate(edges):
        if np.asarray(e).dtype.kind == "f":
            xs += float_samples([e], *shape, F64, 27 + d)
        else:
            xs += int_samples([e], *shape, None, 27 + d)
    vt = F32 if dom == "f64" else F64
    a, b = tgc.nan_grid(rng, shape, vt), tgc.nan_grid(rng, shape, vt)
    w = int_weights(rng, shape, vt)
    if dom == "i64":
        a = vx.grid(rng, shape, np.int32)
        w = w.astype(np.int32)
    return edges, xs, a, b, w, {"f64": 0, "i64": 1, "mixed": 3}[dom]


@pytest.mark.parametrize("home", HOMES)
@pytest.mark.parametrize("dom", DOMS)
def test_generic_domain_and_home(xh, dom, home):
    edges, xs, a, b, w, cmp = generic_data(dom, home)
    hit, _, _ = case(xh, edges, xs, a, b, w, cmp=cmp, fine=False, ddof=1, what="%s %s" % (dom, home))
    assert hit["family"] == "generic" and hit["slots"] == ("lds" if home == "lds" else "global") and hit["cmp"] == cmp, hit


# ---------------------------------------------------------------------------------------------------------------------
# ragged tiles: three of the four forms read their tile in two halves (values_fast_body's fast_halves) and have an internal
# split point; float32 pairs read theirs whole
# ---------------------------------------------------------------------------------------------------------------------
TILE_FORMS = {  # sample dtype, inputs, the tile T in elements (256 x VEC x UNROLL), the parts it is read in
    "f64_D1": (F64, 1, 2_048, 2), "f32_D1": (F32, 1, 4_096, 2), "f64_D2": (F64, 2, 2_048, 2), "f32_D2": (F32, 2, 2_048, 1),
}
TILE_BINS = {1: (400,), 2: (20, 20)}  # a few samples per bin, so that W stays small enough for powers of two up to 2^8


def tile_cols(form):
    """T - 1, T + 1, 2T - 1, and one element either side of each internal split point"""
    _, _, T, parts = TILE_FORMS[form]
    cols = [T - 1, T + 1, 2 * T - 1]
    for k in range(1, parts):
        cols += [k * T // parts - 1, k * T // parts + 1]
    return sorted(cols)


def tile_data(form, n_rows, n_cols):
    """(edges, samples, a, b, w) of one tile-edge case: every sample inside the bins and no NaN anywhere, so every element of
    a row counts"""
    st, D, _, _ = TILE_FORMS[form]
    seed = 2_800 + 7 * n_cols + n_rows
    edges = [edges_of("k2" if d == 0 else "k1", nb, seed=3 + d) for d, nb in enumerate(TILE_BINS[D])]
    rng = np.random.default_rng(seed)
    xs = [rng.uniform(e[0], e[-1], (n_rows, n_cols)).astype(st) for e in edges]
    for x, e in zip(xs, edges):  # (float32 rounding may leave the range: back onto the outer edges' float32 neighbours inside)
        lo = tvc.f32_neighbours(e[:1])[1][0] if st == F32 else e[0]
        hi = tvc.f32_neighbours(e[-1:])[0][0] if st == F32 else e[-1]
        np.clip(x, lo, hi, out=x)
        x[:, 0], x[:, -1] = lo, hi
    return edges, xs, vx.grid(rng, (n_rows, n_cols), st), vx.grid(rng, (n_rows, n_cols), st), int_weights(rng, (n_rows, n_cols), st)


@pytest.mark.parametrize("n_rows", [1, 3])
@pytest.mark.parametrize("form", list(TILE_FORMS))
def test_ragged_last_tile(xh, form, n_rows):
    st, D, T, parts = TILE_FORMS[form]
    vec = 16 // np.dtype(st).itemsize
    assert T == 256 * vec * (4 if D == 1 else 8 // vec)
    for n_cols in tile_cols(form):
        edges, xs, a, b, w = tile_data(form, n_rows, n_cols)
        what = "%s rows %d cols %d" % (form, n_rows, n_cols)
        hit, W, _ = case(xh, edges, xs, a, b, w, what=what)
        assert hit["family"] == "fast" and hit["D"] == D, hit
        np.testing.assert_array_equal(W.reshape(n_rows, -1).sum(axis=1), w.astype(F64).sum(axis=1), err_msg=what)


# ---------------------------------------------------------------------------------------------------------------------
# alignment, one stream at a time
# ---------------------------------------------------------------------------------------------------------------------
STREAMS = ("samples", "a", "b", "w")
ALIGN_SHAPES = ((3, 20_011), (65, 301))


def align_data(sdt, shape):
    st = _st(sdt)
    edges = [edges_of("k2", 900, seed=2)] if st == F32 else [edges_of("k2", 60, seed=2), edges_of("k1", 15, seed=3)]
    rng = np.random.default_rng(2_071 + shape[1])
    xs = float_samples(edges, shape[0], shape[1], st, shape[1])
    return edges, xs, tgc.nan_grid(rng, shape, st), tgc.nan_grid(rng, shape, st), int_weights(rng, shape, st)


@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_alignment_one_stream(xh, sdt, stream):
    """unit column stride; one of samples / a / b / w starts one element past a 16-byte boundary while the others are aligned:
    aligned to the element, not to the vector load.  Odd row lengths, so that every other row starts off 16 bytes in all four"""
    for shape in ALIGN_SHAPES:
        edges, xs, a, b, w = align_data(sdt, shape)
        dev = ([cs._offset(x, int(stream == "samples")) for x in xs], cs._offset(a, int(stream == "a")), cs._offset(b, int(stream == "b")),
               cs._offset(w, int(stream == "w")))
        off = [t.data_ptr() % 16 != 0 for t in dev[0]] + [t.data_ptr() % 16 != 0 for t in dev[1:]]
        assert off == [stream == "samples"] * len(xs) + [stream == s for s in STREAMS[1:]]
        hit, _, _ = case(xh, edges, xs, a, b, w, dev=dev, what="%s offset, %s" % (stream, shape))
        assert hit["family"] == "fast", hit


# ---------------------------------------------------------------------------------------------------------------------
# b and the weights, each alone: a column stride or another dtype gives up the fast family, a row stride of 0 does not
# ---------------------------------------------------------------------------------------------------------------------
LAYOUT_SHAPE = (6, 12_007)
LAYOUT_BINS = 700


def layout_data(sdt, which, how):
    """(edges, samples, a, b, w): the logical arrays of one layout case; `which` of b / w is laid out `how`: "stride2" (column
    stride 2), "dtype" (the other float type) or "row0" (one row for every row)"""
    st = _st(sdt)
    R, C = LAYOUT_SHAPE
    edges = [edges_of("k1", LAYOUT_BINS, seed=4)]
    rng = np.random.default_rng(2_083 + 5 * STREAMS.index(which) + ["stride2", "dtype", "row0"].index(how))
    xs = float_samples(edges, R, C, st, 83)
    a = tgc.nan_grid(rng, (R, C), st)
    other = F32 if st == F64 else F64
    shape = {"b": (R, C), "w": (R, C)}
    shape[which] = (1, C) if how == "row0" else (R, C)
    dt = {"b": st, "w": st}
    dt[which] = other if how == "dtype" else st
    b = tgc.nan_grid(rng, shape["b"], dt["b"]) if shape["b"][0] > 1 else vx.grid(rng, shape["b"], dt["b"])
    w = int_weights(rng, shape["w"], dt["w"])
    return edges, xs, a, b, w


@pytest.mark.parametrize("how", ["stride2", "dtype", "row0"])
@pytest.mark.parametrize("which", ["b", "w"])
@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_one_extra_stream_decides(xh, sdt, which, how):
    """dense samples and a through the C ABI; one of b / w at column stride 2 or of another dtype while the other qualifies: the
    line shows the generic family and the results stay exact.  At row stride 0 (weights over (lat, lon) broadcast over time,
    or such a b) the fast family stays"""
    st = _st(sdt)
    R, C = LAYOUT_SHAPE
    edges, xs, a, b, w = layout_data(sdt, which, how)
    keep, views, extra = [], {}, {}
    for name, t in (("b", b), ("w", w)):
        if name == which and how == "stride2":
            wide = np.full((R, 2 * C), np.nan if name == "b" else 5.0, t.dtype)  # (the elements between: NaN, or other weights)
            wide[:, ::2] = t
            d, kw, x_cs = _dev(wide), dict(row_stride=2 * C, col_stride=2), 2
        elif name == which and how == "row0":
            d, kw, x_cs = _dev(t), dict(row_stride=0, col_stride=1), 1
        else:
            d, kw, x_cs = _dev(t), dict(row_stride=C, col_stride=1), 1
        keep.append(d)
        views[name] = cs._view(d, t.dtype, **kw)
        extra[name] = (t.dtype, x_cs, d.data_ptr())
    xd, ad = _dev(xs[0]), _dev(a)
    dense = dict(row_stride=C, col_stride=1)
    hit, _, _ = case(xh, edges, xs, a, b, w, views=([cs._view(xd, st, **dense)], cs._view(ad, st, **dense), views["b"], views["w"]),
                     extra=(extra["b"], extra["w"]), what="%s %s %s" % (sdt, which, how))
    del keep
    assert hit["family"] == ("fast" if how == "row0" else "generic"), hit


# ---------------------------------------------------------------------------------------------------------------------
# copies of the slots
# ---------------------------------------------------------------------------------------------------------------------
COPIES = [((20,), 16), ((40,), 8), ((80,), 4), ((160,), 2), ((300,), 1)]


def copies_data(nbs, sdt):
    """two rows of 8 columns per bin: W around the powers of two 8, 16 and 32"""
    st = _st(sdt)
    seed = 3_000 + nbs[0] + (st == F32)
    edges = [edges_of("lin", nb, seed=seed + d) for d, nb in enumerate(nbs)]
    xs = float_samples(edges, 2, 8 * nbs[0] + 1, st, seed)
    rng = np.random.default_rng(seed)
    return edges, xs, tgc.nan_grid(rng, xs[0].shape, st), tgc.nan_grid(rng, xs[0].shape, st), int_weights(rng, xs[0].shape, st)


@pytest.mark.parametrize("sdt", ["f64", "f32"])
@pytest.mark.parametrize("nbs,copies", COPIES, ids=[str(n[0]) for n, _ in COPIES])
def test_copies(xh, nbs, copies, sdt):
    edges, xs, a, b, w = copies_data(nbs, sdt)
    hit, W, exact = case(xh, edges, xs, a, b, w, arith=True, what="copies %d" % copies)
    assert hit["family"] == "fast" and hit["copies"] == copies, hit
    assert split(W, exact)[1] >= 1


# ---------------------------------------------------------------------------------------------------------------------
# one LDS border, both sides: the last bin count whose 56-byte slots fit a workgroup's 160 KiB, and the next one
# ---------------------------------------------------------------------------------------------------------------------
BORDER = tvc.LDS_MAX // tgc.SLOT2  # 2925
BORDER_SHAPE = (1, 30_011)


def border_data(nb):
    edges = [edges_of("lin", nb, seed=3_700 + nb)]
    xs = float_samples(edges, *BORDER_SHAPE, F64, 3_700 + nb)
    rng = np.random.default_rng(3_700 + nb)
    return edges, xs, tgc.nan_grid(rng, BORDER_SHAPE, F64), tgc.nan_grid(rng, BORDER_SHAPE, F64), int_weights(rng, BORDER_SHAPE, F64)


@pytest.mark.parametrize("side", [0, 1])
def test_lds_border(xh, side):
    edges, xs, a, b, w = border_data(BORDER + side)
    hit, _, _ = case(xh, edges, xs, a, b, w, arith=True, what="border side %d" % side)
    assert (hit["family"], hit["slots"], hit["scan"]) == (("fast", "lds", 5) if side == 0 else ("generic", "global", 0)), hit


# ---------------------------------------------------------------------------------------------------------------------
# row chunks: more rows than one launch takes, through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
P_W = 1039  # the period of the weights: coprime to those of the samples, a and b


def _planes_expected(rows, xs_t, a_t, b_t, w_t):
    """W, mean_a, mean_b, M2_a, C_ab, M2_b of the given rows, [len(rows), 2] each: every row holds one triple or none"""
    bin_, counted, a, b = cs._rows_expected("cov", rows, xs_t, a_t, b_t)
    wt = w_t[rows % P_W].to(torch.float64)
    here = counted[:, None] & (bin_[:, None] == torch.arange(2, device=rows.device)[None, :])
    nan = torch.full(here.shape, float("nan"), dtype=torch.float64, device=rows.device)
    zero = torch.zeros_like(nan)
    W = torch.where(here, wt[:, None], zero)
    has = W > 0
    return [W, torch.where(has, a[:, None].expand_as(W), nan), torch.where(has, b[:, None].expand_as(W), nan)] + [torch.where(has, zero, nan)] * 3


@pytest.mark.parametrize("family", ["fast", "generic"])
def test_more_than_one_row_chunk(xh, family):
    """cs.N_ROWS rows of one column through grouped views of four periodic arrays, built as the cov case of
    test_gpu_values_census_streams.test_more_than_one_row_chunk: the planes are N_ROWS * 2 elements apart whatever the chunk,
    while the pointers advance by the chunk's rows.  Every row holds one triple or none, so every plane is known bit for bit
    (every bin with a positive weight is on the bit-for-bit path).  generic: the weights are float32"""
    from xhistogram_amd import _native

    N = cs.N_ROWS
    _need(N * 2 * 8 * 8)
    xs, a, b = cs._periodic("cov")
    wt = F64 if family == "fast" else F32
    w = int_weights(np.random.default_rng(93), P_W, wt)
    xs_t, a_t, b_t, w_t = _dev(xs), _dev(a), _dev(b), _dev(w)
    views = ([_native.make_view(xs_t.data_ptr(), _native.F64, 1, 1, inner_rows=cs.P_S, outer_stride=0)],
             _native.make_view(a_t.data_ptr(), _native.F64, 1, 1, inner_rows=cs.P_A, outer_stride=0),
             _native.make_view(b_t.data_ptr(), _native.F64, 1, 1, inner_rows=cs.P_B, outer_stride=0),
             _native.make_view(w_t.data_ptr(), _tag(wt), 1, 1, inner_rows=P_W, outer_stride=0))
    plan, W, mean, co = abi_cw(xh, [cs.CHUNK_EDGES], views, N, 1)
    planes = [W, mean[0], mean[1], co[0], co[1], co[2]]
    want = tgc.predict_cov(_cus(), [cs.CHUNK_EDGES], 0, F64, F64, N, 1, True, True, streams_fast(F64, 1, (F64, 1, 0), (wt, 1, 0)))
    got = tgc.assert_cov_variant(as_cov_line(plan.describe()), want)
    assert got["family"] == family and got["segs"] == 1, got
    chunk = cs.chunk_rows(got["block"], got["segs"])
    assert -(-N // chunk) == (3 if family == "fast" else 5), chunk
    dev = W.device
    bounds = [torch.arange(max(0, c - 32), min(N, c + 32)) for c in range(0, N + 1, chunk)]
    g = torch.Generator(device="cpu")
    g.manual_seed(5)
    row_sets = {"chunk boundaries and last rows": torch.cat(bounds + [torch.arange(N - 4096, N)]).to(dev),
                "random rows": torch.randint(0, N, (8192,), generator=g).to(dev)}
    for name, rows in row_sets.items():
        exp = _planes_expected(rows, xs_t, a_t, b_t, w_t)
        assert int((exp[0] > 1).sum()) > 0  # (rows on the bit-for-bit path among them)
        for k, (o, e) in enumerate(zip(planes, exp)):
            torch.testing.assert_close(o[rows], e, rtol=0, atol=0, equal_nan=True, msg=lambda m, k=k, name=name: "plane %d, %s: %s" % (k, name, m))
    # whole planes: per bin the exact sums of W and of the means (multiples of 2^-10 in any order), and where the moments are 0
    # and where NaN
    want_sum = [torch.zeros(2, dtype=torch.float64, device=dev) for _ in range(3)]
    want_has = torch.zeros(2, dtype=torch.int64, device=dev)
    got_nan = [torch.zeros(2, dtype=torch.int64, device=dev) for _ in planes]
    got_sum = [torch.zeros(2, dtype=torch.float64, device=dev) for _ in planes]
    for r0 in range(0, N, 1 << 23):
        rows = torch.arange(r0, min(N, r0 + (1 << 23)), device=dev)
        exp = _planes_expected(rows, xs_t, a_t, b_t, w_t)
        want_has += (exp[0] > 0).sum(0)
        for s, e in zip(want_sum, exp[:3]):
            s += torch.nan_to_num(e, nan=0.0).sum(0)
        for k, o in enumerate(planes):
            part = o[r0: r0 + (1 << 23)]
            got_nan[k] += torch.isnan(part).sum(0)
            got_sum[k] += torch.nan_to_num(part, nan=0.0).sum(0)
    assert int(want_has.min()) > N // 8  # (both bins take a good part of the rows)
    for k in range(3):
        assert torch.equal(got_sum[k], want_sum[k]), k
    assert torch.equal(got_nan[0], torch.zeros_like(got_nan[0]))
    for k in range(1, 6):
        assert torch.equal(got_nan[k], N - want_has), k
    for k in (3, 4, 5):
        assert torch.equal(got_sum[k], torch.zeros_like(got_sum[k])), k


# ---------------------------------------------------------------------------------------------------------------------
# the NaN and zero rules
# ---------------------------------------------------------------------------------------------------------------------
def special_data():
    nan, inf = np.nan, np.inf
    edges = [np.arange(8.0)]
    # bin 0: NaN in a only / in b only (dropped), W = 4 | bin 1: a NaN weight on a complete pair | bin 2: a NaN weight on an
    # incomplete pair (dropped) | bin 3: w = 0 next to an infinite value | bin 4: weights that sum to 0 | bin 5: W = 1 | bin 6: empty
    x = np.array([0.5, 0.5, 0.5, 0.5, 1.5, 1.5, 2.5, 2.5, 2.5, 3.5, 3.5, 4.5, 4.5, 5.5, 9.0])
    a = np.array([1.0, 3.0, nan, 5.0, 1.0, 2.0, 1.0, nan, 2.0, inf, 2.0, 1.0, 2.0, 3.0, 1.0])
    b = np.array([2.0, 6.0, 1.0, nan, 1.0, 2.0, 4.0, 1.0, 2.0, 1.0, 2.0, 5.0, 6.0, 7.0, 1.0])
    w = np.array([2.0, 2.0, 7.0, 7.0, nan, 1.0, 3.0, nan, 1.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0])
    return edges, x, a, b, w


def special_expected(ddof):
    nan = np.nan
    v = (lambda q, W: q / (W - ddof) if W > ddof else nan)
    W = [4.0, nan, 4.0, 1.0, 0.0, 1.0, 0.0]
    ma = [2.0, nan, 1.25, nan, nan, 3.0, nan]  # bin 3: 0 * inf is NaN, as in np.average
    mb = [4.0, nan, 3.5, 2.0, nan, 7.0, nan]
    va = [v(4.0, 4), nan, v(0.75, 4), nan, nan, v(0.0, 1), nan]
    vb = [v(16.0, 4), nan, v(3.0, 4), v(0.0, 1), nan, v(0.0, 1), nan]
    cab = [v(8.0, 4), nan, v(-1.5, 4), nan, nan, v(0.0, 1), nan]
    return W, ma, mb, va, vb, cab


@pytest.mark.parametrize("ddof", [0, 1])
def test_nan_and_zero_rules(xh, ddof):
    edges, x, a, b, w = special_data()
    xd = [_dev(x[None])]
    got = run_cw(xh, xd, _dev(a[None]), _dev(b[None]), _dev(w[None]), edges, ddof=ddof)
    want_line = tgc.predict_cov(_cus(), edges, 0, F64, F64, 1, x.size, True, True, True)
    hit = tgc.assert_cov_variant(as_cov_line(_plan_for(xh, xd, edges).describe()), want_line)
    assert hit["family"] == "fast"
    for g, e, name in zip(got, special_expected(ddof), ("W", "mean_a", "mean_b", "var_a", "var_b", "cov_ab")):
        np.testing.assert_array_equal(g[0], e, err_msg=name)  # (every sum of these small integers is exact: bit for bit)
    oracle = cwo.histogram_weighted_cov(x[None], values=(a[None], b[None]), weights=w[None], bins=edges, axis=1, ddof=ddof, exact=True)
    for g, o in zip(got, oracle):
        np.testing.assert_array_equal(g, o)
    assert got[0][0, 0] == 4.0 and got[0][0, 2] == 4.0  # bins on the bit-for-bit path: W = 2^2, their moments as computed by hand
    # the same through the generic family (float32 weights)
    got32 = run_cw(xh, xd, _dev(a[None]), _dev(b[None]), _dev(w[None].astype(F32)), edges, ddof=ddof)
    assert "pass1=covw_sum_generic " in _plan_for(xh, xd, edges).describe()
    for g, g32 in zip(got, got32):
        np.testing.assert_array_equal(g32, g)
    # empty inputs, and inputs with no counted sample
    for xe in (np.zeros(0), np.full(5, 9.0)):
        out = xh.histogram_weighted_cov(xe, values=(np.ones(xe.shape), np.ones(xe.shape)), weights=np.ones(xe.shape), bins=edges)
        np.testing.assert_array_equal(out[0], np.zeros(7))
        assert out[0].dtype == F64 and all(np.isnan(o).all() for o in out[1:6])


# ---------------------------------------------------------------------------------------------------------------------
# identities: w == 1, repeated samples, b = a
# ---------------------------------------------------------------------------------------------------------------------
IDENT_SHAPE = (3, 20_011)


def ident_data():
    edges = [edges_of("k1", 900, seed=11)]
    rng = np.random.default_rng(2_011)
    xs = float_samples(edges, *IDENT_SHAPE, F64, 11)
    return edges, xs, tgc.nan_grid(rng, IDENT_SHAPE, F64), tgc.nan_grid(rng, IDENT_SHAPE, F64), int_weights(rng, IDENT_SHAPE, F64)


def _same_moments(got, ref, pow2, what):
    """three moments of two calls: bit for bit where both are exact, to the rtol of test_gpu_cov's identities elsewhere"""
    assert pow2.any(), what
    for g, r in zip(got, ref):
        np.testing.assert_array_equal(g[pow2], r[pow2], err_msg=what)
        np.testing.assert_allclose(g, r, rtol=1e-12, atol=0, err_msg=what)


def test_unit_weights_are_histogram_cov(xh):
    edges, xs, a, b, _ = ident_data()
    xd, ad, bd = [_dev(x) for x in xs], _dev(a), _dev(b)
    hit, W, exact = case(xh, edges, xs, a, b, np.ones(IDENT_SHAPE), dev=(xd, ad, bd, _dev(np.ones(IDENT_SHAPE))), ddof=1, what="w == 1")
    got = run_cw(xh, xd, ad, bd, _dev(np.ones(IDENT_SHAPE)), edges, ddof=1)
    ref = tgc.run_cov(xh, xd, ad, bd, edges, ddof=1)
    np.testing.assert_array_equal(got[0], ref[0].astype(F64))
    tvc._bits(got[1], ref[1], "mean_a against histogram_cov")
    tvc._bits(got[2], ref[2], "mean_b against histogram_cov")
    cnt = ref[0]
    _same_moments(got[3:], ref[3:], vx.is_pow2(cnt) & (cnt > 1) & (cnt <= mwo.POW2_EXACT), "w == 1")


def test_integer_weights_are_repeated_samples(xh):
    """one row: integer weights m in 0..7 == histogram_cov on np.repeat'ed samples and values"""
    edges, xs, a, b, w = ident_data()
    x, a, b, m = xs[0][0], a[0], b[0], w[0].astype(np.int64)
    hit, W, exact = case(xh, edges, [x[None]], a[None], b[None], w[:1], what="integer weights")
    got = xh.histogram_weighted_cov(x, values=(a, b), weights=m, bins=edges)[:6]
    ref = xh.histogram_cov(np.repeat(x, m), values=(np.repeat(a, m), np.repeat(b, m)), bins=edges)[:6]
    np.testing.assert_array_equal(got[0], ref[0].astype(F64))
    tvc._bits(got[1], ref[1], "mean_a against repeated samples")
    tvc._bits(got[2], ref[2], "mean_b against repeated samples")
    cnt = ref[0]
    _same_moments(got[3:], ref[3:], vx.is_pow2(cnt) & (cnt > 1) & (cnt <= mwo.POW2_EXACT), "repeated samples")


def test_b_equal_a_is_weighted_mean_var(xh):
    edges, xs, a, _, w = ident_data()
    xd, ad, wd = [_dev(x) for x in xs], _dev(a), _dev(w)
    hit, W, exact = case(xh, edges, xs, a, a, w, dev=(xd, ad, ad, wd), what="b = a")
    got = run_cw(xh, xd, ad, ad, wd, edges)
    Wm, mean, var, _ = xh.histogram_mean_var(*xd, values=ad, weights=wd, bins=edges, axis=1)
    Wm, mean, var = _np(Wm), _np(mean), _np(var)
    np.testing.assert_array_equal(got[0], Wm)
    tvc._bits(got[1], mean, "mean_a against the weighted mean_var")
    tvc._bits(got[2], mean, "mean_b against the weighted mean_var")
    pow2 = cwx.w_exact(Wm) & (Wm > 1)
    _same_moments(got[3:], (var, var, var), pow2, "b = a")


# ---------------------------------------------------------------------------------------------------------------------
# backends
# ---------------------------------------------------------------------------------------------------------------------
def backend_data():
    rng = np.random.default_rng(2_071)
    edges = [np.linspace(-3, 3, 201)]  # (15 samples a bin: W stays around the powers of two 32 and 64)
    x = rng.standard_normal((5, 3000))
    return edges, x, tgc.nan_grid(rng, x.shape, F64), vx.grid(rng, (1, 3000)), int_weights(rng, (1, 3000), F64)


def test_backends(xh):
    from xhistogram_amd.devicearray import DeviceArray

    edges, x, a, b, w = backend_data()
    got_np = xh.histogram_weighted_cov(x, values=(a, b), weights=w, bins=edges, axis=1)
    assert all(isinstance(g, np.ndarray) and g.dtype == F64 for g in got_np[:6])
    check_exact([x], edges, a, b, w, got_np[:6], what="numpy in")
    xd, ad, bd, wd = _dev(x), _dev(a), _dev(np.broadcast_to(b, x.shape)), _dev(w).expand(*x.shape)
    got_t = xh.histogram_weighted_cov(xd, values=(ad, bd), weights=wd, bins=edges, axis=1)
    assert all(t.device.type == "cuda" and t.dtype == torch.float64 for t in got_t[:6])
    torch.cuda.synchronize()
    want_line = tgc.predict_cov(_cus(), edges, 0, F64, F64, *x.shape, True, True, True)
    assert tgc.assert_cov_variant(as_cov_line(_plan_for(xh, [xd], edges).describe()), want_line)["family"] == "fast"
    check_exact([x], edges, a, b, w, [_np(t) for t in got_t[:6]], what="torch in")
    got_d = xh.histogram_weighted_cov(DeviceArray.from_numpy(x, 0), values=(DeviceArray.from_numpy(a, 0), DeviceArray.from_numpy(b, 0)),
                                      weights=DeviceArray.from_numpy(w, 0), bins=edges, axis=1)
    assert all(isinstance(g, np.ndarray) for g in got_d[:6])
    check_exact([x], edges, a, b, w, got_d[:6], what="DeviceArray in")


def xarray_data():
    """(edges, T, o2, temp over (time, lat, lon), area over (lat, lon))"""
    rng = np.random.default_rng(2_081)
    return (np.linspace(0, 10, 13), rng.uniform(0, 10, (4, 6, 8)), tgc.nan_grid(rng, (4, 6, 8), F64), vx.grid(rng, (4, 6, 8)),
            int_weights(rng, (6, 8), F64))


def test_xarray(xh):
    try:
        import xarray as xr
    except ImportError:  # the small double of tests/doubles, as tests/test_xarray_wrapper.py uses it
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "doubles"))
        import xarray as xr
    from xhistogram_amd import xarray as xhx

    edges, Tv, o2v, tempv, areav = xarray_data()
    coords = {"time": np.arange(4), "lat": np.arange(6) * 1.5, "lon": np.arange(8) * 2.0}
    T = xr.DataArray(Tv, dims=("time", "lat", "lon"), name="T", coords=coords)
    o2 = xr.DataArray(o2v, dims=("time", "lat", "lon"), name="o2", coords=coords)
    temp = xr.DataArray(tempv, dims=("time", "lat", "lon"), name="temp", coords=coords)
    area = xr.DataArray(areav, dims=("lat", "lon"), name="area", coords={"lat": coords["lat"], "lon": coords["lon"]})
    out = xhx.histogram_weighted_cov(T, values=(o2, temp), weights=area, bins=[edges], dim=["lat", "lon"], keep_coords=True)
    assert list(out) == ["o2_temp_sum_of_weights", "o2_mean", "temp_mean", "o2_var", "temp_var", "o2_temp_cov"]
    assert all(tuple(v.dims) == ("time", "T_bin") for v in out.values())
    np.testing.assert_array_equal(np.asarray(out["o2_temp_cov"].coords["time"].values), coords["time"])
    np.testing.assert_array_equal(np.asarray(out["o2_temp_cov"].coords["T_bin"].values), 0.5 * (edges[:-1] + edges[1:]))
    rows = [T.values.reshape(4, 48)]
    check_exact(rows, [edges], o2.values.reshape(4, 48), temp.values.reshape(4, 48), np.broadcast_to(area.values, (4, 6, 8)).reshape(4, 48),
                [np.asarray(v.values) for v in out.values()], what="xarray")


def test_dask_chunked_equals_unchunked():
    env = dict(os.environ)
    sys_cxx = "/usr/lib/x86_64-linux-gnu/libstdc++.so.6"  # (as tests/test_dask_branch.py: conda's libstdc++ is older)
    if os.path.exists(sys_cxx):
        env["LD_PRELOAD"] = (sys_cxx + ":" + env["LD_PRELOAD"]) if env.get("LD_PRELOAD") else sys_cxx
    r = subprocess.run([PY39, "-W", "ignore", SCRIPT], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "COV-WEIGHTED-DASK-OK" in r.stdout
