"""histogram_sum on the GPU: every result bit for bit against tests/sum_oracle.py (zeros compared by value), every case
asserting from the plan's describe() that it ran the family, home, digitize form and number of copies it is named for.

The shapes are those of tests/test_gpu_values_census.py's cover, so that all 18 binning instantiations of pass 2 (sum_fast<ST, D,
SCAN>, sum_generic<CMP, LDS>) and sum_finalize are selected: the closing census (tests/test_zz_gpu_census_total.py) fails
otherwise."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import exact_weights as xw
import sum_cases as sc
import sum_oracle as so
from test_gpu_census import edges_of
from test_gpu_parity import _plan_for, xh  # noqa: F401  (xh: the module fixture)
from test_gpu_values_census import _domain_edges, float_samples, int_samples, table_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F64, F32 = np.float64, np.float32


# ---------------------------------------------------------------------------------------------------------------------
# the check
# ---------------------------------------------------------------------------------------------------------------------
def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def parse(desc):
    assert desc.startswith("sum pass1=extrema_"), desc
    kv = dict(re.findall(r"(\w+)=(\S+)", desc))
    fam = kv["pass2"].replace("sum_", "")
    assert kv["pass1"] == "extrema_" + fam, desc
    assert len(set(re.findall(r"slots=(\S+)", desc))) == 1, desc  # (both passes in the same home)
    return dict(family=fam, home=kv["slots"], scan=int(kv["scan"]), copies=int(kv["copies"]), D=int(kv["D"]), cmp=int(kv["cmp"]),
                block=int(kv["block"]), segs=[int(s) for s in kv["segs"].split("/")], lds=[int(s) for s in kv["lds_bytes"].split("/")])


def _cmp_domain(samples, edges):
    """per input what the library compares: float64 if either side is a float, else the integers (datetime64 as int64)"""
    out_s, out_e = [], []
    for s, e in zip(samples, edges):
        s, e = np.asarray(s), np.asarray(e)
        if s.dtype.kind == "M":
            s, e = s.view(np.int64), e.astype(s.dtype).view(np.int64)
        elif s.dtype.kind == "f" or e.dtype.kind == "f":
            s, e = s.astype(F64), e.astype(F64)
        out_s.append(s)
        out_e.append(e)
    return out_s, out_e


def check(core, xs_dev, v_dev, edges, host_xs, host_v, want=None, what=""):
    """histogram_sum over axis 1 of [R, C] inputs against the oracle; `want`: the describe() fields this case is named for"""
    cnt, tot, _ = core.histogram_sum(*xs_dev, values=v_dev, bins=edges, axis=1)
    if hasattr(cnt, "detach"):
        torch.cuda.synchronize()
    cnt, tot = _np(cnt), _np(tot)
    assert cnt.dtype == np.int64 and tot.dtype == np.float64
    s, e = _cmp_domain(host_xs, edges)
    want_cnt, want_tot = so.sum_rows(s, e, np.broadcast_to(np.asarray(host_v), host_xs[0].shape))
    np.testing.assert_array_equal(cnt, want_cnt, err_msg="count " + what)
    sc.same_bits(tot, want_tot, what)
    got = None
    if want is not None:
        got = parse(_plan_for(core, xs_dev, edges).describe())
        for key, val in want.items():
            assert got[key] == val, "%s: landed elsewhere, %s = %r, wanted %r (%s)" % (what, key, got[key], val, got)
    return cnt, tot, got


def mixed_values(rng, shape, dt=F64, specials=True):
    """values over 2^40 in magnitude and both signs, with NaN, a few infinities and zeros of both signs"""
    v = rng.standard_normal(shape) * np.exp2(rng.integers(-20, 21, shape))
    if specials:
        flat = v.reshape(-1)
        idx = rng.permutation(flat.size)
        flat[idx[: max(1, flat.size // 100)]] = np.nan
        flat[idx[-6:]] = [np.inf, -np.inf, np.inf, 0.0, -0.0, 5e-324][: min(6, flat.size)]
    return v.astype(dt)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the fast family: tile borders
# ---------------------------------------------------------------------------------------------------------------------
TILES = {  # form -> (sample type, D, the tile in samples, columns)
    "f64_D1": (F64, 1, 2048, (1, 2047, 2048, 2049, 4097)),
    "f32_D1": (F32, 1, 4096, (4095, 4096, 4097)),
    "f64_D2": (F64, 2, 2048, (2047, 2048, 2049)),
    "f32_D2": (F32, 2, 2048, (2047, 2048, 2049)),
}


@pytest.mark.parametrize("n_rows", [1, 3])
@pytest.mark.parametrize("form", list(TILES))
def test_fast_tile_borders(xh, form, n_rows):
    st, D, tile, cols = TILES[form]
    assert tile == 256 * (16 // np.dtype(st).itemsize) * (4 if D == 1 else 8 // (16 // np.dtype(st).itemsize))
    edges = [np.linspace(-4, 4, 6)] + ([np.array([-4.0, 0.5, 4.0])] if D == 2 else [])
    rng = np.random.default_rng(n_rows + 10 * list(TILES).index(form))
    for n_cols in cols:
        xs = [rng.uniform(-4, 4, (n_rows, n_cols)).astype(st) for _ in range(D)]  # (every element counts)
        v = mixed_values(rng, (n_rows, n_cols), st, specials=n_cols > 100)
        cnt, _, got = check(xh, [dev(x) for x in xs], dev(v), edges, xs, v, dict(family="fast", home="lds", D=D, cmp=0),
                            what="%s rows %d cols %d" % (form, n_rows, n_cols))
        assert cnt.sum() == n_rows * n_cols - np.isnan(v).sum()
        assert got["copies"] == 16  # 5 and 10 bins of 30 bytes: 16 copies stay within 24 KiB


# ---------------------------------------------------------------------------------------------------------------------
# 2. the fast family: digitize forms, for each (ST, D)
# ---------------------------------------------------------------------------------------------------------------------
FORMS = {  # form -> (edge kind, bins for D = 1, bins for D = 2, scan)
    "scan1": ("k1", (300,), (24, 30), 1),
    "scan2": ("k2", (300,), (24, 30), 2),
    "arith": ("lin", (5_400,), (2, 2_700), 5),  # 30-byte slots with no room for a fine table: arithmetic edges, table-free
}


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("sdt", ["f64", "f32"])
@pytest.mark.parametrize("form", list(FORMS))
def test_fast_digitize_forms(xh, form, sdt, D):
    kind, nb1, nb2, scan = FORMS[form]
    st = F64 if sdt == "f64" else F32
    seed = 100 + 10 * list(FORMS).index(form) + 2 * D + (st == F32)
    edges = [edges_of(kind, nb, seed=seed + d) for d, nb in enumerate(nb1 if D == 1 else nb2)]
    xs = float_samples(edges, 3, 20_011, st, seed)
    v = mixed_values(np.random.default_rng(seed), xs[0].shape, st)
    check(xh, [dev(x) for x in xs], dev(v), edges, xs, v, dict(family="fast", home="lds", scan=scan, D=D, cmp=0, block=256),
          what="%s %s D=%d" % (form, sdt, D))


def predict_copies(edges, st):
    """the copies of the fast family's 30-byte slots: the most (up to 16) within 24 KiB, as for every statistic, then as many as
    leave eight workgroups on a CU (tables and whole groups of four slots within 20 KiB)"""
    nb = int(np.prod([len(e) - 1 for e in edges]))
    tb = table_bytes(edges, "fine32" if st == F32 else "fine64")
    cl = 0
    while cl < 4 and (nb * 30 << (cl + 1)) <= 24 * 1024 and tb + (nb * 30 << (cl + 1)) <= 160 * 1024:
        cl += 1
    while cl > 0 and tb + -(-(nb << cl) // 4) * 120 > 160 * 1024 // 8:
        cl -= 1
    return 1 << cl


@pytest.mark.parametrize("nb,copies", [(5, 16), (30, 16), (50, 8), (100, 4), (200, 2), (409, 1), (600, 1)])
@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_fast_copies(xh, nb, copies, sdt):
    """copies_log2 > 0 with few bins (C4's 50 and C2's 100 among them), one copy above 384 bins"""
    st = F64 if sdt == "f64" else F32
    edges = [edges_of("lin", nb, seed=nb)]
    assert predict_copies(edges, st) == copies
    xs = float_samples(edges, 2, 30_011, st, nb)
    v = mixed_values(np.random.default_rng(nb), xs[0].shape, st)
    _, _, got = check(xh, [dev(x) for x in xs], dev(v), edges, xs, v, dict(family="fast", home="lds", copies=copies), what="copies %d" % copies)
    # pass 2: groups of four 30-byte slots; pass 1 keeps one copy of its own slots
    assert got["lds"][1] - got["lds"][0] == -(-nb * copies // 4) * 120 - nb * (16 if st == F64 else 8)
    assert copies == 1 or got["lds"][1] <= 160 * 1024 // 8


# ---------------------------------------------------------------------------------------------------------------------
# 3. the generic family: domains, value layouts, homes
# ---------------------------------------------------------------------------------------------------------------------
HOME_BINS = {"lds": 200, "global": 5_200}  # (30-byte slots behind the tables: these bins leave the 160 KiB)
GENERIC = ("int32_samples", "strided_values", "f32_samples_f64_values", "datetime", "datetime_float")


@pytest.mark.parametrize("home", list(HOME_BINS))
@pytest.mark.parametrize("case", GENERIC)
def test_generic(xh, case, home):
    rng = np.random.default_rng(50 + 3 * GENERIC.index(case) + list(HOME_BINS).index(home))
    nb = HOME_BINS[home]
    n_rows, n_cols = 2, 20_011
    xs_dev = v_dev = None
    if case == "int32_samples":
        edges = [np.linspace(-1000.5, 1000.5, nb + 1)]
        xs = [rng.integers(-1100, 1101, (n_rows, n_cols)).astype(np.int32)]
        v = rng.integers(-(1 << 30), 1 << 30, (n_rows, n_cols)).astype(np.int32)  # integer values, taken as float64
        cmp = 0
    elif case == "strided_values":
        edges = [edges_of("k1", nb, seed=7)]
        xs = float_samples(edges, n_rows, n_cols, F64, 7)
        wide = mixed_values(rng, (n_rows, 2 * n_cols))
        v, v_dev, cmp = wide[:, ::2], dev(wide)[:, ::2], 0
        assert v_dev.stride() == (2 * n_cols, 2)
    elif case == "f32_samples_f64_values":
        edges = [edges_of("k1", nb, seed=8)]
        xs = float_samples(edges, n_rows, n_cols, F32, 8)
        v, cmp = mixed_values(rng, (n_rows, n_cols)), 0
    elif case == "datetime":
        edges = _domain_edges("dt", nb, rng)
        xs = int_samples(edges, n_rows, n_cols, None, 9)
        v, cmp = mixed_values(rng, (n_rows, n_cols)), 1
        xs_dev, v_dev = xs, v  # (torch holds no datetime64: numpy inputs, uploaded by the call)
    else:
        edges = [_domain_edges("dt", max(2, nb // 6), rng)[0], edges_of("k2", 6, seed=3)]
        xs = int_samples(edges[:1], n_rows, n_cols, None, 10) + float_samples(edges[1:], n_rows, n_cols, F64, 11)
        v, cmp = mixed_values(rng, (n_rows, n_cols)), 3
        xs_dev, v_dev = xs, v
    xs_dev = xs_dev if xs_dev is not None else [dev(x) for x in xs]
    v_dev = v_dev if v_dev is not None else dev(v)
    check(xh, xs_dev, v_dev, edges, xs, v, dict(family="generic", home=home, cmp=cmp, copies=1, block=512, D=len(edges)),
          what="%s %s" % (case, home))


# ---------------------------------------------------------------------------------------------------------------------
# 4. directed data
# ---------------------------------------------------------------------------------------------------------------------
_DIRECTED = {}


def directed():
    """the layout of every case of sum_cases and the oracle's per-case (count, total), computed once"""
    if not _DIRECTED:
        x, v, edges, names = sc.layout(seed=1)
        want = [so.bin_sum(sc.CASES[n]) for n in names]
        _DIRECTED.update(x=x, v=v, edges=edges, names=names, cnt=np.array([w[0] for w in want]), tot=np.array([w[1] for w in want]))
    return _DIRECTED


def _far_edges(edges, n_more):
    """the same bins, then n_more bins beyond every sample: the first bins keep their samples, the slots leave LDS"""
    return np.r_[edges, edges[-1] + 1.0 + np.arange(n_more)]


@pytest.mark.parametrize("variant", ["fast", "generic_lds", "generic_global"])
def test_directed_cases(xh, variant):
    d = directed()
    x, v, names = d["x"], d["v"], d["names"]
    edges = d["edges"] if variant != "generic_global" else _far_edges(d["edges"], 5_300)
    xd = dev(x)[None, :]
    if variant == "fast":
        vd = dev(v)[None, :]
    else:  # the same values at a column stride of 2: the generic family
        vd = dev(np.repeat(v, 2))[None, ::2]
    cnt, tot, _ = xh.histogram_sum(xd, values=vd, bins=[edges], axis=1)
    torch.cuda.synchronize()
    got = parse(_plan_for(xh, [xd], [edges]).describe())
    fam, home = {"fast": ("fast", "lds"), "generic_lds": ("generic", "lds"), "generic_global": ("generic", "global")}[variant]
    assert (got["family"], got["home"]) == (fam, home), got
    cnt, tot = _np(cnt)[0], _np(tot)[0]
    np.testing.assert_array_equal(cnt[: len(names)], d["cnt"])
    assert not cnt[len(names):].any() and not tot[len(names):].any()
    for j, n in enumerate(names):
        sc.same_bits(tot[j], d["tot"][j], n)
        if n in sc.EXPECT:
            assert cnt[j] == sc.EXPECT[n][0]
            sc.same_bits(tot[j], sc.EXPECT[n][1], n + " (stated)")
        if sc.EXPECT.get(n, (0, 1.0))[1] == 0:
            assert not np.signbit(tot[j]), n
    # the wide-span bin equals the oracle (above) and is, separately, within the bound of the exactly rounded sum
    w = sc.CASES["wide"]
    j = names.index("wide")
    assert abs(tot[j] - math.fsum(w)) <= math.ulp(tot[j]) / 2 + so.bound(w) and so.bound(w) > 0


# ---------------------------------------------------------------------------------------------------------------------
# 5. order independence
# ---------------------------------------------------------------------------------------------------------------------
def test_order_and_geometry_independence(xh):
    """1e8 + 1e3 N(0, 1): five permutations, the fast and the generic family, LDS and global memory, one row alone and among
    three — the same bits per bin, math.fsum's"""
    rng = np.random.default_rng(21)
    n = 3 * 2048 + 5
    coarse = np.linspace(-4, 4, 6)
    x = rng.uniform(-4, 4, (3, n))
    v = 1e8 + 1e3 * rng.standard_normal((3, n))
    code = np.clip(np.searchsorted(coarse, x, side="right") - 1, 0, 4)
    want = np.array([[math.fsum(v[r][code[r] == b]) for b in range(5)] for r in range(3)])
    assert not np.array_equal(want, np.array([[np.sum(v[r][code[r] == b]) for b in range(5)] for r in range(3)]))  # (np.sum differs)

    def run(xa, va, edges, fam, home):
        cnt, tot, _ = xh.histogram_sum(xa, values=va, bins=[edges], axis=1)
        torch.cuda.synchronize()
        got = parse(_plan_for(xh, [xa], [edges]).describe())
        assert (got["family"], got["home"]) == (fam, home), got
        return _np(tot)[:, :5]

    for k in range(5):
        p = rng.permutation(n) if k else np.arange(n)
        sc.same_bits(run(dev(x[:, p]), dev(v[:, p]), coarse, "fast", "lds"), want, "permutation %d" % k)
    v2 = dev(np.repeat(v, 2, axis=1))[:, ::2]
    sc.same_bits(run(dev(x), v2, coarse, "generic", "lds"), want, "generic lds")
    sc.same_bits(run(dev(x), v2, _far_edges(coarse, 5_300), "generic", "global"), want, "generic global")
    for r in range(3):
        sc.same_bits(run(dev(x[r:r + 1]), dev(v[r:r + 1]), coarse, "fast", "lds"), want[r:r + 1], "row %d alone" % r)
        sc.same_bits(run(dev(x[r:r + 1]), v2[r:r + 1], _far_edges(coarse, 5_300), "generic", "global"), want[r:r + 1], "row %d alone, global" % r)


# ---------------------------------------------------------------------------------------------------------------------
# 6. identities
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_identities(xh, sdt):
    st = F64 if sdt == "f64" else F32
    rng = np.random.default_rng(31)
    edges = [edges_of("k1", 40, seed=1)]
    xs = float_samples(edges, 3, 20_011, st, 31)
    xd = [dev(x) for x in xs]
    # the count is histogram_mean_var's
    v = mixed_values(rng, xs[0].shape, st)
    cnt, _, _ = xh.histogram_sum(*xd, values=dev(v), bins=edges, axis=1)
    cnt_mv, _, _, _ = xh.histogram_mean_var(*xd, values=dev(v), bins=edges, axis=1)
    assert torch.equal(cnt, cnt_mv)
    # exactly summable weights: the weighted histogram's bits
    w = xw.make(st, signs="both")(rng, xs[0].shape)
    xw.assert_summable(xs[0].shape[1], st)
    _, tot, _ = xh.histogram_sum(*xd, values=dev(w), bins=edges, axis=1)
    h, _ = xh.histogram(*xd, bins=edges, weights=dev(w), axis=1)
    sc.same_bits(_np(tot), _np(h), "exact weights")
    # full mantissas: within the any-order bound of the float64 atomics' result
    w = rng.standard_normal(xs[0].shape).astype(st)
    n_b, tot, _ = xh.histogram_sum(*xd, values=dev(w), bins=edges, axis=1)
    h, _ = xh.histogram(*xd, bins=edges, weights=dev(w), axis=1)
    s, e = _cmp_domain(xs, edges)
    a = so.sum_rows(s, e, np.abs(w.astype(F64)))[1]  # (the sum of |w| itself, correctly rounded)
    xw.assert_within_f64_bound(_np(h), _np(tot), a, _np(n_b), what="full mantissas")


# ---------------------------------------------------------------------------------------------------------------------
# 7. the public API and the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_backends_and_axes(xh):
    from xhistogram_amd.devicearray import DeviceArray

    rng = np.random.default_rng(41)
    x = rng.uniform(-4.2, 4.2, (6, 50, 40))
    v = mixed_values(rng, x.shape)
    edges = [np.linspace(-4, 4, 8)]
    for axis in ((2,), (1,), (0,), (0, 2), (2, 0), None, (1, 2), (0, 1, 2)):  # trailing, middle, leading, split, all
        want = so.histogram_sum(x, values=v, bins=edges, axis=axis)
        outs = [xh.histogram_sum(x, values=v, bins=edges, axis=axis),
                xh.histogram_sum(dev(x), values=dev(v), bins=edges, axis=axis),
                xh.histogram_sum(DeviceArray.from_numpy(x), values=DeviceArray.from_numpy(v), bins=edges, axis=axis)]
        assert isinstance(outs[0][0], np.ndarray) and hasattr(outs[1][0], "detach") and isinstance(outs[2][1], np.ndarray)
        for cnt, tot, _ in outs:
            cnt, tot = _np(cnt), _np(tot)
            assert cnt.dtype == np.int64 and cnt.shape == want[0].shape
            np.testing.assert_array_equal(cnt, want[0], err_msg="axis %s" % (axis,))
            sc.same_bits(tot, want[1], "axis %s" % (axis,))
    # values broadcast from a smaller array, int bins: the edges of the unweighted histogram
    cnt, tot, e = xh.histogram_sum(x, values=v[:1], bins=20, axis=(1, 2))
    np.testing.assert_array_equal(e[0], xh.histogram(x, bins=20)[1][0])
    want = so.histogram_sum(x, values=np.broadcast_to(v[:1], x.shape), bins=[e[0]], axis=(1, 2))
    np.testing.assert_array_equal(cnt, want[0])
    sc.same_bits(tot, want[1], "broadcast values")


def test_empty_inputs(xh):
    e = [np.linspace(0, 1, 4)]
    for args, val in (([np.zeros(0)], np.zeros(0)), ([torch.zeros(0, dtype=torch.float64, device="cuda")], torch.zeros(0, dtype=torch.float64, device="cuda"))):
        cnt, tot, _ = xh.histogram_sum(*args, values=val, bins=e)
        cnt, tot = _np(cnt), _np(tot)
        assert cnt.shape == (3,) and cnt.dtype == np.int64 and not cnt.any() and not tot.any() and not np.signbit(tot).any()
    cnt, tot, _ = xh.histogram_sum(np.zeros((4, 0)), values=np.zeros((4, 0)), bins=e, axis=1)  # n_cols == 0
    assert cnt.shape == tot.shape == (4, 3) and not cnt.any() and not tot.any()
    cnt, tot, _ = xh.histogram_sum(np.zeros((0, 5)), values=np.zeros((0, 5)), bins=e, axis=1)
    assert cnt.shape == tot.shape == (0, 3)


SENTINEL = -0x0123456789ABCDEF


def _guarded(native, n):
    lead, tail = 65, 64
    host = np.full(lead + n + tail, SENTINEL, np.int64)
    buf = native.DeviceBuffer(0, host.nbytes)
    buf.upload(host)
    return buf, host, lead


def test_plan_execute_sum_writes_its_outputs_and_nothing_else(xh):
    from xhistogram_amd import _native as native

    rng = np.random.default_rng(51)
    n_rows, n_cols = 3, 9_001
    edges = [np.linspace(-4, 4, 12)]
    x = rng.uniform(-4.4, 4.4, (n_rows, n_cols))
    v = mixed_values(rng, x.shape)
    v[:, :40][x[:, :40] > 3.0] = np.nan
    xt, vt = dev(x), dev(v)
    plan = xh._get_plan(edges, native.CMP_F64, 0)
    n = n_rows * plan.n_bins
    (bc, hc, lead), (bt, ht, _) = _guarded(native, n), _guarded(native, n)
    torch.cuda.synchronize()
    plan.execute_sum([native.make_view(xt.data_ptr(), native.F64, n_cols, 1)], native.make_view(vt.data_ptr(), native.F64, n_cols, 1),
                     n_rows, n_cols, bc.ptr + 8 * lead, bt.ptr + 8 * lead)
    torch.cuda.synchronize()
    assert parse(plan.describe())["family"] == "fast"
    want_cnt, want_tot = so.sum_rows([x], edges, v)
    for buf, host, want in ((bc, hc, want_cnt), (bt, ht, want_tot)):
        buf.download(host)
        buf.close()
        assert (host[:lead] == SENTINEL).all() and (host[lead + n:] == SENTINEL).all(), "the guard bands were written"
        assert not (host[lead:lead + n] == SENTINEL).any(), "elements were never written"
        if want.dtype == np.int64:
            np.testing.assert_array_equal(host[lead:lead + n].reshape(want.shape), want)
        else:
            sc.same_bits(host[lead:lead + n].view(F64).reshape(want.shape), want, "execute_sum")


def test_rows_of_2_31_columns_are_refused_before_any_launch(xh):
    from xhistogram_amd import _native as native

    n = 1 << 31
    x = torch.full((1,), 0.5, dtype=torch.float64, device="cuda").expand(n)
    assert x.stride() == (0,)
    edges = [np.array([0.0, 1.0])]
    plan = xh._get_plan(edges, native.CMP_F64, 0)
    xh.histogram_sum(x[:10], values=x[:10], bins=edges)
    before = plan.describe()
    with pytest.raises(NotImplementedError, match=r"fewer than 2\^31"):
        xh.histogram_sum(x, values=x, bins=edges)
    # ... and by the library itself: the outputs keep their sentinels, so not even the zeroing ran
    (bc, hc, lead), (bt, ht, _) = _guarded(native, 1), _guarded(native, 1)
    view = native.make_view(x.data_ptr(), native.F64, 0, 0)
    with pytest.raises(NotImplementedError, match=r"fewer than 2\^31 samples per output row"):
        plan.execute_sum([view], view, 1, n, bc.ptr + 8 * lead, bt.ptr + 8 * lead)
    torch.cuda.synchronize()
    for buf, host in ((bc, hc), (bt, ht)):
        buf.download(host)
        buf.close()
        assert (host == SENTINEL).all()
    assert plan.describe() == before
    cnt, tot, _ = xh.histogram_sum(x[:4096], values=x[:4096], bins=edges)  # (and a valid call still runs)
    assert int(cnt[0]) == 4096 and float(tot[0]) == 2048.0


# ---------------------------------------------------------------------------------------------------------------------
# 8. dask, in the interpreter that has it
# ---------------------------------------------------------------------------------------------------------------------
PY39 = "/opt/conda/bin/python3.9"
SCRIPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sum_dask_script.py")


def _have_dask_python():
    return os.path.exists(PY39) and subprocess.run([PY39, "-c", "import dask.array, numpy"], capture_output=True).returncode == 0


@pytest.mark.skipif(not _have_dask_python(), reason="no interpreter with dask in this image")
def test_dask_blocks_complete_along_the_reduced_axes():
    env = dict(os.environ)
    sys_cxx = "/usr/lib/x86_64-linux-gnu/libstdc++.so.6"  # (as tests/test_dask_branch.py: conda's libstdc++ is older)
    if os.path.exists(sys_cxx):
        env["LD_PRELOAD"] = (sys_cxx + ":" + env["LD_PRELOAD"]) if env.get("LD_PRELOAD") else sys_cxx
    r = subprocess.run([PY39, "-W", "ignore", SCRIPT], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "SUM-DASK-OK" in r.stdout
