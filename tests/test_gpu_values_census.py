"""A directed census of the launch variants of histogram_extrema and histogram_mean_var (xhist_values.hip.h).

The kernel census (tests/test_gpu_census.py) sees which kernel symbol a call picks; most of what the values launcher decides
happens at run time inside one symbol: the copies of the fast family's slots, where the tables are read from, the LDS borders
of each family and home, segments per row, row chunks, grouped rows, unaligned row starts.  Every case here is built for one
such variant, runs BOTH statistics on resident data, and asserts:
  - the describe() line of each statistic equals `predict()`, a restatement of choose_values / values_geometry from the plan's
    table sizes, the slot sizes and the 160 KiB of LDS a workgroup may take (a case that lands elsewhere fails);
  - extrema bit for bit against tests/extrema_oracle.py;
  - the mean_var count equal to the oracle's and to the histogram's, the mean bit for bit, M2 / var bit for bit for
    power-of-two counts up to 2^9 and within the float64 bound of tests/values_exact.py otherwise.
Samples come from test_gpu_census.samples_for (on edges, on their neighbours, outside, NaN, +-inf); float32 samples also sit on
both float32 neighbours of float64 edges.  Values are on the exactly summable grid of tests/values_exact.py.

The row-chunk tests run more than 2^31 rows of one column through grouped views of small periodic arrays."""
import re

import numpy as np
import pytest

import extrema_oracle as eo
import meanvar_oracle as mo
import values_exact as vx
from test_gpu_census import edges_of, samples_for
from test_gpu_parity import _plan_for, xh  # noqa: F401  (xh: the module fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F64, F32 = np.float64, np.float32
LDS_MAX = 160 * 1024
# a bin's LDS slot in bytes per statistic and pass (0: no such pass): the generic family / the fast family on float32 values
SLOTS = {"mean_var": ((16, 24), (16, 24)), "extrema": ((16, 0), (8, 0))}
COPIES = {"mean_var": True, "extrema": False}


# ---------------------------------------------------------------------------------------------------------------------
# the launcher's choice, restated (xhist_plan.hip.h build_domain for the table sizes, xhist_values.hip.h for the rest)
# ---------------------------------------------------------------------------------------------------------------------
def _lut_k(n_edges, lut16):
    if n_edges > 65535:
        return 0
    k = 8
    while k < min(4 * n_edges, 1 << 20):
        k *= 2
    k = min(4096, max(8, k))
    return 2 * k if lut16 else k


def _tbytes(words):
    return (words + 1) // 2 * 16


def table_bytes(edges, which):
    """LDS bytes of a plan's table set: "native" (float64 / int64 edges, 4-byte bucket entries), "fine64" (float64 edges, 2-byte
    entries), "fine32" (float32 thresholds, 2-byte entries); every edge array carries 4 sentinels"""
    ns = [len(e) for e in edges]
    if which == "fine32":
        eo_ = sum((n + 5) // 2 for n in ns)
    else:
        eo_ = sum(n + 4 for n in ns)
    per = 2 if which == "native" else 4
    off = per * eo_ + sum(_lut_k(n, which != "native") for n in ns)
    return _tbytes((off + per - 1) // per)


def _copies_log2(n_bins, slot, tbytes):
    cl = 0
    while cl < 4 and (n_bins * slot << (cl + 1)) <= 24 * 1024 and tbytes + (n_bins * slot << (cl + 1)) <= LDS_MAX:
        cl += 1
    return cl


def predict(stat, cus, edges, cmp, sdt, vdt, n_rows, n_cols, fine=True, arith=False, layout_fast=True):
    """the describe() fields of `stat` on this input: family, slots, copies, block, segs, lds_bytes, tables_in_lds, D, cmp.
    fine: the edges put at most two edges into a bucket of the fine grid (True), or exactly that many (1 / 2); arith: the plan found them arithmetic; layout_fast:
    unit column strides (or one column) for samples and values"""
    D = len(edges)
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    f32 = np.dtype(sdt) == F32
    out = dict(D=D, cmp=cmp, scan=0, copies=1)
    bytes_g, bytes_32 = SLOTS[stat]
    fast_ok = (cmp == 0 and D <= 2 and np.dtype(sdt) in (np.dtype(F64), np.dtype(F32)) and np.dtype(vdt) == np.dtype(sdt)
               and n_bins < (1 << 24) and layout_fast)
    lds_bytes = None
    if fast_ok:
        b = bytes_32 if f32 else bytes_g
        slot = max(b)
        tb_fine = table_bytes(edges, "fine32" if f32 else "fine64")
        tb = None
        if fine and tb_fine + n_bins * slot <= LDS_MAX:
            tb, out["scan"] = tb_fine, "fine" if fine is True else fine
        elif arith and n_bins * slot <= LDS_MAX:
            tb, out["scan"] = 0, 5
        if tb is not None:
            cl = _copies_log2(n_bins, slot, tb) if COPIES[stat] else 0
            out.update(family="fast", slots="lds", tables_in_lds=1, copies=1 << cl)
            lds_bytes = [tb + (n_bins * k << cl) if k else 0 for k in b]
    if lds_bytes is None:
        tb = table_bytes(edges, "native")
        til = tb + 1024 <= LDS_MAX
        lds = til and n_bins < (1 << 24) and tb + n_bins * max(bytes_g) <= LDS_MAX
        out.update(family="generic", slots="lds" if lds else "global", tables_in_lds=int(til))
        lds_bytes = [(tb + (n_bins * k if lds else 0)) if til and k else 0 for k in bytes_g]
    fast = out["family"] == "fast"
    block = 256 if fast else 512
    vec = 4 if f32 else 2
    per_tile = block * (4 * vec if D == 1 else 8) if fast else block
    lds = max(lds_bytes)
    bpc = 2048 // block
    if lds:
        bpc = max(1, min(bpc, 160 * 1024 // lds))
    tiles = -(-n_cols // per_tile)
    segs = max(1, min(tiles, -(-cus * bpc // n_rows)))
    segs = max(segs, -(-(tiles * per_tile) // (1 << 31)))
    out.update(block=block, segs=segs, lds_bytes=lds_bytes if stat == "mean_var" else lds_bytes[:1])
    return out


def parse(desc):
    """describe() of a values call -> the fields `predict` gives"""
    kv = dict(re.findall(r"(\w+)=(\S+)", desc))
    if desc.startswith("mean_var"):
        fam = kv["pass1"].replace("mv_sum_", "")
        assert kv["pass2"] == "mv_dev_" + fam, desc
    else:
        fam = kv["family"]
    out = dict(family=fam, slots=kv["slots"], scan=int(kv["scan"]), block=int(kv["block"]), segs=int(kv["segs"]),
               tables_in_lds=int(kv["tables_in_lds"]), D=int(kv["D"]), cmp=int(kv["cmp"]), copies=int(kv.get("copies", 1)),
               lds_bytes=[int(t) for t in kv["lds_bytes"].split("/")])
    return out


def assert_variant(desc, want):
    got = parse(desc)
    w = dict(want)
    if w["scan"] == "fine":
        assert got["scan"] in (1, 2), (desc, want)
        w["scan"] = got["scan"]
    assert got == w, "landed elsewhere:\n  got  %s\n  want %s\n  (%s)" % (got, w, desc)
    return got


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------
def f32_neighbours(e):
    """both float32 neighbours of each float64 edge: the largest float32 below it and the smallest at or above it"""
    e = np.asarray(e, F64)
    f = e.astype(F32)
    up = np.where(f.astype(F64) < e, np.nextafter(f, F32(np.inf)), f)
    down = np.where(up.astype(F64) < e, up, np.nextafter(up, F32(-np.inf)))
    return down, up


def float_samples(edges, n_rows, n_cols, dt, seed):
    xs = samples_for(edges, n_rows, n_cols, dt, seed)
    if np.dtype(dt) == F32:
        rng = np.random.default_rng(seed + 5)
        for x, e in zip(xs, edges):
            down, up = f32_neighbours(e)
            flat = x.reshape(-1)
            k = max(2, flat.size // 16)
            pos = rng.permutation(flat.size)[:k]
            j = rng.integers(0, len(e), k)
            flat[pos] = np.where(rng.random(k) < 0.5, down[j], up[j])
    return xs


def int_samples(edges, n_rows, n_cols, dt, seed):
    """integer / datetime samples against integer edges: on edges, one beside them, inside, outside"""
    rng = np.random.default_rng(seed)
    out = []
    for e in edges:
        ei = np.asarray(e).view(np.int64) if np.asarray(e).dtype.kind == "M" else np.asarray(e)
        lo, hi = ei[0], ei[-1]
        span = hi - lo
        uns = ei.dtype == np.uint64
        if uns:  # (above 2^63: inside the range and one past it)
            x = lo + rng.integers(0, int(span) + int(span) // 20 + 1, (n_rows, n_cols)).astype(np.uint64)
        else:
            x = rng.integers(int(lo) - int(span) // 20, int(hi) + int(span) // 20 + 1, (n_rows, n_cols)).astype(ei.dtype)
        flat = x.reshape(-1)
        idx = rng.permutation(flat.size)
        on = idx[: flat.size // 8]
        flat[on] = ei[rng.integers(0, len(ei), on.size)]
        nb = idx[flat.size // 8: flat.size // 6]
        step = np.ones(nb.size, np.int64) if uns else rng.choice([-1, 1], nb.size)
        flat[nb] = (ei[rng.integers(0, len(ei), nb.size)].astype(np.int64) + step).astype(ei.dtype) if not uns else \
            ei[rng.integers(0, len(ei), nb.size)] + np.uint64(1)
        flat[idx[-2:]] = [lo, hi]
        out.append(x.astype(np.asarray(e).dtype) if np.asarray(e).dtype.kind == "M" else x)
    return out


def grid_values(rng, shape, vdt):
    v = vx.grid(rng, shape, vdt)
    if np.dtype(vdt).kind == "f":
        v.reshape(-1)[rng.permutation(v.size)[: max(1, v.size // 100)]] = np.nan
    return v


# ---------------------------------------------------------------------------------------------------------------------
# the check
# ---------------------------------------------------------------------------------------------------------------------
def _want(samples, edges, values):
    """oracle results for [R, C] host arrays: (vmin, vmax), (count, mean, M2*, bound, exact), the histogram's counts (NaN
    values included); flat shapes [R * n_bins]"""
    cmp_s, cmp_e = [], []
    for s, e in zip(samples, edges):  # per input: float64 if either side is a float (numpy's promotion), else the integers
        s, e = np.asarray(s), np.asarray(e)
        if s.dtype.kind == "M":
            s, e = s.view(np.int64), e.astype(s.dtype).view(np.int64)
        elif s.dtype.kind == "f" or e.dtype.kind == "f":
            s, e = s.astype(F64), e.astype(F64)
        cmp_s.append(s)
        cmp_e.append(e)
    lo, hi = eo.extrema_rows(cmp_s, cmp_e, values)
    ok, flat, nbs = mo._flat_bins(cmp_s, cmp_e)
    m = samples[0].shape[0]
    n_bins = int(np.prod(nbs))
    flat = flat + (np.arange(m, dtype=np.int64) * n_bins)[:, None]
    hist = np.bincount(flat[ok], minlength=m * n_bins)
    return (lo.reshape(-1), hi.reshape(-1)), vx.expected(flat[ok], np.asarray(values)[ok], m * n_bins), hist


def _bits(got, want, what):
    got = np.asarray(got, F64).reshape(-1)
    want = np.asarray(want, F64).reshape(-1)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN bins differ (%s)" % what
    ok = ~np.isnan(want)
    bad = got[ok].view(np.int64) != want[ok].view(np.int64)
    assert not bad.any(), "%d bins differ (%s): first %r != %r" % (bad.sum(), what, got[ok][bad][0], want[ok][bad][0])


def check_results(samples, edges, values, ext, mv, hist_count, ddof=None, what=""):
    """ext: (vmin, vmax); mv: (count, mean, M2) or, with ddof, (count, mean, var); hist_count: the histogram's counts, which
    differ from mean_var's by the counted samples whose value is NaN"""
    (lo, hi), (cnt, mean, m2, bound, exact), hist = _want(samples, edges, values)
    _bits(ext[0], lo, "extrema min " + what)
    _bits(ext[1], hi, "extrema max " + what)
    got_cnt = np.asarray(mv[0]).reshape(-1)
    assert got_cnt.dtype == np.int64
    np.testing.assert_array_equal(got_cnt, cnt, err_msg="count " + what)
    np.testing.assert_array_equal(np.asarray(hist_count).reshape(-1), hist, err_msg="histogram count " + what)
    nan_v = np.zeros(cnt.size, np.int64)
    vf = np.broadcast_to(np.asarray(values, F64), samples[0].shape)
    if np.isnan(vf).any():
        _, (cnt_all, *_), _ = _want(samples, edges, np.where(np.isnan(vf), 0.0, vf))
        nan_v = cnt_all - cnt
    np.testing.assert_array_equal(got_cnt + nan_v, np.asarray(hist_count).reshape(-1), err_msg="count + NaN values " + what)
    _bits(mv[1], mean, "mean " + what)
    if ddof is None:
        vx.assert_m2(mv[2], m2, bound, exact, "M2 " + what)
    else:
        var, vb = vx.var_bound(cnt, m2, bound, ddof)
        vx.assert_m2(mv[2], var, vb, exact, "var " + what)
    return cnt, exact


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


HITS = []  # (stat, parsed describe) of every case: the variants reached, for the closing test


def _expect_both(plan_desc_fn, run, want_ev, want_mv):
    """run(stat) runs one statistic; the plan's describe() after it must be the predicted variant"""
    outs = {}
    for stat, want in (("extrema", want_ev), ("mean_var", want_mv)):
        outs[stat] = run(stat)
        torch.cuda.synchronize()
        HITS.append((stat, assert_variant(plan_desc_fn(), want)))
    return outs


def run_public(core, xs_dev, v_dev, edges, axis, ddof, plan):
    """both statistics and the histogram through the public API on resident tensors"""
    def run(stat):
        if stat == "extrema":
            vmin, vmax, _ = core.histogram_extrema(*xs_dev, values=v_dev, bins=edges, axis=axis)
            return _np(vmin), _np(vmax)
        cnt, mean, var, _ = core.histogram_mean_var(*xs_dev, values=v_dev, bins=edges, axis=axis, ddof=ddof)
        return _np(cnt), _np(mean), _np(var)
    return run


def case_public(core, cus, edges, xs, v, *, cmp=0, fine=True, arith=False, layout_fast=True, ddof=0, xs_dev=None, v_dev=None,
                logical=None, what=""):
    """xs, v: host arrays [R, C] (or v broadcastable to it); xs_dev / v_dev: the device tensors to hand over (default: copies of
    xs / v); logical: the [R, C] host arrays the device tensors hold, when they are views of something else"""
    xs_dev = xs_dev if xs_dev is not None else [torch.as_tensor(x).cuda() for x in xs]
    v_dev = v_dev if v_dev is not None else torch.as_tensor(v).cuda()
    xl, vl = logical if logical is not None else (xs, np.broadcast_to(v, xs[0].shape))
    n_rows, n_cols = xl[0].shape
    plan = _plan_for(core, xs_dev, edges)
    sdt, vdt = xl[0].dtype, vl.dtype
    want_e = predict("extrema", cus, edges, cmp, sdt, vdt, n_rows, n_cols, fine, arith, layout_fast)
    want_m = predict("mean_var", cus, edges, cmp, sdt, vdt, n_rows, n_cols, fine, arith, layout_fast)
    outs = _expect_both(plan.describe, run_public(core, xs_dev, v_dev, edges, 1, ddof, plan), want_e, want_m)
    h, _ = core.histogram(*xs_dev, bins=edges, axis=1)
    check_results(list(xl), edges, vl, outs["extrema"], outs["mean_var"], _np(h), ddof=ddof, what=what)
    return outs


def _cus():
    from xhistogram_amd import _native

    return _native.device_info(0)["compute_units"]


# ---------------------------------------------------------------------------------------------------------------------
# 1. family x digitize form, on the fast family's dtypes
# ---------------------------------------------------------------------------------------------------------------------
FORM_EDGES = {  # (kind, bins per input for D = 1, 2), fine, arith: what the plan makes of them
    "k1": (("k1", (300,), (24, 30)), 1, False),
    "k2": (("k2", (300,), (24, 30)), 2, False),
    "lin": (("lin", (300,), (24, 30)), 1, True),
    "arith": (("lin", (5_000,), (3, 2_000)), 1, True),  # mean_var's fine tables no longer fit next to its slots: table-free
    "k3": (("k3", (300,), (24, 30)), False, False),  # three edges in one bucket, no fine table: the generic family
}


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("sdt", ["f64", "f32"])
@pytest.mark.parametrize("form", list(FORM_EDGES))
def test_family_and_digitize(xh, form, sdt, D):
    (kind, nb1, nb2), fine, arith = FORM_EDGES[form]
    st = F64 if sdt == "f64" else F32
    seed = 100 + 10 * list(FORM_EDGES).index(form) + 2 * D + (st == F32)
    edges = [edges_of(kind, nb, seed=seed + d) for d, nb in enumerate(nb1 if D == 1 else nb2)]
    xs = float_samples(edges, 3, 20_011, st, seed)
    v = grid_values(np.random.default_rng(seed), xs[0].shape, st)
    case_public(xh, _cus(), edges, xs, v, fine=fine, arith=arith, what="%s %s D=%d" % (form, sdt, D))
    if form == "k1":  # the same samples with values of another type: the generic family
        vo = grid_values(np.random.default_rng(seed + 1), xs[0].shape, F32 if st == F64 else F64)
        case_public(xh, _cus(), edges, xs, vo, fine=fine, arith=arith, ddof=1, what="%s %s D=%d other values" % (form, sdt, D))


# ---------------------------------------------------------------------------------------------------------------------
# 2. generic domains x homes
# ---------------------------------------------------------------------------------------------------------------------
def _domain_edges(dom, nb, rng):
    """bin edges of `nb` bins per input for compare domain 0 (float64, reached through values of another type), 1 (int64,
    datetime64, uint64 above 2^63) or 3 (an int64 input next to a float64 one)"""
    base = 1 << 58
    if dom == "f64":
        return [edges_of("k1", nb, seed=int(rng.integers(1000)))]
    if dom == "i64":
        return [base + np.sort(rng.choice(40 * nb, nb + 1, replace=False)).astype(np.int64)]
    if dom == "dt":
        return [(np.datetime64("2020-01-01") + np.sort(rng.choice(20 * nb, nb + 1, replace=False)).astype("timedelta64[m]")).astype("datetime64[s]")]
    if dom == "u64":
        return [np.uint64(1 << 63) + np.sort(rng.choice(40 * nb, nb + 1, replace=False)).astype(np.uint64)]
    if dom == "mixed":
        return [base + np.sort(rng.choice(40 * nb, nb + 1, replace=False)).astype(np.int64), edges_of("k2", 6, seed=3)]
    raise ValueError(dom)


HOME_BINS = {"lds": 200, "global_tables_lds": 9_000, "global_tables_l2": 21_000}  # (mixed: times the 6 float bins)


@pytest.mark.parametrize("home", list(HOME_BINS))
@pytest.mark.parametrize("dom", ["f64", "i64", "dt", "u64", "mixed"])
def test_generic_domain_and_home(xh, dom, home):
    rng = np.random.default_rng(50 + 3 * ["f64", "i64", "dt", "u64", "mixed"].index(dom) + list(HOME_BINS).index(home))
    nb = HOME_BINS[home] if dom != "mixed" else max(2, HOME_BINS[home] // 6)
    if dom == "mixed" and home == "global_tables_l2":
        nb = 21_000  # (the int64 input's edges alone must leave LDS)
    edges = _domain_edges(dom, nb, rng)
    n_rows, n_cols = 2, 20_011
    cmp = {"f64": 0, "i64": 1, "dt": 1, "u64": 1, "mixed": 3}[dom]
    xs = []
    for d, e in enumerate(edges):
        if np.asarray(e).dtype.kind == "f":
            xs += float_samples([e], n_rows, n_cols, F64, 7 + d)
        else:
            xs += int_samples([e], n_rows, n_cols, None, 7 + d)
    v = grid_values(rng, (n_rows, n_cols), F32 if dom == "f64" else F64)
    if dom == "i64":
        v = vx.grid(rng, (n_rows, n_cols), np.int32)  # integer values
    host = dom in ("dt", "u64")  # (torch holds neither datetime64 nor these uint64 samples: numpy inputs, uploaded by the call)
    case_public(xh, _cus(), edges, xs, v, cmp=cmp, fine=False, xs_dev=xs if host else None, v_dev=v if host else None,
                what="%s %s" % (dom, home))
    assert HITS[-1][1]["slots"] == ("lds" if home == "lds" else "global")
    assert HITS[-1][1]["tables_in_lds"] == (0 if home == "global_tables_l2" else 1)


# ---------------------------------------------------------------------------------------------------------------------
# 3. copies of the mean_var slots
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,copies", [(50, 16), (100, 8), (200, 4), (400, 2), (600, 1)])
@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_mean_var_copies(xh, nb, copies, sdt):
    st = F64 if sdt == "f64" else F32
    edges = [edges_of("lin", nb, seed=nb)]
    assert predict("mean_var", _cus(), edges, 0, st, st, 1, 1)["copies"] == copies
    xs = float_samples(edges, 2, 40_009, st, nb)
    v = grid_values(np.random.default_rng(nb), xs[0].shape, st)
    case_public(xh, _cus(), edges, xs, v, arith=True, what="copies %d" % copies)
    assert HITS[-1][0] == "mean_var" and HITS[-1][1]["copies"] == copies


# ---------------------------------------------------------------------------------------------------------------------
# 4. LDS borders: the last bin count a family or home takes, and the next one, which must move
# ---------------------------------------------------------------------------------------------------------------------
def _last(fn):
    n = 2
    while fn(n + 1):
        n += 1
    return n


def border_cases():
    """(stat, sample dtype, border, bins, expected family / home) for both sides of every border"""
    out = []
    for stat in ("mean_var", "extrema"):
        for sdt in (F64, F32):
            b = SLOTS[stat][1 if sdt == F32 else 0]
            slot = max(b)
            fine_t = "fine32" if sdt == F32 else "fine64"
            n = _last(lambda n: table_bytes([np.zeros(n + 1)], fine_t) + n * slot <= LDS_MAX)
            out += [(stat, sdt, "fine", n, "k1"), (stat, sdt, "fine", n + 1, "k1"), (stat, sdt, "fine", n + 1, "lin")]
            n = LDS_MAX // slot
            out += [(stat, sdt, "arith", n, "lin"), (stat, sdt, "arith", n + 1, "lin")]
        slot = max(SLOTS[stat][0])
        n = _last(lambda n: table_bytes([np.zeros(n + 1)], "native") + n * slot <= LDS_MAX)
        out += [(stat, "gen", "generic_lds", n, "k1"), (stat, "gen", "generic_lds", n + 1, "k1")]
    n = _last(lambda n: table_bytes([np.zeros(n + 1)], "native") + 1024 <= LDS_MAX)
    out += [("any", "gen", "tables_in_lds", n, "k1"), ("any", "gen", "tables_in_lds", n + 1, "k1")]
    return out


BORDERS = border_cases()


@pytest.mark.parametrize("i", range(len(BORDERS)), ids=["%s-%s-%s-%d-%s" % (s, getattr(t, "__name__", t), b, n, k) for s, t, b, n, k in BORDERS])
def test_lds_border(xh, i):
    stat, sdt, border, nb, kind = BORDERS[i]
    seed = 300 + i
    edges = [edges_of(kind, nb, seed=seed)]
    st = F64 if sdt in ("gen", F64) else F32
    xs = float_samples(edges, 1, 30_011, st, seed)
    vdt = F32 if sdt == "gen" else st  # (another value type: the generic family)
    v = grid_values(np.random.default_rng(seed), xs[0].shape, vdt)
    case_public(xh, _cus(), edges, xs, v, fine=kind != "geom", arith=kind == "lin", what="border %s %s %d" % (stat, border, nb))
    # the border itself: the family / home on each side, for the statistic the border belongs to
    for s, got in HITS[-2:]:
        if s != stat and stat != "any":
            continue
        want = predict(s, _cus(), edges, 0, st, vdt, 1, 30_011, True, kind == "lin")
        assert got["family"] == want["family"] and got["slots"] == want["slots"]


def test_lds_borders_sit_where_the_slots_say():
    """the borders of border_cases, spelled out: each statistic's largest bin counts per family and home (1-D)"""
    sides = {}
    for stat, sdt, border, nb, kind in BORDERS:
        sides.setdefault((stat, getattr(sdt, "__name__", sdt), border), []).append(nb)
    assert sides[("mean_var", "float64", "arith")] == [6826, 6827]  # 160 KiB / 24 B
    assert sides[("extrema", "float64", "arith")] == [10240, 10241]  # / 16 B
    assert sides[("extrema", "float32", "arith")] == [20480, 20481]  # / 8 B
    # extrema's float64 and float32 fine borders fill LDS to the byte: `<=` and not `<` decides them
    for sdt, nb in ((F64, sides[("extrema", "float64", "fine")][0]), (F32, sides[("extrema", "float32", "fine")][0])):
        t = table_bytes([np.zeros(nb + 1)], "fine32" if sdt == F32 else "fine64")
        assert t + nb * (8 if sdt == F32 else 16) == LDS_MAX


# ---------------------------------------------------------------------------------------------------------------------
# 5. geometry, alignment and value layouts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_geometry_segments(xh, sdt):
    st = F64 if sdt == "f64" else F32
    edges = [edges_of("k1", 40, seed=1)]
    rng = np.random.default_rng(11)
    tile = 256 * 4 * (4 if st == F32 else 2)  # (the fast family's tile of one input)
    # rows that fill the device over two tiles each / segments per row / below one tile
    for n_rows, n_cols, one in ((2_048, tile + 1, True), (64, 20_000, False), (2, 200_003, False), (5, 700, True)):
        xs = float_samples(edges, n_rows, n_cols, st, n_rows)
        v = grid_values(rng, xs[0].shape, st)
        case_public(xh, _cus(), edges, xs, v, what="rows %d cols %d" % (n_rows, n_cols))
        for _, h in HITS[-2:]:
            assert (h["segs"] == 1) == one, (n_rows, n_cols, h)
    # the generic family with its slots in LDS (512-thread blocks, three tiles a row): rows fill the device at cus * 4
    xs = float_samples(edges, 1_100, 1_100, st, 3)
    v = grid_values(rng, xs[0].shape, F64 if st == F32 else F32)
    case_public(xh, _cus(), edges, xs, v, what="generic rows fill")
    assert HITS[-1][1]["segs"] == 1


@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_alignment(xh, sdt):
    """row starts and data pointers element-aligned but not 16-byte aligned: the fast family's vector loads take them"""
    st = F64 if sdt == "f64" else F32
    edges = [edges_of("k2", 60, seed=2), edges_of("k1", 7, seed=3)]
    rng = np.random.default_rng(12)
    for shape in ((3, 20_011), (4, 9_999), (65, 301)):  # odd row lengths: every other row starts off 16 bytes
        xs = float_samples(edges, shape[0], shape[1] + 1, st, shape[1])
        v = grid_values(rng, xs[0].shape, st)
        xd = [torch.as_tensor(x).cuda() for x in xs]
        vd = torch.as_tensor(v).cuda()
        xo, vo = [t[:, 1:] for t in xd], vd[:, 1:]  # data offset by one element
        assert all(t.data_ptr() % 16 for t in xo) and vo.data_ptr() % 16
        case_public(xh, _cus(), edges, None, None, xs_dev=xo, v_dev=vo, logical=([x[:, 1:] for x in xs], v[:, 1:]),
                    what="offset %s" % (shape,))
        assert HITS[-1][1]["family"] == "fast"
        xs1 = [np.ascontiguousarray(x[:, 1:]) for x in xs]  # odd row lengths, contiguous
        case_public(xh, _cus(), edges, xs1, np.ascontiguousarray(v[:, 1:]), what="odd rows %s" % (shape,))
        assert HITS[-1][1]["family"] == "fast"
    # a 1-D array that starts one element in
    x1 = float_samples(edges[:1], 1, 50_001, st, 9)[0].reshape(-1)
    v1 = grid_values(rng, x1.shape, st)
    xd, vd = torch.as_tensor(x1).cuda()[1:], torch.as_tensor(v1).cuda()[1:]
    vmin, vmax, _ = xh.histogram_extrema(xd, values=vd, bins=edges[:1])
    cnt, mean, var, _ = xh.histogram_mean_var(xd, values=vd, bins=edges[:1])
    h, _ = xh.histogram(xd, bins=edges[:1])
    check_results([x1[None, 1:]], edges[:1], v1[None, 1:], (_np(vmin), _np(vmax)), (_np(cnt), _np(mean), _np(var)), _np(h), ddof=0,
                  what="x[1:]")


@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_values_broadcast(xh, sdt):
    """values broadcast with stride 0 across rows (fast layout) and along rows (one value per row: the generic family)"""
    st = F64 if sdt == "f64" else F32
    edges = [edges_of("k1", 80, seed=4)]
    rng = np.random.default_rng(13)
    xs = float_samples(edges, 6, 12_007, st, 13)
    across = vx.grid(rng, (1, 12_007), st)
    case_public(xh, _cus(), edges, xs, across, v_dev=torch.as_tensor(across).cuda().expand(6, 12_007),
                logical=(xs, np.broadcast_to(across, (6, 12_007))), what="across rows")
    assert HITS[-1][1]["family"] == "fast"
    along = vx.grid(rng, (6, 1), st)
    case_public(xh, _cus(), edges, xs, along, v_dev=torch.as_tensor(along).cuda().expand(6, 12_007), layout_fast=False,
                logical=(xs, np.broadcast_to(along, (6, 12_007))), ddof=1, what="along rows")
    assert HITS[-1][1]["family"] == "generic"


# ---------------------------------------------------------------------------------------------------------------------
# 6. the C ABI's row shapes: grouped rows, one column at a column stride
# ---------------------------------------------------------------------------------------------------------------------
def _tag(dt):
    from xhistogram_amd import _native

    return _native.F64 if np.dtype(dt) == F64 else _native.F32


def run_views(core, edges, views, vview, n_rows, n_cols, host_samples, host_values, want_e, want_m, what):
    """both statistics and the histogram on C ABI views; host_*: the logical [n_rows, n_cols] arrays"""
    from xhistogram_amd import _native

    plan = core._get_plan([np.asarray(e, F64) for e in edges], _native.CMP_F64, 0)
    nbins = plan.n_bins
    stream = torch.cuda.current_stream().cuda_stream
    ext = torch.empty((2, n_rows, nbins), dtype=torch.float64, device="cuda")
    cnt = torch.empty((n_rows, nbins), dtype=torch.int64, device="cuda")
    mean = torch.empty((n_rows, nbins), dtype=torch.float64, device="cuda")
    m2 = torch.empty((n_rows, nbins), dtype=torch.float64, device="cuda")
    hist = torch.zeros((n_rows, nbins), dtype=torch.int64, device="cuda")

    def run(stat):
        if stat == "extrema":
            plan.execute_extrema(views, vview, n_rows, n_cols, ext[0].data_ptr(), ext[1].data_ptr(), stream=stream)
        else:
            plan.execute_mean_var(views, vview, n_rows, n_cols, cnt.data_ptr(), mean.data_ptr(), m2.data_ptr(), stream=stream)

    _expect_both(plan.describe, run, want_e, want_m)
    plan.execute(views, None, n_rows, n_cols, hist.data_ptr(), False, _native.MEM_DEVICE, stream=stream)
    torch.cuda.synchronize()
    check_results(host_samples, edges, host_values, (_np(ext[0]), _np(ext[1])), (_np(cnt), _np(mean), _np(m2)), _np(hist), what=what)


@pytest.mark.parametrize("family", ["fast", "generic"])
@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_grouped_rows(xh, family, sdt):
    """rows in groups (inner_rows != 0): G groups of I rows.  fast: [G, I + 1, C] with the last row of each group skipped (unit
    column stride); generic: [G, C, I], the rows the contiguous direction (column stride I)"""
    from xhistogram_amd import _native

    st = F64 if sdt == "f64" else F32
    G, I, C = 5, 7, 3_001
    edges = [edges_of("k1", 30, seed=5), edges_of("lin", 9, seed=6)]
    xs = float_samples(edges, G * I, C, st, 21)
    v = grid_values(np.random.default_rng(21), (G * I, C), st)
    if family == "fast":
        def lay(a):  # [G*I, C] -> [G, I + 1, C], the logical rows at [g, i, :]
            big = np.full((G, I + 1, C), np.nan, a.dtype)
            big[:, :I, :] = a.reshape(G, I, C)
            return torch.as_tensor(big).cuda(), dict(row_stride=C, col_stride=1, inner_rows=I, outer_stride=(I + 1) * C)
    else:
        def lay(a):  # [G*I, C] -> [G, C, I]
            return torch.as_tensor(np.ascontiguousarray(a.reshape(G, I, C).transpose(0, 2, 1))).cuda(), \
                dict(row_stride=1, col_stride=I, inner_rows=I, outer_stride=C * I)
    dev = [lay(x) for x in xs]
    vdev = lay(v)
    views = [_native.make_view(t.data_ptr(), _tag(st), **kw) for t, kw in dev]
    vview = _native.make_view(vdev[0].data_ptr(), _tag(st), **vdev[1])
    lf = family == "fast"
    want_e = predict("extrema", _cus(), edges, 0, st, st, G * I, C, True, False, lf)
    want_m = predict("mean_var", _cus(), edges, 0, st, st, G * I, C, True, False, lf)
    assert want_m["family"] == family
    run_views(xh, edges, views, vview, G * I, C, xs, v, want_e, want_m, "grouped %s" % family)


@pytest.mark.parametrize("sdt", ["f64", "f32"])
def test_one_column_at_a_column_stride(xh, sdt):
    """n_cols == 1 with column strides 7 and 0: the fast family takes it (no vector load crosses a column)"""
    from xhistogram_amd import _native

    st = F64 if sdt == "f64" else F32
    R = 3_000
    edges = [edges_of("k2", 20, seed=8)]
    x = float_samples(edges, R, 1, st, 31)[0]
    v = grid_values(np.random.default_rng(31), (R, 1), st)
    xb = np.zeros((R, 3), st)
    xb[:, 0] = x[:, 0]
    vb = np.zeros((R, 3), st)
    vb[:, 0] = v[:, 0]
    xd, vd = torch.as_tensor(xb).cuda(), torch.as_tensor(vb).cuda()
    for cs in (7, 0):
        views = [_native.make_view(xd.data_ptr(), _tag(st), 3, cs)]
        vview = _native.make_view(vd.data_ptr(), _tag(st), 3, cs)
        want_e = predict("extrema", _cus(), edges, 0, st, st, R, 1)
        want_m = predict("mean_var", _cus(), edges, 0, st, st, R, 1)
        assert want_m["family"] == "fast"
        run_views(xh, edges, views, vview, R, 1, [x], v, want_e, want_m, "one column, stride %d" % cs)


# ---------------------------------------------------------------------------------------------------------------------
# 7. row chunks: more than 2^31 launch rows
# ---------------------------------------------------------------------------------------------------------------------
N_BIG = (1 << 31) + (1 << 20)
P_S, P_V = 1021, 1031  # the periods of samples and values (coprime: every pair of phases meets once per P_S * P_V rows)


def _periodic():
    rng = np.random.default_rng(77)
    xs = rng.uniform(-0.25, 1.25, P_S)  # edges [0, 1]: about a third outside
    xs[:4] = [0.0, 1.0, np.nan, -0.0]
    xs[rng.integers(4, P_S, 20)] = np.nan
    vs = vx.grid(rng, P_V)
    vs[rng.integers(0, P_V, 60)] = np.nan
    return xs, vs


def _need(nbytes):
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes + (6 << 30):
        pytest.skip("needs %.1f GB of free device memory, %.1f GB free" % (nbytes / 1e9, free / 1e9))


def _rows_expected(rows, xs_t, vs_t):
    """(counted, value) of the given rows (int64 tensor)"""
    x = xs_t[rows % P_S]
    v = vs_t[rows % P_V]
    counted = (x >= 0.0) & (x <= 1.0) & ~torch.isnan(v)
    return counted, v


def _check_rows(rows, xs_t, vs_t, outs, stat):
    counted, v = _rows_expected(rows, xs_t, vs_t)
    nan = torch.full_like(v, float("nan"))
    val = torch.where(counted, v, nan)
    if stat == "extrema":
        for o in outs:
            torch.testing.assert_close(o[rows, 0], val, rtol=0, atol=0, equal_nan=True)
    else:
        cnt, mean, m2 = outs
        torch.testing.assert_close(cnt[rows, 0], counted.to(torch.int64), rtol=0, atol=0)
        torch.testing.assert_close(mean[rows, 0], val, rtol=0, atol=0, equal_nan=True)
        torch.testing.assert_close(m2[rows, 0], torch.where(counted, torch.zeros_like(v), nan), rtol=0, atol=0, equal_nan=True)


def _whole(xs, vs):
    """(rows counted, sum of their values) over all N_BIG rows, from the periods"""
    cx = (xs >= 0.0) & (xs <= 1.0)
    cv = ~np.isnan(vs)
    per = P_S * P_V
    q, rem = divmod(N_BIG, per)
    n = q * int(cx.sum()) * int(cv.sum())
    s = q * int(cx.sum()) * float(np.sum(vs[cv]))
    r = np.arange(N_BIG - rem, N_BIG, dtype=np.int64)
    c = cx[r % P_S] & cv[r % P_V]
    return n + int(c.sum()), s + float(np.sum(vs[r % P_V][c]))


def _chunked_sum(t, fn, step=1 << 28):
    tot = 0
    for a in range(0, t.shape[0], step):
        tot += fn(t[a: a + step, 0]).item()
    return tot


@pytest.mark.parametrize("stat", ["extrema", "mean_var"])
def test_more_than_2_31_rows(xh, stat):
    """N_BIG rows of one column, grouped views of period P_S (samples) and P_V (values): row r reads element r mod P.  The rows
    go out in chunks of rows (every launch below 2^31 workgroups and 2^32 lanes); the rows on both sides of every chunk boundary,
    random rows and whole-array sums against the periodic arrays."""
    from xhistogram_amd import _native

    _need(N_BIG * (16 if stat == "extrema" else 32))
    xs, vs = _periodic()
    xs_t, vs_t = torch.as_tensor(xs).cuda(), torch.as_tensor(vs).cuda()
    edges = [np.array([0.0, 1.0])]
    plan = xh._get_plan(edges, _native.CMP_F64, 0)
    sview = _native.make_view(xs_t.data_ptr(), _native.F64, 1, 1, inner_rows=P_S, outer_stride=0)
    vview = _native.make_view(vs_t.data_ptr(), _native.F64, 1, 1, inner_rows=P_V, outer_stride=0)
    stream = torch.cuda.current_stream().cuda_stream
    if stat == "extrema":
        outs = [torch.empty((N_BIG, 1), dtype=torch.float64, device="cuda") for _ in range(2)]
        plan.execute_extrema([sview], vview, N_BIG, 1, outs[0].data_ptr(), outs[1].data_ptr(), stream=stream)
    else:
        outs = [torch.empty((N_BIG, 1), dtype=torch.int64, device="cuda")] + \
            [torch.empty((N_BIG, 1), dtype=torch.float64, device="cuda") for _ in range(2)]
        plan.execute_mean_var([sview], vview, N_BIG, 1, *[o.data_ptr() for o in outs], stream=stream)
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    print("\n%s over %d rows: %s; device memory in use after the call %.1f GB" % (stat, N_BIG, plan.describe(), (total - free) / 1e9))
    got = parse(plan.describe())
    assert got["family"] == "fast" and got["segs"] == 1, plan.describe()
    # the launches' chunks of rows: below 2^31 workgroups and 2^32 lanes (values_geometry); both sides of every boundary
    chunk = min((1 << 31) - 1, ((1 << 32) - 1) // got["block"]) // got["segs"]
    assert -(-N_BIG // chunk) > 100
    dev = outs[0].device
    bounds = [torch.arange(max(0, c - 32), min(N_BIG, c + 32)) for c in range(0, N_BIG + 1, chunk)]
    b31 = (1 << 31) - 1
    edges_rows = torch.cat(bounds + [torch.arange(b31 - 2048, b31 + 2048), torch.arange(N_BIG - 4096, N_BIG)]).to(dev)
    g = torch.Generator(device="cpu")
    g.manual_seed(3)
    rand_rows = torch.randint(0, N_BIG, (8192,), generator=g).to(dev)
    for rows in (edges_rows, rand_rows):
        _check_rows(rows, xs_t, vs_t, outs, stat)
    n_counted, s_counted = _whole(xs, vs)
    if stat == "extrema":
        for o in outs:
            assert _chunked_sum(o, lambda t: (~torch.isnan(t)).sum()) == n_counted
            assert _chunked_sum(o, lambda t: torch.nan_to_num(t, nan=0.0).sum()) == s_counted
    else:
        cnt, mean, m2 = outs
        assert _chunked_sum(cnt, lambda t: t.sum()) == n_counted
        assert _chunked_sum(mean, lambda t: torch.nan_to_num(t, nan=0.0).sum()) == s_counted
        assert _chunked_sum(m2, lambda t: (t == 0).sum()) == n_counted
        assert _chunked_sum(m2, lambda t: torch.isnan(t).sum()) == N_BIG - n_counted


# ---------------------------------------------------------------------------------------------------------------------
# what the sweep reached
# ---------------------------------------------------------------------------------------------------------------------
def test_zz_variants_reached():
    """every row of the variant table reached by some case of this module (a partial run checks only what it ran)"""
    if len(HITS) < 150:
        pytest.skip("only part of the module ran")
    mv = [h for s, h in HITS if s == "mean_var"]
    ex = [h for s, h in HITS if s == "extrema"]
    assert {h["copies"] for h in mv if h["family"] == "fast"} >= {1, 2, 4, 8, 16}
    for hs in (mv, ex):
        fast = {(h["scan"], h["D"], h["lds_bytes"][0] > 0) for h in hs if h["family"] == "fast"}
        assert {s for s, _, _ in fast} >= {1, 2, 5}
        assert {d for _, d, _ in fast} == {1, 2}
        gen = {(h["cmp"], h["slots"], h["tables_in_lds"]) for h in hs if h["family"] == "generic"}
        for cmp in (0, 1, 3):
            assert {(cmp, "lds", 1), (cmp, "global", 1), (cmp, "global", 0)} <= gen, (cmp, sorted(gen))
        assert {h["segs"] == 1 for h in hs} == {True, False}
