"""A directed census of the launch variants of histogram_quantile and histogram_weighted_quantile (xhist_quantile.hip.h and the
two drivers, xhist_quantile.hip / xhist_quantile_w.hip).

The quantile drivers decide more at run time than any other statistic: the tier of the (G, d) search, the trade of the group
size G against the digit width d, d below 4 under the scratch cap, the home of each of the three binning passes (pass 0, the
digit pass, the unweighted family's successor pass), the row chunks of the radix scratch, and the rows per workgroup and the
sorted elements of the short-row family.  The kernel census sees which symbol ran, not which of these branches it took.  Every
case here is built for one such variant and asserts
  - its whole describe() line, field by field, against `predict_quantile`, a restatement of quantile_radix, pick_pass,
    launch_quantile_short, choose_values and values_geometry from the plan's table sizes and the struct sizes of the headers (a
    case that lands elsewhere fails);
  - unweighted: the result equal to tests/quantile_oracle.py (np.nanquantile per bin) with np.testing.assert_array_equal, for
    all five methods where the case is cheap and for "linear" and "nearest" elsewhere ("linear" and "midpoint" where the case
    is about the successor pass);
  - weighted: the result bit for bit against tests/weighted_quantile_oracle.py on the integer weights 0..7 (zero results by
    value, as tests/test_gpu_weighted_quantile.py compares them).
There is no tolerance anywhere in this module.

A radix case whose non-empty bins hold one value each proves nothing (q_init settles such bins at once and no digit pass is ever
live), so `radix_data` puts the samples of a row into a few dozen chosen flat bins (the first, the last = the highest flat
index, both sides of a row boundary of a 2-D histogram), at least 40 values each, by the recipe of test_gpu_quantile._hard:
ties, +-0, +-inf, NaN values, both signs (the first digit decides), keys that share 52 and more leading bits, and two keys that
differ in their lowest bit only (the last digit decides; with d = 3 it has one bit).  The other samples sit on edges, outside the
range and at NaN.  What needs no GPU of all this (the borders, what each case's prediction must show, the data conditions) is
spelled out in tests/test_quantile_census_cpu.py."""
import re

import numpy as np
import pytest

import exact_weights as xw
import quantile_oracle as qo
import test_gpu_quantile as tgq
import test_gpu_weighted_quantile as tgwq
import weighted_quantile_oracle as wqo
from test_gpu_census import edges_of
from test_gpu_meanvar_weighted import int_weights
from test_gpu_parity import _plan_for, xh  # noqa: F401  (xh: the module fixture)
from test_gpu_quantile import _record_describe  # noqa: F401  (the describe() line after every execute_quantile -> tgq.DESCS)
from test_gpu_values_census import LDS_MAX, _cus, _tag, float_samples, int_samples, table_bytes
from test_gpu_values_census_streams import _cmp
from test_gpu_weighted_quantile import _record_describe as _record_describe_w  # noqa: F401  (-> tgwq.DESCS)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F64, F32 = np.float64, np.float32
METHODS = tgq.METHODS
HITS = []  # (weighted, parsed describe, n_q) of every case: the variants reached, for the closing test

# xhist_quantile.hip.h / xhist_quantile_w.hip.h
Q_GROUP = 8  # kQGroup
SCRATCH_CAP = 256 << 20  # kQScratchCap
LDS_BUDGET = 40 * 1024  # kQLdsBudget
SHORT_COLS = {False: 4096, True: 2048}  # kQShortCols, kQWShortCols
SHORT_ELEM = {False: 12, True: 20}  # a sorted (bin, key) pair / (key, weight, slot) triple
SIZEOF = {"QWin": 40, "QTgt": 40, "QWWin": 24, "QWTgt": 32}
Q_LDS_MAX = LDS_MAX - 64  # (the launch header q_hdr() is static LDS next to the dynamic slots)


# ---------------------------------------------------------------------------------------------------------------------
# the drivers' choices, restated
# ---------------------------------------------------------------------------------------------------------------------
def win_bytes(weighted, T):
    """LDS bytes of a bin's slots in a window pass of T windows (the weighted pass 0 keeps one record of 24 bytes)"""
    return 24 if weighted else 36 * T


def digit_bytes(weighted, G, d):
    """LDS bytes of a bin's slots in a digit pass: G targets of 2^d uint32 counters (float64 sums)"""
    return G * (24 + ((8 if weighted else 4) << d))


def radix_row_bytes(weighted, bins, G, d):
    """the radix family's scratch per row of a chunk"""
    if weighted:
        return bins * (SIZEOF["QWWin"] + G * (SIZEOF["QWTgt"] + (8 << d)))
    return bins * (SIZEOF["QWin"] + G * (SIZEOF["QTgt"] + SIZEOF["QWin"] + (8 << d)))


def streams_fast(sdt, dtypes, layouts, n_cols):
    """choose_values' layout rule: every stream (samples, values, weights) has the sample dtype, unit column stride (or the row
    one column) and an element-aligned pointer.  layouts: (column stride, pointer) per stream, None: dense and aligned"""
    sdt = np.dtype(sdt)
    layouts = layouts or [(1, 0)] * len(dtypes)
    assert len(layouts) == len(dtypes)
    return all(np.dtype(dt) == sdt and (cs == 1 or n_cols == 1) and ptr % sdt.itemsize == 0 for dt, (cs, ptr) in zip(dtypes, layouts))


def choose(edges, cmp, sdt, slot, layout_fast, fine=1, arith=True):
    """choose_values with a single slot size and no copies, in Q_LDS_MAX bytes: (fast, lds, scan, lds_bytes)"""
    D = len(edges)
    n_bins = int(np.prod([len(e) - 1 for e in edges], dtype=np.int64))
    f32 = np.dtype(sdt) == F32
    if cmp == 0 and D <= 2 and np.dtype(sdt) in (np.dtype(F64), np.dtype(F32)) and n_bins < (1 << 24) and layout_fast:
        tb = table_bytes(edges, "fine32" if f32 else "fine64")
        if fine and tb + n_bins * slot <= Q_LDS_MAX:
            return True, True, fine, tb + n_bins * slot
        if arith and n_bins * slot <= Q_LDS_MAX:
            return True, True, 5, n_bins * slot
    tb = table_bytes(edges, "native")
    til = tb + 1024 <= Q_LDS_MAX
    lds = til and n_bins < (1 << 24) and tb + n_bins * slot <= Q_LDS_MAX
    return False, lds, 0, (tb + (n_bins * slot if lds else 0)) if til else 0


def radix_search(weighted, n_bins, n_q, lds_of):
    """quantile_radix: (tier, G, d).  lds_of(slot) -> choose(...) of a digit pass with that slot"""
    best, G, d, tier = None, 0, 0, None
    for t in range(3):
        if G:
            break
        for g in range(min(Q_GROUP, n_q), 0, -1):
            for dd in range(8, (4 if t < 2 else 1) - 1, -1):
                cost = -(-n_q // g) * -(-64 // dd)
                if best is not None and cost >= best:
                    continue
                if radix_row_bytes(weighted, n_bins, g, dd) > SCRATCH_CAP and not (g == 1 and dd == 1):
                    continue
                _, lds, _, lds_bytes = lds_of(digit_bytes(weighted, g, dd))
                if lds != (t < 2) or (t == 0 and lds_bytes > LDS_BUDGET):
                    continue
                best, G, d, tier = cost, g, dd, t
    return tier, G, d


def geometry(cus, D, sdt, fast, lds, n_rows, n_cols):
    """values_geometry: (block, segs) of a pass over launches of n_rows rows"""
    block = 256 if fast else 512
    vec = 4 if np.dtype(sdt) == F32 else 2
    per_tile = block * (4 * vec if D == 1 else 8) if fast else block
    bpc = 2048 // block
    if lds:
        bpc = max(1, min(bpc, 160 * 1024 // lds))
    tiles = -(-n_cols // per_tile)
    segs = max(1, min(tiles, -(-cus * bpc // n_rows)))
    return block, max(segs, -(-(tiles * per_tile) // (1 << 31)))


def predict_quantile(weighted, cus, edges, cmp, sdt, vdt, wdt, layouts, n_rows, n_cols, n_q, fine=1, arith=True):
    """every field of the describe() line of a quantile call, as `parse_quantile` gives them.  layouts: (column stride, pointer)
    of each stream in the order samples..., values[, weights] (None: dense, aligned); fine / arith: what the plan makes of the
    edges (np.linspace edges: one edge per bucket of the fine grid, and arithmetic)"""
    D = len(edges)
    n_bins = int(np.prod([len(e) - 1 for e in edges], dtype=np.int64))
    head = "weighted_quantile" if weighted else "quantile"
    if n_cols <= SHORT_COLS[weighted]:
        R = max(1, min(SHORT_COLS[weighted] // max(n_cols, 1), ((1 << 32) - 2) // n_bins))
        N = 2
        while N < R * n_cols:
            N <<= 1
        out = dict(head=head, family="short", rows_per_wg=R, lds_bytes=N * SHORT_ELEM[weighted], groups=-(-n_q // Q_GROUP), block=256,
                   D=D, cmp=cmp)
        out["triples" if weighted else "pairs"] = N
        return out
    dtypes = [sdt] * D + [vdt] + ([wdt] if weighted else [])
    lf = streams_fast(sdt, dtypes, layouts, n_cols)

    def lds_of(slot):
        return choose(edges, cmp, sdt, slot, lf, fine, arith)

    tier, G, d = radix_search(weighted, n_bins, n_q, lds_of)
    passes = -(-64 // d)
    chunk = max(1, min(n_rows, SCRATCH_CAP // radix_row_bytes(weighted, n_bins, G, d)))
    fam = lambda c: "%s/%s" % ("fast" if c[0] else "generic", "lds" if c[1] else "global")  # noqa: E731
    digit, win0 = lds_of(digit_bytes(weighted, G, d)), lds_of(win_bytes(weighted, 1))
    block, segs = geometry(cus, D, sdt, digit[0], digit[3], chunk, n_cols)
    out = dict(head=head, family="radix", window=fam(win0), digits=fam(digit), scan="%d/%d" % (win0[2], digit[2]), d=d, group=G,
               groups=-(-n_q // G), passes=passes, chunks=-(-n_rows // chunk), rows_per_chunk=chunk, block=block, segs=segs,
               lds_bytes="%d/%d" % (win0[3], digit[3]), D=D, cmp=cmp)
    if not weighted:
        succ = lds_of(win_bytes(False, G))
        out["successor"] = "%s/%d" % (fam(succ), succ[3])
    return out


def parse_quantile(desc):
    """a quantile describe() line -> its first word and every field, numbers as integers"""
    head, _, rest = desc.partition(" ")
    kv = re.findall(r"(\w+)=(\S+)", rest)
    assert " ".join("%s=%s" % p for p in kv) == rest, desc  # (the whole line is fields)
    out = dict(head=head)
    for k, v in kv:
        assert k not in out, desc
        out[k] = int(v) if re.fullmatch(r"-?\d+", v) else v
    return out


def assert_line(desc, want):
    got = parse_quantile(desc)
    assert got == want, "landed elsewhere:\n  got  %s\n  want %s" % (got, want)
    return got


def tier_of(hit):
    """the tier of the (G, d) search a parsed radix line shows: digits in global memory 2, within kQLdsBudget 0, else 1"""
    if hit["digits"].endswith("/global"):
        return 2
    return 0 if int(hit["lds_bytes"].split("/")[1]) <= LDS_BUDGET else 1


def homes_of(hit):
    """(pass 0, successor, digits) homes of a parsed unweighted radix line"""
    return tuple(hit[k].split("/")[1] for k in ("window", "successor", "digits"))


def last_true(fn, lo, hi):
    """the largest n in [lo, hi) with fn(n), for fn true up to a border and false beyond (bisection)"""
    assert fn(lo) and not fn(hi), (lo, hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fn(mid) else (lo, mid)
    return lo


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------
QPOOL = (0.5, 0.25, 1.0, 0.0, 0.9, 0.1, 0.75, 1.0 / 3.0, 2.0 / 3.0, 0.99, 0.01, 0.6, 0.4, 0.05, 0.95, 0.2, 0.8)
N_CHOSEN, PER_BIN = 30, 60  # chosen flat bins of a row, samples in each (at most 2 of the values NaN)
N_KINDS = 8


def q_of(n_q):
    return np.array(QPOOL[:n_q])


def _uint(dt):
    return np.uint64 if np.dtype(dt) == F64 else np.uint32


def hard_values(kind, k, rng, vdt):
    """k values of `vdt` for one chosen bin, by the recipe of test_gpu_quantile._hard (k even)"""
    vdt = np.dtype(vdt)
    if vdt.kind != "f":  # integer values: ties and both signs
        return (np.full(k, 7) if kind == 0 else rng.integers(-50, 50, k)).astype(vdt)
    u = _uint(vdt)
    one = vdt.type(1.0)
    if kind == 0:  # every value equal: settled by q_init
        v = np.full(k, 2.5)
    elif kind == 1:  # +-0: two keys that differ in the top bit only
        v = np.where(rng.random(k) < 0.5, -0.0, 0.0)
    elif kind == 2:  # +-inf with finite values of both signs
        v = rng.choice([-np.inf, np.inf, 1.0, -2.0, 3.5, -0.5], k)
    elif kind == 3:  # 1 + j ulp
        v = (one.view(u) + rng.integers(0, 9, k).astype(u)).view(vdt)
    elif kind == 4:  # keys sharing 52 leading bits (float32 values: all but their low 11 mantissa bits)
        v = (vdt.type(1.5).view(u) + rng.integers(0, 1 << 11, k).astype(u)).view(vdt)
    elif kind == 5:  # heavy ties, both signs
        v = rng.integers(-2, 3, k).astype(F64)
    elif kind == 6:
        v = rng.standard_normal(k)
    else:  # two neighbouring values, half of the bin each: only the last key bit (of the value's type) tells them apart
        v = (vdt.type(-3.25).view(u) + (np.arange(k) % 2).astype(u)).view(vdt)
    v = np.asarray(v).astype(vdt)
    if kind not in (0, 7):
        v[rng.permutation(k)[:2]] = np.nan
    return v


def chosen_bins(nbs, n, rng):
    """n distinct flat bins of a histogram of shape nbs: the first, the last (the highest flat index), both sides of a row
    boundary of a 2-D histogram, and random ones"""
    total = int(np.prod(nbs, dtype=np.int64))
    must = [0, total - 1] + ([nbs[-1] - 1, nbs[-1]] if len(nbs) > 1 else [])
    must = list(dict.fromkeys(b for b in must if 0 <= b < total))
    n = min(n, total)
    rest = [int(b) for b in rng.permutation(total)[: n + len(must)] if b not in must] if total < (1 << 20) else \
        [int(b) for b in np.unique(rng.integers(0, total, 2 * n)) if b not in must]
    rng.shuffle(rest)
    return (must + rest)[:n]


def _inside(e, i, dt, rng):
    """samples of dtype dt inside bin i of edges e, one per element of i: mostly the middle, some on the left edge (float32
    samples stay off the edges: the rounding of an edge may leave the bin)"""
    e = np.asarray(e)
    if e.dtype.kind in "iu":
        return e[i].astype(dt)
    mid = 0.5 * (e[i] + e[i + 1])
    if np.dtype(dt) == F32:
        return mid.astype(dt)
    return np.where(rng.random(len(i)) < 0.2, e[i], mid).astype(dt)


def radix_data(edges, n_rows, n_cols, sdt, vdt, seed, sdts=None):
    """(samples [R, C] per input, values [R, C], the chosen flat bins of each row): N_CHOSEN bins of PER_BIN samples per row,
    their values by `hard_values` in rotation; the other samples on edges (a few dozen), outside the range and at NaN"""
    rng = np.random.default_rng(seed)
    nbs = [len(e) - 1 for e in edges]
    sdts = sdts or [sdt] * len(edges)
    xs = [np.empty((n_rows, n_cols), dt) for dt in sdts]
    v = np.empty((n_rows, n_cols), vdt)
    chosen = []
    for r in range(n_rows):
        bins = chosen_bins(nbs, N_CHOSEN, rng)
        chosen.append(bins)
        n_in = len(bins) * PER_BIN
        assert n_in + 100 <= n_cols
        flat = np.repeat(np.array(bins, np.int64), PER_BIN)
        idx = np.unravel_index(flat, nbs)
        cols = [_inside(e, i, dt, rng) for e, i, dt in zip(edges, idx, sdts)]
        vals = np.concatenate([hard_values((j + 1 + r) % N_KINDS, PER_BIN, rng, vdt) for j in range(len(bins))])
        n_fill = n_cols - n_in
        fill_v = rng.standard_normal(n_fill)
        fill_v[::7] = np.nan
        on_edge = 60
        fills = []
        for e, dt in zip(edges, sdts):
            e = np.asarray(e)
            lo, hi = e[0], e[-1]
            if e.dtype.kind in "iu":
                f = np.where(rng.random(n_fill) < 0.5, lo - 1 - rng.integers(0, 5, n_fill), hi + 1 + rng.integers(0, 5, n_fill)).astype(dt)
            else:
                f = np.where(rng.random(n_fill) < 0.5, lo - 0.5 - rng.random(n_fill), hi + 0.5 + rng.random(n_fill))
                f[rng.random(n_fill) < 0.3] = np.nan
                f = f.astype(dt)
            f[:on_edge] = e[rng.integers(0, len(e), on_edge)].astype(dt)
            fills.append(f)
        # a sample on an edge that would fall into a chosen bin goes outside instead: the chosen bins hold what `hard_values`
        # gave them and nothing else (their own samples sit on their left edges too)
        fb = np.zeros(on_edge, np.int64)
        for f, e, nb in zip(fills, edges, nbs):
            s, e = (f[:on_edge], np.asarray(e)) if np.asarray(e).dtype.kind in "iu" else (f[:on_edge].astype(F64), np.asarray(e, F64))
            fb = fb * nb + np.clip(np.where(s == e[-1], nb, np.searchsorted(e, s, side="right")) - 1, 0, nb - 1)
        fills[0][:on_edge][np.isin(fb, bins)] = np.asarray(edges[0])[-1] + 1
        for k, (c, f) in enumerate(zip(cols, fills)):
            xs[k][r] = np.concatenate([c, f])
        v_all = np.concatenate([vals, fill_v.astype(vdt) if np.dtype(vdt).kind == "f" else rng.integers(-9, 9, n_fill).astype(vdt)])
        p = rng.permutation(n_cols)
        for x in xs:
            x[r] = x[r][p]
        v[r] = v_all[p]
    return xs, v, chosen


def weights_for(shape, wdt, seed):
    """the integer weights 0..7 (exactly summable in any order), about one in eight of them 0"""
    return int_weights(np.random.default_rng(seed + 77), shape, wdt)


def keys_of(v):
    """the order-preserving uint64 keys of the float64 values v (extrema_key64), NaN values dropped"""
    v = np.asarray(v, F64)
    b = v[~np.isnan(v)].view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


# ---------------------------------------------------------------------------------------------------------------------
# running one case
# ---------------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _assert_same_w(got, want, what):
    """bit for bit, zero results by value (numpy keeps the input order of -0.0 and +0.0, the library orders -0.0 < +0.0)"""
    xw.assert_bits_equal(np.where(got == 0, 0.0, got), np.where(want == 0, 0.0, want), what)


def run_public(core, weighted, edges, dev, q, method, n_rows):
    """the public call on [R, C] device tensors reduced over axis 1: (result [n_q, R, bins], describe())"""
    xs_d, v_d, w_d = dev
    if weighted:
        got, _ = core.histogram_weighted_quantile(*xs_d, values=v_d, weights=w_d, q=q, bins=edges, axis=1)
        desc = tgwq.DESCS[-1]
    else:
        got, _ = core.histogram_quantile(*xs_d, values=v_d, q=q, bins=edges, axis=1, method=method)
        desc = tgq.DESCS[-1]
    return _np(got).reshape(len(q), n_rows, -1), desc


def run_abi(core, weighted, edges, views, q, method, n_rows, n_cols):
    """the C ABI call on views (sample views, value view, weight view or None) in the float64 domain"""
    from xhistogram_amd import _native

    plan = core._get_plan([np.asarray(e, F64) for e in edges], _native.CMP_F64, 0)
    sv, vv, wv = views
    out = torch.empty((len(q), n_rows, plan.n_bins), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if weighted:
        plan.execute_quantile_weighted(sv, vv, wv, n_rows, n_cols, out.data_ptr(), q, stream=stream)
    else:
        plan.execute_quantile(sv, vv, n_rows, n_cols, out.data_ptr(), q, _native.QUANTILE_METHODS.index(method), stream=stream)
    torch.cuda.synchronize()
    return _np(out), plan.describe()


def check_case(core, weighted, edges, xs, v, w, q, methods, *, cmp=0, layouts=None, dev=None, views=None, wdt=None, bits=False, what=""):
    """xs, v, w: the logical host arrays [R, C] (v, w broadcastable to it); dev: the (samples, values, weights) to hand to the
    public API (default: device copies of the host arrays); views: C ABI views to run instead; layouts: (column stride,
    pointer) per stream as the launcher sees them; wdt: the weights' dtype as the launcher sees it.  Returns the parsed line"""
    n_rows, n_cols = xs[0].shape
    q = np.asarray(q, F64)
    sdt, vdt = xs[0].dtype, np.asarray(v).dtype
    wdt = (wdt or np.asarray(w).dtype) if weighted else None
    want = predict_quantile(weighted, _cus(), edges, cmp, sdt, vdt, wdt, layouts, n_rows, n_cols, len(q))
    xc, ec = _cmp(xs, edges)
    vl = np.broadcast_to(np.asarray(v), xs[0].shape).astype(F64)
    if views is None and dev is None:
        dev = ([_dev(x) for x in xs], _dev(v), _dev(w) if weighted else None)
    hit = None
    for m in ((None,) if weighted else methods):
        if views is not None:
            got, desc = run_abi(core, weighted, edges, views, q, m, n_rows, n_cols)
        else:
            got, desc = run_public(core, weighted, edges, dev, q, m, n_rows)
        hit = assert_line(desc, want)
        msg = "%s %s %s" % (what, m, desc)
        if weighted:
            wl = np.broadcast_to(np.asarray(w), xs[0].shape).astype(F64)
            ref, _ = wqo.weighted_quantile_rows(xc, ec, vl, wl, q)
            _assert_same_w(got, ref.reshape(got.shape), msg)
        else:
            ref = qo.quantile_rows(xc, ec, vl, q, m).reshape(got.shape)
            if bits:
                xw.assert_bits_equal(got, ref, msg)
            np.testing.assert_array_equal(got, ref, err_msg=msg)
    HITS.append((weighted, hit, len(q)))
    return hit


# ---------------------------------------------------------------------------------------------------------------------
# 1. the radix family: tiers, G against d, homes, the scratch cap, chunks with groups, generic domains
# ---------------------------------------------------------------------------------------------------------------------
LIN_CUS = 256  # (the borders below do not depend on the CU count: it moves segs only)


def _lin(nbs):
    return [edges_of("lin", nb) for nb in nbs]


def _p(weighted, nbs, n_q, st=F64, n_rows=1, n_cols=4200):
    return predict_quantile(weighted, LIN_CUS, _lin(nbs), 0, st, st, st, None, n_rows, n_cols, n_q)


def border(weighted, st, what):
    """the last 1-D bin count of np.linspace edges, samples and values of dtype st, at which
    "digits": the d = 4 digit pass of one target still fits LDS (the next count is tier 2);
    "successor": the successor pass of a group of two targets still fits LDS (unweighted);
    "pass0": pass 0 still fits LDS"""
    if what == "digits":
        return last_true(lambda n: _p(weighted, (n,), 1, st)["digits"].endswith("/lds"), 100, 20_000)
    if what == "successor":
        return last_true(lambda n: "/lds/" in _p(False, (n,), 2, st)["successor"], 100, 20_000)
    return last_true(lambda n: _p(weighted, (n,), 1, st)["window"].endswith("/lds"), 100, 20_000)


def cap_border(weighted, d):
    """the last bin count at which a digit of d bits (one target) stays under the scratch cap"""
    return last_true(lambda n: radix_row_bytes(weighted, n, 1, d) <= SCRATCH_CAP, 1000, 1 << 23)


def _case(weighted, nbs, n_q, expect, methods=METHODS, st=F64, n_rows=1, n_cols=4200, dom="f64"):
    return dict(weighted=weighted, nbs=tuple(nbs), n_q=n_q, expect=expect, methods=methods, st=st, n_rows=n_rows, n_cols=n_cols, dom=dom)


LERP = ("linear", "midpoint")  # the methods that run the successor pass
FEW = ("linear", "nearest")


def generic_border(weighted, dom):
    """the last bin count (of the int64 input) at which the generic family's d = 4 digit pass of one target fits LDS next to the
    native tables; dom "i64": one int64 input, "mixed": an int64 input next to a float64 one of 3 bins"""
    def fits(n):
        edges = [np.zeros(n + 1, np.int64)] + ([np.zeros(4)] if dom == "mixed" else [])
        return choose(edges, 1 if dom == "i64" else 3, np.int64, digit_bytes(weighted, 1, 4), False)[1]
    return last_true(fits, 10, 20_000)


def radix_cases():
    c = {}
    U, W = False, True
    # tier 0: each d, the budget border, G against d
    for nb, d in ((4, 8), (40, 7), (100, 6), (200, 5)):
        c["u-tier0-d%d" % d] = _case(U, (nb,), 1, dict(tier=0, d=d, G=1))
    c["u-tier0-d4-G2"] = _case(U, (200,), 2, dict(tier=0, d=4, G=2))
    c["u-budget-19"] = _case(U, (19,), 2, dict(tier=0, d=8, G=2, digit_lds=40_528))
    c["u-budget-20"] = _case(U, (20,), 2, dict(tier=0, d=7, G=2))
    c["u-G7-d7"] = _case(U, (10,), 11, dict(tier=0, d=7, G=7, groups=2, last_group=4))
    c["u-G4-d4"] = _case(U, (100,), 5, dict(tier=0, d=4, G=4, groups=2, last_group=1))
    for nb, d in ((4, 8), (20, 7), (40, 6), (100, 5), (200, 4)):
        c["w-tier0-d%d" % d] = _case(W, (nb,), 1, dict(tier=0, d=d, G=1))
    c["w-budget-19"] = _case(W, (19,), 1, dict(tier=0, d=8, G=1, digit_lds=40_072))
    c["w-G7-d6"] = _case(W, (10,), 11, dict(tier=0, d=6, G=7, groups=2, last_group=4))
    c["w-G2-d4"] = _case(W, (100,), 5, dict(tier=0, d=4, G=2, groups=3, last_group=1))
    # tier 1
    c["u-tier1-d6"] = _case(U, (400,), 1, dict(tier=1, d=6, G=1))
    c["u-tier1-G4"] = _case(U, (465,), 5, dict(tier=1, d=4, G=4))
    c["u-tier1-G3"] = _case(U, (466,), 5, dict(tier=1, d=4, G=3))
    c["w-tier1-d5"] = _case(W, (400,), 1, dict(tier=1, d=5, G=1))
    c["w-tier1-G3"] = _case(W, (300,), 5, dict(tier=1, d=4, G=3, groups=2, last_group=2))
    # the last digit pass in LDS and the first in global memory; the homes of pass 0 / successor / digits apart
    for st, t in ((F64, "f64"), (F32, "f32")):
        b1, s2, p0 = border(U, st, "digits"), border(U, st, "successor"), border(U, st, "pass0")
        c["u-%s-digits-last-lds-%d" % (t, b1)] = _case(U, (b1,), 1, dict(tier=1, d=4, G=1, homes=("lds", "lds", "lds")), LERP, st)
        c["u-%s-digits-first-global-%d" % (t, b1 + 1)] = _case(U, (b1 + 1,), 1, dict(tier=2, d=8, G=1, homes=("lds", "lds", "global")), LERP, st)
        c["u-%s-apart-q2-%d" % (t, b1 + 9)] = _case(U, (b1 + 9,), 2, dict(tier=2, d=8, G=2, homes=("lds", "lds", "global")), LERP, st)
        c["u-%s-apart-q5-%d" % (t, b1 + 9)] = _case(U, (b1 + 9,), 5, dict(tier=2, d=8, G=5, homes=("lds", "global", "global")), LERP, st)
        c["u-%s-successor-last-lds-%d" % (t, s2)] = _case(U, (s2,), 2, dict(tier=2, d=8, G=2, homes=("lds", "lds", "global")), LERP, st)
        c["u-%s-successor-first-global-%d" % (t, s2 + 1)] = _case(U, (s2 + 1,), 2, dict(tier=2, d=8, G=2, homes=("lds", "global", "global")), LERP, st)
        c["u-%s-apart-q2-2500" % t] = _case(U, (2500,), 2, dict(tier=2, d=8, G=2, homes=("lds", "global", "global")), LERP, st)
        c["u-%s-pass0-last-lds-%d" % (t, p0)] = _case(U, (p0,), 1, dict(tier=2, d=8, G=1, homes=("lds", "lds", "global")), LERP, st, n_cols=6000)
        c["u-%s-pass0-first-global-%d" % (t, p0 + 1)] = _case(U, (p0 + 1,), 1, dict(tier=2, d=8, G=1, homes=("global", "global", "global")), LERP, st, n_cols=6000)
        b1, p0 = border(W, st, "digits"), border(W, st, "pass0")
        c["w-%s-digits-last-lds-%d" % (t, b1)] = _case(W, (b1,), 1, dict(tier=1, d=4, G=1, homes=("lds", "lds")), st=st)
        c["w-%s-digits-first-global-%d" % (t, b1 + 1)] = _case(W, (b1 + 1,), 1, dict(tier=2, d=8, G=1, homes=("lds", "global")), st=st)
        c["w-%s-pass0-last-lds-%d" % (t, p0)] = _case(W, (p0,), 2, dict(tier=2, d=8, G=2, homes=("lds", "global")), st=st, n_cols=6000)
        c["w-%s-pass0-first-global-%d" % (t, p0 + 1)] = _case(W, (p0 + 1,), 2, dict(tier=2, d=8, G=2, homes=("global", "global")), st=st, n_cols=6000)
    # the scratch cap: 2-D, generic/global, three rows in three chunks of one row
    for s, d, passes in ((1024, 4, 16), (1100, 3, 22), (1300, 2, 32), (1400, 1, 64), (1500, 1, 64)):
        c["u-cap-%d-d%d" % (s, d)] = _case(U, (s, s), 1, dict(tier=2, d=d, G=1, passes=passes, chunks=3, rows_per_chunk=1,
                                                             homes=("global", "global", "global")), FEW, n_rows=3)
    for s, d, passes in ((1200, 4, 16), (1300, 3, 22), (1600, 2, 32), (1800, 1, 64), (2000, 1, 64)):
        c["w-cap-%d-d%d" % (s, d)] = _case(W, (s, s), 1, dict(tier=2, d=d, G=1, passes=passes, chunks=3, rows_per_chunk=1,
                                                             homes=("global", "global")), n_rows=3)
    # row chunks together with groups: 20 (30) rows in chunks of 8 (14), two groups of 8 and 3 targets
    c["u-chunks-groups"] = _case(U, (1870,), 11, dict(tier=2, d=8, G=8, groups=2, last_group=3, chunks=3, rows_per_chunk=8), FEW, n_rows=20)
    c["w-chunks-groups"] = _case(W, (1100,), 11, dict(tier=2, d=8, G=8, groups=2, last_group=3, chunks=3, rows_per_chunk=14), n_rows=30)
    # the generic family's domains at the LDS border of the native tables: the last d = 4 digit pass in LDS, the first in tier 2
    for wt, t in ((U, "u"), (W, "w")):
        for dom in ("i64", "mixed"):
            n = generic_border(wt, dom)
            nbs = (n,) if dom == "i64" else (n, 3)
            c["%s-%s-last-lds-%d" % (t, dom, n)] = _case(wt, nbs, 1, dict(tier=1, d=4, G=1, digits="generic/lds"), FEW, dom=dom)
            nbs = (n + 1,) if dom == "i64" else (n + 1, 3)
            c["%s-%s-first-global-%d" % (t, dom, n + 1)] = _case(wt, nbs, 1, dict(tier=2, digits="generic/global"), FEW, dom=dom)
    return c


RADIX = radix_cases()


def radix_edges(case, seed=0):
    rng = np.random.default_rng(seed)
    if case["dom"] == "f64":
        return _lin(case["nbs"])
    ints = (1 << 58) + np.sort(rng.choice(40 * case["nbs"][0], case["nbs"][0] + 1, replace=False)).astype(np.int64)
    return [ints] if case["dom"] == "i64" else [ints, edges_of("lin", case["nbs"][1])]


def radix_inputs(name):
    """(edges, cmp, samples, values, weights or None, q) of a radix case"""
    case = RADIX[name]
    seed = sorted(RADIX).index(name)
    edges = radix_edges(case, seed)
    cmp = {"f64": 0, "i64": 1, "mixed": 3}[case["dom"]]
    st = case["st"]
    sdts = {"f64": None, "i64": [np.int64], "mixed": [np.int64, F64]}[case["dom"]]
    xs, v, chosen = radix_data(edges, case["n_rows"], case["n_cols"], st, st, seed, sdts)
    w = weights_for(v.shape, st, seed) if case["weighted"] else None
    return edges, cmp, xs, v, w, q_of(case["n_q"]), chosen


def radix_predict(name, cus=LIN_CUS):
    case = RADIX[name]
    edges = radix_edges(case, sorted(RADIX).index(name))
    cmp = {"f64": 0, "i64": 1, "mixed": 3}[case["dom"]]
    sdt = case["st"] if case["dom"] == "f64" else np.int64
    return predict_quantile(case["weighted"], cus, edges, cmp, sdt, case["st"], case["st"], None, case["n_rows"], case["n_cols"], case["n_q"])


def assert_expected(name, hit):
    """the parsed (or predicted) line has what the case's name claims"""
    case = RADIX[name]
    e = dict(case["expect"])
    assert tier_of(hit) == e.pop("tier"), (name, hit)
    if "homes" in e:
        homes = e.pop("homes")
        got = homes_of(hit) if not case["weighted"] else (hit["window"].split("/")[1], hit["digits"].split("/")[1])
        assert got == homes, (name, hit)
    if "G" in e:
        assert hit["group"] == e.pop("G"), (name, hit)
    if "last_group" in e:
        assert case["n_q"] - (hit["groups"] - 1) * hit["group"] == e.pop("last_group") < hit["group"], (name, hit)
    if "digit_lds" in e:
        assert int(hit["lds_bytes"].split("/")[1]) == e.pop("digit_lds") <= LDS_BUDGET, (name, hit)
    for k, val in e.items():
        assert hit[k] == val, (name, k, hit)


@pytest.mark.parametrize("name", list(RADIX))
def test_radix_variant(xh, name):
    case = RADIX[name]
    edges, cmp, xs, v, w, q, _ = radix_inputs(name)
    hit = check_case(xh, case["weighted"], edges, xs, v, w, q, case["methods"], cmp=cmp, what=name)
    assert hit["family"] == "radix"
    assert_expected(name, hit)


# ---------------------------------------------------------------------------------------------------------------------
# 2. layouts: through the public API, and the C ABI's views where the public API cannot make them
# ---------------------------------------------------------------------------------------------------------------------
def _view(t, st, **kw):
    from xhistogram_amd import _native

    return _native.make_view(t.data_ptr(), _tag(st), **kw)


def _offset(a, k):
    """a contiguous [R, C] device tensor of `a` that starts k elements past a 16-byte boundary"""
    flat = torch.empty(a.size + k, dtype=torch.as_tensor(a[:0]).dtype, device="cuda")
    assert flat.data_ptr() % 16 == 0
    t = flat[k:].view(a.shape)
    t.copy_(torch.as_tensor(np.ascontiguousarray(a)))
    return t


LAYOUTS = ("middle_axis", "values_row_stride_0", "values_col_stride_2", "values_offset_1",
           "weights_f32", "weights_col_stride_0", "weights_col_stride_2", "weights_offset_1", "weights_row_stride_0")
# the family each layout must take by choose_values: the sample dtype, unit column stride and an ELEMENT-aligned pointer keep
# the fast family, so a stream that starts one element past a 16-byte boundary stays fast (the fast body loads rows whose
# starts are not 16-byte aligned, as every odd row length makes them); any other column stride or dtype gives it up
LAYOUT_FAMILY = dict(middle_axis="generic", values_row_stride_0="fast", values_col_stride_2="generic", values_offset_1="fast",
                     weights_f32="generic", weights_col_stride_0="generic", weights_col_stride_2="generic", weights_offset_1="fast",
                     weights_row_stride_0="fast")


def layout_streams(layout, weighted, R, C):
    """((column stride, pointer offset in elements) per stream, the weights' dtype) of a layout case of float64 samples"""
    n = 3 if weighted else 2
    lay = [(1, 0)] * n
    wdt = F64
    if layout == "middle_axis":
        lay = [(4, 0)] * n
    elif layout == "values_col_stride_2":
        lay[1] = (2, 0)
    elif layout == "values_offset_1":
        lay[1] = (1, 8)
    elif layout == "weights_f32":
        wdt = F32
    elif layout == "weights_col_stride_0":
        lay[2] = (0, 0)
    elif layout == "weights_col_stride_2":
        lay[2] = (2, 0)
    elif layout == "weights_offset_1":
        lay[2] = (1, 8)
    return lay, wdt


LAYOUT_CASES = [(lay, wt) for lay in LAYOUTS for wt in (False, True) if wt or not lay.startswith("weights")]


@pytest.mark.parametrize("layout,weighted", LAYOUT_CASES, ids=["%s-%s" % (lay, "w" if wt else "u") for lay, wt in LAYOUT_CASES])
def test_layouts(xh, layout, weighted):
    R, C = (12, 4200) if layout == "middle_axis" else (3, 4200)
    edges = _lin((100,))
    seed = 300 + LAYOUTS.index(layout)
    xs, v, _ = radix_data(edges, R, C, F64, F64, seed)
    lay, wdt = layout_streams(layout, weighted, R, C)
    w = weights_for((R, C), wdt, seed) if weighted else None
    q = q_of(2)
    dense = dict(row_stride=C, col_stride=1)
    kw = dict(layouts=lay, wdt=wdt, what=layout)
    if layout == "middle_axis":  # [3, C, 4] reduced over axis 1 by the public API: rows (i, k), the columns at stride 4
        def lay3(a):
            return _dev(a.reshape(3, 4, C).transpose(0, 2, 1))
        xd, vd, wd = lay3(xs[0]), lay3(v), lay3(w) if weighted else None
        if weighted:
            got, _ = xh.histogram_weighted_quantile(xd, values=vd, weights=wd, q=q, bins=edges, axis=1)
            desc = tgwq.DESCS[-1]
            ref, _ = wqo.weighted_quantile_rows(xs, edges, v, w.astype(F64), q)
            _assert_same_w(_np(got).reshape(2, R, -1), ref.reshape(2, R, -1), layout)
        else:
            got, _ = xh.histogram_quantile(xd, values=vd, q=q, bins=edges, axis=1, method="midpoint")
            desc = tgq.DESCS[-1]
            np.testing.assert_array_equal(_np(got).reshape(2, R, -1), qo.quantile_rows(xs, edges, v, q, "midpoint").reshape(2, R, -1))
        hit = assert_line(desc, predict_quantile(weighted, _cus(), edges, 0, F64, F64, wdt, lay, R, C, 2))
        HITS.append((weighted, hit, 2))
    else:
        xd = _dev(xs[0])
        keep = [xd]
        vl, wl = v, w
        if layout == "values_row_stride_0":
            vl = v[:1]
            vd = _dev(vl)
            vv = _view(vd, F64, row_stride=0, col_stride=1)
        elif layout == "values_col_stride_2":
            wide = np.full((R, 2 * C), np.nan)
            wide[:, ::2] = v
            wide[:, 1::2] = v[:, ::-1]
            vd = _dev(wide)
            vv = _view(vd, F64, row_stride=2 * C, col_stride=2)
        else:
            vd = _offset(v, 1 if layout == "values_offset_1" else 0)
            vv = _view(vd, F64, **dense)
        keep.append(vd)
        wv = None
        if weighted:
            if layout == "weights_col_stride_0":  # one weight per row
                wl = w[:, :1]
                wd = _dev(wl)
                wv = _view(wd, wdt, row_stride=1, col_stride=0)
            elif layout == "weights_col_stride_2":
                wide = weights_for((R, 2 * C), wdt, seed + 1)
                wide[:, ::2] = w
                wd = _dev(wide)
                wv = _view(wd, wdt, row_stride=2 * C, col_stride=2)
            elif layout == "weights_row_stride_0":
                wl = w[:1]
                wd = _dev(wl)
                wv = _view(wd, wdt, row_stride=0, col_stride=1)
            else:
                wd = _offset(w, 1 if layout == "weights_offset_1" else 0)
                wv = _view(wd, wdt, **dense)
            keep.append(wd)
        lay = [(cs, t.data_ptr()) for (cs, _), t in zip(lay, keep)]
        if layout.endswith("offset_1"):
            assert (vd if layout.startswith("values") else wd).data_ptr() % 16 == 8
        kw["layouts"] = lay
        hit = check_case(xh, weighted, edges, xs, vl, wl, q, LERP, views=([_view(xd, F64, **dense)], vv, wv), **kw)
        del keep
    want = LAYOUT_FAMILY[layout] + "/lds"
    assert hit["window"] == hit["digits"] == want, hit
    if not weighted:
        assert hit["successor"].startswith(want), hit


# ---------------------------------------------------------------------------------------------------------------------
# 3. the short-row family: rows per workgroup R, sorted elements N, the last workgroup, groups of targets
# ---------------------------------------------------------------------------------------------------------------------
# (rows, columns, bins, n_q, sample dtype) -> what the shape was chosen for: (R, N, rows of the last workgroup)
SHORT = {
    False: {(5000, 1, (20,), 9, F64): (4096, 4096, 904), (7, 2, (1,), 1, F32): (2048, 4096, 7), (10, 1365, (100,), 8, F64): (3, 4096, 1),
            (9, 1366, (60,), 17, F32): (2, 4096, 1), (3, 4096, (100,), 1, F64): (1, 4096, 1), (5, 2049, (7, 5), 9, F32): (1, 4096, 1)},
    True: {(5000, 1, (20,), 9, F64): (2048, 2048, 904), (7, 2, (1,), 1, F32): (1024, 2048, 7), (10, 682, (100,), 8, F64): (3, 2048, 1),
           (9, 683, (60,), 17, F32): (2, 2048, 1), (3, 2048, (100,), 1, F64): (1, 2048, 1), (5, 1025, (7, 5), 9, F32): (1, 2048, 1)},
}
SHORT_CASES = [(w,) + k for w in (False, True) for k in SHORT[w]]


def short_inputs(weighted, n_rows, n_cols, nbs, n_q, st):
    seed = 500 + n_rows + n_cols
    edges = [edges_of("k1" if nb >= 3 else "lin", nb, seed=seed + d) for d, nb in enumerate(nbs)]
    xs = float_samples(edges, n_rows, n_cols, st, seed)
    rng = np.random.default_rng(seed)
    v = np.round(rng.standard_normal((n_rows, n_cols)) * 4.0, 1)
    sp = rng.random((n_rows, n_cols))
    v[sp < 0.02] = -0.0
    v[(sp >= 0.02) & (sp < 0.03)] = np.inf
    v[(sp >= 0.03) & (sp < 0.04)] = -np.inf
    v[(sp >= 0.04) & (sp < 0.07)] = np.nan
    v = v.astype(st)
    return edges, xs, v, (weights_for(v.shape, st, seed) if weighted else None), q_of(n_q)


@pytest.mark.parametrize("weighted,n_rows,n_cols,nbs,n_q,st", SHORT_CASES,
                         ids=["%s-%dx%d-q%d" % ("w" if c[0] else "u", c[1], c[2], c[4]) for c in SHORT_CASES])
def test_short_variant(xh, weighted, n_rows, n_cols, nbs, n_q, st):
    edges, xs, v, w, q = short_inputs(weighted, n_rows, n_cols, nbs, n_q, st)
    hit = check_case(xh, weighted, edges, xs, v, w, q, FEW if n_rows > 1000 else METHODS, what="short %dx%d" % (n_rows, n_cols))
    R, N, last = SHORT[weighted][(n_rows, n_cols, nbs, n_q, st)]
    assert hit["family"] == "short" and hit["rows_per_wg"] == R and hit["triples" if weighted else "pairs"] == N, hit
    assert n_rows - (-(-n_rows // R) - 1) * R == last and hit["groups"] == -(-n_q // Q_GROUP)
    assert R * int(np.prod(nbs)) < 100_000


# ---------------------------------------------------------------------------------------------------------------------
# 4. numpy's index arithmetic on small counts
# ---------------------------------------------------------------------------------------------------------------------
SMALL_BINS = 64
SMALL_EDGES = np.arange(SMALL_BINS + 1.0)


def small_count_data(n_cols, seed, n_used=SMALL_BINS):
    """one row over 64 unit bins: bin b < n_used holds exactly b + 1 distinct values (and some NaN values, not counted); the
    other columns are out-of-range samples"""
    rng = np.random.default_rng(seed)
    n = n_used * (n_used + 1) // 2
    assert n <= n_cols
    x = np.concatenate([b + rng.uniform(0.05, 0.95, b + 1) for b in range(n_used)])
    v = rng.permutation(np.round(np.linspace(-300.0, 300.0, n) + rng.uniform(-0.1, 0.1, n), 3))
    assert len(np.unique(v)) == n
    pad = n_cols - n
    xp = np.where(rng.random(pad) < 0.5, -1.0 - rng.random(pad), SMALL_BINS + 1.0 + rng.random(pad))
    vp = rng.standard_normal(pad)
    k = min(pad, 40)  # NaN values inside the bins: dropped before the count
    xp[:k] = rng.integers(0, n_used, k) + 0.5
    vp[:k] = np.nan
    p = rng.permutation(n_cols)
    return np.concatenate([x, xp])[p][None, :], np.concatenate([v, vp])[p][None, :]


def _with_neighbours(q):
    q = np.asarray(q, F64)
    q = np.concatenate([q, np.nextafter(q, -1.0), np.nextafter(q, 2.0)])
    return np.unique(q[(q >= 0.0) & (q <= 1.0)])


def index_q():
    """q at which (n - 1) q lands on or one ulp beside a whole number or a half, n = 2..65, and the usual ones"""
    base = [0.0, 1.0, 0.5, 1.0 / 3.0, 2.0 / 3.0, 0.1, 0.7, np.nextafter(1.0, 0.0), np.nextafter(0.0, 1.0), 1e-300]
    whole, half = [], []
    for n in range(2, SMALL_BINS + 2):
        for k in (1, (n - 1) // 2, n - 2):
            whole.append(k / (n - 1))
            half.append((k + 0.5) / (n - 1))
    return np.unique(np.concatenate([base, _with_neighbours(whole), _with_neighbours(half)]))


def weighted_step_q(x, v, w):
    """every cdf step C_j / W of every bin as numpy forms it (the cumulative sum of the weights in value order, divided by its
    last element), and the float64 neighbours of each"""
    steps = []
    keep = ~np.isnan(v[0]) & (x[0] >= 0) & (x[0] < SMALL_BINS)
    b = np.floor(x[0][keep]).astype(int)
    for k in range(SMALL_BINS):
        vb, wb = v[0][keep][b == k], w[0][keep][b == k].astype(F64)
        if vb.size:
            cdf = np.cumsum(wb[np.argsort(vb, kind="stable")])
            steps.append(cdf / cdf[-1])
    return _with_neighbours(np.concatenate(steps))


def small_weights(x, v, seed):
    """integer weights 0..7, at least one positive in every bin"""
    w = weights_for(v.shape, F64, seed)
    inside = ~np.isnan(v[0]) & (x[0] >= 0) & (x[0] < SMALL_BINS)
    for k in range(SMALL_BINS):
        i = np.flatnonzero(inside & (np.floor(x[0]) == k))
        if i.size and not (w[0][i] > 0).any():
            w[0][i[0]] = 3.0
    return w


@pytest.mark.parametrize("n_cols,family", [(2080, "short"), (4200, "radix")])
@pytest.mark.parametrize("method", METHODS)
def test_index_arithmetic_on_small_counts(xh, method, n_cols, family):
    x, v = small_count_data(n_cols, 900 + n_cols)
    dev = ([_dev(x)], _dev(v), None)
    q = index_q()
    for i in range(0, len(q), 64):
        hit = check_case(xh, False, [SMALL_EDGES], [x], v, None, q[i:i + 64], (method,), dev=dev, bits=True, what="small counts")
        assert hit["family"] == family


STEP_CASES = [(2048, "short", 63), (4200, "radix", 64)]


@pytest.mark.parametrize("n_cols,family,n_used", STEP_CASES)
def test_weighted_cdf_steps_on_small_counts(xh, n_cols, family, n_used):
    """(a short row holds 2048 values: bins 0..62 of the 64 take 2016 of them)"""
    x, v = small_count_data(n_cols, 950 + n_cols, n_used)
    w = small_weights(x, v, 950 + n_cols)
    dev = ([_dev(x)], _dev(v), _dev(w))
    q = weighted_step_q(x, v, w)
    for i in range(0, len(q), 64):
        hit = check_case(xh, True, [SMALL_EDGES], [x], v, w, q[i:i + 64], None, dev=dev, what="cdf steps")
        assert hit["family"] == family


# ---------------------------------------------------------------------------------------------------------------------
# what the sweep reached
# ---------------------------------------------------------------------------------------------------------------------
def n_cases():
    """the cases the tests above record when all of them run"""
    small = 2 * len(METHODS) * -(-len(index_q()) // 64)
    steps = 0
    for n_cols, _, n_used in STEP_CASES:
        x, v = small_count_data(n_cols, 950 + n_cols, n_used)
        steps += -(-len(weighted_step_q(x, v, small_weights(x, v, 950 + n_cols))) // 64)
    return len(RADIX) + len(LAYOUT_CASES) + len(SHORT_CASES) + small + steps


def test_zz_variants_reached():
    """every variant of the table reached by some case of this module (a partial run checks only what it ran)"""
    if len(HITS) < n_cases():
        pytest.skip("only part of the module ran (%d of %d cases)" % (len(HITS), n_cases()))
    for weighted in (False, True):
        hs = [h for wt, h, _ in HITS if wt == weighted and h["family"] == "radix"]
        assert any(h["groups"] > 1 and 0 < n_q - (h["groups"] - 1) * h["group"] < h["group"]
                   for wt, h, n_q in HITS if wt == weighted and h["family"] == "radix"), weighted  # a last group below G
        assert {tier_of(h) for h in hs} == {0, 1, 2}, weighted
        assert {h["d"] for h in hs} == set(range(1, 9)), weighted
        assert any(h["group"] > 1 and h["groups"] > 1 for h in hs), weighted  # G < n_q
        assert any(h["chunks"] > 1 and h["groups"] > 1 for h in hs), weighted
        short = [h for wt, h, _ in HITS if wt == weighted and h["family"] == "short"]
        assert {h["rows_per_wg"] for h in short} >= {1, 2, 3, SHORT_COLS[weighted]}, weighted
        assert {h["groups"] for h in short} >= {1, 2, 3}, weighted
    un = [h for wt, h, _ in HITS if not wt and h["family"] == "radix"]
    assert {homes_of(h) for h in un} >= {("lds", "lds", "lds"), ("lds", "lds", "global"), ("lds", "global", "global"),
                                         ("global", "global", "global")}
