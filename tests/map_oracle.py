"""The per-sample maps on the CPU: what bin_index, histogram_lookup and histogram_anomaly must give, restated on
oracle.oracle_np.digitize_inclusive / joint_index, and the host's choice of kernel family and table home (xhist_map.hip's use of
choose_values / values_geometry), restated from the plan's table sizes as tests/test_gpu_values_census.py restates the
statistics'.

Every expected result here is exact.  The index is integer work.  The lookup copies table elements.  The anomaly is one float64
subtraction (and one division) per sample of numbers the caller hands in, so it is IEEE's result bit for bit; `anomaly` computes
the means itself only for values on the exactly summable grid of tests/values_exact.py, where fl(S / n) does not depend on the
order of the additions."""
import numpy as np

from oracle import oracle_np as onp

LDS_MAX = 160 * 1024
OPS = ("index", "take", "anomaly")


# ---------------------------------------------------------------------------------------------------------------------
# results
# ---------------------------------------------------------------------------------------------------------------------
def compare_domain(samples, edges):
    """per input, the arrays numpy compares: int64 views of datetimes, float64 if either side is a float, else the integers"""
    cs, ce = [], []
    for s, e in zip(samples, edges):
        s, e = np.asarray(s), np.asarray(e)
        if s.dtype.kind == "M":
            s, e = s.view(np.int64), e.astype(s.dtype).view(np.int64)
        elif s.dtype.kind == "f" or e.dtype.kind == "f":
            s, e = s.astype(np.float64), e.astype(np.float64)
        cs.append(s)
        ce.append(e)
    return cs, ce


def per_input_bins(samples, edges):
    """(counted, [bin of every sample per input]) in the broadcast shape; a bin is meaningless where its input drops the sample"""
    cs, ce = compare_domain(samples, edges)
    cs = np.broadcast_arrays(*cs)
    ok = np.ones(cs[0].shape, bool)
    bins = []
    for s, e in zip(cs, ce):
        code = onp.digitize_inclusive(s, e)  # 0: below, 1 .. E-1: bins, E: above or NaN
        ok &= (code >= 1) & (code <= len(e) - 1)
        bins.append(code - 1)
    return ok, bins


def index(samples, edges):
    """bin_index: int64 in the broadcast sample shape, the C-order flat index over the bin axes, -1 where histogram drops the sample"""
    ok, bins = per_input_bins(samples, edges)
    nbs = [len(e) - 1 for e in edges]
    # joint_index is a Horner recurrence over axes of length n + 1: handed n - 1 it ravels over the nb_d real bins
    flat = onp.joint_index([np.where(ok, b, 0) for b in bins], [n - 1 for n in nbs])
    return np.where(ok, flat, -1).astype(np.int64)


def _rows(a, axis, ndim):
    """[kept (C order), reduced (ascending axis number)] arrangement of an array in the sample shape, and how to undo it"""
    red = list(range(ndim)) if axis is None else sorted(int(x) % ndim for x in np.atleast_1d(axis))
    kept = [i for i in range(ndim) if i not in red]
    moved = np.transpose(a, kept + red)
    m = int(np.prod([a.shape[i] for i in kept], dtype=np.int64))
    c = int(np.prod([a.shape[i] for i in red], dtype=np.int64))  # (said outright: numpy infers no extent of an array without elements)
    return moved.reshape(m, c), moved.shape, np.argsort(kept + red)


def lookup(samples, edges, table, axis=None):
    """histogram_lookup: float64 in the sample shape, table[kept index, bin], NaN where the sample is not counted"""
    idx = index(samples, edges)
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    i2, shape, back = _rows(idx, axis, idx.ndim)
    t2 = np.asarray(table).astype(np.float64).reshape(i2.shape[0], n_bins)
    out = np.full(i2.shape, np.nan)
    r, c = np.nonzero(i2 >= 0)
    out[r, c] = t2[r, i2[r, c]]
    return np.transpose(out.reshape(shape), back)


def exact_mean(samples, edges, values, axis=None, weights=None):
    """the per-bin mean of values on the exactly summable grid, fl(S / n) or fl(sum(w v) / W): [rows, n_bins], NaN where n
    (W) is 0.  Weights must be small integers, so that every w v and every partial sum is exact."""
    import values_exact as vx

    idx = index(samples, edges)
    v = np.broadcast_to(np.asarray(values).astype(np.float64), idx.shape)
    assert vx.on_grid(v)
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    i2, _, _ = _rows(idx, axis, idx.ndim)
    v2, _, _ = _rows(v, axis, idx.ndim)
    take = (i2 >= 0) & ~np.isnan(v2)
    flat = (i2 + np.arange(i2.shape[0], dtype=np.int64)[:, None] * n_bins)[take]
    if weights is None:
        w = np.ones(flat.shape)
    else:
        w2, _, _ = _rows(np.broadcast_to(np.asarray(weights).astype(np.float64), idx.shape), axis, idx.ndim)
        w = w2[take]
        assert np.all(w == np.round(w)) and np.all(np.abs(w) < 256)
    s = np.zeros(i2.shape[0] * n_bins)
    x = np.zeros(i2.shape[0] * n_bins)
    np.add.at(s, flat, w * v2[take])  # (exact in any order)
    np.add.at(x, flat, w)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(x != 0, s / x, np.nan)
    return mean.reshape(i2.shape[0], n_bins)


def anomaly(samples, edges, values, mean, scale=None, axis=None):
    """histogram_anomaly from given tables: float64(v) - mean[bin], divided by scale[bin] where given; NaN where not counted"""
    shape = np.broadcast_shapes(*[np.shape(s) for s in samples], np.shape(values))
    v = np.broadcast_to(np.asarray(values).astype(np.float64), shape)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        out = v - lookup(samples, edges, mean, axis)
        if scale is not None:
            out = out / lookup(samples, edges, scale, axis)
    return out


def variance_star(samples, edges, values, axis=None, ddof=0, weights=None):
    """(var*, b), each [rows, n_bins]: what histogram_mean_var's variance must be and how far the kernels' may lie from it,
    from the project's own bounds.  Unweighted: values_exact.expected followed by var_bound; weighted:
    meanvar_weighted_oracle's exact mode, m2_bound and var_bound (what tests/test_gpu_meanvar_weighted.check_exact applies).
    b == 0 where the variance is bit for bit (the power-of-two counts of values_exact.m2_exact, the power-of-two sums of
    weights of the weighted oracle); both NaN where the variance is (no value in the bin, n <= ddof)."""
    import meanvar_weighted_oracle as mwo
    import values_exact as vx

    idx = index(samples, edges)
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    i2, _, _ = _rows(idx, axis, idx.ndim)
    m = i2.shape[0]
    if idx.size == 0:
        return np.full((m, n_bins), np.nan), np.full((m, n_bins), np.nan)
    v2, _, _ = _rows(np.broadcast_to(np.asarray(values).astype(np.float64), idx.shape), axis, idx.ndim)
    if weights is None:
        take = i2 >= 0
        flat = (i2 + np.arange(m, dtype=np.int64)[:, None] * n_bins)[take]
        cnt, _, m2, bound, pow2 = vx.expected(flat, v2[take], m * n_bins)
        var, b = vx.var_bound(cnt, m2, bound, ddof)
    else:
        xl = [_rows(np.broadcast_to(np.asarray(s), idx.shape), axis, idx.ndim)[0] for s in samples]
        w2, _, _ = _rows(np.broadcast_to(np.asarray(weights).astype(np.float64), idx.shape), axis, idx.ndim)
        wsum, mean, m2 = mwo.mean_var_w_rows(xl, edges, v2, w2, exact=True)
        var, b, pow2 = mwo.var_bound(wsum, m2, mwo.m2_bound(xl, edges, v2, w2, mean), ddof)
    b = np.where(np.isnan(var), np.nan, np.where(pow2.reshape(var.shape), 0.0, b))
    return var.reshape(m, n_bins), b.reshape(m, n_bins)


def standardized_bracket(a, var, b):
    """where (float64(v) - mean[bin]) / sqrt(var[bin]) may lie, per sample: `a` the anomaly (exact bits), `var` and `b` the
    sample's bin's var* and bound (NaN where the sample is not counted or the variance is NaN).
      must_nan  a or var is NaN: the result is NaN
      exact     b == 0: the result is `want` = fl(a / fl(sqrt(var*))), IEEE's bit for bit (0 / 0 included: NaN)
      elsewhere the closed interval [lo, hi] spanned by fl(a / s_lo) and fl(a / s_hi), s_lo = sqrt(max(0, var* - b)) one ulp
                down and s_hi = sqrt(var* + b) one ulp up; with s_lo == 0 the interval is open towards +-inf on a's side,
                and NaN (0 / 0) is allowed for a == 0 alone (`nan_ok`)"""
    a, var, b = (np.asarray(x, np.float64) for x in (a, var, b))
    must_nan = np.isnan(a) | np.isnan(var)
    exact = ~must_nan & (b == 0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        want = a / np.sqrt(var)
        s_hi = np.nextafter(np.sqrt(var + b), np.inf)
        s_lo = np.sqrt(np.maximum(var - b, 0.0))
        s_lo = np.where(s_lo > 0, np.nextafter(s_lo, 0.0), 0.0)
        e_hi, e_lo = a / s_hi, a / s_lo
    open_ = ~must_nan & ~exact & (s_lo == 0)
    zero = np.zeros_like(a)
    lo = np.where(open_, np.where(a > 0, e_hi, np.where(a < 0, -np.inf, zero)), np.fmin(e_lo, e_hi))
    hi = np.where(open_, np.where(a > 0, np.inf, np.where(a < 0, e_hi, zero)), np.fmax(e_lo, e_hi))
    return dict(must_nan=must_nan, exact=exact, want=want, lo=lo, hi=hi, nan_ok=open_ & (a == 0))


def assert_standardized(got, a, var, b, what=""):
    """the standardized anomaly held to standardized_bracket -> (samples held bit for bit, samples held to the interval)"""
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == np.shape(a), (what, got.dtype, got.shape, np.shape(a))
    k = standardized_bracket(a, var, b)
    gn = np.isnan(got)
    assert gn[k["must_nan"]].all(), "%s: a number where the sample, the value or the bin's variance gives NaN" % what
    ex = k["exact"]
    assert_bits(got[ex], k["want"][ex], what + " (bit for bit)")
    rest = ~k["must_nan"] & ~ex
    bad = rest & gn & ~k["nan_ok"]
    assert not bad.any(), "%s: NaN at %d samples whose bin has a variance" % (what, bad.sum())
    inside = rest & ~gn
    bad = inside & ~((k["lo"] <= got) & (got <= k["hi"]))
    assert not bad.any(), "%s: %d samples outside the bracket, first at %s: %r not in [%r, %r]" % (
        what, bad.sum(), np.argwhere(bad)[0], got[bad][0], k["lo"][bad][0], k["hi"][bad][0])
    return int(ex.sum()), int(inside.sum())


def assert_bits(got, want, what=""):
    """bit for bit: the same shape and dtype, NaN in the same places, and every other element the same 8 bytes (so -0.0 is not
    +0.0).  A NaN is held to its place only: IEEE leaves sign and payload of an operation's NaN result open."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind == "f":
        gn, wn = np.isnan(got), np.isnan(want)
        assert np.array_equal(gn, wn), "%s: NaN at %d places, expected at %d" % (what, gn.sum(), wn.sum())
        got, want = np.where(gn, 0.0, got).view(np.int64), np.where(wn, 0.0, want).view(np.int64)
    bad = got != want
    assert not bad.any(), "%s: %d of %d elements differ, first at %s: %r != %r" % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0], np.asarray(got)[bad][0], np.asarray(want)[bad][0])


# ---------------------------------------------------------------------------------------------------------------------
# the host's choice, restated (xhist_map.hip; the table sizes as tests/test_gpu_values_census.py states them)
# ---------------------------------------------------------------------------------------------------------------------
def _lut_k(n_edges, lut16):
    """buckets of a dimension's grid (xhist_plan.hip.h build_domain): 2-byte entries get twice as many"""
    if n_edges > 65535:
        return 0
    k = 8
    while k < min(4 * n_edges, 1 << 20):
        k *= 2
    k = min(4096, max(8, k))
    return 2 * k if lut16 else k


def table_bytes(edges, which):
    """LDS bytes of a plan's table set: "native" (float64 / int64 edges, 4-byte bucket entries), "fine64" (float64 edges, 2-byte
    entries), "fine32" (float32 thresholds, 2-byte entries); every edge array carries 4 sentinels.  The statement of
    tests/test_gpu_values_census.py, kept here so that this module needs no GPU test module (tests/test_map_cpu.py holds the
    two to each other where that one can be imported)."""
    ns = [len(e) for e in edges]
    eo_ = sum((n + 5) // 2 for n in ns) if which == "fine32" else sum(n + 4 for n in ns)
    per = 2 if which == "native" else 4
    off = per * eo_ + sum(_lut_k(n, which != "native") for n in ns)
    return ((off + per - 1) // per + 1) // 2 * 16


def last(fn):
    """the largest n >= 2 up to which fn(n) holds"""
    n = 2
    while fn(n + 1):
        n += 1
    return n


def slot_bytes(op, scale=False):
    """what a bin keeps in LDS: its centre, and its scale where one is given; bin_index keeps nothing"""
    return 0 if op == "index" else 16 if scale else 8


def predict(op, cus, edges, cmp, sdt, vdt, n_rows, n_cols, scale=False, fine=True, arith=False, layout_fast=True):
    """the describe() fields of a map call: op, family, table (home), scan, cmp, segs, block, lds_bytes, tables_in_lds, scale, D.
    vdt: the values' dtype (anomaly; None otherwise).  fine / arith / layout_fast as test_gpu_values_census.predict takes them."""
    D = len(edges)
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    f32 = np.dtype(sdt) == np.float32
    slot = slot_bytes(op, scale)
    out = dict(op=op, D=D, cmp=cmp, scan=0, scale=int(bool(scale)))
    fast_ok = (cmp == 0 and D <= 2 and np.dtype(sdt) in (np.dtype(np.float64), np.dtype(np.float32))
               and (vdt is None or np.dtype(vdt) == np.dtype(sdt)) and n_bins < (1 << 24) and layout_fast)
    lds = None
    if fast_ok:
        tb_fine = table_bytes(edges, "fine32" if f32 else "fine64")
        if fine and tb_fine + n_bins * slot <= LDS_MAX:
            lds, out["scan"] = tb_fine + n_bins * slot, "fine" if fine is True else fine
        elif arith and n_bins * slot <= LDS_MAX:
            lds, out["scan"] = n_bins * slot, 5
        if lds is not None:
            out.update(family="fast", table="none" if op == "index" else "lds", tables_in_lds=1)
    if lds is None:
        tb = table_bytes(edges, "native")
        til = tb + 1024 <= LDS_MAX
        in_lds = til and n_bins < (1 << 24) and tb + n_bins * slot <= LDS_MAX
        out.update(family="generic", table="none" if op == "index" else "lds" if in_lds else "global", tables_in_lds=int(til))
        lds = (tb if til else 0) + (n_bins * slot if in_lds else 0)
    fast = out["family"] == "fast"
    block = 256 if fast else 512
    vec = 4 if f32 else 2
    per_tile = block * (4 * vec if D == 1 else 8) if fast else block
    bpc = 2048 // block
    if lds:
        bpc = max(1, min(bpc, 160 * 1024 // lds))
    tiles = -(-n_cols // per_tile)
    segs = max(1, min(tiles, -(-cus * bpc // n_rows)))
    segs = max(segs, -(-(tiles * per_tile) // (1 << 31)))
    out.update(block=block, segs=segs, lds_bytes=lds)
    return out


def parse(desc):
    """describe() of a map call -> the fields `predict` gives"""
    import re

    assert desc.startswith("map "), desc
    kv = dict(re.findall(r"(\w+)=(\S+)", desc))
    return dict(op=kv["op"], family=kv["family"], table=kv["table"], scan=int(kv["scan"]), cmp=int(kv["cmp"]), segs=int(kv["segs"]),
                block=int(kv["block"]), lds_bytes=int(kv["lds_bytes"]), tables_in_lds=int(kv["tables_in_lds"]), scale=int(kv["scale"]),
                D=int(kv["D"]))


def assert_variant(desc, want):
    """the call landed on the kernel family, table home and geometry the restatement predicts ("fine": SCAN 1 or 2)"""
    got = parse(desc)
    w = dict(want)
    if w["scan"] == "fine":
        assert got["scan"] in (1, 2), (desc, want)
        w["scan"] = got["scan"]
    assert got == w, "landed elsewhere:\n  got  %s\n  want %s\n  (%s)" % (got, w, desc)
    return got


def tile_of(sdt, D):
    """samples per tile of the fast family: 256 lanes x VEC x UNROLL"""
    vec = 16 // np.dtype(sdt).itemsize
    return 256 * vec * (4 if D == 1 else 8 // vec)
