"""What tests/test_gpu_sum_order_properties.py runs on histogram_sum and bin_order, in plain numpy: which drawn cases of
tests/values_cases.py are replayed and with what values, what the two entry points must give on them, the values whose sums
tell integer limbs from float atomics, and the periodic data, table and closed form of the row-batch test.  No GPU and no test
functions here: tests/test_sum_order_cases_cpu.py holds every claim made below to the oracles (tests/sum_oracle.py,
tests/bin_order_oracle.py, tests/map_oracle.py), as tests/map_cases.py is held by tests/test_map_cpu.py.

Nothing here touches tests/values_cases.py's stream of choices: the cases are replayed as they are drawn, and whatever is drawn
in addition comes from a generator of its own (the case's seed plus VALUE_SEED)."""
import functools

import numpy as np

import bin_order_oracle as bo
import extrema_oracle as eo
import map_cases as mc
import map_oracle as mo
import sum_oracle as so
import values_cases as vc

F64, F32 = np.float64, np.float32

# ---------------------------------------------------------------------------------------------------------------------
# (a), (b) the replayed cases
# ---------------------------------------------------------------------------------------------------------------------
# histogram_sum replays "extrema" as drawn (+-inf, +-0.0, int64 near 2^62, float16, bool: the definition's clause 6 and the
# float64 conversion) and "mean_var" with its values replaced: grid values sum exactly in any order, so they cannot tell
# integer limbs from float atomics.  bin_order replays the samples of "argextrema" (whose positions it defines itself by) and
# of "quantile".
SUM_STATS = ("extrema", "mean_var")
REPLACED = ("mean_var",)
ORDER_STATS = ("argextrema", "quantile")
VALUE_SEED = 52_361  # (added to the case's seed: the generator of the replacement values, the case's own stream untouched)
EXPONENTS = {"float64": 20, "float32": 20, "float16": 6}  # magnitudes over 2^+-this: what float16 holds without overflow


def full_mantissa(rng, shape, dt=F64):
    """values of the kind test_gpu_sum.mixed_values makes: normal deviates times 2^-k .. 2^k, so both signs and full
    mantissas whose float sum depends on the order; in an array of 8 elements or more one element in a hundred (at least
    one) is NaN, and up to six more are the smallest subnormal, -0.0, +inf, +0.0, -inf, +inf (one per 8 elements: a small
    array keeps finite totals)"""
    dt = np.dtype(dt)
    k = EXPONENTS[dt.name]
    v = (rng.standard_normal(shape) * np.exp2(rng.integers(-k, k + 1, shape))).astype(dt)
    flat = v.reshape(-1)
    n = flat.size
    if n >= 8:
        at = rng.permutation(n)
        flat[at[: max(1, n // 100)]] = np.nan
        specials = [np.finfo(dt).smallest_subnormal, -0.0, np.inf, 0.0, -np.inf, np.inf][: min(6, n // 8)]
        flat[at[n - len(specials):]] = specials
    return v


def value_dtype(case):
    """the dtype of the replacement values: the case's own where it is a float type, float64 otherwise"""
    dt = np.dtype(case["values"][0].split(":")[1])
    return dt if dt.kind == "f" else np.dtype(F64)


def replacement(case):
    """(allocation, view) of the case's replacement values, laid out by the case's own values layout"""
    lay = case["layouts"][len(case["sample_dtypes"])]
    rng = np.random.default_rng(case["seed"] + VALUE_SEED)
    return vc.lay_out(full_mantissa(rng, vc._drawn_shape(case["shape"], lay), value_dtype(case)), lay, case["shape"])


def build_sum(case):
    """values_cases.build's arrays of a SUM_STATS case, the values replaced where the statistic is in REPLACED"""
    b = vc.build(case)
    if case["stat"] not in REPLACED:
        return b
    bufs, views, host = list(b.bufs), list(b.views), list(b.host)
    bufs[b.d], views[b.d] = replacement(case)
    host[b.d] = np.ascontiguousarray(np.broadcast_to(views[b.d], case["shape"]))
    return vc.Built(case, b.edges, bufs, views, host)


def sum_call(built, arrays):
    """(sample arrays, keyword arguments) of histogram_sum on `arrays` (Built.inputs() or host): the case's per-call
    parameters are its statistic's, not histogram_sum's"""
    d = built.d
    return list(arrays[:d]), dict(values=arrays[d], bins=built.edges if d > 1 else built.edges[0], axis=built.case["axis"])


def sum_want(samples, values, edges, axis):
    """(count, total) of the oracle on contiguous host arrays, in the compare domain (integer samples on float edges as
    float64: map_oracle.compare_domain is test_gpu_sum._cmp_domain, the CPU file holds the two to each other)"""
    xs, es = mo.compare_domain(samples, edges)
    return so.histogram_sum(*xs, values=values, bins=es, axis=axis)


def n_bins_of(edges):
    return int(np.prod([len(e) - 1 for e in edges], dtype=np.int64))


def order_want(samples, edges, axis):
    """(order, offsets, the bin indices as rows [kept axes..., c]) of the oracle on contiguous host samples"""
    rows = bo.rows_of(mo.index(samples, edges), axis)
    order, offsets = bo.order_offsets(rows, n_bins_of(edges))
    return order, offsets, rows


def argmax_through_order(order, offsets, v_row):
    """one row: per bin the position of the first maximum of the values found through `order`, -1 where the bin holds no
    value.  The positions of a bin ascend along its segment, so the first maximum of the segment is the smallest position
    that holds it; NaN values are skipped and the order is the total one (-0.0 < +0.0), as histogram_argextrema states both."""
    v = np.asarray(v_row).astype(F64)
    out = np.full(len(offsets) - 1, -1, np.int64)
    for b in range(len(out)):
        seg = order[offsets[b]:offsets[b + 1]]
        ok = ~np.isnan(v[seg])
        if ok.any():
            out[b] = seg[ok][int(np.argmax(eo.key(v[seg][ok])))]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# (e) more rows than one launch of the value passes: rows are grouped views of small periodic arrays
# ---------------------------------------------------------------------------------------------------------------------
ROWS_COLS, ROWS_BINS, P_S, P_V, ROWS_EXTRA = mc.ROWS_COLS, mc.ROWS_BINS, mc.P_S, mc.P_V, mc.ROWS_EXTRA
ROW_FAMILIES = ("fast", "generic")
ROW_BLOCK = {"fast": 256, "generic": 512}
# per values dtype: mantissa bits, the exponent of value row 0, and how far below its row's exponent a value may lie.  The
# exponent steps by 50 from one value row to the next (p % 5), more than the largest of the shifts: two neighbouring rows
# never share a unit.  With the shifts a bin's smaller values reach down into limb 0 and its largest fills limb 2.
ROW_VALUES = {"fast": (F64, 53, -100, (0, 13, 27)), "generic": (F32, 24, -80, (0, 20, 45))}
ROW_EXP_STEP = 50


def rows_data(family):
    """(edges, samples [P_S, 3], values [P_V, 3]) of a row-batch case.  fast: float64 samples and float64 values; generic:
    int64 samples on int64 edges (compare domain 1) and float32 values.  About a third of the samples lie outside the edges,
    some on one, float ones are NaN now and then.  A value is +-m * 2^(50 (p mod 5) + e0 - shift) / 2^(bits - 1) with m an odd
    integer of all `bits` mantissa bits, p its row: a unit taken from another row's keys truncates set bits or shifts them out
    of place.  Twenty values are NaN."""
    rng = np.random.default_rng(1300 + ROW_FAMILIES.index(family))
    if family == "generic":
        edges = [np.array([0, 5, 10], np.int64)]
        xs = rng.integers(-3, 14, (P_S, ROWS_COLS)).astype(np.int64)
        xs.reshape(-1)[:3] = [0, 5, 10]
    else:
        edges = [np.array([0.0, 0.5, 1.0])]
        xs = rng.uniform(-0.25, 1.25, (P_S, ROWS_COLS))
        flat = xs.reshape(-1)
        flat[:5] = [0.0, 0.5, 1.0, -0.0, np.nan]
        flat[rng.integers(5, flat.size, 40)] = np.nan
    vdt, bits, e0, shifts = ROW_VALUES[family]
    p = np.arange(P_V)[:, None]
    m = rng.integers(1 << (bits - 1), 1 << bits, (P_V, ROWS_COLS)) | 1
    e = ROW_EXP_STEP * (p % 5) + e0 - (bits - 1) - rng.choice(np.array(shifts), (P_V, ROWS_COLS))
    wide = np.ldexp(m.astype(F64), e) * rng.choice(np.array([-1.0, 1.0]), (P_V, ROWS_COLS))
    vs = wide.astype(vdt)
    assert np.array_equal(vs.astype(F64), wide) and np.isfinite(vs).all() and (np.abs(vs) >= np.finfo(vdt).tiny).all()
    vs.reshape(-1)[rng.choice(vs.size, 20, replace=False)] = np.nan
    return edges, xs, vs


@functools.lru_cache(maxsize=None)
def rows_table(family):
    """(count, total), each [P_S * P_V, 2]: sum_oracle.sum_rows on every distinct row there is, samples row i with values row
    j at i * P_V + j (the periods are coprime: every pair occurs)"""
    edges, xs, vs = rows_data(family)
    i, j = np.divmod(np.arange(P_S * P_V), P_V)
    return so.sum_rows([xs[i]], edges, vs[j].astype(F64))


def rows_index(rows):
    """where row r's results stand in rows_table: r reads samples row r mod P_S and values row r mod P_V (integer arrays of
    numpy or tensors of torch)"""
    return (rows % P_S) * P_V + rows % P_V


def total_with_keys(values, key_values):
    """one bin's total when pass 2 takes the unit from the keys of `key_values` (another bin's values) and the finalize from the
    bin's own, by the definition of tests/sum_oracle.py: the quanta are formed in units of 2^U', summed, and read as units of
    2^U.  Finite values only.  (A left shift the definition does not know, beyond 43, wraps in the kernel's 64-bit words and
    does not here: the claim held with this is that the total CHANGES, not what it becomes.)"""
    v = np.asarray(values, F64).reshape(-1)
    v = v[~np.isnan(v)]
    k = np.asarray(key_values, F64).reshape(-1)
    k = k[~np.isnan(k)]
    assert np.isfinite(v).all() and np.isfinite(k).all()
    if v.size == 0 or not np.any(v):
        return 0.0
    own = so.unit_exponent(float(np.max(np.abs(v))))
    other = so.unit_exponent(float(np.max(np.abs(k)))) if k.size and np.any(k) else so.UNIT_MIN
    s = 0
    for x in v.tolist():
        neg, q = so.quantum(x, other)
        s += -q if neg else q
    return so.round_scaled(s, own)


def rows_bins(family, rows):
    """the values of every bin of the given rows: a list per row of ROWS_BINS float64 arrays (NaN values left in)"""
    edges, xs, vs = rows_data(family)
    out = []
    for r in np.asarray(rows).tolist():
        b = mo.index([xs[r % P_S]], edges)
        v = vs[r % P_V].astype(F64)
        out.append([v[b == k] for k in range(ROWS_BINS)])
    return out
