"""The inputs of the dispatch-surface census (tests/test_gpu_census.py), in plain numpy: the edges that decide the digitize form,
the samples, the table of histogram homes, the product of the float families and the inputs of the special families.

Nothing here touches a GPU or torch, so the case tables built on it (tests/output_contract_cases.py, tests/extreme_cases.py) can be
held to their conditions on any machine.  The generators draw from their random generators in exactly the order the census's
bodies always did: what a census case selects does not depend on who asks for its inputs."""
import numpy as np

F64, F32 = np.float64, np.float32


# ---------------------------------------------------------------------------------------------------------------------
# edges that decide the digitize form
# ---------------------------------------------------------------------------------------------------------------------
def _grid_buckets(n_edges):
    """buckets of the plan's fine (uint16) table over [e0, eL]: xhist_plan.hip.h build (K = 2 * min(4096, max(8, pow2(4 E))))"""
    k = 8
    while k < min(4 * n_edges, 1 << 20):
        k *= 2
    return 2 * min(4096, max(8, k))


def edges_of(kind, nb, lo=-4.0, hi=4.0, seed=0):
    """nb bins on [lo, hi] whose edges put 1 / 2 / 3 / 4 / many edges into some bucket of the plan's grid ("k1" ... "k4",
    "crowd"), np.linspace edges ("lin": the arithmetic forms), or geometric ones ("geom": the float-bits grid)"""
    rng = np.random.default_rng(seed)
    if kind == "lin":
        return np.linspace(lo, hi, nb + 1)
    if kind == "geom":  # (four decades on the positive axis, whatever lo / hi say: a linear grid cannot separate these)
        return np.geomspace(1e-2, 1e2, nb + 1)
    per = {"k1": 1, "k2": 2, "k3": 3, "k4": 4, "crowd": 7}[kind]
    extra = per - 1
    base_n = nb + 1 - extra
    assert base_n >= 3, (kind, nb)
    base = np.linspace(lo, hi, base_n)
    # not arithmetic: every interior edge moved by a small fraction of the bin width (still one per bucket)
    width = (hi - lo) / (base_n - 1)
    base[1:-1] += rng.uniform(-0.2, 0.2, base_n - 2) * min(width, (hi - lo) / _grid_buckets(nb + 1))
    if extra:  # `per` edges inside ONE bucket of the grid: between 1/4 and 3/4 of the bucket that holds the middle edge
        j = base_n // 2
        bw = (hi - lo) / _grid_buckets(nb + 1)
        b0 = lo + (np.floor((base[j] - lo) / bw) + 0.25) * bw
        cluster = b0 + (bw / (2.0 * per)) * np.arange(per)
        base = np.sort(np.concatenate([np.delete(base, j), cluster]))
        base = base[np.concatenate([[True], np.diff(base) > 0])]
        while len(base) < nb + 1:  # (a neighbour fell into the cluster's bucket and was merged: put an edge back further out)
            gaps = np.diff(base)
            g = int(np.argmax(gaps))
            base = np.insert(base, g + 1, 0.5 * (base[g] + base[g + 1]))
        base = base[: nb + 1] if len(base) > nb + 1 else base
        base[0], base[-1] = lo, hi
    assert len(base) == nb + 1 and np.all(np.diff(base) > 0)
    return base


def samples_for(edges_list, n_rows, n_cols, dtype, seed):
    """[n_rows, n_cols] per input: normal samples spread over the range, then samples ON edges (the right edge included),
    on their float neighbours, outside the range, NaN and +-inf"""
    rng = np.random.default_rng(seed)
    out = []
    for d, e in enumerate(edges_list):
        lo, hi = e[0], e[-1]
        x = rng.uniform(lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo), (n_rows, n_cols))
        flat = x.reshape(-1)
        k = flat.size
        idx = rng.permutation(k)
        on = idx[: k // 16]
        flat[on] = e[rng.integers(0, len(e), on.size)]
        nxt = idx[k // 16: k // 12]
        flat[nxt] = np.nextafter(e[rng.integers(0, len(e), nxt.size)], np.inf if d % 2 else -np.inf)
        flat[idx[k // 12: k // 12 + max(1, k // 200)]] = np.nan
        flat[idx[-3:]] = [np.inf, -np.inf, hi]
        out.append(x.astype(dtype))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
def _split_bins(total, D):
    """D bin counts whose product is about `total` (distinct, so a transposed index would show)"""
    if D == 1:
        return [total]
    if D == 2:
        a = max(2, int(round(total ** 0.5 * 1.25)))
        return [a, max(2, total // a)]
    a = max(2, int(round(total ** (1 / 3) * 1.3)))
    b = max(2, int(round(total ** (1 / 3))))
    return [a, b, max(2, total // (a * b))]


KINDS = ("lin", "k1", "k2", "k3", "k4", "crowd", "geom")
_MIN_NB = {"lin": 2, "k1": 3, "k2": 4, "k3": 5, "k4": 6, "crowd": 9, "geom": 4}

# home -> total bins per number of inputs for a (float64-weighted, counting) histogram, [rows, cols], plan parameters
# (sizes: the smallest that reach the home; partitioned homes need n_cols >= 4 with "partition" = 1)
_BIG_W, _BIG_U = {1: 40_000, 2: 40_000, 3: 40_000}, {1: 90_000, 2: 90_000, 3: 90_000}
_LDS = {1: 96, 2: 400, 3: 2_000}
_LANE = {1: 40, 2: 110, 3: 220}
HOMES = {
    "lds": dict(bins=(_LDS, _LDS), shape=(3, 20_011), params={}),
    "lds_many_copies": dict(bins=({1: 24, 2: 30, 3: 60}, {1: 24, 2: 30, 3: 60}), shape=(1, 50_003), params={}),
    "packed16": dict(bins=(None, {1: 50_000, 2: 50_000, 3: 50_000}), shape=(2, 30_011), params={}),  # unweighted only: uint16 counters two per word
    "global": dict(bins=(_LDS, _LDS), shape=(2, 10_007), params={"force_global": 1}),
    "global_big": dict(bins=({1: 60_000, 2: 60_000, 3: 60_000}, {1: 120_000, 2: 120_000, 3: 120_000}), shape=(1, 20_011), params={"partition": -1, "slices": -1}),
    "sliced": dict(bins=(_BIG_W, _BIG_U), shape=(2, 20_011), params={"slices": 1}),
    "route": dict(bins=(_BIG_W, _BIG_U), shape=(1, 40_013), params={"partition": 1}),
    "route_rows": dict(bins=(_BIG_W, _BIG_U), shape=(3, 20_011), params={"partition": 1}),
    "route_rows_spl4": dict(bins=(_BIG_W, _BIG_U), shape=(3, 20_011), params={"partition": 1, "route_spl": 4}),
    "route_spl4": dict(bins=(_BIG_W, _BIG_U), shape=(1, 40_013), params={"partition": 1, "route_spl": 4}),
    "route_exact": dict(bins=(_BIG_W, None), shape=(1, 40_013), params={"partition": 1, "records48": -1}),  # float64 weights as full records
    "three_pass": dict(bins=(_BIG_W, _BIG_U), shape=(1, 40_013), params={"partition": 1, "fused": -1}),
    "lanes": dict(bins=(_LANE, _LANE), shape=(3_001, 37), params={"lanes": 1}),
    "lanes_wide": dict(bins=({1: 600, 2: 600, 3: 700}, {1: 600, 2: 600, 3: 700}), shape=(2_003, 53), params={"lanes": 1}),
    "lanes_long": dict(bins=(None, _LANE), shape=(40, 66_001), params={"lanes": 1}),  # rows beyond 65535 samples: packed uint16 counters, the columns cut into segments of at most 65535
    "flat_rows": dict(bins=({1: 50, 2: 90, 3: 90}, {1: 50, 2: 90, 3: 90}), shape=(5_003, 181), params={"flat_rows": 1}),
    # reductions over a LEADING axis: the rows are the contiguous direction (row stride 1) and the row-per-lane kernels take the
    # view as it lies; beyond 65535 samples per row the counts stay packed uint16, in column segments of at most 65535 samples each
    "lanes_lead": dict(bins=(_LANE, _LANE), shape=(301, 1_009), params={}, lead=True),
    "lanes_lead_long": dict(bins=(None, _LANE), shape=(48, 66_001), params={}, lead=True),
    # BASELINE C4's shape class (>= 64 rows of >= 2^19 float32 samples, counts): tiles twice as long
    "long_rows_f32": dict(bins=(None, {1: 50}), shape=(64, 1 << 19), params={}, only_st=F32, only_kinds=("lin", "k1", "k2")),
}
# one input: where the edges of a histogram near the LDS capacity still fit it decides between LDS copies, packed uint16
# counters, bin slices and the partitioned passes — a ladder of bin counts around those borders
for _nb in (12_000, 14_000, 16_000, 17_000, 20_000, 24_000, 30_000, 36_000):
    for _tag, _pp in (("", {}), ("_part", {"partition": 1}), ("_3pass", {"partition": 1, "fused": -1}), ("_sliced", {"slices": 1})):
        HOMES["d1_%d%s" % (_nb, _tag)] = dict(bins=({1: _nb}, {1: _nb}), shape=(1, 30_011), params=_pp)
FORM_PARAMS = {  # digitize-form overrides tried for every (kind, home): {} = the pickers' own choice
    "lin": ({}, {"arith": 1}, {"arith": -1}, {"arith32": 1}, {"arith": -1, "pack": 1}),
    "k1": ({}, {"pack": 1}),
    "k2": ({}, {"pack": -1}, {"pack": 1}),
    "k3": ({}, {"pack": -1}, {"pack": 1}),
    "k4": ({}, {"pack": -1}, {"pack": 1}),
    "crowd": ({}, {"pack": -1}, {"pack": 1}),
    "geom": ({}, {"pack": -1}, {"pack": 1}),
}


def _cases(st, wt, D):
    weighted = wt is not None
    for home, h in HOMES.items():
        per_d = h["bins"][0 if weighted else 1]
        if per_d is None or D not in per_d:
            continue
        for kind in KINDS:
            nbs = _split_bins(per_d[D], D)
            if min(nbs) < _MIN_NB[kind]:
                continue
            if home.startswith("d1_") and kind == "geom":
                continue
            if h.get("only_st") is not None and st is not h["only_st"]:
                continue
            if h.get("only_kinds") is not None and kind not in h["only_kinds"]:
                continue
            for form in FORM_PARAMS[kind]:
                if "arith32" in form and st is not F32:
                    continue
                yield dict(home=home, kind=kind, nbs=nbs, shape=h["shape"], params=dict(h["params"], **form), lead=bool(h.get("lead")))


_ST = {"f64": F64, "f32": F32}
_WT = {"none": None, "f32": F32, "f64": F64}


def _key(st, wt, D, case):
    return "%s|%s|%d|%s|%s|%s" % (st, wt, D, case["home"], case["kind"], ",".join("%s=%d" % kv for kv in sorted(case["params"].items())))


def _uniform(lo, hi):
    return lambda rng, shape: rng.uniform(lo, hi, shape)


# ---------------------------------------------------------------------------------------------------------------------
# the other kernel families: small integer / half samples, the exact int64 domain, dtype mixtures, two weights, generic.
# Each generator takes an optional weights factory (rng, shape) -> weights: None draws full-mantissa weights; an exactly summable
# one (tests/exact_weights.py) makes every weighted result bitwise.  A yielded case is a dict of `samples`, `edges`, `w` (None:
# counts), `params`, `weighted`, `lead` and what names it (`home`, `kind`).
# ---------------------------------------------------------------------------------------------------------------------
def small_samples_inputs(dtype, make_w=None):
    rng = np.random.default_rng(7)
    dt = np.dtype(dtype)
    for kind in ("k1", "crowd", "lin"):
        for home, shape, params in (("lds", (3, 20_011), {}), ("global", (2, 10_007), {"force_global": 1}), ("lanes_lead", (301, 1_009), {}),
                                    ("lanes_lead_long", (48, 66_001), {})):
            for weighted in (False, True):
                nb = 60
                e = edges_of(kind, nb, lo=0.0 if dt.kind == "u" else -100.0, hi=200.0 if dt.kind == "u" else 100.0, seed=3)
                if dt.kind in "iu":
                    x = rng.integers(-20 if dt.kind == "u" else -120, 220 if dt.kind == "u" else 120, shape).clip(np.iinfo(dt).min, np.iinfo(dt).max).astype(dt)
                else:
                    x = rng.uniform(-110, 110, shape).astype(dt)
                    x.reshape(-1)[::97] = np.nan
                w = (make_w or _uniform(0.5, 1.5))(rng, shape) if weighted else None
                yield dict(home=home, kind=kind, samples=[x], edges=[e], w=w, params=params, weighted=weighted, lead=home.startswith("lanes_lead"))


def int64_domain_inputs(make_w=None):
    rng = np.random.default_rng(8)
    for home, shape, params in (("lds", (3, 20_011), {}), ("global", (2, 10_007), {"force_global": 1})):
        for weighted in (False, True):
            base = (1 << 60)
            e = base + np.sort(rng.choice(100_000, 65, replace=False)).astype(np.int64)
            x = base + rng.integers(-1000, 101_000, shape).astype(np.int64)
            w = (make_w or _uniform(0.5, 1.5))(rng, shape) if weighted else None
            yield dict(home=home, kind="int64", samples=[x], edges=[e], w=w, params=params, weighted=weighted, lead=False)


def generic_integer_domains_inputs(make_w=None):
    rng = np.random.default_rng(10)
    base = 1 << 58
    shape = (3, 20_011)
    ei = base + np.sort(rng.choice(50_000, 41, replace=False)).astype(np.int64)
    ej = base + np.sort(rng.choice(50_000, 33, replace=False)).astype(np.int64)
    ef = edges_of("k2", 24, lo=-3.0, hi=3.0, seed=1)
    xi = base + rng.integers(-500, 50_500, shape).astype(np.int64)
    xj = base + rng.integers(-500, 50_500, shape).astype(np.int64)
    xf = rng.uniform(-3.3, 3.3, shape)
    big = base + np.sort(rng.choice(4_000_000, 30_001, replace=False)).astype(np.int64)  # 30001 int64 edges: 240 KB, beyond LDS
    xb = base + rng.integers(-5_000, 4_005_000, shape).astype(np.int64)
    bigf = np.sort(rng.uniform(-3, 3, 30_001))

    def case(kind, samples, edges, w, params, weighted):
        return dict(home="global" if params.get("force_global") else "lds", kind=kind, samples=samples, edges=edges, w=w, params=params,
                    weighted=weighted, lead=False)

    for weighted in (False, True):
        w = (make_w or _uniform(0.5, 1.5))(rng, shape) if weighted else None
        for params in ({}, {"force_global": 1}):
            yield case("int64_int64", [xi, xj], [ei, ej], w, params, weighted)       # int64 domain, two inputs
            yield case("int64_float", [xi, xf], [ei, ef], w, params, weighted)       # per-input domains
            yield case("float_int64", [xf, xj], [ef, ej], w, params, weighted)
        yield case("big_int64", [xb], [big], w, {}, weighted)                        # tables that do not fit LDS: int64 domain
        yield case("big_int64_float", [xb, xf], [big, ef], w, {}, weighted)          # ... per-input domains
        yield case("big_float", [xf * 1.0], [bigf], w, {"force_generic": 1}, weighted)  # ... float64 domain


def mixed_dtypes_inputs(D, make_w=None):
    rng = np.random.default_rng(9 + D)
    dts = [np.float32, np.int32, np.float64][:D] if D > 1 else [np.float32]
    for kind in ("lin", "k1", "k2", "k3", "crowd"):
        for params in ({}, {"arith": -1}, {"arith": 1}, {"force_generic": 1}, {"force_global": 1}, {"force_generic": 1, "force_global": 1}):
            for wkind in (None, np.int32, np.float64):
                nbs = _split_bins({1: 96, 2: 400, 3: 2_000}[D], D)
                if min(nbs) < _MIN_NB[kind]:
                    continue
                edges = [edges_of(kind, nb, lo=-50.0, hi=50.0, seed=d) for d, nb in enumerate(nbs)]
                shape = (3, 20_011)
                xs = []
                for d in range(D):
                    v = rng.uniform(-55, 55, shape)
                    xs.append(np.rint(v).astype(dts[d]) if np.dtype(dts[d]).kind == "i" else v.astype(dts[d]))
                w = None if wkind is None else (rng.integers(1, 5, shape).astype(wkind) if np.dtype(wkind).kind == "i" else (make_w or _uniform(0.5, 2))(rng, shape))
                if D == 1 and wkind is None:
                    continue  # (homogeneous: the float product above)
                yield dict(home="global" if params.get("force_global") else "lds", kind=kind, samples=xs, edges=edges, w=w, params=params,
                           weighted=w is not None, lead=False, wkind=wkind)


def two_weights_inputs(st, wt, D, make_w=None):
    """the pair of weight arrays as `w` and `w2`"""
    rng = np.random.default_rng(11 * D)
    for kind in ("lin", "k1", "k2"):
        nbs = _split_bins({1: 96, 2: 400, 3: 900}[D], D)
        edges = [edges_of(kind, nb, seed=d) for d, nb in enumerate(nbs)]
        shape = (2, 20_011)
        xs = samples_for(edges, shape[0], shape[1], _ST[st], 5)
        wa, wb = ((make_w or _uniform(0.5, 2.0))(rng, shape).astype(_WT[wt]) for _ in range(2))
        for params in ({}, {"arith": -1}):
            yield dict(home="lds", kind=kind, samples=xs, edges=edges, w=wa, w2=wb, params=params, weighted=True, lead=False)
