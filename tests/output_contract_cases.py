"""The cases of tests/test_gpu_output_contract.py: what xhist_plan_execute, xhist_plan_execute_two_weights and xhist_bincount_rows
write, and where, in every histogram home — plain numpy, importable without torch or a GPU (tests/test_output_contract_cpu.py
holds every claim made here).

A case is the inputs of one call (samples, edges, weights, plan parameters, layout), the oracle's histogram H of them and a prefill
P of the destination.  The GPU module bins each case three times: as the census does (torch.empty output), with accumulate=0 into a
block of sentinels (every element written, nothing around it), and with accumulate=1 into the block uploaded as P (the block must
then hold P + H, exactly).

The float families take one case per (home, sample dtype, weight dtype, inputs) of the census with its "k1" edges ("lin" where the
census has no "k1" case), and a "lin" twin where one input of "k1" edges cannot reach the home (float_lin_twins).

Counts.  P[r, b] = 2^33 + 0xFFFFFFFF - (b % 3) + (r << 36): the low word sits one to three counts below a carry — a 32-bit add,
or a store of the call's own counts, shows at once — and the high word differs per row.

Weights are exactly summable throughout (tests/exact_weights.py: multiples of 2^-25 in [0.5, 1), float32 ones multiples of 2^-24;
the int32 weights of the mixed family are 1 ... 4), of both signs wherever the home takes them; the homes that route packed records
(float64 weights of ONE sign) get one sign for two inputs and both signs — the packed attempt discarded, the exact passes redoing
the call — for one and three.  P = +-m * 2^-25 with 1 <= m < 2^50, drawn per bin from the case's name: never a zero.  With fewer
than 2^27 samples in a bin every partial sum of P and the weights is a multiple of 2^-25 below 2^28: 53 bits, exact in any order,
so P + H is compared bit for bit.

The sentinel is 0x5A5A5A5A5A5A5A5A (tests/test_gpu_dense_front.py): not 0, not a NaN, and no expected element of any case."""
import zlib

import numpy as np

import exact_weights as ew
from census_inputs import (F32, F64, HOMES, _MIN_NB, _ST, _WT, _cases, edges_of, generic_integer_domains_inputs, int64_domain_inputs,
                           mixed_dtypes_inputs, samples_for, small_samples_inputs, two_weights_inputs)
from oracle import oracle_np as onp

SENTINEL = 0x5A5A5A5A5A5A5A5A
UNIT_LOG2 = -25  # every weight, prefill and sum is an integer number of 2^-25
STS, WTS, DS = ("f64", "f32"), ("none", "f32", "f64"), (1, 2, 3)

# float64 weights travel as packed records here unless both signs turn up
PACKED_HOMES = ("route", "route_rows", "route_rows_spl4", "route_spl4")


def count_prefill(n_rows, n_bins):
    b = np.arange(n_bins, dtype=np.int64)
    r = np.arange(n_rows, dtype=np.int64)[:, None]
    return (1 << 33) + 0xFFFFFFFF - (b % 3) + (r << 36)


def weighted_prefill_units(seed, n_rows, n_bins):
    """+-m, 1 <= m < 2^50, as int64 numbers of 2^-25"""
    rng = np.random.default_rng(seed)
    m = rng.integers(1, 1 << 50, (n_rows, n_bins), dtype=np.int64)
    return np.where(rng.integers(0, 2, m.shape).astype(bool), -m, m)


def from_units(units):
    """int64 numbers of 2^-25 (below 2^53 in magnitude: exact) as float64"""
    assert np.abs(units).max(initial=0) < (1 << 53)
    return np.ldexp(units.astype(F64), UNIT_LOG2)


class Case:
    """one call.  `samples` are [n_rows, n_cols] arrays as the call takes them (`lead`: handed over with the rows as the contiguous
    direction), `oracle_samples` as the oracle takes them (the float families compare in float64); `w2`: the second weight array of
    a two-weights call; `expect`: what the describe() line of the call must contain"""

    def __init__(self, name, family, home, samples, edges, w=None, params=None, lead=False, w2=None, oracle_samples=None, expect=()):
        self.name, self.family, self.home = name, family, home
        self.samples, self.edges, self.w, self.w2 = samples, [np.asarray(e) for e in edges], w, w2
        self.oracle_samples = samples if oracle_samples is None else oracle_samples
        self.params, self.lead, self.expect = dict(params or {}), lead, tuple(expect)
        self.n_rows, self.n_cols = samples[0].shape
        self.n_bins = int(np.prod([len(e) - 1 for e in self.edges], dtype=np.int64))
        self.weighted = w is not None
        self.seed = zlib.crc32(name.encode())
        self._want = {}

    def __repr__(self):
        return "Case(%s)" % self.name

    def weights(self):
        return [w for w in (self.w, self.w2) if w is not None]

    def want(self, k=0):
        """the oracle's [n_rows, n_bins] histogram of the case (of its k-th weight array): int64 counts or float64 sums"""
        if k not in self._want:
            w = None if not self.weighted else np.asarray(self.weights()[k]).astype(F64)
            self._want[k] = onp.bincount_rows(self.oracle_samples, self.edges, w).reshape(self.n_rows, self.n_bins)
        return self._want[k]

    def prefill_units(self, k=0):
        assert self.weighted
        return weighted_prefill_units(self.seed + k, self.n_rows, self.n_bins)

    def prefill(self, k=0):
        return from_units(self.prefill_units(k)) if self.weighted else count_prefill(self.n_rows, self.n_bins)

    def flat_index(self):
        """[n_rows, n_cols] flat bin index of every sample, -1 where the oracle drops it (oracle_np's digitize and joint index)"""
        codes = [onp.digitize_inclusive(s, e) for s, e in zip(self.oracle_samples, self.edges)]
        flat = np.zeros(codes[0].shape, np.int64)
        keep = np.ones(codes[0].shape, bool)
        for c, e in zip(codes, self.edges):
            keep &= (c >= 1) & (c <= len(e) - 1)
            flat = flat * (len(e) - 1) + np.clip(c - 1, 0, len(e) - 2)
        return np.where(keep, flat, -1)


# ---------------------------------------------------------------------------------------------------------------------
# the float families: one case per (home, st, wt, D) of the census
# ---------------------------------------------------------------------------------------------------------------------
def signs_of(home, wt, D):
    return "one" if home in PACKED_HOMES and wt == "f64" and D == 2 else "both"


def float_case_specs(st, wt, D):
    """(census index, census case) per home: edge kind "k1", or "lin" where _MIN_NB or only_kinds rules "k1" out, and the home's
    own parameters (no digitize-form override)"""
    picked = {}
    for i, case in enumerate(_cases(_ST[st], _WT[wt], D)):
        home = case["home"]
        if case["params"] != HOMES[home]["params"] or case["kind"] not in ("k1", "lin"):
            continue
        if home not in picked or case["kind"] == "k1":
            picked[home] = (i, case)
    return [picked[h] for h in HOMES if h in picked]


LIN_TWIN_BINS = 12_000


def float_lin_twins(st, wt, D):
    """one input and 12 000 bins or more (the d1_* ladder, packed16, sliced, global_big and the partitioned homes): that many "k1"
    edges crowd the buckets of the plan's grid, the vector kernels have no table for them and the call ends in the generic
    family behind memory-side atomics, whatever the home's parameters ask for.  Only np.linspace edges (the arithmetic digitize)
    reach these homes with one input — so each of them gets a "lin" twin next to its "k1" case: (census index, census case)"""
    if D != 1:
        return []
    primary = {c["home"]: c["kind"] for _, c in float_case_specs(st, wt, D)}
    return [(i, c) for i, c in enumerate(_cases(_ST[st], _WT[wt], D))
            if c["kind"] == "lin" and primary[c["home"]] == "k1" and c["params"] == HOMES[c["home"]]["params"] and c["nbs"][0] >= LIN_TWIN_BINS]


def float_case(st, wt, D, i, case, twin=False):
    """the census's own shapes, edges and samples (seed 1000 D + 17 i, as test_dispatch_surface_float_samples draws them)"""
    seed = 1000 * D + 17 * i
    edges = [edges_of(case["kind"], nb, seed=seed + d) for d, nb in enumerate(case["nbs"])]
    n_rows, n_cols = case["shape"]
    xs = samples_for(edges, n_rows, n_cols, _ST[st], seed)
    w = None
    if _WT[wt] is not None:
        w = ew.make(_WT[wt], signs=signs_of(case["home"], wt, D))(np.random.default_rng(seed + 99), (n_rows, n_cols))
    return Case("%s|%s|%d|%s%s" % (st, wt, D, case["home"], "|lin" if twin else ""), "float", case["home"], xs, edges, w, case["params"],
                case["lead"], oracle_samples=[x.astype(F64) for x in xs])


def float_cases(st, wt, D):
    for i, case in float_case_specs(st, wt, D):
        yield float_case(st, wt, D, i, case)
    for i, case in float_lin_twins(st, wt, D):
        yield float_case(st, wt, D, i, case, twin=True)


# ---------------------------------------------------------------------------------------------------------------------
# the special families: one small case per family, home and number of inputs, from the census's generators
# ---------------------------------------------------------------------------------------------------------------------
_BOTH = ew.make(F64, signs="both")
SMALL_DTYPES = ("int32", "int64", "int16", "uint8", "float16")
_SMALL_PICK = {("lds", False), ("global", True), ("lanes_lead", True), ("lanes_lead_long", False)}


def _special(family, tag, c, **more):
    return Case("%s|%s|%s|%s|%s" % (family, tag, c["home"], c["kind"], "w" if c["weighted"] else "n"), family, c["home"], c["samples"], c["edges"],
                c["w"], c["params"], c["lead"], **more)


def small_sample_cases(dtype):
    for c in small_samples_inputs(dtype, _BOTH):
        if c["kind"] != "k1":
            break  # ("k1" comes first)
        if (c["home"], c["weighted"]) in _SMALL_PICK:
            yield _special("small", dtype, c)


def int64_domain_cases():
    for c in int64_domain_inputs(_BOTH):
        yield _special("int64", "1", c)


_GENERIC_PICK = {("int64_int64", "lds", False), ("float_int64", "global", False), ("big_int64_float", "lds", False),
                 ("int64_int64", "global", True), ("int64_float", "lds", True), ("big_int64", "lds", True), ("big_float", "lds", True)}


def generic_integer_cases():
    for c in generic_integer_domains_inputs(_BOTH):
        if (c["kind"], c["home"], c["weighted"]) in _GENERIC_PICK:
            yield _special("generic", str(len(c["samples"])), c)


def mixed_dtype_cases(D):
    """edge kind "k1": the pickers' own choice with int32 and with float64 weights, memory-side atomics with float64 weights, the
    generic family behind memory-side atomics without weights (with float64 weights for one input)"""
    want = [({}, np.int32), ({}, np.float64), ({"force_global": 1}, np.float64),
            ({"force_generic": 1, "force_global": 1}, None if D > 1 else np.float64)]
    for c in mixed_dtypes_inputs(D, _BOTH):
        if c["kind"] == "k2":
            break  # ("lin", then "k1")
        if c["kind"] == "k1" and (c["params"], c["wkind"]) in want:
            tag = "%d,%s,%s" % (D, "+".join(sorted(c["params"])) or "auto", np.dtype(c["wkind"]).name if c["wkind"] else "none")
            yield _special("mixed", tag, c)


def two_weight_cases(st, wt, D):
    for c in two_weights_inputs(st, wt, D, ew.make(_WT[wt], signs="both")):
        if c["kind"] == "k1" and not c["params"]:
            yield Case("two|%s|%s|%d" % (st, wt, D), "two", "lds", c["samples"], c["edges"], c["w"], {}, False, w2=c["w2"],
                       oracle_samples=[x.astype(F64) for x in c["samples"]])


def table_column_cases():
    """an (n, K) table histogrammed over its leading axis with more bins than the row-per-lane kernels hold (execute_table_columns:
    the columns are gathered into dense rows): the smallest shape of test_table_columns_with_many_bins_are_gathered_into_rows, with
    the smaller of its bin counts that the row-per-lane kernels refuse — 3000 float64 sums, but 150 000 counts (3000 uint16
    counters of four rows still fit their LDS)"""
    rng = np.random.default_rng(41)
    n, K = 30_011, 4
    t = rng.standard_normal((n, K)).astype(F32)
    t[7, 1] = np.nan
    x = np.ascontiguousarray(t.T)
    for weighted in (False, True):
        e = np.linspace(-4, 4, (3000 if weighted else 150_000) + 1)
        w = ew.f64(rng, (K, n), "both") if weighted else None
        yield Case("table|f32|%d|%s" % (K, "w" if weighted else "n"), "table", "table_columns", [x], [e], w, {}, True,
                   oracle_samples=[x.astype(F64)], expect=("family=fast",))


C5_EDGES = [np.linspace(-4, 4, 1025), np.linspace(-4, 4, 1025)]
EXCHANGE_N = (4097, 1_000_003)
# tag -> (signs, plan parameters, what the describe() line must say)
EXCHANGE_KINDS = {
    "packed8_one_sign": ("one", {"partition": 1, "exchange": 1, "records48": 0}, ("exchange=forced", "exchange_records=packed8")),
    "exact12_both_signs": ("both", {"partition": 1, "exchange": 1, "records48": -1}, ("exchange=forced", "exchange_records=exact12")),
    # the packed attempt is discarded inside the call, its exact passes finish it
    "packed8_both_signs": ("both", {"partition": 1, "exchange": 1, "records48": 0}, ("exchange=forced", "exchange_records=packed8")),
    # no time for the mode at all: the classic passes queued behind take the call
    "no_budget": ("one", {"partition": 1, "exchange": 1, "records48": 0, "exchange_budget_ms": -1}, ("route=fused",)),
    # the same both-signs-with-packing call on the classic routing home
    "classic_both_signs": ("both", {"partition": 1, "exchange": -1, "records48": 0}, ("exchange=no", "records=packed48")),
}


def exchange_cases(n):
    """C5's edges (1024 x 1024 bins, float64 weights), the exchange mode forced"""
    rng = np.random.default_rng(900 + n % 97)
    x, y = rng.standard_normal((1, n)), rng.standard_normal((1, n))
    for tag, (signs, params, expect) in EXCHANGE_KINDS.items():
        yield Case("exchange|%d|%s" % (n, tag), "exchange", "exchange", [x, y], C5_EDGES, ew.f64(rng, (1, n), signs), params, expect=expect)


def host_route_cases():
    """one counting and one float64-weighted case each of lds, global, lanes and route (its "lin" twin: the one that reaches the
    partitioned passes with one input), for the calls on host memory"""
    for wt in ("none", "f64"):
        for i, case in float_case_specs("f64", wt, 1):
            if case["home"] in ("lds", "global", "lanes"):
                yield float_case("f64", wt, 1, i, case)
        for i, case in float_lin_twins("f64", wt, 1):
            if case["home"] == "route":
                yield float_case("f64", wt, 1, i, case, twin=True)


HOST_ROUTE_LINES = {"lds": "hist=lds ", "global": "hist=global ", "lanes": "family=lanes ", "route": "hist=partitioned "}


def all_cases():
    """every case of the table, one at a time (they are built when asked for)"""
    for st in STS:
        for wt in WTS:
            for D in DS:
                yield from float_cases(st, wt, D)
    for dtype in SMALL_DTYPES:
        yield from small_sample_cases(dtype)
    yield from int64_domain_cases()
    yield from generic_integer_cases()
    for D in DS:
        yield from mixed_dtype_cases(D)
    for st in STS:
        for wt in ("f32", "f64"):
            for D in DS:
                yield from two_weight_cases(st, wt, D)
    yield from table_column_cases()
    for n in EXCHANGE_N:
        yield from exchange_cases(n)


# The cases whose every bin receives a sample: few bins under many samples per row, as the census shapes them (a home's smallest
# shape fixes both).  Every other case leaves at least one bin of its block empty: leg (b) must have written a zero there.
NO_EMPTY_BIN = frozenset("""
    f64|none|1|lds f64|none|1|lds_many_copies f64|none|1|global f64|none|1|lanes_long f64|none|1|lanes_lead
    f64|none|1|lanes_lead_long f64|none|2|lds f64|none|2|lds_many_copies f64|none|2|global f64|none|2|lanes_long
    f64|none|2|lanes_lead_long f64|none|3|lds_many_copies f64|none|3|lanes_long f64|none|3|lanes_lead_long f64|f32|1|lds
    f64|f32|1|lds_many_copies f64|f32|1|global f64|f32|1|lanes_lead f64|f32|2|lds f64|f32|2|lds_many_copies
    f64|f32|2|global f64|f32|3|lds_many_copies f64|f64|1|lds f64|f64|1|lds_many_copies f64|f64|1|global
    f64|f64|1|lanes_lead f64|f64|2|lds f64|f64|2|lds_many_copies f64|f64|2|global f64|f64|3|lds_many_copies
    f32|none|1|lds f32|none|1|lds_many_copies f32|none|1|global f32|none|1|lanes_long f32|none|1|lanes_lead
    f32|none|1|lanes_lead_long f32|none|1|long_rows_f32 f32|none|2|lds f32|none|2|lds_many_copies f32|none|2|global
    f32|none|2|lanes_long f32|none|2|lanes_lead_long f32|none|3|lds_many_copies f32|none|3|lanes_long f32|none|3|lanes_lead_long
    f32|f32|1|lds f32|f32|1|lds_many_copies f32|f32|1|global f32|f32|1|lanes_lead f32|f32|2|lds
    f32|f32|2|lds_many_copies f32|f32|2|global f32|f32|3|lds_many_copies f32|f64|1|lds f32|f64|1|lds_many_copies
    f32|f64|1|global f32|f64|1|lanes_lead f32|f64|2|lds f32|f64|2|lds_many_copies f32|f64|2|global
    f32|f64|3|lds_many_copies
    small|int32|lds|k1|n small|int32|global|k1|w small|int32|lanes_lead|k1|w small|int32|lanes_lead_long|k1|n
    small|int64|lds|k1|n small|int64|global|k1|w small|int64|lanes_lead|k1|w small|int64|lanes_lead_long|k1|n
    small|int16|lds|k1|n small|int16|global|k1|w small|int16|lanes_lead|k1|w small|int16|lanes_lead_long|k1|n
    small|uint8|lds|k1|n small|uint8|global|k1|w small|uint8|lanes_lead|k1|w small|uint8|lanes_lead_long|k1|n
    small|float16|lds|k1|n small|float16|global|k1|w small|float16|lanes_lead|k1|w small|float16|lanes_lead_long|k1|n
    int64|1|lds|int64|n int64|1|lds|int64|w
    mixed|1,auto,int32|lds|k1|w mixed|1,auto,float64|lds|k1|w mixed|1,force_global,float64|global|k1|w
    mixed|1,force_generic+force_global,float64|global|k1|w mixed|2,auto,int32|lds|k1|w mixed|2,auto,float64|lds|k1|w
    mixed|2,force_global,float64|global|k1|w mixed|2,force_generic+force_global,none|global|k1|n
    two|f64|f32|1 two|f64|f32|2 two|f64|f32|3 two|f64|f64|1 two|f64|f64|2 two|f64|f64|3
    two|f32|f32|1 two|f32|f32|2 two|f32|f32|3 two|f32|f64|1 two|f32|f64|2 two|f32|f64|3
""".split())
