"""What tests/test_gpu_sorted_properties.py runs on the six calls built on the sorted order (bin_sort, bin_rank, histogram_mode,
bin_unique, bin_weighted_unique, histogram_weighted_mode), in plain numpy: which drawn cases of tests/values_cases.py each call
replays and with what per-call parameters, what the calls must give on host arrays (the five oracles, put into the public shapes),
what a drawn case holds (`census`), the data and the scratch requests of the dirty-scratch and thread tests, and the closed form
of a row of more than 256 tiles.  No GPU and no test functions here: tests/test_sorted_cases_cpu.py holds every claim made below
to the oracles (tests/bin_sort_oracle.py, bin_rank_oracle.py, mode_oracle.py, bin_unique_oracle.py, weighted_unique_oracle.py).

Nothing here touches tests/values_cases.py's stream of choices: the cases are replayed as they are drawn, and a per-call parameter
is a function of the case's seed alone."""
import math

import numpy as np

import bin_order_oracle as bo
import bin_rank_cases as rc
import bin_rank_oracle as ro
import bin_sort_oracle as so
import bin_unique_oracle as uo
import exact_weights as xw
import map_oracle as mo
import mode_oracle as mdo
import values_cases as vc
import weighted_unique_oracle as wo

F64, F32 = np.float64, np.float32
WORD, TILE_WORDS, TILE = wo.WORD, wo.TILE_WORDS, wo.TILE

# ---------------------------------------------------------------------------------------------------------------------
# (a), (b) the replayed cases: which statistic's draws a call takes, and the call's own parameters from the case's seed
# ---------------------------------------------------------------------------------------------------------------------
# bin_sort and bin_rank order anything: "argextrema" draws +-inf, +-0.0, int64 near 2^62 (ties only as float64), float16 and bool
# next to the grid values, "quantile" the grid values.  The two tallies take "argextrema" and "mean_var"; the weighted twins the
# two draws with weights, whose integer weights 0..7 sum exactly in any order.
DRAWS = {"bin_sort": ("argextrema", "quantile"), "bin_rank": ("argextrema", "quantile"),
         "histogram_mode": ("argextrema", "mean_var"), "bin_unique": ("argextrema", "mean_var"),
         "bin_weighted_unique": ("mean_var_w", "quantile_w"), "histogram_weighted_mode": ("mean_var_w", "quantile_w")}
CALLS = tuple(DRAWS)
PAIRS = [(call, stat) for call in CALLS for stat in DRAWS[call]]
ALL_DRAWS = ("argextrema", "quantile", "mean_var", "mean_var_w", "quantile_w")
# what the refusal of a cut reduced axis calls the partials of each call (core._check_one_chunk's message)
NOUNS = {"bin_sort": "sorted orders", "bin_rank": "ranks", "histogram_mode": "modes", "bin_unique": "distinct values",
         "bin_weighted_unique": "distinct values", "histogram_weighted_mode": "modes"}


# Directed cases on top of the 60 drawn ones of a statistic, as values_cases.case_of makes them of these numbers.  The drawn 60 of
# "quantile" and "quantile_w" hold a tie run inside a bin in 37 and 39 cases and "quantile_w" the same value in two bins of a row
# in 39 (the floor of each is 40), and "mean_var_w" rows longer than one word in 33 (35); every case below holds all five of the
# measures tests/test_sorted_cases_cpu.py puts a floor under, in at most 6000 samples.
DIRECTED_EXTRA = {"quantile": (1021, 1030, 1045, 1056, 1063), "mean_var_w": (1032, 1038, 1061, 1074), "quantile_w": (1021, 1024, 1038)}


def directed(stat):
    return [vc.case_of(stat, entropy) for entropy in DIRECTED_EXTRA.get(stat, ())]


def descending_of(case):
    return bool((case["seed"] >> 4) & 1)


def rank_mode_of(case):
    """(method, descending, pct): bin_rank_cases.MODES indexed by the case's seed"""
    return rc.MODES[case["seed"] % len(rc.MODES)]


def size_of(case, u_max, none=None):
    """bin_unique's `size` from the seed: None (`none`: what stands for it), 0, 1, U_max // 2, U_max, U_max + 3"""
    return (none, 0, 1, u_max // 2, u_max, u_max + 3)[case["seed"] % 6]


def inverse_of(case):
    return bool((case["seed"] // 6) & 1)


def n_bins_of(edges):
    return int(np.prod([len(e) - 1 for e in edges], dtype=np.int64))


def bins_shape(edges):
    return tuple(len(e) - 1 for e in edges)


def rows(host, d, edges, axis):
    """(the bin indices as rows [kept axes..., c], the arrays after the samples as such rows) of contiguous host arrays
    samples..., values[, weights] of one shape"""
    idx = mo.index(host[:d], edges)
    return bo.rows_of(idx, axis), [bo.rows_of(np.broadcast_to(h, idx.shape), axis) for h in host[d:]]


def moved_back(flat, shape, axis):
    """[kept axes..., c] of the oracles' rows -> the sample shape"""
    ndim = len(shape)
    red = list(range(ndim)) if axis is None else sorted(int(a) % ndim for a in np.atleast_1d(axis))
    kept = [i for i in range(ndim) if i not in red]
    full = np.asarray(flat).reshape([shape[i] for i in kept] + [shape[i] for i in red])
    return np.ascontiguousarray(np.moveaxis(full, range(len(kept), ndim), red)) if kept else full


def _flat(a, c):
    """[rows, c] of [kept axes..., c] (said outright: numpy infers no extent next to 0)"""
    return a.reshape(int(np.prod(a.shape[:-1], dtype=np.int64)), c)


def sort_want(host, d, edges, axis, descending=False):
    """(order [kept, c], offsets [kept, B + 1])"""
    idx, (v,) = rows(host[:d + 1], d, edges, axis)
    return so.order_offsets(idx, v, n_bins_of(edges), descending)


def rank_want(host, d, edges, axis, method, descending, pct):
    """rank, float64 in the sample shape"""
    idx, (v,) = rows(host[:d + 1], d, edges, axis)
    return moved_back(ro.rank_rows(idx, v, n_bins_of(edges), method, descending, pct), host[0].shape, axis)


def _binned(outs, lead, edges):
    return tuple(np.ascontiguousarray(o).reshape(lead + bins_shape(edges)) for o in outs)


def mode_want(host, d, edges, axis):
    """(count, nunique, mode, mode_count), each [kept, bins...]"""
    idx, (v,) = rows(host[:d + 1], d, edges, axis)
    return _binned(mdo.mode_rows(idx, v, n_bins_of(edges)), idx.shape[:-1], edges)


def unique_want(host, d, edges, axis, size=None):
    """(uniques [kept, W], counts [kept, W], offsets [kept, B + 1], inverse in the sample shape)"""
    idx, (v,) = rows(host[:d + 1], d, edges, axis)
    uniques, counts, offsets, inverse = uo.unique_rows(idx, v, n_bins_of(edges), size)
    return uniques, counts, offsets, moved_back(inverse, host[0].shape, axis)


def wunique_want(host, d, edges, axis, size=None):
    """(uniques, counts, weight_sums [kept, W], offsets [kept, B + 1], inverse in the sample shape)"""
    idx, (v, w) = rows(host, d, edges, axis)
    uniques, counts, sums, offsets, inverse = wo.wunique_rows(idx, v, w, n_bins_of(edges), size)
    return uniques, counts, sums, offsets, moved_back(inverse, host[0].shape, axis)


def wmode_want(host, d, edges, axis):
    """(count, nunique, mode, mode_weight), each [kept, bins...]"""
    idx, (v, w) = rows(host, d, edges, axis)
    return _binned(wo.wmode_rows(idx, v, w, n_bins_of(edges)), idx.shape[:-1], edges)


def u_max(offsets):
    """the largest row total of distinct (bin, value) pairs"""
    return int(offsets[..., -1].max()) if offsets.size else 0


def stable_by_value(order, offsets, v_rows):
    """bin_order's (order, offsets) -> bin_sort's ascending order: every segment, the dropped samples' included, sorted stably by
    the value key; all [kept, ...] rows"""
    out = np.empty_like(order)
    c = order.shape[-1]
    flat_o, flat_f, flat_v, flat_out = _flat(order, c), _flat(offsets, offsets.shape[-1]), _flat(v_rows, c), _flat(out, c)
    for r in range(flat_o.shape[0]):
        ends = np.concatenate([flat_f[r, 1:], [c]])
        for a, b in zip(flat_f[r], ends):
            seg = flat_o[r, a:b]
            flat_out[r, a:b] = seg[np.argsort(so.value_keys(flat_v[r][seg]), kind="stable")]
    return out


def census(built, axis):
    """what one drawn case holds, from the oracles alone: a dict of booleans and two sizes"""
    d = built.d
    idx, rest = rows(built.host, d, built.edges, axis)
    v = rest[0].astype(F64)
    n_bins = n_bins_of(built.edges)
    c = idx.shape[-1]
    flat_i, flat_v = _flat(idx, c), _flat(v, c)
    count, _, _, mode_count = mdo.mode_rows(idx, v, n_bins)
    two_bins = both_zeros = False
    for i, x in zip(flat_i, flat_v):
        if not two_bins:
            b, vals, _, _ = uo.runs_row(i, x, n_bins)
            two_bins = len(np.unique(vals)) < len(vals)  # (np.unique: -0.0 and +0.0 are one value)
        if not both_zeros:
            z = (x == 0) & (i >= 0)
            both_zeros = bool(np.intersect1d(i[z & np.signbit(x)], i[z & ~np.signbit(x)]).size)
        if two_bins and both_zeros:
            break
    return {"an extent of 0": 0 in built.case["shape"], "no counted sample": not (idx >= 0).any(),
            "a bin of two or more values": bool((count >= 2).any()), "a tie run inside a bin": bool((mode_count >= 2).any()),
            "a NaN in a counted bin": bool(((idx >= 0) & np.isnan(v)).any()), "the same value in two bins of a row": two_bins,
            "both zeros in one bin": both_zeros, "rows longer than 64": c > WORD and idx.size > 0, "row": c if idx.size else 0,
            "rows": flat_i.shape[0]}


# ---------------------------------------------------------------------------------------------------------------------
# (c), (e) the data of the dirty-scratch and thread tests, and the scratch a call asks the cache for
# ---------------------------------------------------------------------------------------------------------------------
# 3 rows of 70 001 samples in 127 bins: a row is 1094 words of 64 sorted positions, the last of them 49 wide (70 001 = 1093 * 64 +
# 49), and two tiles of 1024 words, the second of 70; no row but the first starts on a word of the flat arrays.
SCRATCH_ROWS, SCRATCH_COLS, SCRATCH_BINS = 3, 70_001, 127
SCRATCH_RUN, SCRATCH_RUN_BIN, SCRATCH_RUN_VALUE = 66_000, 63, 7.5
SCRATCH_EDGES = np.linspace(-4.0, 4.0, SCRATCH_BINS + 1)


def scratch_data(seed):
    """(x, v, w), each float64 [3, 70 001]: samples N(0, 1.5) with a few NaN and some outside the edges; values round(N(0, 1), 1)
    with 1 % NaN; per row 66 000 positions in bin 63 (of 127: about half of the others sort before it) that hold one value, 7.5,
    which no rounded deviate equals, so that run crosses the tile border at sorted position 65 536; weights exactly summable, of both
    signs"""
    rng = np.random.default_rng(seed)
    shape = (SCRATCH_ROWS, SCRATCH_COLS)
    x = rng.normal(0.0, 1.5, shape)
    x[rng.random(shape) < 0.002] = np.nan
    v = np.round(rng.standard_normal(shape), 1)
    v[rng.random(shape) < 0.01] = np.nan
    mid = 0.5 * (SCRATCH_EDGES[SCRATCH_RUN_BIN] + SCRATCH_EDGES[SCRATCH_RUN_BIN + 1])
    for r in range(SCRATCH_ROWS):
        at = rng.permutation(SCRATCH_COLS)[:SCRATCH_RUN]
        x[r, at] = mid
        v[r, at] = SCRATCH_RUN_VALUE
    return x, v, xw.f64(rng, shape, "both")


# the nine calls of (c), the eight of (e) among them: name -> (the public function, its keyword arguments, whether it reads weights)
SCRATCH_CUT = 40_000  # a size below the rows' distinct (bin, value) pairs: entries beyond it are stored nowhere
SCRATCH_CALLS = {
    "bin_sort": ("bin_sort", {}, False),
    "bin_rank": ("bin_rank", {}, False),
    "bin_rank_pct": ("bin_rank", dict(method="dense", pct=True), False),
    "histogram_mode": ("histogram_mode", {}, False),
    "bin_unique": ("bin_unique", {}, False),
    "bin_unique_inverse": ("bin_unique", dict(return_inverse=True), False),
    "bin_weighted_unique": ("bin_weighted_unique", {}, True),
    "bin_weighted_unique_cut": ("bin_weighted_unique", dict(size=SCRATCH_CUT), True),
    "histogram_weighted_mode": ("histogram_weighted_mode", {}, True),
}
THREAD_CALLS = ("bin_sort", "bin_rank", "bin_rank_pct", "histogram_mode", "bin_unique_inverse", "bin_weighted_unique",
                "histogram_weighted_mode", "bin_order")


def scratch_want(name, x, v, w):
    """the oracle's outputs of one of SCRATCH_CALLS on [R, C] host arrays over axis 1, in the public call's order"""
    fn, kw, weighted = SCRATCH_CALLS[name]
    host, edges = [x, v] + ([w] if weighted else []), [SCRATCH_EDGES]
    if fn == "bin_sort":
        return sort_want(host, 1, edges, 1)
    if fn == "bin_rank":
        return (rank_want(host, 1, edges, 1, kw.get("method", "average"), False, kw.get("pct", False)),)
    if fn == "histogram_mode":
        return mode_want(host, 1, edges, 1)
    if fn == "bin_unique":
        return unique_want(host, 1, edges, 1)[:4 if kw.get("return_inverse") else 3]
    if fn == "bin_weighted_unique":
        return wunique_want(host, 1, edges, 1, kw.get("size"))[:4]
    return wmode_want(host, 1, edges, 1)


def sort_requests(cus, n_rows, n_cols):
    """the bytes xhist_sort_run asks the scratch cache for, in its order, for a plan with bins and n_cols > 0: the bin keys, two
    blocks of 8-byte keys, two of 4-byte positions, the counters of one launch's (row, chunk) units and, where a row is more
    than one chunk, the slices' (xhist_sort.hip; 256 counters of 4 bytes each)"""
    g = so.geometry(cus, n_rows, n_cols)
    n, launch_rows = n_rows * n_cols, min(g["rows_per_launch"], n_rows)
    out = [n * 8] * 3 + [n * 4] * 2 + [launch_rows * g["chunks"] * 256 * 4]
    return out + ([launch_rows * g["slices"] * 256 * 4] if g["chunks"] > 1 else [])


def wruns_bytes(n_rows, n_cols, by_position):
    """xhist_rank.hip's wruns_scratch: per word lead and tail, per tile a sum and a flag, and, `by_position`, a float64 per sample"""
    words = -(-n_cols // WORD)
    tiles = -(-words // TILE_WORDS)
    return (n_rows * words * 2 + n_rows * tiles * 2 + (n_rows * n_cols if by_position else 0)) * 8


def domain_bytes(n_rows, n_cols, n_bins, pct=False, extra=0):
    """the one block sorted_domain_run carves (xhist_rank.hip): order, offsets, head and NaN words, the divisors when pct, then
    the 4-byte before / last / next per word and the tiles' three scalars; `extra` bytes of the weighted twins in front"""
    words = -(-n_cols // WORD)
    nw, tiles = n_rows * words, -(-words // TILE_WORDS)
    return extra + (n_rows * n_cols + n_rows * (n_bins + 1) + 2 * nw + (n_rows * n_bins if pct else 0)) * 8 + (3 * nw + 3 * n_rows * tiles) * 4


def scratch_requests(name, cus, n_rows=SCRATCH_ROWS, n_cols=SCRATCH_COLS, n_bins=SCRATCH_BINS):
    """every request one of SCRATCH_CALLS makes of the scratch cache, in order: the carved block first (bin_sort has none), then
    the sort's"""
    fn, kw, _ = SCRATCH_CALLS[name]
    sort = sort_requests(cus, n_rows, n_cols)
    if fn == "bin_sort":
        return sort
    extra = 0
    if fn == "bin_weighted_unique":  # (a width above 0)
        extra = wruns_bytes(n_rows, n_cols, False)
    elif fn == "histogram_weighted_mode":
        extra = wruns_bytes(n_rows, n_cols, True)
    return [domain_bytes(n_rows, n_cols, n_bins, bool(kw.get("pct")), extra)] + sort


# ---------------------------------------------------------------------------------------------------------------------
# (d) one row of more than 256 tiles, from a closed form
# ---------------------------------------------------------------------------------------------------------------------
LONG_N = 256 * TILE + 70_001  # 258 tiles: rank_scan's 256 threads take ceil(258 / 256) = 2 tiles each
LONG_M = 7_368_787  # coprime to LONG_N: position i holds sorted slot (i * M) mod n
LONG_N0, LONG_N1 = 10_108_333, 5_054_099  # about 0.6 n (no multiple of 64) and 0.3 n
LONG_RUN0, LONG_RUN1, LONG_RUN_DROPPED, LONG_NANS = 100_003, 3, 5, 1000
LONG_EDGES = np.array([0.0, 1.0, 2.0])


class LongRow:
    """One row of n samples in 2 bins whose sorted order is known without sorting: input position i holds the sorted slot
    s = (i * m) mod n (m coprime to n: a permutation).  Slots [0, n0) are bin 0, [n0, n0 + n1) bin 1, the rest is dropped (a
    sample outside the edges).  The value of a slot is its place in its segment divided by the segment's run length (run0 in
    bin 0: runs longer than a tile; run1 in bin 1: many heads per word; 5 among the dropped), as float32; the last `nans` slots of
    bin 0 are NaN.  Inside a run the sort orders by input position, so the slot of a sample is its sorted position only up to the
    order inside its run: everything below is a function of the run alone."""

    def __init__(self, n=LONG_N, m=LONG_M, n0=LONG_N0, n1=LONG_N1, run0=LONG_RUN0, run1=LONG_RUN1, nans=LONG_NANS):
        assert math.gcd(m, n) == 1 and 0 < nans < n0 and n0 + n1 < n and (n // run1) < (1 << 24) and n * m < (1 << 62)
        self.n, self.n0, self.n1, self.nans = n, n0, n1, nans
        self.s = (np.arange(n, dtype=np.int64) * m) % n
        s = self.s
        self.bin = np.where(s < n0, 0, np.where(s < n0 + n1, 1, -1)).astype(np.int64)
        self.start = np.array([0, n0, n0 + n1], np.int64)  # of a segment, by bin (-1: the dropped, last)
        self.length = np.array([run0, run1, LONG_RUN_DROPPED], np.int64)  # of a run, by bin
        self.run = (s - self.start[self.bin]) // self.length[self.bin]  # the run of a sample inside its segment
        self.nan = (s >= n0 - nans) & (s < n0)
        self.valid = (self.bin >= 0) & ~self.nan
        self.m = np.array([n0 - nans, n1], np.int64)  # the non-NaN values of a bin
        self.u = -(-self.m // self.length[:2])  # its distinct values
        self.offsets = np.array([0, self.u[0], self.u[0] + self.u[1]], np.int64)

    def samples(self):
        return np.where(self.bin == 0, 0.5, np.where(self.bin == 1, 1.5, 2.5))

    def values(self):
        v = self.run.astype(F32)
        v[self.nan] = np.nan
        return v

    def rank(self, method, descending=False, pct=False):
        """float64 [n]: NaN for the dropped and the NaN values"""
        b = np.where(self.valid, self.bin, 0)
        m, length, u = self.m[b], self.length[b], self.u[b]
        lt = self.run * length
        eq = np.minimum(lt + length, m) - lt
        if descending:
            lt = m - lt - eq
        if method == "min":
            r = (lt + 1).astype(F64)
        elif method == "max":
            r = (lt + eq).astype(F64)
        elif method == "average":
            r = (2 * lt + eq + 1) / 2.0
        elif method == "dense":
            r = (u - self.run if descending else self.run + 1).astype(F64)
        else:
            raise ValueError(method)
        if pct:
            r = r / (u if method == "dense" else m).astype(F64)
        return np.where(self.valid, r, np.nan)

    def mode(self):
        """(count, nunique, mode, mode_count), each [2]: the first of a bin's longest runs is its run 0, the value 0.0"""
        return self.m.copy(), self.u.copy(), np.zeros(2), np.minimum(self.length[:2], self.m)

    def unique(self):
        """(uniques float64 [U], counts int64 [U], offsets int64 [3], inverse int64 [n]), uncut"""
        uniques = np.concatenate([np.arange(k, dtype=F64) for k in self.u])
        counts = np.concatenate([np.minimum(self.length[b], self.m[b] - np.arange(self.u[b]) * self.length[b]) for b in range(2)])
        inverse = np.where(self.valid, self.offsets[np.where(self.valid, self.bin, 0)] + self.run, -1)
        return uniques, counts.astype(np.int64), self.offsets.copy(), inverse

    def weight_sums(self, w):
        """float64 [U]: exactly summable weights summed by entry (np.bincount adds in position order; every partial sum is exact)"""
        inverse = self.unique()[3]
        return np.bincount(inverse[self.valid], weights=w[self.valid], minlength=int(self.offsets[2]))

    def weighted_mode(self, w):
        """(count, nunique, mode, mode_weight): per bin the first entry that holds the largest sum"""
        sums = self.weight_sums(w)
        first = [int(np.argmax(sums[a:b])) for a, b in zip(self.offsets, self.offsets[1:])]
        return self.m.copy(), self.u.copy(), np.array(first, F64), np.array([sums[a + k] for a, k in zip(self.offsets, first)])

    def heads(self):
        """the sorted positions that start a tie run, ascending: every run start of the three segments and every NaN"""
        parts = []
        for b, (a, e) in enumerate(zip(self.start, [self.n0 - self.nans, self.n0 + self.n1, self.n])):
            parts.append(np.arange(a, e, self.length[b]))
            if b == 0:
                parts.append(np.arange(self.n0 - self.nans, self.n0))
        return np.concatenate(parts)
