"""The cases of tests/test_gpu_bin_rank.py.  The layout cases are written as runs (bin, value, count) and the positions of a row
are shuffled, so where a tie run, a bin border or the first NaN of a bin falls among the words of 64 sorted positions is known
by construction; a descending call takes the same runs with the values negated, which puts every border where the ascending
call has it.  The others take the bin indices of tests/bin_order_cases.py and the value patterns of tests/bin_sort_cases.py.
Every case names the conditions it claims; tests/test_bin_rank_cpu.py holds each case to them without a GPU, in both directions,
for the 256 compute units of an MI355X."""
import numpy as np

import bin_order_cases as bc
import bin_rank_oracle as ro
import bin_sort_cases as sc
import bin_sort_oracle as so
import extreme_cases as xc

F64, F32, F16 = np.float64, np.float32, np.float16
CUS = sc.CUS
WORD = ro.WORD
TILE = 1024  # words of one tile of the scan over the head words (kRankTile)
SIZES = [1, 63, 64, 65, 127, 128, 129, 513]
VALUE_DTYPES = [np.float64, np.float32, np.float16, np.int64, np.int32, np.uint8, np.bool_]
BINS = [[1], [100], [40960], [279, 339]]
MODES = [(m, d, p) for m in ro.METHODS for d in (False, True) for p in (False, True)]
NAN = float("nan")


def singles(b, start, count):
    return [(b, float(start + k), 1) for k in range(count)]


def layout_runs(name, chunk):
    """the runs of a layout case, in ascending sorted order: (bin, value, count), bin -1: dropped"""
    if name == "run_ends_at_word_border":  # [0, 64), then [69, 128)
        return [(0, 1.0, 64), (0, 2.0, 5), (0, 3.0, 59), (1, 1.0, 30)]
    if name == "run_starts_at_word_border":  # 64 values alone, then [64, 84)
        return singles(0, 0, 64) + [(0, 100.0, 20), (0, 101.0, 3), (2, 0.5, 9)]
    if name == "run_spans_three_words":  # [10, 160)
        return [(0, -1.0, 10), (0, 7.0, 150), (0, 8.0, 5), (2, 7.0, 40), (-1, 7.0, 9)]
    if name == "run_over_three_chunk_borders":
        n = 3 * chunk + 100
        return singles(1, 0, 500) + [(1, 1000.0, n)] + singles(2, 0, 4000 - 500 - n)
    if name == "big_tie":  # more than one tile of head words, one head in all of them
        return [(3, 2.25, 70_000)]
    if name == "equal_values_across_bin_borders":  # the border 0 | 1 at sorted position 64, lane 0; 1 | 2 at 98, mid word
        return [(0, 1.0, 34), (0, 5.0, 30), (1, 5.0, 30), (1, 6.0, 4), (2, 6.0, 10), (2, 7.0, 3), (-1, 7.0, 5)]
    if name == "bin_of_only_nans":
        return [(0, 1.0, 10), (1, NAN, 70), (2, 2.0, 10), (2, NAN, 5), (3, NAN, 1)]
    if name == "nan_run_starts_at_word_border":  # bin 0: 64 values, then 30 NaN from position 64
        return singles(0, 0, 50) + [(0, 99.0, 14), (0, NAN, 30), (1, 3.0, 20), (1, NAN, 2)]
    if name == "bin_with_one_value":
        return [(0, 1.0, 1), (1, 2.0, 1), (1, NAN, 3), (3, 4.0, 7), (-1, 4.0, 2)]
    if name == "signed_zeros":
        return [(0, -1.0, 3), (0, -0.0, 20), (0, 0.0, 25), (0, 1.0, 3), (1, 0.0, 40), (1, -0.0, 41), (2, -0.0, 1), (2, 0.0, 1), (-1, 0.0, 4),
                (-1, -0.0, 4)]
    raise ValueError(name)


LAYOUTS = {
    "run_ends_at_word_border": ("a tie run ends at a word border",),
    "run_starts_at_word_border": ("a tie run starts at a word border",),
    "run_spans_three_words": ("a tie run spans three words",),
    "run_over_three_chunk_borders": ("a tie run crosses three chunk borders", "several chunks"),
    "big_tie": ("70000 equal values in one bin", "two tiles"),
    "equal_values_across_bin_borders": ("equal values across a bin border on lane 0", "equal values across a bin border mid word"),
    "bin_of_only_nans": ("a bin of only NaNs",),
    "nan_run_starts_at_word_border": ("a NaN run starts at a word border",),
    "bin_with_one_value": ("a bin with one value",),
    "signed_zeros": ("both zeros in one tie run",),
}


def from_runs(runs, n_rows, seed, descending):
    """(idx int32 [n_rows, c], v float64 [n_rows, c]): the runs laid out one after the other, every row shuffled on its own"""
    idx = np.concatenate([np.full(n, b, np.int32) for b, _, n in runs])
    v = np.concatenate([np.full(n, x, F64) for _, x, n in runs])
    if descending:
        v = -v  # (NaN stays NaN; the zeros swap signs, and the descending order puts them where the ascending one did)
    rng = np.random.default_rng(seed)
    perms = [rng.permutation(len(idx)) for _ in range(n_rows)]
    return np.stack([idx[p] for p in perms]), np.stack([v[p] for p in perms])


def chunk_of(case, cus):
    return so.geometry(cus, case["n_rows"], case["n_cols"])["chunk"]


def case_data(case, cus, descending=False):
    """(edges, the bin indices [n_rows, n_cols], the D sample arrays, the values) of a case for a call in that direction"""
    n_bins = int(np.prod(case["nbs"]))
    edges = bc.edges_for(case["nbs"])
    if case["layout"]:
        idx, v = from_runs(layout_runs(case["name"], chunk_of(case, cus)), case["n_rows"], case["seed"], descending)
        v = v.astype(case["vt"])
    else:
        idx = bc.indices(case["pattern"], case["n_rows"], case["n_cols"], n_bins, case["seed"])
        if case["vpattern"] == "all_nan":
            v = np.full(idx.shape, np.nan, case["vt"])
        else:
            v = sc.values(case["vpattern"], case["vt"], case["n_rows"], case["n_cols"], case["seed"])
        if case["name"] == "a_row_of_dropped_and_nan":
            v = v.copy()
            v[1, idx[1] >= 0] = np.nan
    return edges, idx, xc.emit(idx, edges, case["st"]), v


def gpu_cases(cus):
    out = []

    def add(name, nbs, st, vt, n_rows, n_cols, pattern, vpattern, *claims, layout=False):
        out.append(dict(name=name, nbs=list(nbs), st=st, vt=np.dtype(vt), n_rows=n_rows, n_cols=n_cols, pattern=pattern, vpattern=vpattern,
                        claims=claims, layout=layout, seed=xc.seed_of("bin_rank", name)))

    for i, (name, claims) in enumerate(LAYOUTS.items()):
        n_rows = 1 if name == "big_tie" else 2
        probe = dict(n_rows=n_rows, n_cols=4000)
        n_cols = sum(n for _, _, n in layout_runs(name, chunk_of(probe, cus)))
        add(name, [4], F32 if i % 2 else F64, F64, n_rows, n_cols, None, None, *claims, layout=True)
    for i, n in enumerate(SIZES):
        add("size_%d" % n, [100], F64 if i % 2 else F32, F32 if i % 2 else F64, 1 + 2 * (i % 2), n, "random", "random", "chunks=1")
    add("several_chunks_1row", [100], F64, F64, 1, sc.REF_COLS, "random", "random", "several chunks")
    add("several_chunks_3rows", [100], F32, F32, 3, sc.REF_COLS, "random", "random", "several chunks")
    add("two_slices", [100], F64, F32, 1, sc.TWO_SLICES, "random", "random", "several chunks", "two slices")
    add("all_distinct", [100], F64, F64, 3, 513, "random", "alone", "every value distinct")
    add("every_sample_alone", [5000], F64, F64, 2, 3000, "alone", "random", "every sample alone in its bin")
    add("all_dropped", [7], F32, F64, 2, 3000, "dropped", "random", "all dropped")
    add("all_values_nan", [7], F64, F32, 2, 1000, "random", "all_nan", "all values NaN")
    add("a_row_of_dropped_and_nan", [7], F64, F64, 3, 1000, "random", "random", "a row of dropped and NaN")
    add("specials_f64", [100], F64, F64, 2, sc.REF_COLS, "random", "special", "specials")
    add("specials_f32", [100], F32, F32, 2, sc.REF_COLS, "random", "special", "specials")
    add("specials_f16", [100], F64, F16, 2, sc.REF_COLS, "random", "special", "specials")
    for vt in VALUE_DTYPES:
        add("values_%s" % so.DTYPE_NAME[np.dtype(vt)], [100], F64, vt, 3, 1000, "random", "random")
    for nbs in BINS:
        add("bins_%s" % "x".join(map(str, nbs)), nbs, F32 if nbs[0] % 2 else F64, F32, 2, 5000, "random", "random")
    return out


def runs_of(head):
    """(starts, ends) of the tie runs of one row in the sorted domain"""
    starts = np.flatnonzero(head)
    return starts, np.concatenate([starts[1:], [len(head)]])


def check_claims(case, idx, v, cus, descending=False):
    """AssertionError unless the case reaches what it claims (idx: its bin indices, v: its values) in a call of that direction"""
    n_bins = int(np.prod(case["nbs"]))
    g = so.geometry(cus, case["n_rows"], case["n_cols"])
    rows = [ro.sorted_domain(i, x, n_bins, descending) for i, x in zip(idx, v)]
    for claim in case["claims"]:
        hit = []
        for _, ks, vs, head in rows:
            s, e = runs_of(head)
            counted = ks[s] < n_bins
            long = (e - s > 1) & counted
            nan = np.isnan(vs)
            if claim == "a tie run ends at a word border":
                hit.append((long & (e % WORD == 0) & (s % WORD != 0)).any() and (long & (e % WORD == 0) & (e - s == WORD)).any())
            elif claim == "a tie run starts at a word border":
                hit.append((long & (s % WORD == 0) & (s > 0) & (e % WORD != 0)).any())
            elif claim == "a tie run spans three words":
                hit.append((long & ((e - 1) // WORD - s // WORD >= 2) & (s % WORD != 0) & (e % WORD != 0)).any())
            elif claim == "a tie run crosses three chunk borders":
                hit.append((long & ((e - 1) // g["chunk"] - s // g["chunk"] >= 3)).any())
            elif claim == "70000 equal values in one bin":
                hit.append(len(s) == 1 and e[0] == 70_000 and counted[0])
            elif claim == "two tiles":
                hit.append(-(-case["n_cols"] // WORD) > TILE)
            elif claim.startswith("equal values across a bin border"):
                i = np.flatnonzero((ks[1:] != ks[:-1]) & (vs[1:] == vs[:-1]) & (ks[1:] < n_bins)) + 1
                hit.append(head[i].all() and ((i % WORD == 0).any() if claim.endswith("lane 0") else (i % WORD != 0).any()))
            elif claim == "a bin of only NaNs":
                hit.append(any(nan[ks == b].all() and (ks == b).sum() > WORD for b in range(n_bins) if (ks == b).any()))
            elif claim == "a NaN run starts at a word border":
                first = np.flatnonzero(nan & (ks < n_bins) & np.concatenate([[True], ~nan[:-1] | (ks[1:] != ks[:-1])]))
                hit.append((first % WORD == 0).any() and (first > 0).all())
            elif claim == "a bin with one value":
                hit.append(any(((ks == b) & ~nan).sum() == 1 for b in range(n_bins)) and any((ks == b).sum() == 1 for b in range(n_bins)))
            elif claim == "both zeros in one tie run":
                z = (vs == 0) & (ks < n_bins)
                mixed = z[1:] & z[:-1] & (ks[1:] == ks[:-1]) & (np.signbit(vs[1:]) != np.signbit(vs[:-1]))
                hit.append(mixed.any() and not head[1:][mixed].any())
            elif claim == "chunks=1":
                hit.append(g["chunks"] == 1)
            elif claim == "several chunks":
                hit.append(g["chunks"] >= 3)
            elif claim == "two slices":
                hit.append(g["slices"] == 2)
            elif claim == "every value distinct":
                hit.append(head.all())
            elif claim == "every sample alone in its bin":
                hit.append(len(np.unique(ks)) == len(ks))
            elif claim == "all dropped":
                hit.append((ks == n_bins).all())
            elif claim == "all values NaN":
                hit.append(nan.all() and (ks < n_bins).any())
            elif claim == "a row of dropped and NaN":
                hit.append(True)
            elif claim == "specials":
                f = vs[ks < n_bins]
                tiny = np.finfo(v.dtype).tiny
                hit.append(((f == 0) & np.signbit(f)).any() and ((f == 0) & ~np.signbit(f)).any() and (f == np.inf).any()
                           and (f == -np.inf).any() and ((np.abs(f) < tiny) & (f != 0)).any() and np.isnan(f).any())
            else:
                raise AssertionError("unknown claim %r" % claim)
        if claim == "a row of dropped and NaN":
            _, ks, vs, _ = rows[1]
            hit = [((ks == n_bins) | np.isnan(vs)).all() and (ks < n_bins).any() and not np.isnan(rows[0][2]).all()]
        assert all(hit), (case["name"], claim, descending, hit)
