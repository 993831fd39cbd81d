"""The cases of tests/test_gpu_bin_unique.py.  The layout cases are written as runs (bin, value, count) in the sorted domain, as
tests/mode_cases.py writes its own, and the positions of a row are shuffled: where a run, a bin border or the end of a bin's
segment falls among the words of 64 sorted positions and the tiles of 1024 words, whose scalars locate a run, is known by
construction.  The others take the bin indices of tests/bin_order_cases.py and the value patterns of tests/bin_sort_cases.py.
Every case names the conditions it claims; tests/test_bin_unique_cpu.py holds each case to them without a GPU, for the 256
compute units of an MI355X.  A case's `inverse` says whether its call asks for the inverse; every case runs at size=None."""
import numpy as np

import bin_order_cases as bc
import bin_rank_cases as rc
import bin_rank_oracle as ro
import bin_sort_cases as sc
import bin_sort_oracle as so
import bin_unique_oracle as uo
import extreme_cases as xc

F64, F32, F16 = np.float64, np.float32, np.float16
CUS = sc.CUS
WORD = ro.WORD
TILE = rc.TILE
SIZES = [1, 63, 64, 65, 513]
VALUE_DTYPES = rc.VALUE_DTYPES  # seven
# 1023, 1024 and 1025 bins: B + 1 offsets one short of, exactly and one past a scan tile of the workgroup (uo.SCAN_TILE)
BINS = [[1], [2], [257], [1023], [1024], [1025], [279, 339]]
NAN = float("nan")
singles = rc.singles


def layout_runs(name):
    """the runs of a layout case, in ascending sorted order: (bin, value, count), bin -1: dropped"""
    if name == "run_ends_at_word_border":  # [5, 64)
        return [(0, 1.0, 5), (0, 2.0, 59), (0, 3.0, 30), (1, 1.0, 30)]
    if name == "run_starts_at_word_border":  # 64 values alone, then [64, 84)
        return singles(0, 0, 64) + [(0, 100.0, 20), (0, 101.0, 3), (2, 0.5, 9)]
    if name == "run_spans_a_word_border":  # [40, 90)
        return [(0, 1.0, 40), (0, 2.0, 50), (0, 3.0, 45), (1, 2.0, 7)]
    if name == "run_spans_three_words":  # [10, 160): its end is the word's `next`
        return [(0, -1.0, 10), (0, 7.0, 150), (0, 8.0, 5), (2, 7.0, 40), (-1, 7.0, 9)]
    if name == "big_tie":  # more than one tile of head words between the run's head and its end
        return [(3, 1.0, 3), (3, 2.25, 70_000), (3, 5.0, 7)]
    if name == "one_sample_per_bin_in_one_word":  # 64 bins, 64 positions
        return [(b, float(b % 3), 1) for b in range(64)]
    if name == "segments_end_on_lane_63_and_lane_0":  # bin 0: [0, 64), bin 1: [64, 65), bin 2 after it
        return [(0, 1.0, 30), (0, 2.0, 34), (1, 3.0, 1), (2, 4.0, 20), (2, 5.0, 21)]
    if name == "same_value_across_bin_borders":  # the border 0 | 1 at sorted position 64, lane 0; 1 | 2 at 98, mid word
        return [(0, 1.0, 34), (0, 5.0, 30), (1, 5.0, 30), (1, 6.0, 4), (2, 6.0, 10), (2, 7.0, 3), (-1, 7.0, 5)]
    if name == "bin_of_only_nans":
        return [(0, 1.0, 10), (1, NAN, 70), (2, 2.0, 10), (2, NAN, 5), (3, NAN, 1)]
    if name == "nans_outnumber_the_values":
        return [(0, 1.0, 2), (0, 2.0, 3), (0, NAN, 70), (1, 1.0, 1), (1, NAN, 5), (2, 3.0, 2)]
    if name == "dropped_hold_the_longest_run":
        return [(0, 1.0, 3), (0, 2.0, 2), (1, 3.0, 4), (-1, 2.0, 100), (-1, 9.0, 3)]
    if name == "signed_zeros":  # bins 0, 1, 2: both zeros, one entry; bin 3: +0.0 alone
        return [(0, -1.0, 3), (0, -0.0, 20), (0, 0.0, 25), (0, 1.0, 3), (1, 0.0, 40), (1, -0.0, 41), (2, -0.0, 1), (2, 0.0, 1), (2, 4.0, 1),
                (3, 0.0, 6), (3, 1.0, 2), (-1, 0.0, 4), (-1, -0.0, 4)]
    if name == "every_value_distinct":  # no sample dropped, no NaN: U = c, and the padding is empty
        return singles(0, 0, 100) + singles(1, 50, 70) + singles(3, -20, 343)
    if name == "one_value_only":
        return [(0, 2.5, 300), (1, 2.5, 1), (3, 2.5, 399)]
    if name == "all_dropped":
        return [(-1, 1.0, 100), (-1, 2.0, 200), (-1, NAN, 30)]
    if name == "all_nan":
        return [(0, NAN, 100), (2, NAN, 130), (-1, NAN, 20)]
    raise ValueError(name)


LAYOUTS = {
    "run_ends_at_word_border": ("a run ends at a word border",),
    "run_starts_at_word_border": ("a run starts at a word border",),
    "run_spans_a_word_border": ("a run spans a word border",),
    "run_spans_three_words": ("a run spans three words",),
    "big_tie": ("70000 equal values in one bin", "two tiles"),
    "one_sample_per_bin_in_one_word": ("64 bins of one sample each in one word",),
    "segments_end_on_lane_63_and_lane_0": ("a bin's segment ends on lane 63", "a bin's segment ends on lane 0"),
    "same_value_across_bin_borders": ("the same value on both sides of a bin border is two entries",),
    "bin_of_only_nans": ("a bin of only NaNs has no entry",),
    "nans_outnumber_the_values": ("NaNs more numerous than values",),
    "dropped_hold_the_longest_run": ("dropped samples hold the row's longest run",),
    "signed_zeros": ("both zeros are one entry that reads -0.0", "+0.0 alone reads +0.0"),
    "every_value_distinct": ("every value distinct (U = c)",),
    "one_value_only": ("one value only",),
    "all_dropped": ("all dropped (U = 0)",),
    "all_nan": ("all NaN (U = 0)",),
}


def case_data(case, cus):
    """(edges, the bin indices [n_rows, n_cols], the D sample arrays, the values) of a case"""
    n_bins = int(np.prod(case["nbs"]))
    edges = bc.edges_for(case["nbs"])
    if case["layout"]:
        idx, v = rc.from_runs(layout_runs(case["name"]), case["n_rows"], case["seed"], False)
        v = v.astype(case["vt"])
    else:
        idx = bc.indices(case["pattern"], case["n_rows"], case["n_cols"], n_bins, case["seed"])
        v = sc.values(case["vpattern"], case["vt"], case["n_rows"], case["n_cols"], case["seed"])
    return edges, idx, xc.emit(idx, edges, case["st"]), v


def gpu_cases(cus):
    out = []

    def add(name, nbs, st, vt, n_rows, n_cols, pattern, vpattern, *claims, layout=False):
        out.append(dict(name=name, nbs=list(nbs), st=st, vt=np.dtype(vt), n_rows=n_rows, n_cols=n_cols, pattern=pattern, vpattern=vpattern,
                        claims=claims, layout=layout, inverse=len(out) % 3 != 2, seed=xc.seed_of("bin_unique", name)))

    for i, (name, claims) in enumerate(LAYOUTS.items()):
        n_cols = sum(n for _, _, n in layout_runs(name))
        add(name, [64] if name.startswith("one_sample") else [4], F32 if i % 2 else F64, F64, 1 if name == "big_tie" else 2, n_cols, None, None,
            *claims, layout=True)
    for i, n in enumerate(SIZES):
        add("size_%d" % n, [50], F64 if i % 2 else F32, F32 if i % 2 else F64, 1 + 2 * (i % 2), n, "random", "random", "chunks=1")
    add("several_chunks_3rows", [50], F32, F32, 3, sc.REF_COLS, "random", "random", "several chunks")
    add("specials_f64", [50], F64, F64, 2, sc.REF_COLS, "random", "special", "specials")
    add("specials_f32", [50], F32, F32, 2, sc.REF_COLS, "random", "special", "specials")
    add("specials_f16", [50], F64, F16, 2, sc.REF_COLS, "random", "special", "specials")
    for vt in VALUE_DTYPES:
        add("values_%s" % so.DTYPE_NAME[np.dtype(vt)], [50], F64, vt, 3, 1000, "random", "random")
    for nbs in BINS:
        add("bins_%s" % "x".join(map(str, nbs)), nbs, F32 if nbs[0] % 2 else F64, F32, 2, 5000, "random", "random",
            *(("the scan carries over a tile",) if int(np.prod(nbs)) + 1 > uo.SCAN_TILE else ()))
    return out


def check_claims(case, idx, v, cus):
    """AssertionError unless the case reaches what it claims (idx: its bin indices, v: its values)"""
    n_bins = int(np.prod(case["nbs"]))
    g = so.geometry(cus, case["n_rows"], case["n_cols"])
    for row_i, row_v in zip(idx, v):
        _, ks, vs, head = ro.sorted_domain(row_i, row_v, n_bins)
        uniques, counts, offsets, inverse = uo.unique_row(row_i, row_v, n_bins)
        total, c = int(offsets[-1]), len(ks)
        nunique = np.diff(offsets)
        s, e = rc.runs_of(head)
        nan = np.isnan(vs)
        valid = (ks[s] < n_bins) & ~nan[s]
        length = e - s
        long = valid & (length > 1)
        seg_end = np.flatnonzero(np.concatenate([ks[1:] != ks[:-1], [True]]) & (ks < n_bins))  # the last position of a bin's segment
        for claim in case["claims"]:
            if claim == "a run ends at a word border":
                hit = (long & (e % WORD == 0) & (s % WORD != 0)).any()
            elif claim == "a run starts at a word border":
                hit = (long & (s % WORD == 0) & (s > 0) & (e % WORD != 0)).any()
            elif claim == "a run spans a word border":
                hit = (long & ((e - 1) // WORD - s // WORD == 1) & (s % WORD != 0) & (e % WORD != 0)).any()
            elif claim == "a run spans three words":
                hit = (long & ((e - 1) // WORD - s // WORD >= 2) & (s % WORD != 0) & (e % WORD != 0)).any()
            elif claim == "70000 equal values in one bin":
                hit = counts.max() == 70_000
            elif claim == "two tiles":
                hit = -(-case["n_cols"] // WORD) > TILE
            elif claim == "64 bins of one sample each in one word":
                hit = c == 64 and n_bins == 64 and (nunique == 1).all() and (counts == 1).all()
            elif claim == "a bin's segment ends on lane 63":
                hit = (seg_end % WORD == 63).any()
            elif claim == "a bin's segment ends on lane 0":
                hit = ((seg_end % WORD == 0) & (seg_end > 0)).any()
            elif claim == "the same value on both sides of a bin border is two entries":
                i = np.flatnonzero((ks[1:] != ks[:-1]) & (vs[1:] == vs[:-1]) & (ks[1:] < n_bins)) + 1
                hit = (i % WORD == 0).any() and (i % WORD != 0).any() and all((uniques[:total] == vs[j]).sum() >= 2 for j in i)
                hit = hit and all(uniques[offsets[int(ks[j])]] == vs[j] == uniques[offsets[int(ks[j])] - 1] for j in i)
            elif claim == "a bin of only NaNs has no entry":
                hit = any(nan[ks == b].all() and (ks == b).sum() > WORD and nunique[b] == 0 for b in range(n_bins) if (ks == b).any())
            elif claim == "NaNs more numerous than values":
                hit = any((nan & (ks == b)).sum() > (~nan & (ks == b)).sum() > 0 for b in range(n_bins))
            elif claim == "dropped samples hold the row's longest run":
                hit = length[ks[s] == n_bins].max() > counts.max() > 0
            elif claim == "both zeros are one entry that reads -0.0":
                z = np.flatnonzero((uniques[:total] == 0) & np.signbit(uniques[:total]))
                hit = len(z) >= 2 and all(((vs == 0) & ~np.signbit(vs) & (ks == np.searchsorted(offsets, u, "right") - 1)).any() for u in z)
            elif claim == "+0.0 alone reads +0.0":
                hit = ((uniques[:total] == 0) & ~np.signbit(uniques[:total])).any()
            elif claim == "every value distinct (U = c)":
                hit = total == c and head.all() and (counts == 1).all() and (np.sort(inverse) == np.arange(c)).all()
            elif claim == "one value only":
                hit = (nunique <= 1).all() and total >= 2 and len(set(uniques[:total])) == 1
            elif claim == "all dropped (U = 0)":
                hit = (ks == n_bins).all() and total == 0 and (inverse == -1).all()
            elif claim == "all NaN (U = 0)":
                hit = nan.all() and (ks < n_bins).any() and total == 0 and (inverse == -1).all()
            elif claim == "chunks=1":
                hit = g["chunks"] == 1
            elif claim == "several chunks":
                hit = g["chunks"] >= 3
            elif claim == "the scan carries over a tile":
                hit = n_bins + 1 > uo.SCAN_TILE and offsets[uo.SCAN_TILE - 1] > 0 and total > offsets[uo.SCAN_TILE - 1]
            elif claim == "specials":
                f = vs[ks < n_bins]
                tiny = np.finfo(v.dtype).tiny
                hit = (((f == 0) & np.signbit(f)).any() and ((f == 0) & ~np.signbit(f)).any() and (f == np.inf).any() and (f == -np.inf).any()
                       and ((np.abs(f) < tiny) & (f != 0)).any() and np.isnan(f).any())
            else:
                raise AssertionError("unknown claim %r" % claim)
            assert hit, (case["name"], claim)


# the sizes of tests/test_gpu_bin_unique.py's cut, for a row of U entries among c samples with 1 < U < c
def sizes_for(total, c):
    assert 1 < total < c
    return [None, 0, 1, total - 1, total, total + 1, c + 7]
