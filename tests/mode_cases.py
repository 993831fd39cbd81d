"""The cases of tests/test_gpu_mode.py.  The layout cases are written as runs (bin, value, count) in the sorted domain, as
tests/bin_rank_cases.py writes its own, and the positions of a row are shuffled: where the winning run of a bin, a bin border or
the end of a bin's segment falls among the words of 64 sorted positions is known by construction.  The others take the bin
indices of tests/bin_order_cases.py and the value patterns of tests/bin_sort_cases.py.  Every case names the conditions it
claims; tests/test_mode_cpu.py holds each case to them without a GPU, for the 256 compute units of an MI355X."""
import numpy as np

import bin_order_cases as bc
import bin_rank_cases as rc
import bin_rank_oracle as ro
import bin_sort_cases as sc
import bin_sort_oracle as so
import extreme_cases as xc
import mode_oracle as mdo

F64, F32, F16 = np.float64, np.float32, np.float16
CUS = sc.CUS
WORD = ro.WORD
TILE = rc.TILE
SIZES = [1, 63, 64, 65, 513]
VALUE_DTYPES = rc.VALUE_DTYPES  # seven
BINS = [[1], [50], [40960], [279, 339]]
NAN = float("nan")
singles = rc.singles


def layout_runs(name):
    """the runs of a layout case, in ascending sorted order: (bin, value, count), bin -1: dropped"""
    if name == "winner_ends_at_word_border":  # bin 0: [5, 64) wins
        return [(0, 1.0, 5), (0, 2.0, 59), (0, 3.0, 30), (1, 1.0, 30)]
    if name == "winner_starts_at_word_border":  # bin 0: 64 values alone, then [64, 84) wins
        return singles(0, 0, 64) + [(0, 100.0, 20), (0, 101.0, 3), (2, 0.5, 9)]
    if name == "winner_spans_a_word_border":  # bin 0: [40, 90) wins
        return [(0, 1.0, 40), (0, 2.0, 50), (0, 3.0, 45), (1, 2.0, 7)]
    if name == "winner_spans_three_words":  # bin 0: [10, 160) wins, its end is the word's `next`
        return [(0, -1.0, 10), (0, 7.0, 150), (0, 8.0, 5), (2, 7.0, 40), (-1, 7.0, 9)]
    if name == "big_tie":  # more than one tile of head words between the run's head and its end
        return [(3, 1.0, 3), (3, 2.25, 70_000), (3, 5.0, 7)]
    if name == "equal_runs_in_one_word":  # bin 0: three runs of 7, bin 1: two runs of 9, all in word 0
        return [(0, 1.0, 3), (0, 2.0, 7), (0, 3.0, 7), (0, 4.0, 7), (0, 5.0, 2), (1, 1.0, 9), (1, 2.0, 9), (2, 8.0, 1)]
    if name == "equal_runs_in_different_words":  # bin 0: runs of 40 from 0, 70 and 145; bin 1: runs of 60 from 190 and 260
        return [(0, 1.0, 40), (0, 2.0, 30), (0, 3.0, 40), (0, 4.0, 35), (0, 5.0, 40), (1, 1.0, 5), (1, 7.0, 60), (1, 8.0, 10), (1, 9.0, 60)]
    if name == "same_value_across_bin_borders":  # the border 0 | 1 at sorted position 64, lane 0; 1 | 2 at 98, mid word
        return [(0, 1.0, 34), (0, 5.0, 30), (1, 5.0, 30), (1, 6.0, 4), (2, 6.0, 10), (2, 7.0, 3), (-1, 7.0, 5)]
    if name == "one_sample_per_bin_in_one_word":  # 64 bins, 64 positions
        return [(b, float(b % 3), 1) for b in range(64)]
    if name == "segments_end_on_lane_63_and_lane_0":  # bin 0: [0, 64), bin 1: [64, 65), bin 2 after it
        return [(0, 1.0, 30), (0, 2.0, 34), (1, 3.0, 1), (2, 4.0, 20), (2, 5.0, 21)]
    if name == "bin_of_only_nans":
        return [(0, 1.0, 10), (1, NAN, 70), (2, 2.0, 10), (2, NAN, 5), (3, NAN, 1)]
    if name == "nans_outnumber_every_value":
        return [(0, 1.0, 2), (0, 2.0, 3), (0, NAN, 70), (1, 1.0, 1), (1, NAN, 5), (2, 3.0, 2)]
    if name == "dropped_hold_the_longest_run":
        return [(0, 1.0, 3), (0, 2.0, 2), (1, 3.0, 4), (-1, 2.0, 100), (-1, 9.0, 3)]
    if name == "signed_zeros":  # bin 0 and bin 1: one run of both zeros wins; bin 3: +0.0 alone wins
        return [(0, -1.0, 3), (0, -0.0, 20), (0, 0.0, 25), (0, 1.0, 3), (1, 0.0, 40), (1, -0.0, 41), (2, -0.0, 1), (2, 0.0, 1), (2, 4.0, 1),
                (3, 0.0, 6), (3, 1.0, 2), (-1, 0.0, 4), (-1, -0.0, 4)]
    raise ValueError(name)


LAYOUTS = {
    "winner_ends_at_word_border": ("the winning run ends at a word border",),
    "winner_starts_at_word_border": ("the winning run starts at a word border",),
    "winner_spans_a_word_border": ("the winning run spans a word border",),
    "winner_spans_three_words": ("the winning run spans three words",),
    "big_tie": ("70000 equal values in one bin", "two tiles"),
    "equal_runs_in_one_word": ("three runs of equal length in one word", "two runs of equal length in one word"),
    "equal_runs_in_different_words": ("three runs of equal length in different words", "two runs of equal length in different words"),
    "same_value_across_bin_borders": ("the same value across a bin border on lane 0", "the same value across a bin border mid word"),
    "one_sample_per_bin_in_one_word": ("64 bins of one sample each in one word",),
    "segments_end_on_lane_63_and_lane_0": ("a bin's segment ends on lane 63", "a bin's segment ends on lane 0"),
    "bin_of_only_nans": ("a bin of only NaNs",),
    "nans_outnumber_every_value": ("NaNs more numerous than any value",),
    "dropped_hold_the_longest_run": ("dropped samples hold the longest run",),
    "signed_zeros": ("a run of both zeros reports -0.0", "a run of +0.0 alone reports +0.0"),
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
                        claims=claims, layout=layout, seed=xc.seed_of("mode", name)))

    for i, (name, claims) in enumerate(LAYOUTS.items()):
        n_cols = sum(n for _, _, n in layout_runs(name))
        add(name, [64] if name.startswith("one_sample") else [4], F32 if i % 2 else F64, F64, 1 if name == "big_tie" else 2, n_cols, None, None,
            *claims, layout=True)
    for i, n in enumerate(SIZES):
        add("size_%d" % n, [50], F64 if i % 2 else F32, F32 if i % 2 else F64, 1 + 2 * (i % 2), n, "random", "random", "chunks=1")
    add("several_chunks_3rows", [50], F32, F32, 3, sc.REF_COLS, "random", "random", "several chunks")
    add("all_distinct", [50], F64, F64, 3, 513, "random", "alone", "every value distinct")
    add("one_value_only", [50], F32, F64, 3, 700, "random", "equal", "one value only")
    add("all_dropped", [7], F32, F64, 2, 3000, "dropped", "random", "all dropped")
    add("specials_f64", [50], F64, F64, 2, sc.REF_COLS, "random", "special", "specials")
    add("specials_f32", [50], F32, F32, 2, sc.REF_COLS, "random", "special", "specials")
    add("specials_f16", [50], F64, F16, 2, sc.REF_COLS, "random", "special", "specials")
    for vt in VALUE_DTYPES:
        add("values_%s" % so.DTYPE_NAME[np.dtype(vt)], [50], F64, vt, 3, 1000, "random", "random")
    for nbs in BINS:
        add("bins_%s" % "x".join(map(str, nbs)), nbs, F32 if nbs[0] % 2 else F64, F32, 2, 5000, "random", "random")
    return out


def check_claims(case, idx, v, cus):
    """AssertionError unless the case reaches what it claims (idx: its bin indices, v: its values)"""
    n_bins = int(np.prod(case["nbs"]))
    g = so.geometry(cus, case["n_rows"], case["n_cols"])
    for row_i, row_v in zip(idx, v):
        _, ks, vs, head = ro.sorted_domain(row_i, row_v, n_bins)
        count, nunique, mode, mode_count = mdo.mode_row(row_i, row_v, n_bins)
        s, e = rc.runs_of(head)
        valid = (ks[s] < n_bins) & ~np.isnan(vs[s])
        length = e - s
        # all runs as long as the winner of their bin, and of those the first of each bin: the winners
        top = valid & (length == mode_count[np.minimum(ks[s], n_bins - 1).astype(np.int64)])
        win = np.array([t and not (top[:j] & (ks[s][:j] == ks[s][j])).any() for j, t in enumerate(top)], bool)
        seg_end = np.flatnonzero(np.concatenate([ks[1:] != ks[:-1], [True]]) & (ks < n_bins))  # the last position of a bin's segment
        for claim in case["claims"]:
            if claim == "the winning run ends at a word border":
                hit = (win & (e % WORD == 0) & (s % WORD != 0) & (length > 1)).any()
            elif claim == "the winning run starts at a word border":
                hit = (win & (s % WORD == 0) & (s > 0) & (e % WORD != 0) & (length > 1)).any()
            elif claim == "the winning run spans a word border":
                hit = (win & ((e - 1) // WORD - s // WORD == 1) & (s % WORD != 0) & (e % WORD != 0)).any()
            elif claim == "the winning run spans three words":
                hit = (win & ((e - 1) // WORD - s // WORD >= 2) & (s % WORD != 0) & (e % WORD != 0)).any()
            elif claim == "70000 equal values in one bin":
                hit = mode_count.max() == 70_000
            elif claim == "two tiles":
                hit = -(-case["n_cols"] // WORD) > TILE
            elif claim.endswith("runs of equal length in one word") or claim.endswith("runs of equal length in different words"):
                want = 3 if claim.startswith("three") else 2
                hit = False
                for b in range(n_bins):
                    at = s[top & (ks[s] == b)] // WORD
                    if len(at) == want:
                        hit |= (len(set(at)) == 1 and (e[top & (ks[s] == b)] - 1 < WORD).all()) if "one word" in claim else len(set(at)) == want
            elif claim.startswith("the same value across a bin border"):
                i = np.flatnonzero((ks[1:] != ks[:-1]) & (vs[1:] == vs[:-1]) & (ks[1:] < n_bins)) + 1
                on = (i % WORD == 0) if claim.endswith("lane 0") else (i % WORD != 0)
                # ... and the value wins the bin on one side with its own count, which the sum over both sides would beat
                hit = on.any() and all(mode_count[ks[j]] < np.sum(vs == vs[j]) for j in i[on]) and any(mode[ks[j]] == vs[j] for j in i[on])
            elif claim == "64 bins of one sample each in one word":
                hit = len(ks) == 64 and n_bins == 64 and (count == 1).all() and (mode_count == 1).all()
            elif claim == "a bin's segment ends on lane 63":
                hit = (seg_end % WORD == 63).any()
            elif claim == "a bin's segment ends on lane 0":
                hit = ((seg_end % WORD == 0) & (seg_end > 0)).any()
            elif claim == "a bin of only NaNs":
                hit = any(np.isnan(vs[ks == b]).all() and (ks == b).sum() > WORD and count[b] == 0 for b in range(n_bins) if (ks == b).any())
            elif claim == "NaNs more numerous than any value":
                hit = any((np.isnan(vs) & (ks == b)).sum() > mode_count[b] > 0 for b in range(n_bins))
            elif claim == "dropped samples hold the longest run":
                hit = length[ks[s] == n_bins].max() > mode_count.max() > 0
            elif claim == "a run of both zeros reports -0.0":
                hit = any(mode[b] == 0 and np.signbit(mode[b]) and ((vs == 0) & ~np.signbit(vs) & (ks == b)).any() for b in range(n_bins))
            elif claim == "a run of +0.0 alone reports +0.0":
                hit = any(mode[b] == 0 and not np.signbit(mode[b]) and count[b] > 0 for b in range(n_bins))
            elif claim == "chunks=1":
                hit = g["chunks"] == 1
            elif claim == "several chunks":
                hit = g["chunks"] >= 3
            elif claim == "every value distinct":
                hit = head.all() and (nunique == count).all() and (mode_count[count > 0] == 1).all()
            elif claim == "one value only":
                hit = (nunique[count > 0] == 1).all() and (mode_count == count).all() and (count > 0).any()
            elif claim == "all dropped":
                hit = (ks == n_bins).all() and (count == 0).all()
            elif claim == "specials":
                f = vs[ks < n_bins]
                tiny = np.finfo(v.dtype).tiny
                hit = (((f == 0) & np.signbit(f)).any() and ((f == 0) & ~np.signbit(f)).any() and (f == np.inf).any() and (f == -np.inf).any()
                       and ((np.abs(f) < tiny) & (f != 0)).any() and np.isnan(f).any())
            else:
                raise AssertionError("unknown claim %r" % claim)
            assert hit, (case["name"], claim)
