"""The cases of tests/test_gpu_bin_weighted_unique.py and tests/test_gpu_weighted_mode.py.  The layout cases are runs (bin, value,
count) in the sorted domain, as tests/bin_unique_cases.py writes its own (some are its own), with the positions of a row
shuffled: where a run lies against the words of 64 sorted positions and the tiles of 1024 words, which decides the kernel that
stores its sum and the tree of its additions, is known by construction.  Every case names what it claims and
tests/test_bin_weighted_unique_cpu.py holds it to that without a GPU.

Weights are exactly summable (tests/exact_weights.py), of both signs; a sample that is dropped or whose value is NaN carries a
weight 2^40 times larger (2^15 and 2^20 in the float16 and int32 cases), so a sum that took one in would be wrong in its leading bits."""
import numpy as np

import bin_order_cases as bc
import bin_rank_cases as rc
import bin_rank_oracle as ro
import bin_unique_cases as uc
import exact_weights as xw
import extreme_cases as xc
import weighted_unique_oracle as wo

F64, F32, F16 = np.float64, np.float32, np.float16
CUS = uc.CUS
WORD, TILE = wo.WORD, wo.TILE
NAN = float("nan")
WEIGHT_DTYPES = [F64, F32, np.int32, F16]
HEAVY = {np.dtype(F64): 2.0 ** 40, np.dtype(F32): 2.0 ** 40, np.dtype(F16): 2.0 ** 15, np.dtype(np.int32): 2.0 ** 20}


def layout_runs(name):
    if name == "run_inside_one_word":  # [5, 25)
        return [(0, 1.0, 5), (0, 2.0, 20), (0, 3.0, 10), (1, 2.0, 4)]
    if name == "run_ends_on_lane_63_before_a_head":  # [30, 64), a head at 64
        return [(0, 1.0, 30), (0, 2.0, 34), (0, 3.0, 10), (2, 1.0, 3)]
    if name == "run_starts_on_lane_63":  # [63, 83)
        return [(0, 1.0, 63), (0, 2.0, 20), (1, 2.0, 2)]
    if name == "run_starts_on_lane_0":  # [64, 84)
        return rc.singles(0, 0, 64) + [(0, 100.0, 20), (0, 101.0, 3), (2, 0.5, 9)]
    if name == "run_over_exactly_two_words":  # [64, 192)
        return [(0, 1.0, 64), (0, 2.0, 128), (0, 3.0, 5)]
    if name == "run_over_three_words":  # [40, 160): word 1 has no head
        return [(0, 1.0, 40), (0, 2.0, 120), (0, 3.0, 9), (3, 2.0, 1)]
    if name == "run_ends_with_the_row":  # [10, 160): the last word has no head
        return [(0, 1.0, 10), (0, 2.0, 150)]
    if name == "run_of_70000":  # [3, 70003): one tile border
        return [(3, 1.0, 3), (3, 2.25, 70_000), (3, 5.0, 7)]
    if name == "run_of_140000":  # [100, 140100): all of tile 1
        return [(1, 1.0, 100), (1, 2.0, 140_000), (1, 3.0, 5)]
    if name == "two_big_runs_in_neighbouring_bins":  # [0, 70000) and [70000, 140000)
        return [(1, 2.0, 70_000), (2, 2.0, 70_000)]
    if name == "nan_between_two_equal_values":
        return [(0, 5.0, 30), (0, NAN, 10), (1, 5.0, 30), (1, NAN, 1), (2, 5.0, 3)]
    return uc.layout_runs(name)


def _runs(idx, v, n_bins):
    """per row: (run starts, run ends, whether the run is an entry)"""
    for row_i, row_v in zip(idx, v):
        _, ks, vs, head = ro.sorted_domain(row_i, row_v, n_bins)
        s, e = rc.runs_of(head)
        yield s, e, (ks[s] < n_bins) & ~np.isnan(vs[s]), ks, vs


CLAIMS = {
    "a run inside one word": lambda s, e, ok: (ok & (e - s > 1) & (s // WORD == (e - 1) // WORD) & (s % WORD > 0) & (e % WORD > 0)).any(),
    "a run ends on lane 63 and the next word starts on a head": lambda s, e, ok: (ok & (e - s > 1) & (e % WORD == 0) & (s % WORD > 0)
                                                                            & np.isin(e, s)).any(),
    "a run starts on lane 63": lambda s, e, ok: (ok & (s % WORD == 63) & (e - s > 1)).any(),
    "a run starts on lane 0": lambda s, e, ok: (ok & (s % WORD == 0) & (s > 0) & (e - s > 1) & (e % WORD > 0)).any(),
    "a run over exactly two words": lambda s, e, ok: (ok & (s % WORD == 0) & (e - s == 2 * WORD)).any(),
    "a run over three words, the middle one without a head": lambda s, e, ok: (ok & ((e - 1) // WORD - s // WORD == 2) & (s % WORD > 0)
                                                                         & (e % WORD > 0)).any(),
    "a run ends with the row in a word without a head": lambda s, e, ok: bool(ok[-1] and e[-1] % WORD > 0 and s[-1] // WORD < (e[-1] - 1) // WORD),
    "a run of 70000 crosses one tile border": lambda s, e, ok: (ok & (e - s == 70_000) & ((e - 1) // TILE - s // TILE == 1)).any(),
    "a run of 140000 covers a tile": lambda s, e, ok: (ok & (e - s == 140_000) & ((e - 1) // TILE - s // TILE == 2)).any(),
    "two runs of 70000 in neighbouring bins": lambda s, e, ok: (ok & (e - s == 70_000)).sum() == 2 and len(s) == 2,
}

LAYOUTS = {
    "run_inside_one_word": ("a run inside one word",),
    "run_ends_on_lane_63_before_a_head": ("a run ends on lane 63 and the next word starts on a head",),
    "run_starts_on_lane_63": ("a run starts on lane 63",),
    "run_starts_on_lane_0": ("a run starts on lane 0",),
    "run_over_exactly_two_words": ("a run over exactly two words",),
    "run_over_three_words": ("a run over three words, the middle one without a head",),
    "run_ends_with_the_row": ("a run ends with the row in a word without a head",),
    "run_of_70000": ("a run of 70000 crosses one tile border",),
    "run_of_140000": ("a run of 140000 covers a tile",),
    "two_big_runs_in_neighbouring_bins": ("two runs of 70000 in neighbouring bins",),
    "nan_between_two_equal_values": ("a NaN value between two equal values' runs",),
    # bin_unique's own layouts, held to their claims by uc.check_claims
    "one_sample_per_bin_in_one_word": uc.LAYOUTS["one_sample_per_bin_in_one_word"],
    "same_value_across_bin_borders": uc.LAYOUTS["same_value_across_bin_borders"],
    "bin_of_only_nans": uc.LAYOUTS["bin_of_only_nans"],
    "dropped_hold_the_longest_run": uc.LAYOUTS["dropped_hold_the_longest_run"],
    "signed_zeros": uc.LAYOUTS["signed_zeros"],
    "every_value_distinct": uc.LAYOUTS["every_value_distinct"],
    "one_value_only": uc.LAYOUTS["one_value_only"],
    "all_dropped": uc.LAYOUTS["all_dropped"],
}
BIG = ("run_of_70000", "run_of_140000", "two_big_runs_in_neighbouring_bins")


def weights_for(idx, v, wt, seed, signs="both"):
    """exactly summable weights of dtype `wt` in idx's shape; HEAVY[wt] times larger where the sample is dropped or its value NaN
    (a power of two that the type still holds exactly: 2^40, 2^15 for float16, 2^20 for int32)"""
    rng = np.random.default_rng(seed + 77)
    wt = np.dtype(wt)
    if wt == F64:
        w = xw.f64(rng, idx.shape, signs)
    elif wt == F32:
        w = xw.f32(rng, idx.shape, signs)
    elif wt == F16:
        w = (rng.integers(1024, 2048, idx.shape) / 2048.0 * np.where(rng.integers(0, 2, idx.shape), -1, 1)).astype(F16)
    else:
        w = rng.integers(-1000, 1001, idx.shape).astype(wt)
    heavy = (idx < 0) | np.isnan(np.broadcast_to(v, idx.shape).astype(F64))
    scaled = (w.astype(F64) * HEAVY[wt]).astype(wt)
    assert np.array_equal(scaled.astype(F64), w.astype(F64) * HEAVY[wt])  # (the type holds the heavy weights exactly)
    return np.where(heavy, scaled, w).astype(wt)


def case_data(case, cus):
    """(edges, the bin indices [n_rows, n_cols], the D sample arrays, the values, the weights) of a case"""
    if case["layout"]:
        edges = bc.edges_for(case["nbs"])
        idx, v = rc.from_runs(layout_runs(case["name"]), case["n_rows"], case["seed"], False)
        v = v.astype(case["vt"])
        xs = xc.emit(idx, edges, case["st"])
    else:
        edges, idx, xs, v = uc.case_data(case, cus)
    return edges, idx, xs, v, weights_for(idx, v, case["wt"], case["seed"])


def gpu_cases(cus):
    out = []
    for i, (name, claims) in enumerate(LAYOUTS.items()):
        n_cols = sum(n for _, _, n in layout_runs(name))
        # (float32 samples where a row of them is a whole number of 16 bytes: the sort's keys then come from the fast family)
        out.append(dict(name=name, nbs=[64] if name.startswith("one_sample") else [4], st=F32 if i % 2 and n_cols % 4 == 0 else F64, vt=np.dtype(F64),
                        wt=np.dtype(F64), n_rows=1 if name in BIG else 2, n_cols=n_cols, claims=claims, layout=True, inverse=i % 3 != 2,
                        seed=xc.seed_of("bin_weighted_unique", name)))
    for i, case in enumerate(c for c in uc.gpu_cases(cus) if not c["layout"]):  # column counts, value dtypes, bin counts
        out.append(dict(case, wt=np.dtype(WEIGHT_DTYPES[i % 4]), inverse=i % 3 != 1))
    return out


def check_claims(case, idx, v, w, cus):
    """AssertionError unless the case reaches what it claims and its weights are exactly summable"""
    n_bins = int(np.prod(case["nbs"]))
    xw.assert_summable(case["n_cols"], case["wt"] if np.dtype(case["wt"]) == F32 else F64)
    own = [c for c in case["claims"] if c in CLAIMS or c.startswith("a NaN value between")]
    theirs = [c for c in case["claims"] if c not in own]
    if theirs:
        uc.check_claims(dict(case, claims=theirs), idx, v, cus)
    for s, e, ok, ks, vs in _runs(idx, v, n_bins):
        for claim in own:
            if claim in CLAIMS:
                assert CLAIMS[claim](s, e, ok), (case["name"], claim)
            else:  # a NaN lies between two runs of one value
                nan = np.flatnonzero(np.isnan(vs) & (ks < n_bins))
                assert any(vs[:i][~np.isnan(vs[:i])][-1:].tolist() == vs[i:][~np.isnan(vs[i:])][:1].tolist() != [] for i in nan), (case["name"], claim)
    heavy = (idx < 0) | np.isnan(v.astype(F64))
    if heavy.any() and (~heavy).any():  # a sum that took a heavy weight in would be wrong in its leading bits, in every weight dtype
        big = np.abs(w[heavy].astype(F64))
        assert big[big > 0].min() > 100 * np.abs(w[~heavy].astype(F64)).max(), case["name"]
