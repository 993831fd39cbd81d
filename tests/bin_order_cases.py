"""The cases of tests/test_gpu_bin_order.py, built from chosen bin indices (tests/extreme_cases.emit turns them into samples:
bin midpoints, and NaN, +-inf and values outside the edges for the dropped ones).  Every case names the conditions it claims;
tests/test_bin_order_cpu.py holds each case to them without a GPU, for the 256 compute units of an MI355X."""
import functools

import numpy as np

import bin_order_oracle as bo
import extreme_cases as xc

F64, F32 = np.float64, np.float32
CUS = 256  # what the CPU file checks the claims for
REF_COLS = 4000  # a single row of a few thousand samples: several chunks in 100 bins
SIZE_BINS = 100


def base_chunk(cus):
    """the chunk of one row of REF_COLS samples in SIZE_BINS bins: the sizes around it are run as rows of their own"""
    return bo.geometry(cus, SIZE_BINS, 1, REF_COLS)["chunk"]


def size_list(cus):
    c = base_chunk(cus)
    nb1 = SIZE_BINS + 1
    return [1, 63, 64, 65, c - 1, c, c + 1, 3 * c + 17, 4 * nb1 - 1, 4 * nb1]  # (the last two: one chunk, then two)


@functools.lru_cache(maxsize=64)
def indices(pattern, n_rows, n_cols, n_bins, seed=0, chunk=0):
    """[n_rows, n_cols] int32 bin indices, -1: dropped (read-only)"""
    rng = np.random.default_rng(seed)
    if pattern == "random":  # every bin and a tenth dropped
        out = rng.integers(0, n_bins, (n_rows, n_cols)).astype(np.int32)
        out[rng.random((n_rows, n_cols)) < 0.1] = -1
    elif pattern == "one":
        out = np.full((n_rows, n_cols), n_bins // 2, np.int32)
    elif pattern == "dropped":
        out = np.full((n_rows, n_cols), -1, np.int32)
    elif pattern == "distinct64":  # the 64 positions of a wave step hold 64 distinct keys, rotated from step to step and row to row
        assert n_bins >= 64
        p = np.arange(n_cols)
        out = np.stack([((p % 64) + p // 64 + r) % 64 + (n_bins - 64) * ((p // 64) % 2) for r in range(n_rows)]).astype(np.int32)
    elif pattern == "alone":  # no two samples of a row share a bin
        assert n_bins >= n_cols
        out = np.stack([rng.permutation(n_bins)[:n_cols] for _ in range(n_rows)]).astype(np.int32)
    elif pattern == "run3":  # one key from the end of chunk 0 to the start of chunk 3, random keys around it
        assert chunk > 0 and n_cols >= 3 * chunk + 17
        out = rng.integers(0, n_bins, (n_rows, n_cols)).astype(np.int32)
        out[rng.random((n_rows, n_cols)) < 0.1] = -1
        out[:, chunk - 5:3 * chunk + 5] = n_bins - 1
    elif pattern == "big_run":  # one key more than 65 535 times, a few others in between
        out = np.full((n_rows, n_cols), 12345 % n_bins, np.int32)
        at = np.arange(0, n_cols, 9973)
        out[:, at] = np.arange(len(at), dtype=np.int32) % n_bins
        out[:, 0] = -1
    else:
        raise ValueError(pattern)
    out.flags.writeable = False
    return out


def edges_for(nbs):
    return [np.linspace(-4.0, 4.0, nb + 1) for nb in nbs]


def case_data(case, cus):
    """(edges, the bin indices [n_rows, n_cols], the D sample arrays)"""
    n_bins = int(np.prod(case["nbs"]))
    chunk = bo.geometry(cus, n_bins, case["n_rows"], case["n_cols"])["chunk"]
    idx = indices(case["pattern"], case["n_rows"], case["n_cols"], n_bins, case["seed"], chunk if case["pattern"] == "run3" else 0)
    edges = edges_for(case["nbs"])
    return edges, idx, xc.emit(idx, edges, case["st"])


def gpu_cases(cus):
    """the direct cases: name, bins per input, sample dtype, shape, pattern, and what the case claims to reach"""
    out = []

    def add(name, nbs, st, n_rows, n_cols, pattern, *claims):
        out.append(dict(name=name, nbs=list(nbs), st=st, n_rows=n_rows, n_cols=n_cols, pattern=pattern, claims=claims,
                        seed=xc.seed_of("bin_order", name)))

    for i, n in enumerate(size_list(cus)):
        add("size_%d" % n, [SIZE_BINS], F64 if i % 2 else F32, 1 + 2 * (i % 2), n, "random")
    add("several_chunks_1row", [SIZE_BINS], F64, 1, REF_COLS, "random", "several chunks")
    add("several_chunks_3rows", [SIZE_BINS], F32, 3, REF_COLS, "random", "several chunks")
    add("run_over_three_chunks", [SIZE_BINS], F64, 2, REF_COLS, "run3", "several chunks", "run crosses chunk borders")
    for nb, bits in ((1, 1), (2, 2), (63, 6), (64, 7), (65, 7)):
        add("bins_%d" % nb, [nb], F32 if nb % 2 else F64, 3, 1000, "random", "bits=%d" % bits)
    add("distinct_keys_per_step", [64], F64, 2, 64 * 40, "distinct64", "several chunks", "every lane a distinct key")
    add("distinct_keys_100_bins", [100], F32, 2, 64 * 40 + 7, "distinct64", "several chunks", "every lane a distinct key")
    add("several_slices", [3], F64, 2, 64 * 150 + 13, "random", "several chunks", "several slices")
    add("slice_units_beyond_the_grid", [1], F32, bo.SLICE_GRID + 1, 100, "random", "units beyond the slice grid")
    add("slices_of_many_tiles", [700], F64, 3, 20_000, "random", "several chunks", "several tiles")
    add("one_bin", [7], F64, 2, 3000, "one", "several chunks", "one key only")
    add("all_dropped", [7], F32, 2, 3000, "dropped", "several chunks", "all dropped")
    add("alone_in_its_bin", [5000], F64, 2, 3000, "alone", "every sample alone")
    add("last_bins_of_4_waves", [bo.LDS_MAX // 16 - 1], F64, 2, 5000, "random", "waves=4")
    add("first_bins_of_2_waves", [bo.LDS_MAX // 16], F32, 2, 5000, "random", "waves=2")
    add("first_bins_of_1_wave", [bo.LDS_MAX // 8], F64, 2, 5000, "random", "waves=1")
    add("lds_bound", [bo.MAX_BINS], F32, 2, 5000, "random", "waves=1", "lds full")
    add("wide_counter", [bo.LDS_MAX // 8 - 1], F64, 1, 70_000, "big_run", "waves=2", "more than 65535 of one key in one chunk")
    add("two_inputs", [9, 11], F64, 3, REF_COLS, "random", "several chunks")
    add("two_inputs_f32", [9, 11], F32, 1, 1000, "random")
    return out


def check_claims(case, idx, cus):
    """AssertionError unless the case reaches what it claims (idx: its bin indices)"""
    n_bins = int(np.prod(case["nbs"]))
    g = bo.geometry(cus, n_bins, case["n_rows"], case["n_cols"])
    key = bo.keys_of(idx, n_bins)
    for claim in case["claims"]:
        if claim == "several chunks":
            assert g["chunks"] >= 3, (case["name"], g)
        elif claim == "several slices":
            slices, _ = bo.slice_units(cus, n_bins, case["n_rows"], case["n_cols"])
            assert slices >= 3 and g["chunks"] % bo.SLICE != 0, (case["name"], g)  # (the last slice is ragged)
        elif claim == "units beyond the slice grid":
            assert g["chunks"] > 1 and bo.slice_units(cus, n_bins, case["n_rows"], case["n_cols"])[1] > bo.SLICE_GRID, (case["name"], g)
        elif claim == "several tiles":
            assert n_bins + 1 > 2 * 256 and (n_bins + 1) % 256 != 0
        elif claim == "run crosses chunk borders":
            for row in key:
                change = np.flatnonzero(np.diff(row) != 0) + 1
                starts, ends = np.concatenate([[0], change]), np.concatenate([change, [len(row)]])
                assert ((ends - 1) // g["chunk"] - starts // g["chunk"]).max() >= 3, case["name"]  # (touches four chunks: spans three borders)
        elif claim.startswith("bits="):
            assert g["bits"] == int(claim[5:]), (case["name"], g)
        elif claim.startswith("waves="):
            assert g["waves"] == int(claim[6:]), (case["name"], g)
        elif claim == "lds full":
            assert g["lds_bytes"] == bo.LDS_MAX and (n_bins + 2) * 4 > bo.LDS_MAX
        elif claim == "every lane a distinct key":
            for row in key:
                full = len(row) // 64 * 64
                steps = row[:full].reshape(-1, 64)
                assert all(len(set(s.tolist())) == 64 for s in steps), case["name"]
        elif claim == "one key only":
            assert len(np.unique(key)) == 1 and key.flat[0] < n_bins
        elif claim == "all dropped":
            assert (key == n_bins).all()
        elif claim == "every sample alone":
            assert n_bins >= case["n_cols"] and all(len(np.unique(row)) == len(row) for row in key)
        elif claim == "more than 65535 of one key in one chunk":
            assert g["chunks"] == 1 and np.bincount(key[0]).max() > 65535
        else:
            raise AssertionError("unknown claim %r" % claim)
