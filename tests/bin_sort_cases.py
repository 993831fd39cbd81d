"""The cases of tests/test_gpu_bin_sort.py: bin indices as tests/bin_order_cases.py builds them (tests/extreme_cases.emit turns
them into samples) and value arrays built from chosen keys.  Every case names the conditions it claims;
tests/test_bin_sort_cpu.py holds each case to them without a GPU, for the 256 compute units of an MI355X."""
import functools

import numpy as np

import bin_order_cases as bc
import bin_order_oracle as bo
import bin_sort_oracle as so
import extreme_cases as xc

F64, F32, F16 = np.float64, np.float32, np.float16
CUS = 256  # what the CPU file checks the claims for
REF_COLS = 4000  # a single row of a few thousand samples: several chunks
TWO_SLICES = 40_000  # more than 64 chunks of at least 512 positions
SIZES = [1, 63, 64, 65, 511, 512, 513]
VALUE_DTYPES = [np.float64, np.float32, np.float16, np.int64, np.int32, np.int16, np.int8, np.uint64, np.uint32, np.uint16, np.uint8,
                np.bool_]
BINS_1D = [1, 2, 255, 256, 257, 40959, 40960, 70000]
TUTORIAL_BINS = [279, 339]

# a float64 key none of whose digits, replaced by any byte, makes a NaN or an infinity: the top digits stay inside
# [0x0010..., 0xFF10...], the finite values
BASE_KEY = 0xC010203040506070


def values_of_keys(keys):
    """float64 values whose core.extrema_keys are `keys` (uint64)"""
    from xhistogram_amd import core

    return core._extrema_values(np.asarray(keys, np.uint64)).reshape(np.shape(keys))


@functools.lru_cache(maxsize=64)
def values(pattern, vt, n_rows, n_cols, seed=0, chunk=0):
    """[n_rows, n_cols] values of dtype vt (read-only)"""
    rng = np.random.default_rng(seed + 77)
    shape = (n_rows, n_cols)
    vt = np.dtype(vt)
    if pattern == "random":  # every kind of the dtype, with ties; floats carry NaN, both zeros and both infinities
        if vt.kind == "f":
            out = np.round(rng.standard_normal(shape) * 8, 1).astype(vt)
            kind = rng.random(shape)
            out[kind < 0.06] = np.nan
            out[(kind >= 0.06) & (kind < 0.08)] = 0.0
            out[(kind >= 0.08) & (kind < 0.10)] = -0.0
            out[(kind >= 0.10) & (kind < 0.11)] = np.inf
            out[(kind >= 0.11) & (kind < 0.12)] = -np.inf
        elif vt.kind == "b":
            out = rng.random(shape) < 0.5
        else:
            info = np.iinfo(vt)
            out = rng.integers(info.min, info.max, shape, dtype=vt, endpoint=True)
            out[rng.random(shape) < 0.3] = vt.type(info.max if vt.kind == "u" else -1)  # (ties)
    elif pattern == "equal":
        out = np.full(shape, 1.5, vt)
    elif pattern.startswith("digit_"):  # keys that differ in one 8-bit digit only
        k = int(pattern[6:])
        assert vt == np.dtype(F64)
        byte = rng.integers(0, 256, shape).astype(np.uint64)
        keys = (np.uint64(BASE_KEY) & ~(np.uint64(0xFF) << np.uint64(8 * k))) | (byte << np.uint64(8 * k))
        out = values_of_keys(keys)
    elif pattern == "special":  # both zeros, both infinities, subnormals, runs of NaN, negative and positive values mixed
        assert vt.kind == "f"
        tiny = np.finfo(vt).smallest_subnormal
        pool = np.array([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, 3 * tiny, np.finfo(vt).tiny / 2, -1.0, 1.0, -2.5, 2.5, np.nan], vt)
        out = pool[rng.integers(0, len(pool), shape)]
        for r in range(n_rows):
            for start in range(37 + 11 * r, n_cols, 700):
                out[r, start:start + 150] = np.nan
    elif pattern == "tie_run3":  # one value from the end of chunk 0 to the start of chunk 3, random values around it
        assert chunk > 0 and n_cols >= 3 * chunk + 17
        out = np.round(rng.standard_normal(shape) * 8, 1).astype(vt)
        out[:, chunk - 5:3 * chunk + 5] = vt.type(0.5)
    elif pattern == "big_tie":  # one value more than 65 535 times, a few others in between
        out = np.full(shape, 2.25, vt)
        at = np.arange(0, n_cols, 9973)
        out[:, at] = (np.arange(len(at)) - 3).astype(vt)
    elif pattern == "distinct64":  # in every digit, the 64 records of a step of the input hold 64 distinct values
        assert vt == np.dtype(F64)
        p = np.arange(n_cols, dtype=np.uint64)
        keys = np.zeros(n_cols, np.uint64)
        for k in range(8):
            byte = ((p % np.uint64(64)) * np.uint64(2 * k + 1) + p // np.uint64(64)) % np.uint64(256 if k < 7 else 64)
            if k == 7:
                byte = byte + np.uint64(0x40)
            keys |= byte << np.uint64(8 * k)
        out = np.broadcast_to(values_of_keys(keys), shape).copy()
    elif pattern == "alone":  # no two values of a row are equal
        out = np.stack([rng.permutation(n_cols) for _ in range(n_rows)]).astype(vt) - vt.type(n_cols // 2)
    else:
        raise ValueError(pattern)
    out = np.ascontiguousarray(out, vt)
    out.flags.writeable = False
    return out


def chunk_of(case, cus):
    return so.geometry(cus, case["n_rows"], case["n_cols"])["chunk"] if case["n_cols"] else 0


def case_data(case, cus):
    """(edges, the bin indices [n_rows, n_cols], the D sample arrays, the values)"""
    n_bins = int(np.prod(case["nbs"]))
    chunk = chunk_of(case, cus)
    idx = bc.indices(case["pattern"], case["n_rows"], case["n_cols"], n_bins, case["seed"])
    edges = bc.edges_for(case["nbs"])
    v = values(case["vpattern"], case["vt"], case["n_rows"], case["n_cols"], case["seed"], chunk if case["vpattern"] == "tie_run3" else 0)
    return edges, idx, xc.emit(idx, edges, case["st"]), v


def gpu_cases(cus):
    """the direct cases: name, bins per input, sample dtype, values dtype, shape, the patterns, and what the case claims"""
    out = []

    def add(name, nbs, st, vt, n_rows, n_cols, pattern, vpattern, *claims):
        out.append(dict(name=name, nbs=list(nbs), st=st, vt=np.dtype(vt), n_rows=n_rows, n_cols=n_cols, pattern=pattern, vpattern=vpattern,
                        claims=claims, seed=xc.seed_of("bin_sort", name)))

    for i, n in enumerate(SIZES):
        add("size_%d" % n, [100], F64 if i % 2 else F32, F32 if i % 2 else F64, 1 + 2 * (i % 2), n, "random", "random", "chunks=1")
    add("several_chunks_1row", [100], F64, F64, 1, REF_COLS, "random", "random", "several chunks")
    add("several_chunks_3rows", [100], F32, F32, 3, REF_COLS, "random", "random", "several chunks")
    add("two_slices", [100], F64, F32, 1, TWO_SLICES, "random", "random", "several chunks", "two slices")
    add("all_equal", [100], F64, F64, 2, REF_COLS, "random", "equal", "several chunks", "all values equal")
    for k in range(8):
        add("digit_%d" % k, [100], F64, F64, 2, REF_COLS, "random", "digit_%d" % k, "several chunks", "differs only in digit %d" % k)
    add("specials_f64", [100], F64, F64, 2, REF_COLS, "random", "special", "several chunks", "specials")
    add("specials_f32", [100], F32, F32, 2, REF_COLS, "random", "special", "several chunks", "specials")
    add("specials_f16", [100], F64, F16, 2, REF_COLS, "random", "special", "several chunks", "specials")
    add("tie_run_over_three_chunks", [3], F64, F64, 2, REF_COLS, "one", "tie_run3", "several chunks", "tie run crosses chunk borders")
    add("big_tie", [7], F64, F64, 1, 70_000, "one", "big_tie", "more than 65535 equal values in one bin")
    add("distinct_digits_per_step", [100], F64, F64, 2, 64 * 40, "random", "distinct64", "several chunks", "every lane a distinct digit")
    add("every_lane_alone", [5000], F64, F64, 2, 3000, "alone", "alone", "every sample alone")
    for vt in VALUE_DTYPES:
        name = so.DTYPE_NAME[np.dtype(vt)]
        add("values_%s" % name, [100], F64, vt, 3, 1000, "random", "random", "value_passes=%d" % so.value_passes(name))
    for nb in BINS_1D:
        add("bins_%d" % nb, [nb], F32 if nb % 2 else F64, F32, 2, 5000, "random", "random", "bin_passes=%d" % so.bin_passes(nb))
    add("tutorial_bins", TUTORIAL_BINS, F64, F64, 2, 5000, "random", "random", "bin_passes=3")
    add("all_dropped", [7], F32, F64, 2, 3000, "dropped", "random", "several chunks", "all dropped")
    add("one_bin", [7], F64, F32, 2, 3000, "one", "random", "several chunks", "one key only")
    return out


def check_claims(case, idx, v, cus):
    """AssertionError unless the case reaches what it claims (idx: its bin indices, v: its values)"""
    n_bins = int(np.prod(case["nbs"]))
    g = so.geometry(cus, case["n_rows"], case["n_cols"])
    key = bo.keys_of(idx, n_bins)
    vk = so.value_keys(v)
    name = so.DTYPE_NAME[case["vt"]]
    for claim in case["claims"]:
        if claim == "chunks=1":
            assert g["chunks"] == 1, (case["name"], g)
        elif claim == "several chunks":
            assert g["chunks"] >= 3, (case["name"], g)
        elif claim == "two slices":
            assert g["slices"] == 2 and g["chunks"] > so.SLICE and g["chunks"] % so.SLICE != 0, (case["name"], g)
        elif claim == "all values equal":
            assert len(np.unique(vk)) == 1
        elif claim.startswith("differs only in digit "):
            k = int(claim[-1])
            diff = np.bitwise_or.reduce((vk ^ vk.flat[0]).reshape(-1))
            assert int(diff) == 0xFF << (8 * k), (case["name"], hex(int(diff)))  # (every bit of the digit, and no other bit)
            assert not np.isnan(v).any() and np.isfinite(v).all()
        elif claim == "specials":
            f = v.astype(np.float64)
            tiny = np.finfo(v.dtype).tiny
            assert ((f == 0) & np.signbit(f)).any() and ((f == 0) & ~np.signbit(f)).any()
            assert (f == np.inf).any() and (f == -np.inf).any() and (f < 0).any() and (f > 0).any()
            assert ((np.abs(f) < tiny) & (f != 0)).any(), "no subnormal"
            for row in np.isnan(f):
                change = np.flatnonzero(np.diff(row.astype(np.int8)) != 0) + 1
                starts, ends = np.concatenate([[0], change]), np.concatenate([change, [len(row)]])
                runs = (ends - starts)[row[starts]]
                assert runs.max() >= 150 and (starts[row[starts]] // g["chunk"] != (ends[row[starts]] - 1) // g["chunk"]).any(), case["name"]
        elif claim == "tie run crosses chunk borders":
            for rk, rv in zip(key, vk):
                both = (np.diff(rk) != 0) | (np.diff(rv) != 0)
                change = np.flatnonzero(both) + 1
                starts, ends = np.concatenate([[0], change]), np.concatenate([change, [len(rk)]])
                assert ((ends - 1) // g["chunk"] - starts // g["chunk"]).max() >= 3, case["name"]  # (touches four chunks)
        elif claim == "more than 65535 equal values in one bin":
            pairs = np.stack([key[0].astype(np.uint64), vk[0]], 1)
            assert np.unique(pairs, axis=0, return_counts=True)[1].max() > 65535
        elif claim == "every lane a distinct digit":
            for row in vk:
                full = len(row) // 64 * 64
                for k in range(8):
                    steps = ((row[:full] >> np.uint64(8 * k)) & np.uint64(0xFF)).reshape(-1, 64)
                    assert all(len(set(s.tolist())) == 64 for s in steps), (case["name"], k)
        elif claim == "every sample alone":
            assert all(len(np.unique(r)) == len(r) for r in key) and all(len(np.unique(r)) == len(r) for r in vk)
        elif claim.startswith("value_passes="):
            assert so.value_passes(name) == int(claim[13:])
        elif claim.startswith("bin_passes="):
            assert so.bin_passes(n_bins) == int(claim[11:]), (case["name"], n_bins)
        elif claim == "one key only":
            assert len(np.unique(key)) == 1 and key.flat[0] < n_bins
        elif claim == "all dropped":
            assert (key == n_bins).all()
        else:
            raise AssertionError("unknown claim %r" % claim)
