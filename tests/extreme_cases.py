"""Inputs with a constructed answer, for the branches only load reaches (tests/test_gpu_extremes.py runs them,
tests/test_extreme_cases_cpu.py holds the construction to the oracle).  No GPU and no test functions here.

The answer is not computed from the samples: an integer bin index is chosen per sample (`indices`: -1 = dropped), the sample is
emitted as the midpoint of that bin's edges cast to the sample dtype (`emit`; dropped ones cycle through NaN, +inf, -inf, below
the first edge, above the last), and the expected histogram is np.bincount of the indices (`expected`).  Patterns:
  one     every sample of row r in bin HOT[(r + shift) % 4], HOT = [0, n_bins - 1, m, m + 1], m the even flat index nearest the
          middle (m and m + 1 are the two halves of one packed 16-bit counter word)
  pair    70 % of a row in its hot bin, 25 % in the other half of its word (hot ^ 1), 5 % uniform over all bins and the dropped
          kinds (15 of them dropped whatever the draw: every kind in every input), positions shuffled
  spread  bins uniform
`periodic_expected` is the closed form for samples that repeat a short pattern (the column chunks of the streaming launch).

The three host restatements at the end take their numbers from plan.describe() and say, the way the host does, whether a call
reached the branch it was built for."""
import functools
import re
import zlib

import numpy as np

import exact_weights as ew
from test_gpu_census import F32, F64, HOMES, _MIN_NB, _split_bins, edges_of

DROP_KINDS = 5   # NaN, +inf, -inf, below e[0], above e[-1]
CPU_COLS = 50_000  # the CPU file builds every case with at most this many columns
PACKED16_COLS = 200_003  # one workgroup per row: the hot half wraps three times (pattern one), twice with carries into its neighbour (pair)
PACKED16_ROWS = 3  # no home with more rows than this keeps its counts in a packed16 histogram
ROUTED_COLS = 6_000_011  # the hot partition of a routed call holds more than kAccBatch = 1024 chunks of 2^10 records
ACC_BATCH = 1024
PATTERNS = ("one", "pair", "spread")


def seed_of(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def hot_bins(n_bins):
    assert n_bins >= 4
    m = (n_bins // 2) & ~1
    return [0, n_bins - 1, m, m + 1]


def partner(hot, n_bins):
    """the other half of hot's counter word (the last bin of an odd bin count has none: its left neighbour)"""
    return hot ^ 1 if (hot ^ 1) < n_bins else hot - 1


@functools.lru_cache(maxsize=24)
def indices(pattern, n_rows, n_cols, n_bins, shift=0, seed=0):
    """[n_rows, n_cols] int32 flat bin indices, -1 = dropped (read-only: cases of one shape and bin count share it)"""
    hot = hot_bins(n_bins)
    rng = np.random.default_rng(seed)
    out = np.empty((n_rows, n_cols), np.int32)
    for r in range(n_rows):
        h = hot[(r + shift) % 4]
        row = out[r]
        if pattern == "one":
            row[:] = h
        elif pattern == "spread":
            row[:] = rng.integers(0, n_bins, n_cols, dtype=np.int32)
        elif pattern == "pair":
            a, b = int(0.70 * n_cols), int(0.25 * n_cols)
            row[:a] = h
            row[a:a + b] = partner(h, n_bins)
            row[a + b:] = np.maximum(rng.integers(-DROP_KINDS, n_bins, n_cols - a - b, dtype=np.int32), -1)
            row[a + b:a + b + 3 * DROP_KINDS] = -1  # (with 10^5 bins the draw above drops next to nothing: every kind once per input)
            rng.shuffle(row)
        else:
            raise ValueError(pattern)
    out.flags.writeable = False
    return out


def midpoints(e, dtype):
    e = np.asarray(e, F64)
    return (0.5 * (e[:-1] + e[1:])).astype(dtype)


def drop_values(e, dtype):
    assert np.dtype(dtype).kind == "f"
    return np.array([np.nan, np.inf, -np.inf, e[0] - 1.0, e[-1] + 1.0]).astype(dtype)


def emit(idx, edges, dtype):
    """the D sample arrays of `idx`: bin midpoints; the k-th dropped sample of the call carries dropped kind k % 5 in input
    (k // 5) % D and a countable value in the others"""
    nbs = [len(e) - 1 for e in edges]
    D = len(edges)
    flat = idx.reshape(-1)
    bad = np.flatnonzero(flat < 0)
    k = np.arange(bad.size)
    rest = np.maximum(flat, 0)  # (a dropped sample's other inputs: the midpoints of bin 0)
    sub = [None] * D
    for d in range(D - 1, 0, -1):  # the last input's bin is the fastest index
        rest, sub[d] = np.divmod(rest, np.int32(nbs[d]))
    sub[0] = rest
    xs = []
    for d, e in enumerate(edges):
        x = midpoints(e, dtype)[sub[d]]
        if bad.size:
            here = (k // DROP_KINDS) % D == d
            x[bad[here]] = drop_values(e, dtype)[k[here] % DROP_KINDS]
        xs.append(x.reshape(idx.shape))
    return xs


def emit_torch(idx, edges, dtype):
    """`emit` on a torch int32 tensor, on its device: the same values, bit for bit (tests/test_extreme_cases_cpu.py)"""
    import torch

    nbs = [len(e) - 1 for e in edges]
    D = len(edges)
    flat = idx.reshape(-1)
    bad = torch.nonzero(flat < 0).reshape(-1)
    k = torch.arange(bad.numel(), device=idx.device)
    rest = flat.clamp(min=0)
    sub = [None] * D
    for d in range(D - 1, 0, -1):
        rest, sub[d] = torch.div(rest, nbs[d], rounding_mode="floor"), rest % nbs[d]
    sub[0] = rest
    xs = []
    for d, e in enumerate(edges):
        x = torch.from_numpy(midpoints(e, dtype)).to(idx.device)[sub[d].long()]
        if bad.numel():
            here = (k // DROP_KINDS) % D == d
            x[bad[here]] = torch.from_numpy(drop_values(e, dtype)).to(idx.device)[k[here] % DROP_KINDS]
        xs.append(x.reshape(idx.shape))
    return xs


@functools.lru_cache(maxsize=12)
def weights_of(wt, signs, n_rows, n_cols, seed):
    """exactly summable weights of dtype WT[wt] (tests/exact_weights.py), read-only"""
    w = ew.make(WT[wt], signs=signs)(np.random.default_rng(seed), (n_rows, n_cols))
    w.flags.writeable = False
    return w


@functools.lru_cache(maxsize=64)
def _expected_of(idx_args, nbs, w_args):
    return expected(indices(*idx_args), list(nbs), None if w_args is None else weights_of(*w_args))


def expected(idx, nbs, w=None):
    """[n_rows, *nbs]: np.bincount of the indices per row, int64 counts or float64 sums of the float64 weights"""
    n_bins = int(np.prod(nbs))
    out = np.zeros((idx.shape[0], n_bins), np.int64 if w is None else F64)
    for r in range(idx.shape[0]):
        ok = idx[r] >= 0
        out[r] = np.bincount(idx[r][ok], weights=None if w is None else w[r][ok].astype(F64), minlength=n_bins)
    return out.reshape((idx.shape[0],) + tuple(nbs))


def one_values(edges, dtype, n_rows, shift=0):
    """pattern one without an index array: ([D, n_rows] the value every sample of row r has in input d, [n_rows] its flat bin)"""
    nbs = [len(e) - 1 for e in edges]
    hot = hot_bins(int(np.prod(nbs)))
    flat = np.array([hot[(r + shift) % 4] for r in range(n_rows)])
    sub = np.unravel_index(flat, nbs)
    return np.stack([midpoints(e, dtype)[sub[d]] for d, e in enumerate(edges)]), flat


def one_expected(flat, nbs, n_cols):
    out = np.zeros((len(flat), int(np.prod(nbs))), np.int64)
    out[np.arange(len(flat)), flat] = n_cols
    return out.reshape((len(flat),) + tuple(nbs))


def periodic_expected(n, bins_pat, n_bins, wpat=None):
    """samples i = 0 .. n-1 lie in bin bins_pat[i % len(bins_pat)] (-1: dropped) and weigh wpat[i % len(wpat)]: the histogram in
    closed form.  The periods are coprime; weights are multiples of 2^-24 and the sums are formed in integers."""
    ps = len(bins_pat)
    if wpat is None:
        out = np.zeros(n_bins, np.int64)
        for a, b in enumerate(bins_pat):
            if b >= 0:
                out[b] += (n - a + ps - 1) // ps
        return out
    pw = len(wpat)
    assert np.gcd(ps, pw) == 1
    num = [int(np.ldexp(float(v), 24)) for v in wpat]
    assert all(np.ldexp(float(k), -24) == float(v) for k, v in zip(num, wpat))
    acc = [0] * n_bins
    for r in range(ps * pw):
        if r < n and bins_pat[r % ps] >= 0:
            acc[bins_pat[r % ps]] += ((n - r + ps * pw - 1) // (ps * pw)) * num[r % pw]
    assert max(abs(a) for a in acc) < 1 << 53
    return np.array([np.ldexp(float(a), -24) for a in acc])


# ---------------------------------------------------------------------------------------------------------------------
# part 1: hot bins in every histogram home
# ---------------------------------------------------------------------------------------------------------------------
LADDER = ("d1_16000", "d1_16000_part", "d1_16000_3pass", "d1_16000_sliced")
HOT_HOMES = tuple(h for h in HOMES if not h.startswith("d1_")) + LADDER
HOT_KINDS = ("lin", "k3")
ST = {"f64": F64, "f32": F32}
WT = {"none": None, "f32": F32, "f64": F64}


def routed(home):
    return home.startswith("route") or home == "three_pass" or home.endswith("_part") or home.endswith("_3pass")


def hot_cases(home, st, wt):
    """the cases of one (home, sample dtype, weight dtype): inputs 1-3 x edge kinds x (pattern one with shift 0 — and 1 for a
    single row —, pattern pair) x (float64 weights: one sign, both signs)"""
    h = HOMES[home]
    per_d = h["bins"][0 if WT[wt] is not None else 1]
    if per_d is None or (h.get("only_st") is not None and ST[st] is not h["only_st"]):
        return
    n_rows, n_cols = h["shape"]
    if routed(home):
        n_cols = ROUTED_COLS
    for D in (1, 2, 3):
        if D not in per_d:
            continue
        nbs = _split_bins(per_d[D], D)
        for kind in HOT_KINDS:
            if min(nbs) < _MIN_NB[kind] or (h.get("only_kinds") is not None and kind not in h["only_kinds"]):
                continue
            if routed(home) and kind != "lin" and not home.startswith("d1_"):  # (6 * 10^6 samples per row and up to three inputs: one edge kind keeps a test function at a few seconds; the ladder has one input and keeps both)
                continue
            for signs in (("one", "both") if wt == "f64" else ("one",)):
                for pattern, shift in (("one", 0), ("one", 1), ("pair", 0)):
                    if shift and n_rows > 1:
                        continue
                    yield dict(home=home, st=st, wt=wt, signs=signs, D=D, kind=kind, nbs=nbs, shape=(n_rows, n_cols), pattern=pattern,
                               shift=shift, params=dict(h["params"]), lead=bool(h.get("lead")),
                               seed=seed_of(pattern, shift))


class Built:
    """a case built: edges, index array, weights (or None), the constructed expectation, the largest per-bin count; the samples
    on the host (`xs`) or, with `device`, emitted there as torch tensors (`xd`, `wd`)"""

    def __init__(self, case, n_cols=None, device=None, samples=True):
        n_rows, full = case["shape"]
        n_cols = full if n_cols is None else min(full, n_cols)
        nbs = tuple(case["nbs"])
        idx_args = (case["pattern"], n_rows, n_cols, int(np.prod(nbs)), case.get("shift", 0), case["seed"])
        w_args = None if WT[case["wt"]] is None else (case["wt"], case["signs"], n_rows, n_cols, case["seed"] + 1)
        self.case = case
        self.edges = case_edges(case)
        self.idx = indices(*idx_args)
        self.w = None if w_args is None else weights_of(*w_args)
        self.want = _expected_of(idx_args, nbs, w_args)
        self.top = int(_expected_of(idx_args, nbs, None).max())
        if not samples:
            return
        if device is None:
            self.xs = emit(self.idx, self.edges, ST[case["st"]])
        else:
            import torch

            self.xd = emit_torch(torch.from_numpy(self.idx.copy()).to(device), self.edges, ST[case["st"]])
            self.wd = None if self.w is None else torch.from_numpy(self.w.copy()).to(device)


def case_edges(case):
    lo, hi = case.get("range", (-4.0, 4.0))
    return [edges_of(case["kind"], nb, lo=lo, hi=hi, seed=case["seed"] % 1000 + d) for d, nb in enumerate(case["nbs"])]


# ---------------------------------------------------------------------------------------------------------------------
# part 2: 16-bit counters at their capacity (pattern one, closed form)
# ---------------------------------------------------------------------------------------------------------------------
def capacity_cases():
    for st in ("f32", "f64"):
        yield dict(name="rows1", st=st, kind="lin", nbs=[40], n_rows=258, shift=0, seed=1)
    for D in (1, 2):
        yield dict(name="flat_rows", st="f32", kind="lin", nbs=_split_bins({1: 50, 2: 90}[D], D), n_rows=4096, shift=0, seed=2)
    yield dict(name="lanes_shared", st="u8", kind="lin", nbs=[100], n_rows=3, shift=0, seed=3, range=(0.0, 200.0))
    yield dict(name="lanes_shared", st="f32", kind="lin", nbs=[20, 20], n_rows=3, shift=0, seed=4)
    yield dict(name="packed16_both_halves", st="f64", kind="lin", nbs=[50_000], n_rows=1, shift=0, seed=5)


CAP_ST = {"f32": F32, "f64": F64, "u8": np.uint8}
BOTH_HALVES_WANT = (65540, 65538)  # counts of the low-half and the high-half bin of both_halves_samples


def both_halves_samples(low, high, pad_to=8192):
    """[1, n] float64: 65535 samples of the high-half bin, 65535 of the low-half bin (both halves of the word at 0xFFFF), 5 more
    of the low half (the first wraps it and, through its carry, the high half), 3 more of the high half; every phase padded with
    NaN to a multiple of `pad_to`, so no two phases meet in one tile"""
    parts = []
    for value, n in ((high, 65535), (low, 65535), (low, 5), (high, 3)):
        parts += [np.full(n, value, F64), np.full((-n) % pad_to, np.nan)]
    return np.concatenate(parts)[None, :]


# ---------------------------------------------------------------------------------------------------------------------
# part 3: the list-full branch of the routing pass
# ---------------------------------------------------------------------------------------------------------------------
ROUTE_N = 20_000_003
ROUTE_VARIANTS = {  # name -> (sample dtype, weight dtype, signs, rows, plan parameters beside partition = 1, exchange = -1)
    "f64_counts": ("f64", "none", "one", 1, {}),
    "f64_w32": ("f64", "f32", "one", 1, {}),
    "f64_w64_packed": ("f64", "f64", "one", 1, {}),
    "f64_w64_both_signs": ("f64", "f64", "both", 1, {}),
    "f64_w64_exact_records": ("f64", "f64", "one", 1, {"records48": -1}),
    "f32_counts_spl8": ("f32", "none", "one", 1, {"route_spl": 8}),
    "f64_counts_3_rows": ("f64", "none", "one", 3, {}),
}


def route_case(variant, pattern, n_cols):
    st, wt, signs, rows, params = ROUTE_VARIANTS[variant]
    return dict(st=st, wt=wt, signs=signs, D=2, kind="lin", nbs=[1024, 1024], shape=(rows, n_cols), pattern=pattern, shift=0,
                params=dict(params, partition=1, exchange=-1), lead=False, seed=seed_of("route", pattern))


# ---------------------------------------------------------------------------------------------------------------------
# part 4: column chunks (a 7-element sample pattern, 11- and 13-element weight patterns)
# ---------------------------------------------------------------------------------------------------------------------
CHUNK_N = (1 << 31) + 12_345
CHUNK_BINS_PAT = [3, 0, -1, 4, 1, -1, 2]  # five bins once each (no bin holds 2 n / 7 > 2^29 samples) and two dropped kinds


def chunk_edges(dtype):
    """five bins; for uint8 samples the midpoints are integers and the range leaves room below and above"""
    return np.linspace(10.0, 60.0, 6) if np.dtype(dtype) == np.uint8 else np.linspace(-5.0, 5.0, 6)


def chunk_sample_pattern(dtype):
    e = chunk_edges(dtype)
    mids = midpoints(e, dtype)
    drops = np.array([3, 200], dtype) if np.dtype(dtype) == np.uint8 else np.array([np.nan, e[-1] + 1.0], dtype)
    out, k = [], 0
    for b in CHUNK_BINS_PAT:
        out.append(mids[b] if b >= 0 else drops[k % 2])
        k += b < 0
    return np.array(out, dtype)


def chunk_weight_pattern(period, seed):
    return ew.f32(np.random.default_rng(seed), (period,), "both")


# ---------------------------------------------------------------------------------------------------------------------
# what the host decides, restated from plan.describe()
# ---------------------------------------------------------------------------------------------------------------------
def field(desc, key):
    m = re.search(r"(?:^| )%s=(\S+)" % re.escape(key), desc)
    assert m, (key, desc)
    return m.group(1)


def per_wg_samples(desc, n_cols):
    """samples the one workgroup of a row sees in a streaming launch with segs = 1: whole tiles of block x vec x unroll"""
    assert int(field(desc, "segs")) == 1, desc
    tile = int(field(desc, "block")) * int(field(desc, "vec")) * int(field(desc, "unroll"))
    return -(-n_cols // tile) * tile


def route_chunks_per_wg(desc, n):
    """chunks a workgroup of the routing pass fills with its share of n samples; more than `block` do not fit its list"""
    chunk = int(field(desc, "chunk"))
    assert chunk & (chunk - 1) == 0, desc
    return (n // int(field(desc, "grid"))) >> (chunk.bit_length() - 1)


def lane_cols_per_seg(desc, n_cols):
    """columns per segment of a row-per-lane launch, from grid=RxC (C segments)"""
    _row_blocks, segs = field(desc, "grid").split("x")
    return -(-n_cols // int(segs))
