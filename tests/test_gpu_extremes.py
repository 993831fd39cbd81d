"""What only load reaches: hot bins in every histogram home, 16-bit counters at their capacity, the list-full branch of the
routing pass, the column chunks of the streaming launch.

The census (tests/test_gpu_census.py) chooses inputs to pick a kernel and spreads its samples evenly; the branches here are
chosen by how many samples there are or how concentrated they lie.  Every input is a legal call whose answer is constructed
(tests/extreme_cases.py: samples emitted from bin indices, the expectation np.bincount of the indices or a closed form;
tests/test_extreme_cases_cpu.py holds that construction to the oracle).  Every comparison is exact: counts equal, weighted sums
of exactly summable weights (tests/exact_weights.py) bit for bit.  Each case asserts from plan.describe() that it reached the
branch it was built for, so a case that falls to another family fails.

Two things differ from a plain reading of the plan's defaults, both so that the branch is really reached:
  - a packed16 histogram wraps a 16-bit half only when ONE workgroup sees more than 65535 samples of a bin; the default grid gives a
    row of 200 003 samples ~70 workgroups, so the packed16 cases run with grid_blocks = rows (one workgroup per row, asserted);
  - both halves of a packed word sitting at 0xFFFF when the low one wraps is a coincidence under any shuffled input: one test lays
    the samples out in that order for a single wavefront (block_threads = 64, grid_blocks = 1)."""
import numpy as np
import pytest

import exact_weights as ew
import extreme_cases as xc
from test_gpu_census import F32, F64, _dev, _dev_lead, _fresh, xh  # noqa: F401  (xh: the module fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _call(core, xd, edges, wd, params, times=1):
    """the call through the C ABI on resident data, `times` times on one plan state: [(result as numpy, description), ...]"""
    dts = [core._np_dtype_of(t) for t in xd]
    cmp_domain, conv, _ = core._compare_domain(dts, edges)
    plan = _fresh(core._get_plan(conv, cmp_domain, 0))
    out = []
    try:
        for k, v in params.items():
            plan.set_param(k, v)
        for _ in range(times):
            got = core._bincount_2d_vectorized(*xd, bins=edges, weights=wd)
            torch.cuda.synchronize()
            out.append((got.cpu().numpy(), plan.describe()))
    finally:
        _fresh(plan)  # (also forgets "both signs": later modules still select the packed kernels)
    return out


def _same(got, want, weighted, what):
    if weighted:
        ew.assert_bits_equal(got, want, what)
    else:
        assert got.dtype.kind in "iu" and got.shape == want.shape, (got.dtype, got.shape, want.shape, what)
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        assert bad.size == 0, "%d bins differ (%s); first at flat %d: %d != %d" % (bad.size, what, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


def _free_gb():
    free, _total = torch.cuda.mem_get_info(0)
    return free / 2**30


# ---------------------------------------------------------------------------------------------------------------------
# 1. hot bins in every histogram home
# ---------------------------------------------------------------------------------------------------------------------
def _lead(t):
    """a [rows, cols] tensor that is already on the GPU, laid out as test_gpu_census._dev_lead lays a host array out: the rows are
    the contiguous direction (strides (1, rows)); test_lead_layout_is_dev_leads holds the two together"""
    return t.T.contiguous().T


def test_lead_layout_is_dev_leads(xh):
    a = np.arange(21, dtype=np.float32).reshape(3, 7)
    mine, theirs = _lead(_dev(a)), _dev_lead(a)
    assert mine.shape == theirs.shape and mine.stride() == theirs.stride() == (1, 3) and torch.equal(mine, theirs)
    t, = _rows_of_one_value(a[:, :1].T, 5, lead=True)
    assert t.shape == (3, 5) and t.stride() == (1, 3) and torch.equal(t, _dev_lead(np.repeat(a[:, :1], 5, axis=1)))


def _home_marker(case, desc):
    """what the description of a call that stayed in the case's home shows, in the home's own parameters — and, for the
    three-edges-per-bucket edges (k3), what it shows where those edges move a call out of the home by the library's own rules:
      - 1-D tables of 16 000+ k3 edges do not fit the LDS next to a histogram (d1_16000*: hist=global, but hist=lds for float32 counts,
        whose tables are half as large), and 40 000+ of them do not fit it at all: the generic family reads them through the L2
        (packed16, sliced and global_big with one input: family=generic hist=global);
      - bin slices take the one- and two-edge scans and the arithmetic digitize only (choose_slices): sliced on k3 edges counts
        behind memory-side atomics, slices=1;
      - hist_flat_rows has its three-edge scan for one input only (xhist_pick_flat.hip): two inputs take the row-streaming kernels.
    The ladder homes d1_16000* sit below the border they were made for: 16 000 bins on np.linspace edges fit the LDS, so none of
    them partitions or slices, whatever its parameters ask for; on k3 edges the histogram leaves the LDS and d1_16000_part and
    d1_16000_3pass do partition (the other two count behind memory-side atomics: slices need a one- or two-edge scan).  hist_flat_rows takes one or two inputs, never three."""
    home, D, k3, weighted = case["home"], case["D"], case["kind"] == "k3", case["wt"] != "none"
    fam, hist = xc.field(desc, "family"), xc.field(desc, "hist")
    if home.startswith("d1_16000"):
        want = "lds" if not k3 or (not weighted and case["st"] == "f32") else "global"
        if want == "global" and home in ("d1_16000_part", "d1_16000_3pass"):  # beyond the LDS, and asked to partition
            # (d1_16000_part: one routing pass only where the tables fit the LDS next to its sort buffers and the edges of the
            # case scan with at most two per bucket, execute_partitioned_fused; else count + prefix + scatter, like d1_16000_3pass)
            return fam == "fast" and hist == "partitioned" and (home == "d1_16000_part" or "route=fused" not in desc)
        return fam == "fast" and hist == want and int(xc.field(desc, "slices")) == 1
    if home in ("lds", "lds_many_copies"):
        return fam == "fast" and hist == "lds"
    if home == "packed16":
        return (fam, hist) == (("generic", "global") if k3 and D == 1 else ("fast", "packed16"))
    if home in ("global", "global_big"):
        return hist == "global" and fam == ("generic" if k3 and D == 1 and home == "global_big" else "fast")
    if home == "sliced":
        if k3:
            return hist == "global" and int(xc.field(desc, "slices")) == 1 and fam == ("generic" if D == 1 else "fast")
        return fam == "fast" and int(xc.field(desc, "slices")) > 1 and hist == ("lds" if weighted else "packed16")
    if home.startswith("route_rows"):
        return "route=fused" in desc and int(xc.field(desc, "rows_per_pass")) == case["shape"][0]
    if home.startswith("route"):
        return "route=fused" in desc and int(xc.field(desc, "rows_per_pass")) == 1
    if home == "three_pass":
        return hist == "partitioned" and "route=fused" not in desc
    if home.startswith("lanes"):
        return fam == "lanes"
    if home == "flat_rows":
        if D == 1 or (D == 2 and not k3):
            return fam == "flat_rows" and hist == ("lds" if weighted else "lds16")
        return fam == "fast" and hist == "lds"
    assert home == "long_rows_f32", home
    return fam == "fast" and hist == "lds" and "unroll=8" in desc


PACKED_RECORD_HOMES = ("route", "route_rows", "route_spl4", "route_rows_spl4")  # float64 weights travel as packed 8-byte records


def _run_hot(core, case):
    b = xc.Built(case, device="cuda")
    put = _lead if case["lead"] else (lambda t: t)
    weighted = b.w is not None
    if weighted:
        ew.assert_summable(b.top, b.w.dtype)
    both = weighted and case["wt"] == "f64" and case["signs"] == "both"
    runs = _call(core, [put(x) for x in b.xd], b.edges, put(b.wd) if weighted else None, case["params"], times=2 if both else 1)
    got, desc = runs[0]
    what = "%r %s" % ({k: case[k] for k in ("home", "st", "wt", "signs", "D", "kind", "pattern", "shift", "shape")}, desc)
    assert _home_marker(case, desc), "not the home's marker: " + what
    _same(got, b.want, weighted, what)
    if "route=fused" in desc and xc.routed(case["home"]):
        # the hot partition holds several batches of kAccBatch chunks for part_accumulate_chunks
        assert b.top // int(xc.field(desc, "chunk")) > xc.ACC_BATCH, what
    if case["home"] in PACKED_RECORD_HOMES and case["wt"] == "f64":
        assert "records=packed48" in desc, what  # (a plan fresh of hints starts with packed records)
    if both and "records=packed48" in desc:
        # the packed attempt met both signs and the exact records redid the call; the next call goes straight to them
        got2, desc2 = runs[1]
        assert "records=u16+f64" in desc2, desc2
        _same(got2, b.want, True, "second call " + what)
    if "hist=packed16" in desc and case["shape"][1] != xc.PACKED16_COLS:
        n_rows = case["shape"][0]
        assert n_rows <= xc.PACKED16_ROWS, what  # (tests/test_extreme_cases_cpu.py builds the longer row for these)
        long = dict(case, shape=(n_rows, xc.PACKED16_COLS), params=dict(case["params"], grid_blocks=n_rows))
        desc = _run_hot(core, long)
        assert "hist=packed16" in desc and "grid=%d segs=1 " % n_rows in desc, desc
    return desc


# (every home x sample dtype x weight dtype that has a case: packed16 and the long rows count only, long_rows_f32 is float32 only)
_HOT = [(h, s, w) for h in xc.HOT_HOMES for s in ("f64", "f32") for w in ("none", "f32", "f64") if next(xc.hot_cases(h, s, w), None) is not None]


@pytest.mark.parametrize("home,st,wt", _HOT, ids=["-".join(t) for t in _HOT])
def test_hot_bins_in_every_home(xh, home, st, wt):
    """every sample of a row in one bin (first, last, both halves of the middle packed word), and 70 % / 25 % in the two halves
    of one word: 1-3 inputs, np.linspace and three-edges-per-bucket edges, counts / float32 / float64 weights (one sign and
    both), in the home's own parameters; every case is held to its home's marker (_home_marker).  The routed homes run 6 000 011
    samples per row, on np.linspace edges only except the two of the ladder, which have one input."""
    for case in xc.hot_cases(home, st, wt):
        _run_hot(xh, case)


# ---------------------------------------------------------------------------------------------------------------------
# 2. 16-bit counters at their capacity
# ---------------------------------------------------------------------------------------------------------------------
def _cap_case(name, st=None, D=None):
    for c in xc.capacity_cases():
        if c["name"] == name and (st is None or c["st"] == st) and (D is None or len(c["nbs"]) == D):
            return c
    raise KeyError((name, st, D))


def _rows_of_one_value(vals, n_cols, lead=False):
    """[n_rows, n_cols] on the GPU per input, every sample of row r = vals[d, r]; lead: the rows are the contiguous direction"""
    out = []
    for v in vals:
        t = torch.from_numpy(np.ascontiguousarray(v)).cuda()
        out.append(_lead(t[:, None].expand(len(v), n_cols)) if lead else t[:, None].expand(len(v), n_cols).contiguous())
    return out


@pytest.mark.parametrize("st", ["f32", "f64"])
def test_rows1_counters_at_65535(xh, st):
    """hist_lanes_rows1 (the fused load-transpose-count kernel): 258 rows of 65535 samples, each row in one bin — every uint16
    counter that is used ends at 0xFFFF, both halves of a word; one column more and another kernel takes the call"""
    c = _cap_case("rows1", st)
    edges = xc.case_edges(c)
    vals, flat = xc.one_values(edges, xc.CAP_ST[st], c["n_rows"])
    for n_cols in (65535, 65536):
        (got, desc), = _call(xh, _rows_of_one_value(vals, n_cols), edges, None, {"lanes": 1})
        if n_cols == 65535:
            assert "family=lanes" in desc and "hist=lds16 " in desc and "transpose=fused" in desc, desc
        else:  # a scratch transpose, then hist_lanes with uint16 counter columns per lane, the columns in segments
            assert "family=lanes" in desc and "hist=lds16 " in desc and "transpose=1 " in desc, desc
            assert xc.lane_cols_per_seg(desc, n_cols) <= 65535, desc
        _same(got, xc.one_expected(flat, c["nbs"], n_cols), False, desc)


@pytest.mark.parametrize("D", [1, 2])
def test_flat_rows_counters_at_65535(xh, D):
    """hist_flat_rows with uint16 counters: 4096 rows of 65535 float32 samples (one input, two inputs), each row in one bin"""
    c = _cap_case("flat_rows", D=D)
    edges = xc.case_edges(c)
    vals, flat = xc.one_values(edges, F32, c["n_rows"])
    for n_cols in (65535, 65536):
        (got, desc), = _call(xh, _rows_of_one_value(vals, n_cols), edges, None, {"flat_rows": 1})
        if n_cols == 65535:
            assert "family=flat_rows" in desc and "hist=lds16" in desc, desc
        else:  # the row-streaming kernels, uint32 counters in LDS
            assert "family=fast " in desc and "hist=lds " in desc, desc
        _same(got, xc.one_expected(flat, c["nbs"], n_cols), False, desc)
        torch.cuda.empty_cache()


@pytest.mark.parametrize("D", [1, 2])
def test_lanes_shared_counters_at_65535(xh, D):
    """hist_lanes with a counter column per row shared by the row's lane groups, uint16 two rows per word: 3 contiguous rows (the
    fourth lane of a group shadows the third row into the other half of its word), as many column segments as the chip's CU
    count asks for, 65535 columns each — a whole segment of a row in one half-word.  One column more: cols_per_seg is 65536
    and the family refuses."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    col_segs = min(cus * 8 * 2, 65535)  # plan_lane_columns: one row block, 8 workgroups per CU by LDS, twice the chip
    n_cols = col_segs * 65535
    c = _cap_case("lanes_shared", D=D)
    edges = xc.case_edges(c)
    sts = ["u8", "f32"] if D == 1 else ["f32"]
    for st in sts:
        vals, flat = xc.one_values(edges, xc.CAP_ST[st], 3)
        xd = _rows_of_one_value(vals, n_cols + 1, lead=True)
        (got, desc), = _call(xh, [x[:, :n_cols] for x in xd], edges, None, {})
        if "family=lanes" not in desc and st != sts[-1]:
            del xd
            torch.cuda.empty_cache()
            continue  # (no small-dtype lane kernel for this shape: float32)
        print("%s: %d CUs, %d columns, cols_per_seg %d: %s" % (st, cus, n_cols, xc.lane_cols_per_seg(desc, n_cols) if "family=lanes" in desc else -1, desc))
        assert "family=lanes" in desc and "hist=lds16(shared)" in desc, desc
        assert xc.field(desc, "grid") == "1x%d" % col_segs and xc.lane_cols_per_seg(desc, n_cols) == 65535, desc
        _same(got, xc.one_expected(flat, c["nbs"], n_cols), False, desc)
        (got, desc), = _call(xh, xd, edges, None, {})
        assert "family=fast " in desc and "hist=lds " in desc, desc  # the rows gathered into dense scratch, then the row-streaming kernels
        _same(got, xc.one_expected(flat, c["nbs"], n_cols + 1), False, desc)
        del xd
        torch.cuda.empty_cache()
        break


def test_packed16_both_halves_wrap_together(xh):
    """the packed16 histogram of the streaming kernels: the high half of a word is brought to 0xFFFF, then the low half, then
    the low half wraps — its carry wraps the high half too, and the lane that saw both books both lost 2^16.  One wavefront
    (block_threads = 64, one workgroup) takes its tiles in order; every phase — the samples that wrap the low half and the
    high-half samples after them too — is padded with dropped samples to a multiple of 8192, more than any tile of 64 lanes,
    so nothing rests on the order in which the lanes of one instruction are served."""
    c = _cap_case("packed16_both_halves")
    edges = xc.case_edges(c)
    mids = xc.midpoints(edges[0], F64)
    m = xc.hot_bins(c["nbs"][0])[2]
    x = xc.both_halves_samples(mids[m], mids[m + 1])
    want = np.zeros((1, c["nbs"][0]), np.int64)
    want[0, m], want[0, m + 1] = xc.BOTH_HALVES_WANT
    (got, desc), = _call(xh, [_dev(x)], edges, None, {"grid_blocks": 1, "block_threads": 64})
    assert "hist=packed16" in desc and "block=64 " in desc and "grid=1 segs=1 " in desc, desc
    _same(got, want, False, desc)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the list-full branch of the routing pass
# ---------------------------------------------------------------------------------------------------------------------
_ROUTE_INPUTS = {}


@pytest.fixture(scope="module")
def route_inputs():
    """samples on the GPU and their index arrays, shared by the variants of one (sample dtype, rows, pattern)"""
    yield _ROUTE_INPUTS
    _ROUTE_INPUTS.clear()
    torch.cuda.empty_cache()


def _route_n_cols(rows):
    """columns per row such that the routing pass sees at least ROUTE_N samples"""
    return -(-xc.ROUTE_N // rows)


@pytest.mark.parametrize("pattern", ["spread", "pair"])
@pytest.mark.parametrize("variant", list(xc.ROUTE_VARIANTS))
def test_route_list_full(xh, route_inputs, variant, pattern):
    """one workgroup of the routing pass (route_grid = 1; 2 with twice the samples) fills more chunks than its list in LDS holds
    and files the rest straight into the partitions' lists; then one accumulating workgroup (acc_grid = 1) walks every
    partition.  1024 x 1024 np.linspace bins, the classic passes (exchange = -1)."""
    st, wt, signs, rows, _params = xc.ROUTE_VARIANTS[variant]
    n1 = _route_n_cols(rows)
    case = xc.route_case(variant, pattern, 2 * n1)
    key = (st, rows, pattern)
    if key not in route_inputs:
        route_inputs[key] = xc.Built(dict(case, wt="none"), device="cuda").xd
    xd = route_inputs[key]
    b = xc.Built(case, samples=False)
    idx, edges, w = b.idx, b.edges, b.w
    wd = None if w is None else torch.from_numpy(w.copy()).cuda()
    if w is not None:
        ew.assert_summable(b.top, w.dtype)  # (the largest bin of all 2 n1 columns: a bound for the first n1 too)
    wants = {n1: xc.expected(idx[:, :n1], case["nbs"], None if w is None else w[:, :n1]), 2 * n1: b.want}
    for n_cols, more in ((n1, {"route_grid": 1}), (2 * n1, {"route_grid": 2}), (n1, {"route_grid": 1, "acc_grid": 1})):
        want = wants[n_cols]
        twice = variant == "f64_w64_both_signs"
        runs = _call(xh, [x[:, :n_cols] for x in xd], edges, None if wd is None else wd[:, :n_cols], dict(case["params"], **more), times=2 if twice else 1)
        got, desc = runs[0]
        if twice:  # the packed attempt is discarded inside the first call; the second goes straight to the exact records
            assert "records=packed48" in desc and "records=u16+f64" in runs[1][1], (desc, runs[1][1])
            assert xc.route_chunks_per_wg(runs[1][1], rows * n_cols) > int(xc.field(runs[1][1], "block")), runs[1][1]
            _same(runs[1][0], wants[n_cols], True, "second call %s %s %r %s" % (variant, pattern, more, runs[1][1]))
        assert "route=fused" in desc and "exchange=no" in desc and int(xc.field(desc, "grid")) == more["route_grid"], desc
        assert "rows_per_pass=%d " % rows in desc, desc
        if "acc_grid" in more:
            assert int(xc.field(desc, "acc_grid")) == 1, desc
        if variant == "f32_counts_spl8":
            assert "tile=8192 " in desc, desc
        if variant == "f64_w64_packed":
            assert "records=packed48" in desc, desc
        if variant == "f64_w64_exact_records":
            assert "records=u16+f64" in desc, desc
        # the host's own condition for the branch: more chunks per workgroup than its list holds
        print("%s %s %r: %d chunks of %s per workgroup, block %s" % (variant, pattern, more, xc.route_chunks_per_wg(desc, rows * n_cols), xc.field(desc, "chunk"), xc.field(desc, "block")))
        assert xc.route_chunks_per_wg(desc, rows * n_cols) > int(xc.field(desc, "block")), desc
        _same(got, want, w is not None, "%s %s %r %s" % (variant, pattern, more, desc))


# ---------------------------------------------------------------------------------------------------------------------
# 4. column chunks of the streaming launch
# ---------------------------------------------------------------------------------------------------------------------
def _periodic(pat, n):
    t = torch.from_numpy(np.ascontiguousarray(pat)).cuda()
    return t.repeat((n + len(pat) - 1) // len(pat))[:n][None, :]


def _chunk_plan(core, x, edges):
    cmp_domain, conv, _ = core._compare_domain([core._np_dtype_of(x)], edges)
    return core._get_plan(conv, cmp_domain, 0)


def _assert_chunked(desc, n):
    print("per_wg_samples %d (2^31 = %d): %s" % (xc.per_wg_samples(desc, n) if "segs=1 " in desc else -1, 2**31, desc))
    assert "grid=1 segs=1 " in desc and xc.per_wg_samples(desc, n) >= 2**31, desc


def test_column_chunks_counts(xh):
    """one workgroup would see 2^31 + 12 345 samples: the columns are cut into launches, each sample pointer advanced by c0.
    Samples repeat a 7-element pattern that no chunk is a multiple of."""
    n = xc.CHUNK_N
    want = xc.periodic_expected(n, xc.CHUNK_BINS_PAT, 5)[None, :]
    for dt in (np.uint8, F32):
        if _free_gb() < n * np.dtype(dt).itemsize / 2**30 + 8:
            pytest.skip("needs %d GB of free device memory" % (n * np.dtype(dt).itemsize / 2**30 + 8))
        x = _periodic(xc.chunk_sample_pattern(dt), n)
        edges = [xc.chunk_edges(dt)]
        (got, desc), = _call(xh, [x], edges, None, {"grid_blocks": 1})
        del x
        torch.cuda.empty_cache()
        if dt == np.uint8 and "grid=1 segs=1 " not in desc:
            continue  # (its vector kernel does not honour grid_blocks: float32)
        _assert_chunked(desc, n)
        _same(got, want, False, desc)
        break


def test_column_chunks_weighted(xh):
    """float32 samples (period 7) + exact float32 weights (period 11): a weight pointer that is not advanced with the samples'
    shows in every bin"""
    n = xc.CHUNK_N
    if _free_gb() < 2 * n * 4 / 2**30 + 8:
        pytest.skip("needs %d GB of free device memory" % (2 * n * 4 / 2**30 + 8))
    wpat = xc.chunk_weight_pattern(11, 41)
    ew.assert_summable(-(-n // 7), F32)
    want = xc.periodic_expected(n, xc.CHUNK_BINS_PAT, 5, wpat)[None, :]
    x, w = _periodic(xc.chunk_sample_pattern(F32), n), _periodic(wpat, n)
    (got, desc), = _call(xh, [x], [xc.chunk_edges(F32)], w, {"grid_blocks": 1})
    del x, w
    torch.cuda.empty_cache()
    _assert_chunked(desc, n)
    _same(got, want, True, desc)


def test_column_chunks_two_weights(xh):
    """histogram_two_weights over the same samples: weight patterns of periods 11 and 13"""
    n = xc.CHUNK_N
    if _free_gb() < 3 * n * 4 / 2**30 + 8:
        pytest.skip("needs %d GB of free device memory" % (3 * n * 4 / 2**30 + 8))
    pa, pb = xc.chunk_weight_pattern(11, 42), xc.chunk_weight_pattern(13, 43)
    ew.assert_summable(-(-n // 7), F32)
    edges = [xc.chunk_edges(F32)]
    x, wa, wb = _periodic(xc.chunk_sample_pattern(F32), n), _periodic(pa, n), _periodic(pb, n)
    plan = _fresh(_chunk_plan(xh, x, edges))
    try:
        plan.set_param("grid_blocks", 1)
        ha, hb, _ = xh.histogram_two_weights(x, bins=edges, axis=1, weights=(wa, wb))
        torch.cuda.synchronize()
        desc = plan.describe()
    finally:
        _fresh(plan)
    ha, hb = ha.cpu().numpy(), hb.cpu().numpy()
    del x, wa, wb
    torch.cuda.empty_cache()
    assert " weights=2" in desc, desc
    _assert_chunked(desc, n)
    _same(ha, xc.periodic_expected(n, xc.CHUNK_BINS_PAT, 5, pa)[None, :], True, "first of the pair " + desc)
    _same(hb, xc.periodic_expected(n, xc.CHUNK_BINS_PAT, 5, pb)[None, :], True, "second of the pair " + desc)
