"""Property, thread and row-chunk tests of the three per-sample maps (bin_index, histogram_lookup, histogram_anomaly) on an
MI355X: what tests/test_gpu_values_properties.py is to the ten per-bin statistics.  tests/test_gpu_map.py builds each case for
one kernel; these walk the Python front of the maps (core._sample_call, _map_out, _launch_outputs, _table_on_device,
_check_table_shape, the ordered route through _value_views) and the row-chunk loop of xhist_map_run, which is a copy of its own and not launch_values_pass.  Every
comparison is bit for bit but one, the standardized anomaly on counts whose M2 rounds, which is held to an interval made of
the project's existing bounds (map_oracle.standardized_bracket); there is no new tolerance.

(a) test_random_cases_match_oracle[stat]: the very 60 derandomised cases of tests/values_cases.py that mean_var and mean_var_w
    draw in tests/test_gpu_values_properties.py (D = 1..3 inputs of ndim 1..4, a dtype and a layout per array, axis in any
    order and sign, extents of 0, three backends), and on each: bin_index against map_oracle.index and against the library's
    own histogram; histogram_lookup of a table drawn by map_cases.table_draw (7 dtypes, 5 containers, 4 layouts);
    histogram_anomaly (with the case's weights) against the exact mean; the standardized anomaly (with the case's ddof)
    against map_oracle.assert_standardized; container, dtype and shape of every output.
(b) test_blocks_as_dask_hands_them[stat]: every axis, kept and reduced alike, cut into 1..3 chunks; core._bin_index_block
    and core._lookup_block on every block of host arrays, the table block as blockwise(concatenate=True) hands it (kept axes
    cut like the samples, every bin axis whole), each against the same slice of the unchunked result.  No dask.
(c) test_maps_one_plan_many_threads: 8 threads, a stream each, one cached plan; inputs made on the thread's stream by device
    arithmetic and not synchronised before the calls.
(d) test_more_rows_than_one_launch[family-op]: one row more than a launch takes, and 4098 beyond, through Plan.execute_map;
    3 columns and 2 bins, tables that are formulas of (row, bin), the WHOLE block against a closed form.
(e) test_joint_bins_beyond_32_bits: 8 inputs of 17 bins, indices on both sides of 2^32; 3 and 5 inputs for take and anomaly.

What the 60 examples per statistic of (a) hold (printed by tests/test_map_cpu.py, which asserts the conditions; mean_var /
mean_var_w): cases with some finite mean 57 / 57, with some finite positive variance 45 / 50, without an element 2 / 3; the
largest case has 28 944 elements; cases whose standardized check takes the bit-for-bit branch 32 / 37, the bracket branch
45 / 50; table dtypes float64 8 / 11, float32 7 / 15, float16 8 / 4, int32 7 / 5, int64 10 / 7, uint8 11 / 9, bool 9 / 9;
containers numpy 10 / 9, nested list 8 / 12, torch on the GPU 13 / 20, torch on the CPU 18 / 8, DeviceArray 11 / 11; layouts
(as laid out: a table without kept axes cannot be broadcast along one) contiguous 18 / 17, transposed 16 / 17, sliced 16 / 17,
broadcast 10 / 9, and 22 / 25 tables of two or more axes that are not one contiguous block.
A drawn case that failed once stays below as a directed case (DIRECTED), whatever becomes of the strategy."""
import threading
import time

import numpy as np
import pytest

import map_cases as mc
import map_oracle as mo
import values_cases as vc
import values_exact as vx
from oracle import oracle_np as onp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
hyp = pytest.importorskip("hypothesis")

from test_gpu_map import SENTINEL, direct_case, guarded_map, samples  # noqa: E402
from test_gpu_parity import _plan_for  # noqa: E402
from test_gpu_values_properties import BLOCK_EXAMPLES, EXAMPLES, cuts_of, for_each_case, xh  # noqa: E402,F401  (xh: the fixture)

F64 = np.float64


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


# ---------------------------------------------------------------------------------------------------------------------
# (a) the public calls on the drawn cases
# ---------------------------------------------------------------------------------------------------------------------
def as_container(spec, buf, view):
    """the drawn table as its container holds it, with the very strides of the host view"""
    kind = spec["container"]
    if kind == "numpy":
        return view
    if kind == "list":
        return view.tolist()
    item = view.dtype.itemsize
    off = (view.__array_interface__["data"][0] - buf.__array_interface__["data"][0]) // item if view.size else 0
    if kind in ("torch_gpu", "torch_cpu"):
        t = torch.as_tensor(buf)
        t = t.cuda() if kind == "torch_gpu" else t
        return t.as_strided(view.shape, [s // item for s in view.strides], off) if view.size else t.new_empty(view.shape)
    from xhistogram_amd.devicearray import DeviceArray

    if not view.size:
        return DeviceArray.from_numpy(np.empty(view.shape, view.dtype), 0)
    dev = DeviceArray.from_numpy(buf, 0)
    return DeviceArray(dev.owner, dev.ptr + off * item, view.shape, view.strides, view.dtype, dev.device)


def check_output(out, arrays, backend, shape, dtype, what):
    """torch in -> torch out on the same device, else numpy; int64 / float64; the broadcast shape -> the numpy array"""
    assert tuple(out.shape) == tuple(shape), (what, tuple(out.shape), shape)
    if backend == "torch":
        assert isinstance(out, torch.Tensor) and out.device == arrays[0].device, (what, type(out))
        assert out.dtype == (torch.int64 if dtype == np.int64 else torch.float64), (what, out.dtype)
    else:
        assert isinstance(out, np.ndarray) and out.dtype == dtype, (what, type(out), getattr(out, "dtype", None))
    return _np(out)


def check_case(core, case):
    built = vc.build(case)
    want = mc.expectations(built)
    backend, shape = case["backend"], case["shape"]
    arrays = built.inputs(backend)
    args, kw = built.call_kwargs(arrays)
    bins, axis, weights = kw["bins"], kw["axis"], kw.get("weights")
    xs = built.host[:built.d]

    idx, e = core.bin_index(*args, bins=bins)
    for got, mine in zip(e, built.edges):
        np.testing.assert_array_equal(_np(got), mine)
    idx = check_output(idx, arrays, backend, shape, np.int64, "bin_index")
    mo.assert_bits(idx, want["index"], "bin_index")
    if 0 not in shape:  # (arrays without elements: see test_gpu_values_properties.run_public)
        h = _np(core.histogram(*args, bins=bins)[0])
        np.testing.assert_array_equal(np.bincount(idx[idx >= 0], minlength=h.size).reshape(h.shape), h)

    spec, buf, view, image = mc.table_draw(case)
    look, _ = core.histogram_lookup(*args, table=as_container(spec, buf, view), bins=bins, axis=axis)
    look = check_output(look, arrays, backend, shape, F64, "histogram_lookup")
    mo.assert_bits(look, mo.lookup(xs, built.edges, image, axis), "histogram_lookup of a %(dtype)s %(container)s table, %(laid)s" % spec)

    an, _ = core.histogram_anomaly(*args, values=kw["values"], bins=bins, axis=axis, weights=weights)
    an = check_output(an, arrays, backend, shape, F64, "histogram_anomaly")
    mo.assert_bits(an, want["anomaly"], "histogram_anomaly")

    z, _ = core.histogram_anomaly(*args, values=kw["values"], bins=bins, axis=axis, weights=weights, ddof=case["params"]["ddof"],
                                  standardize=True)
    z = check_output(z, arrays, backend, shape, F64, "standardized anomaly")
    mo.assert_standardized(z, want["anomaly"], want["var"], want["bound"], "standardized anomaly")


@pytest.mark.parametrize("stat", mc.MAP_STATS)
def test_random_cases_match_oracle(xh, stat):
    for_each_case(stat, EXAMPLES, lambda case: check_case(xh, case))


# Drawn cases that failed once, kept as they were drawn (none so far: the test is a loop, so that an empty list does not skip).
DIRECTED = [
]


def test_drawn_cases_that_failed_once(xh):
    for case in DIRECTED:
        check_case(xh, case)


# ---------------------------------------------------------------------------------------------------------------------
# (b) the blocks of a chunked call, as dask's tasks hand them to core._bin_index_block and core._lookup_block
# ---------------------------------------------------------------------------------------------------------------------
def check_blocks(core, case):
    built = vc.build(case)
    shape, d, edges = case["shape"], built.d, built.edges
    ndim = len(shape)
    rng = np.random.default_rng(case["seed"] + 2)
    axis = onp.normalise_axis(case["axis"], ndim)  # (what _sample_call hands on)
    red = set(vc.reduced_axes(case))
    kept = [i for i in range(ndim) if i not in red]
    cuts = [cuts_of(rng, n) for n in shape]
    full = [np.broadcast_to(a, shape) for a in built.views[:d]]  # (dask broadcasts its arrays before it cuts them)
    _, _, table, image = mc.table_draw(case)
    whole_idx = core._bin_index_block(*full, bins=edges)
    whole_look = core._lookup_block(*full, table, axis=axis, bins=edges)
    mo.assert_bits(whole_idx, mo.index(built.host[:d], edges), "unchunked bin_index")
    mo.assert_bits(whole_look, mo.lookup(built.host[:d], edges, image, axis), "unchunked histogram_lookup")
    for at in np.ndindex(*[len(c) for c in cuts]):
        sl = tuple(slice(*c[j]) for c, j in zip(cuts, at))
        blocks = [a[sl] for a in full]
        mo.assert_bits(core._bin_index_block(*blocks, bins=edges), whole_idx[sl], "bin_index of block %s" % (sl,))
        t_block = table[tuple(sl[i] for i in kept) + (slice(None),) * d]
        mo.assert_bits(core._lookup_block(*blocks, t_block, axis=axis, bins=edges), whole_look[sl], "histogram_lookup of block %s" % (sl,))


@pytest.mark.parametrize("stat", mc.MAP_STATS)
def test_blocks_as_dask_hands_them(xh, stat):
    for_each_case(stat, BLOCK_EXAMPLES, lambda case: check_blocks(xh, case))


DIRECTED_BLOCKS = [
]


def test_blocks_of_drawn_cases_that_failed_once(xh):
    for case in DIRECTED_BLOCKS:
        check_blocks(xh, case)


# ---------------------------------------------------------------------------------------------------------------------
# (c) one plan, many threads
# ---------------------------------------------------------------------------------------------------------------------
def test_maps_one_plan_many_threads(xh):
    """8 threads with a stream and data of their own share one edge array, so one cached plan (and allow_values_lds, and
    histogram_mean_var's scratch for the anomaly).  A thread makes its inputs on its stream by device arithmetic (twice the
    halves uploaded beforehand: exact) and calls the maps without synchronising: the library must queue behind that
    arithmetic.  Counts are powers of two up to 16 (map_cases.pow2_data), so the standardized result is bit for bit too."""
    edges = np.linspace(-1.0, 1.0, 9)
    n = 8
    halves, wants = [], []
    for i in range(n):
        rng = np.random.default_rng(4000 + i)
        x, v = mc.pow2_data(rng, (3, 1100 + 64 * i), edges, (1,))
        t = vx.grid(rng, (3, 8))
        halves.append((torch.as_tensor(x * 0.5).cuda(), torch.as_tensor(v * 0.5).cuda(), torch.as_tensor(t).cuda()))
        mean = mo.exact_mean([x], [edges], v, (1,))
        var, b = mo.variance_star([x], [edges], v, (1,), 1)
        assert not np.nansum(b), "pow2_data: a count whose M2 rounds"
        wants.append(dict(index=mo.index([x], [edges]), look=mo.lookup([x], [edges], t, (1,)),
                          anomaly=mo.anomaly([x], [edges], v, mean, None, (1,)), var=mo.lookup([x], [edges], var, (1,)),
                          bound=mo.lookup([x], [edges], b, (1,))))
    torch.cuda.synchronize()
    results = [[] for _ in range(n)]
    errors = []

    def work(i):
        try:
            s = torch.cuda.Stream()
            xh_, vh_, t = halves[i]
            for _ in range(3):
                with torch.cuda.stream(s):
                    x, v = xh_ * 2.0, vh_ * 2.0  # (on this stream, and nobody waits for it)
                    outs = (xh.bin_index(x, bins=[edges])[0], xh.histogram_lookup(x, table=t, bins=[edges], axis=1)[0],
                            xh.histogram_anomaly(x, values=v, bins=[edges], axis=1)[0],
                            xh.histogram_anomaly(x, values=v, bins=[edges], axis=1, ddof=1, standardize=True)[0])
                    s.synchronize()
                    results[i].append([o.cpu().numpy() for o in outs])
        except Exception as e:  # pragma: no cover
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i, w in enumerate(wants):
        assert len(results[i]) == 3
        for r, (idx, look, an, z) in enumerate(results[i]):
            what = "thread %d round %d" % (i, r)
            mo.assert_bits(idx, w["index"], what + " bin_index")
            mo.assert_bits(look, w["look"], what + " histogram_lookup")
            mo.assert_bits(an, w["anomaly"], what + " histogram_anomaly")
            n_exact, n_bracket = mo.assert_standardized(z, w["anomaly"], w["var"], w["bound"], what + " standardized")
            held = int((~np.isnan(w["anomaly"]) & ~np.isnan(w["var"])).sum())  # (8 bins of at most 16 samples per row)
            assert n_bracket == 0 and n_exact == held and held >= 48


# ---------------------------------------------------------------------------------------------------------------------
# (d) more rows than one launch takes
# ---------------------------------------------------------------------------------------------------------------------
def _need(nbytes, parts):
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes + (2 << 30):
        pytest.skip("needs %d bytes of device memory (%s) and 2 GiB to spare, %d bytes are free" % (nbytes, parts, free))


@pytest.mark.parametrize("family,op", mc.ROW_CASES, ids=["%s-%s" % c for c in mc.ROW_CASES])
def test_more_rows_than_one_launch(xh, family, op):
    """xhist_map_run's own loop over the rows of a launch, second iteration included: 4099 rows more than one launch takes.
    Rows are grouped views of periodic [P, 3] arrays (row r reads row r mod P; coprime periods for samples and values), the
    tables real [n_rows, 2] arrays whose elements are formulas of (row, bin), the expectation a closed form evaluated by row
    arithmetic on the GPU (tests/test_map_cpu.py holds it to the oracle by brute force on both sides of the boundary), and the
    whole block is compared, between guard bands."""
    from xhistogram_amd import _native as native

    edges, xs, vs = mc.rows_data(family, op)
    with_scale = op == "anomaly"
    n_cols, n_bins = mc.ROWS_COLS, mc.ROWS_BINS
    cmp, plan_edges, _ = xh._compare_domain([xs.dtype], edges)
    plan = xh._get_plan(plan_edges, cmp, 0)
    xs_t = torch.as_tensor(xs).cuda()
    views = [native.make_view(xs_t.data_ptr(), native.dtype_tag(xs.dtype), n_cols, 1, inner_rows=mc.P_S, outer_stride=0)]
    vview = vs_t = None
    if vs is not None:
        vs_t = torch.as_tensor(vs).cuda()
        vview = native.make_view(vs_t.data_ptr(), native.dtype_tag(vs.dtype), n_cols, 1, inner_rows=mc.P_V, outer_stride=0)
    lut = torch.as_tensor(mc.SCALE_LUT).cuda()
    bin_base = torch.as_tensor(mo.index([xs], edges)).cuda()  # (once per period, on the host)
    v_base = vs_t.double() if vs is not None else None
    code = {"index": native.MAP_INDEX, "take": native.MAP_TAKE, "anomaly": native.MAP_ANOMALY}[op]

    def run(n_rows, out_ptr, centre, scale):
        plan.execute_map(views, vview, n_rows, n_cols, code, centre.data_ptr() if centre is not None else 0,
                         scale.data_ptr() if scale is not None else 0, out_ptr)
        torch.cuda.synchronize()
        return mo.parse(plan.describe())

    def tables(n_rows):
        if op == "index":
            return None, None
        r = torch.arange(n_rows, device="cuda")[:, None]
        b = torch.arange(n_bins, device="cuda")[None, :]
        return mc.centre_of(torch, r, b).contiguous(), (mc.scale_of(torch, r, b, lut).contiguous() if with_scale else None)

    # a few rows first: the launch geometry of this case, from describe()
    small = torch.empty((8, n_cols), dtype=torch.int64, device="cuda")
    hit = run(8, small.data_ptr(), *tables(8))
    assert hit["family"] == family and hit["block"] == (256 if family == "fast" else 512), hit
    chunk = mc.launch_rows(hit["block"], hit["segs"])
    n_rows = chunk + mc.ROWS_EXTRA
    assert chunk < n_rows <= 2 * chunk  # (two launches)
    n = n_rows * n_cols
    lead, tail = 65, 64
    n_tables = 0 if op == "index" else 2 if with_scale else 1
    _need(8 * (lead + n + tail) + n_tables * 8 * n_rows * n_bins + (1 << 30),
          "%d of output, %d tables of %d, about 2^30 for the comparison" % (8 * n, n_tables, 8 * n_rows * n_bins))
    centre, scale = tables(n_rows)
    buf = torch.full((lead + n + tail,), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hit = run(n_rows, buf.data_ptr() + 8 * lead, centre, scale)
    print("\n%s-%s: %d rows, chunk %d, %.3f s for the call; %s" % (family, op, n_rows, chunk, time.perf_counter() - t0, plan.describe()))
    assert (hit["family"], hit["segs"], hit["scale"]) == (family, 1, int(with_scale)), hit
    assert mc.launch_rows(hit["block"], hit["segs"]) == chunk
    assert bool((buf[:lead] == SENTINEL).all()) and bool((buf[lead + n:] == SENTINEL).all()), "the guard bands were written"
    block = buf[lead:lead + n].view(n_rows, n_cols)
    bad = torch.zeros((), dtype=torch.int64, device="cuda")
    first = None
    step = 1 << 21
    for r0 in range(0, n_rows, step):
        rows = torch.arange(r0, min(n_rows, r0 + step), device="cuda")
        want = mc.rows_expected(torch, op, rows, bin_base, v_base, lut if with_scale else None)
        got = block[r0:r0 + len(rows)]
        if op == "index":
            wrong = got != want
        else:
            wn = torch.isnan(want)
            wrong = (torch.isnan(got.view(torch.float64)) != wn) | (~wn & (got != want.view(torch.int64)))
        k = int(wrong.sum())
        if k and first is None:
            at = torch.nonzero(wrong)[0].tolist()
            first = (r0 + at[0], at[1], got[at[0], at[1]].item(), want.view(torch.int64)[at[0], at[1]].item())
        bad += k
    assert int(bad) == 0, "%d of %d elements differ; first at (row, column, got bits, expected bits) %s" % (int(bad), n, first)


# ---------------------------------------------------------------------------------------------------------------------
# (e) joint bins beyond 32 bits, and more than two inputs
# ---------------------------------------------------------------------------------------------------------------------
def test_joint_bins_beyond_32_bits(xh):
    """bin_index needs no table, so the plan's 2^40 bins are a legal call: 8 inputs of 17 bins, 17^8 = 6 975 757 441 joint
    bins, against np.ravel_multi_index of the per-input oracle bins; the 64-bit flat index of map_generic_body"""
    from xhistogram_amd import _native as native

    edges, xs = mc.joint_inputs()
    ok, bins = mo.per_input_bins(xs, edges)
    want = np.where(ok, np.ravel_multi_index([np.where(ok, b, 0) for b in bins], (mc.JOINT_BINS,) * mc.JOINT_D), -1).astype(np.int64)
    assert (want >= 1 << 32).sum() > 1000 and ((want >= 0) & (want < 1 << 32)).sum() > 1000 and (want < 0).sum() > 100
    idx, _ = xh.bin_index(*xs, bins=edges)
    assert isinstance(idx, np.ndarray)
    mo.assert_bits(idx, want, "numpy inputs")
    xs_t = [torch.as_tensor(x).cuda() for x in xs]
    idx, _ = xh.bin_index(*xs_t, bins=edges)
    assert isinstance(idx, torch.Tensor) and idx.dtype == torch.int64
    mo.assert_bits(_np(idx), want, "torch inputs")
    plan = _plan_for(xh, xs_t, edges)
    views = [native.make_view(t.data_ptr(), native.F64, mc.JOINT_N, 1) for t in xs_t]
    got = guarded_map(native, plan, "index", views, None, 1, mc.JOINT_N)
    hit = mo.parse(plan.describe())
    assert "family=generic table=none" in plan.describe() and hit["D"] == mc.JOINT_D, plan.describe()
    mo.assert_bits(got, want.reshape(1, -1), "Plan.execute_map")


@pytest.mark.parametrize("nbs", [(5, 7, 3), (3, 4, 2, 5, 3)], ids=["D3", "D5"])
@pytest.mark.parametrize("op", ["take", "anomaly"])
def test_three_and_five_inputs(xh, op, nbs):
    """more than two inputs through Plan.execute_map on ordinary bin counts: the table row of the joint bin"""
    from test_gpu_census import edges_of

    seed = 5000 + 10 * len(nbs) + (op == "anomaly")
    edges = [edges_of("k1", nb, seed=seed + d) for d, nb in enumerate(nbs)]
    xs = samples(edges, 3, 700, F64, seed)
    v = vx.grid(np.random.default_rng(seed), xs[0].shape, F64)
    hit = direct_case(xh, op, edges, xs, v, fine=False, with_scale=op == "anomaly", seed=seed, what="%s D=%d" % (op, len(nbs)))
    assert (hit["family"], hit["D"], hit["table"]) == ("generic", len(nbs), "lds")
