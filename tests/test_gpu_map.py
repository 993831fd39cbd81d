"""bin_index, histogram_lookup and histogram_anomaly on the GPU: every comparison is bit for bit (map_oracle.assert_bits), there
is no tolerance anywhere, and every case asserts from the plan's describe() that it reached the kernel it was built for
(map_oracle.predict, the restatement of the host's choice).

Direct cases go through Plan.execute_map with the destination inside a larger DeviceBuffer filled with a sentinel: the sentinel
must be intact on both sides and gone from every element inside.  The lead of the guard is odd in every second case, so the
block starts 8 bytes off 16-byte alignment there.  Samples come from test_gpu_census.samples_for (on every edge, one ulp beside
them, NaN, +-inf, outside) and, for float32, from both float32 neighbours of the float64 edges; values are on the exactly
summable grid of tests/values_exact.py; tables hold grid numbers, NaN, +-inf and +-0.0.

The anomaly's identities with the library's own histogram_mean_var run on data whose per-bin counts are powers of two up to 16:
there the mean AND M2 are exact sums (tests/values_exact.py), so two runs of histogram_mean_var give the same bits and the
identity can be held bit for bit; on other counts float64 atomics move the last bits of M2 from run to run."""
import ctypes as C
import os

import numpy as np
import pytest

import map_oracle as mo
import values_exact as vx
from map_cases import AXES, FAST_FORMS, GENERIC_CASES, GENERIC_SHAPES, HOMES, fast_form, fast_shapes, pow2_data
from test_gpu_census import edges_of
from test_gpu_parity import _plan_for, xh  # noqa: F401  (xh: the module fixture)
from test_gpu_values_census import _cus, _domain_edges, float_samples, int_samples

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F64, F32 = np.float64, np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A5A5A5A5A5A5A5A  # (as int64 beyond any bin index; as float64 2.8e127, beyond anything a table here holds)
OP_CODE = {"index": 0, "take": 1, "anomaly": 2}


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------
def samples(edges, n_rows, n_cols, dt, seed):
    """[n_rows, n_cols] per input with the special values of samples_for / float_samples / int_samples, whatever the size"""
    wide = max(n_cols, 64)
    if all(np.asarray(e).dtype.kind == "f" for e in edges) and np.dtype(dt).kind == "f":
        xs = float_samples(edges, n_rows, wide, dt, seed)
    else:
        xs = []
        for d, e in enumerate(edges):
            if np.asarray(e).dtype.kind == "f":
                xs += float_samples([e], n_rows, wide, F64, seed + d)
            else:
                xs += int_samples([e], n_rows, wide, None, seed + d)
    return [np.ascontiguousarray(x[:, :n_cols]) for x in xs]


def grid_values(rng, shape, dt):
    v = vx.grid(rng, shape, dt)
    if np.dtype(dt).kind == "f" and v.size >= 8:
        v.reshape(-1)[rng.permutation(v.size)[: max(1, v.size // 50)]] = np.nan
    return v


def table_of(rng, n_rows, n_bins, zeros=False):
    """a float64 table of grid numbers with NaN, +-inf and +-0.0 among them (`zeros`: a scale table, some of it 0)"""
    t = vx.grid(rng, (n_rows, n_bins), F64)
    flat = t.reshape(-1)
    k = flat.size
    specials = [np.nan, np.inf, -np.inf, 0.0, -0.0]
    pos = rng.permutation(k)[: min(k, 3 * len(specials))]
    flat[pos] = [specials[i % len(specials)] for i in range(len(pos))]
    if zeros:
        flat[rng.permutation(k)[: max(1, k // 20)]] = 0.0
    return t


def int_grid(a):
    """int32 samples on a float64 range: the integers of a float sample array (NaN and +-inf become integers outside)"""
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(a), np.round(a * 10.0), 1000.0).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# the direct call, with guard bands
# ---------------------------------------------------------------------------------------------------------------------
CASE_NO = [0]


def _tag(native, dt):
    return native.dtype_tag(np.dtype(np.int64) if np.dtype(dt).kind in "mM" else dt)


def guarded_map(native, plan, op, views, vview, n_rows, n_cols, centre=None, scale=None):
    """Plan.execute_map into the middle of a DeviceBuffer of sentinels -> the [n_rows, n_cols] block as int64 bits"""
    CASE_NO[0] += 1
    lead, tail = 64 + CASE_NO[0] % 2, 64
    n = n_rows * n_cols
    host = np.full(lead + n + tail, SENTINEL, np.int64)
    buf = native.DeviceBuffer(0, host.nbytes)
    buf.upload(host)
    torch.cuda.synchronize()
    plan.execute_map(views, vview, n_rows, n_cols, OP_CODE[op], centre.data_ptr() if centre is not None else 0,
                     scale.data_ptr() if scale is not None else 0, buf.ptr + 8 * lead)
    torch.cuda.synchronize()
    buf.download(host)
    buf.close()
    assert (host[:lead] == SENTINEL).all() and (host[lead + n:] == SENTINEL).all(), "the guard bands were written"
    block = host[lead:lead + n].reshape(n_rows, n_cols)
    assert not (block == SENTINEL).any(), "%d elements were never written" % (block == SENTINEL).sum()
    return block


def direct_case(core, op, edges, xs, v, *, cmp=0, fine=True, arith=False, layout_fast=True, with_scale=False, seed=0, what=""):
    """one op on contiguous [R, C] host arrays through Plan.execute_map: the variant, the guard bands, the oracle's bits"""
    from xhistogram_amd import _native as native

    n_rows, n_cols = xs[0].shape
    rng = np.random.default_rng(seed)
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    xs_t = [torch.as_tensor(x).cuda() for x in xs]
    plan = _plan_for(core, xs_t, edges)
    views = [native.make_view(t.data_ptr(), _tag(native, x.dtype), n_cols, 1) for t, x in zip(xs_t, xs)]
    vview = v_t = centre = scale = None
    c_host = s_host = None
    if op != "index":
        c_host = table_of(rng, n_rows, n_bins)
        centre = torch.as_tensor(c_host).cuda()
    if op == "anomaly":
        v_t = torch.as_tensor(v).cuda()
        vview = native.make_view(v_t.data_ptr(), _tag(native, v.dtype), n_cols, 1)
        if with_scale:
            s_host = table_of(rng, n_rows, n_bins, zeros=True)
            scale = torch.as_tensor(s_host).cuda()
    got = guarded_map(native, plan, op, views, vview, n_rows, n_cols, centre, scale)
    desc = plan.describe()
    want = mo.predict(op, _cus(), edges, cmp, xs[0].dtype, v.dtype if op == "anomaly" else None, n_rows, n_cols, scale=with_scale,
                      fine=fine, arith=arith, layout_fast=layout_fast)
    hit = mo.assert_variant(desc, want)
    if op == "index":
        mo.assert_bits(got, mo.index(xs, edges), what)
    elif op == "take":
        mo.assert_bits(got.view(F64), mo.lookup(xs, edges, c_host, axis=1), what)
    else:
        mo.assert_bits(got.view(F64), mo.anomaly(xs, edges, v, c_host, s_host, axis=1), what)
    return hit


# ---------------------------------------------------------------------------------------------------------------------
# 1. the fast family: op x sample type x inputs x digitize form, around the tile
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("sdt", ["f64", "f32"])
@pytest.mark.parametrize("form", list(FAST_FORMS))
@pytest.mark.parametrize("op", mo.OPS)
def test_fast_family(xh, op, form, sdt, D):
    st = F64 if sdt == "f64" else F32
    seed = 1000 + 100 * mo.OPS.index(op) + 10 * list(FAST_FORMS).index(form) + 2 * D + (st == F32)
    for i, (n_rows, n_cols) in enumerate(fast_shapes(st, D)):
        scaled = op == "anomaly" and i % 2 == 1
        kind, nbs, fine, arith = fast_form(form, op, st, D, scaled)
        edges = [edges_of(kind, nb, seed=seed + d) for d, nb in enumerate(nbs)]
        xs = samples(edges, n_rows, n_cols, st, seed + i)
        v = grid_values(np.random.default_rng(seed + i), xs[0].shape, st)
        hit = direct_case(xh, op, edges, xs, v, fine=fine, arith=arith, with_scale=scaled, seed=seed + i,
                          what="%s %s %s D=%d %dx%d" % (op, form, sdt, D, n_rows, n_cols))
        assert hit["family"] == "fast" and hit["scan"] == (5 if form == "arith" else fine)
        if n_cols > 2 * mo.tile_of(st, D):
            assert hit["segs"] == 3  # (several workgroups per row, each with its own table row)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the generic family: op x compare domain x table home, around the block
# ---------------------------------------------------------------------------------------------------------------------
def generic_inputs(dom, nb, n_rows, n_cols, seed):
    """edges and samples of compare domain 0 (int32 samples on float64 edges), 1 (int64 on int64) and 3 (int64 next to float64)"""
    rng = np.random.default_rng(seed)
    if dom == "f64":
        edges = [np.linspace(-40.0, 40.0, nb + 1)]
        xs = [int_grid(samples([np.linspace(-4.0, 4.0, 9)], n_rows, n_cols, F64, seed)[0])]
        return edges, xs, 0
    edges = _domain_edges("i64" if dom == "i64" else "mixed", nb, rng)
    return edges, samples(edges, n_rows, n_cols, None, seed), 1 if dom == "i64" else 3


@pytest.mark.parametrize("dom", ["f64", "i64", "mixed"])
@pytest.mark.parametrize("op,home", GENERIC_CASES, ids=["%s-%s" % c for c in GENERIC_CASES])
def test_generic_family(xh, op, home, dom):
    nb, with_scale = HOMES[home]
    seed = 2000 + 100 * mo.OPS.index(op) + 10 * ["f64", "i64", "mixed"].index(dom) + list(HOMES).index(home)
    for i, (n_rows, n_cols) in enumerate(GENERIC_SHAPES):
        edges, xs, cmp = generic_inputs(dom, nb, n_rows, n_cols, seed + i)
        v = grid_values(np.random.default_rng(seed + i), xs[0].shape, [F64, F32, np.int32][i % 3])
        hit = direct_case(xh, op, edges, xs, v, cmp=cmp, fine=False, with_scale=with_scale, seed=seed + i,
                          what="%s %s %s %dx%d" % (op, dom, home, n_rows, n_cols))
        assert hit["family"] == "generic" and hit["cmp"] == cmp
        if op != "index":
            assert hit["table"] == ("lds" if home == "lds" else "global")
        assert hit["tables_in_lds"] == (0 if home == "global_l2" else 1)
        if n_cols == 1500:
            assert hit["segs"] == 3


def test_anomaly_values_of_another_type_take_the_generic_family(xh):
    """float64 samples whose values are float32 (and the reverse): compare domain 0 in the generic family, with a scale table"""
    edges = [edges_of("k1", 300, seed=5)]
    for st, vt in ((F64, F32), (F32, F64)):
        xs = samples(edges, 3, 1500, st, 31)
        v = grid_values(np.random.default_rng(31), xs[0].shape, vt)
        hit = direct_case(xh, "anomaly", edges, xs, v, layout_fast=False, with_scale=True, seed=31, what="values of another type")
        assert (hit["family"], hit["table"], hit["cmp"]) == ("generic", "lds", 0)


# ---------------------------------------------------------------------------------------------------------------------
# 3. layouts through the C ABI: unaligned base pointers, broadcast rows and columns, transposed and grouped views
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sdt", ["f64", "f32"])
@pytest.mark.parametrize("op", mo.OPS)
def test_base_pointer_off_16_byte_alignment(xh, op, sdt):
    """x[1:]: the fast family's 16-byte loads start one element off 16-byte alignment (rows of an odd length: every second row
    of the samples AND of the output block is off as well)"""
    from xhistogram_amd import _native as native

    st = F64 if sdt == "f64" else F32
    n_rows, n_cols = 3, mo.tile_of(st, 1) + 3
    edges = [edges_of("k2", 50, seed=9)]
    x = samples(edges, 1, n_rows * n_cols + 1, st, 41)[0].reshape(-1)
    v = grid_values(np.random.default_rng(41), x.shape, st)
    x_t, v_t = torch.as_tensor(x).cuda(), torch.as_tensor(v).cuda()
    assert x_t.data_ptr() % 16 == 0 and v_t.data_ptr() % 16 == 0
    item = x.itemsize
    plan = _plan_for(xh, [x_t], edges)
    rng = np.random.default_rng(41)
    c_host = table_of(rng, n_rows, 50)
    centre = torch.as_tensor(c_host).cuda() if op != "index" else None
    views = [native.make_view(x_t.data_ptr() + item, _tag(native, st), n_cols, 1)]
    vview = native.make_view(v_t.data_ptr() + item, _tag(native, st), n_cols, 1) if op == "anomaly" else None
    got = guarded_map(native, plan, op, views, vview, n_rows, n_cols, centre)
    hit = mo.assert_variant(plan.describe(), mo.predict(op, _cus(), edges, 0, st, st if op == "anomaly" else None, n_rows, n_cols, fine=2))
    assert hit["family"] == "fast"
    xs, vv = [x[1:].reshape(n_rows, n_cols)], v[1:].reshape(n_rows, n_cols)
    want = mo.index(xs, edges) if op == "index" else mo.lookup(xs, edges, c_host, 1) if op == "take" else mo.anomaly(xs, edges, vv, c_host, None, 1)
    mo.assert_bits(got if op == "index" else got.view(F64), want, "x[1:] %s %s" % (op, sdt))


@pytest.mark.parametrize("layout", ["row_broadcast", "col_broadcast", "transposed", "grouped"])
def test_strided_views(xh, layout):
    """the views the C ABI describes by strides: rows broadcast at stride 0 (still the fast family), columns broadcast at
    stride 0, a transposed block (row stride 1) and grouped rows (kept axes on both sides of the reduced one): the output is the
    dense [rows, cols] block whatever the inputs' strides are"""
    from xhistogram_amd import _native as native

    edges = [edges_of("k1", 40, seed=3)]
    rng = np.random.default_rng(77)
    if layout == "row_broadcast":
        n_rows, n_cols = 3, 2 * mo.tile_of(F64, 1) + 5
        base = samples(edges, 1, n_cols, F64, 51)[0]
        logical, (rs, cs, ir, os_) = np.broadcast_to(base, (n_rows, n_cols)), (0, 1, 0, 0)
    elif layout == "col_broadcast":
        n_rows, n_cols = 3, 700
        base = samples(edges, 1, n_rows, F64, 52)[0].reshape(n_rows, 1)
        logical, (rs, cs, ir, os_) = np.broadcast_to(base, (n_rows, n_cols)), (1, 0, 0, 0)
    elif layout == "transposed":
        n_rows, n_cols = 3, 1500
        base = samples(edges, n_cols, n_rows, F64, 53)[0]  # [C, R] in memory
        logical, (rs, cs, ir, os_) = base.T, (1, n_rows, 0, 0)
    else:  # (a, B, c) reduced over B: rows are (a, c) pairs, inner_rows = c, outer_stride = B * c, column stride c
        a, b, c = 2, 513, 3
        n_rows, n_cols = a * c, b
        base = samples(edges, a, b * c, F64, 54)[0].reshape(a, b, c)
        logical, (rs, cs, ir, os_) = np.moveaxis(base, 1, 2).reshape(n_rows, n_cols), (1, c, c, b * c)
    v = grid_values(rng, (n_rows, n_cols), F64)
    c_host, s_host = table_of(rng, n_rows, 40), table_of(rng, n_rows, 40, zeros=True)
    x_t, v_t = torch.as_tensor(np.ascontiguousarray(base)).cuda(), torch.as_tensor(v).cuda()
    centre, scale = torch.as_tensor(c_host).cuda(), torch.as_tensor(s_host).cuda()
    plan = _plan_for(xh, [x_t], edges)
    views = [native.make_view(x_t.data_ptr(), native.F64, rs, cs, ir, os_)]
    vview = native.make_view(v_t.data_ptr(), native.F64, n_cols, 1)
    xs = [np.ascontiguousarray(logical)]
    fast = layout == "row_broadcast"
    for op in mo.OPS:
        got = guarded_map(native, plan, op, views, vview if op == "anomaly" else None, n_rows, n_cols,
                          centre if op != "index" else None, scale if op == "anomaly" else None)
        hit = mo.assert_variant(plan.describe(), mo.predict(op, _cus(), edges, 0, F64, F64 if op == "anomaly" else None, n_rows, n_cols,
                                                             scale=(op == "anomaly"), fine=1, layout_fast=fast))
        assert hit["family"] == ("fast" if fast else "generic")
        want = mo.index(xs, edges) if op == "index" else mo.lookup(xs, edges, c_host, 1) if op == "take" else \
            mo.anomaly(xs, edges, v, c_host, s_host, 1)
        mo.assert_bits(got if op == "index" else got.view(F64), want, "%s %s" % (layout, op))


# ---------------------------------------------------------------------------------------------------------------------
# 4. the public API: backends, layouts, axes, dtypes
# ---------------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


@pytest.mark.parametrize("backend", ["torch", "numpy", "device"])
@pytest.mark.parametrize("axis", AXES, ids=[str(a) for a in AXES])
def test_public_api_backends_and_axes(xh, backend, axis):
    """the three functions on a 3-D block over trailing, middle, leading and split axes: against the oracle, and the identities
    with the library's own histogram and histogram_mean_var (weights and ddof included), all bit for bit"""
    from xhistogram_amd.devicearray import DeviceArray

    rng = np.random.default_rng(300 + AXES.index(axis))
    shape = (5, 37, 11)
    edges = np.linspace(-1.0, 1.0, 9)
    x, v = pow2_data(rng, shape, edges, axis)
    w = rng.integers(0, 2, shape).astype(F64) * 2.0  # (weights 0 or 2: W stays a power of two or 0 only by luck: mean only)
    put = {"torch": lambda a: torch.as_tensor(a).cuda(), "numpy": lambda a: a, "device": lambda a: DeviceArray.from_numpy(a, 0)}[backend]
    xd, vd, wd = put(x), put(v), put(w)
    kind = torch.Tensor if backend == "torch" else np.ndarray

    idx, e = xh.bin_index(xd, bins=[edges])
    assert isinstance(idx, kind) and _np(idx).dtype == np.int64 and np.array_equal(e[0], edges)
    idx = _np(idx)
    mo.assert_bits(idx, mo.index([x], [edges]), "bin_index")
    h, _ = xh.histogram(xd, bins=[edges])
    np.testing.assert_array_equal(np.bincount(idx[idx >= 0], minlength=8), _np(h))

    cnt, mean, var, _ = xh.histogram_mean_var(xd, values=vd, bins=[edges], axis=axis, ddof=1)
    assert set(np.unique(_np(cnt))) <= {0, 1, 2, 4, 8, 16}
    look, _ = xh.histogram_lookup(xd, table=mean, bins=[edges], axis=axis)
    assert isinstance(look, kind)
    mo.assert_bits(_np(look), mo.lookup([x], [edges], _np(mean), axis), "lookup of the mean")
    ar, _ = xh.histogram_lookup(xd, table=np.broadcast_to(np.arange(8.0), _np(mean).shape), bins=[edges], axis=axis)
    for other in (_np(mean).tolist(), DeviceArray.from_numpy(_np(mean), 0)):  # (a plain sequence; a table already resident)
        same, _ = xh.histogram_lookup(xd, table=other, bins=[edges], axis=axis)
        mo.assert_bits(_np(same), _np(look), "lookup of a %s table" % type(other).__name__)
    np.testing.assert_array_equal(_np(ar)[idx >= 0], idx[idx >= 0])
    assert np.isnan(_np(ar)[idx < 0]).all()

    an, _ = xh.histogram_anomaly(xd, values=vd, bins=[edges], axis=axis)
    assert isinstance(an, kind) and _np(an).shape == shape
    mo.assert_bits(_np(an), v - _np(look), "anomaly = values - lookup(mean)")
    mo.assert_bits(_np(an), mo.anomaly([x], [edges], v, mo.exact_mean([x], [edges], v, axis), None, axis), "anomaly against the oracle")
    z, _ = xh.histogram_anomaly(xd, values=vd, bins=[edges], axis=axis, ddof=1, standardize=True)
    sd = np.sqrt(_np(var)) if backend != "torch" else _np(torch.sqrt(var))
    slook, _ = xh.histogram_lookup(xd, table=sd, bins=[edges], axis=axis)
    with np.errstate(invalid="ignore", divide="ignore"):
        mo.assert_bits(_np(z), (v - _np(look)) / _np(slook), "standardized anomaly")

    aw, _ = xh.histogram_anomaly(xd, values=vd, bins=[edges], axis=axis, weights=wd)
    _, wmean, _, _ = xh.histogram_mean_var(xd, values=vd, bins=[edges], axis=axis, weights=wd)
    wlook, _ = xh.histogram_lookup(xd, table=wmean, bins=[edges], axis=axis)
    mo.assert_bits(_np(aw), v - _np(wlook), "weighted anomaly = values - lookup(weighted mean)")
    mo.assert_bits(_np(aw), mo.anomaly([x], [edges], v, mo.exact_mean([x], [edges], v, axis, w), None, axis), "weighted anomaly, oracle")


@pytest.mark.parametrize("layout", ["offset", "transposed", "fortran", "sliced", "broadcast"])
def test_public_api_layouts(xh, layout):
    """torch views that are not contiguous blocks: x[1:], a transpose, F order, a strided slice, stride-0 broadcasting"""
    rng = np.random.default_rng(400)
    edges = [edges_of("k2", 30, seed=1), edges_of("k1", 20, seed=2)]
    full = [float_samples([e], 40, 301, F64, 60 + d)[0] for d, e in enumerate(edges)]
    vfull = vx.grid(rng, (40, 301), F64)
    dev = [torch.as_tensor(a).cuda() for a in full + [vfull]]
    if layout == "offset":
        cut = lambda a: a.reshape(-1)[1:]  # noqa: E731
    elif layout == "transposed":
        cut = lambda a: a.T  # noqa: E731
    elif layout == "fortran":
        cut = lambda a: a.T.contiguous().T if hasattr(a, "contiguous") else np.asfortranarray(a)  # noqa: E731
    elif layout == "sliced":
        cut = lambda a: a[3:, ::2]  # noqa: E731
    else:
        cut = None
    if cut is not None:
        xs, v = [cut(a) for a in full[:2]], cut(vfull)
        xs_d, v_d = [cut(a) for a in dev[:2]], cut(dev[2])
    else:  # samples (R, 1) and (1, C), values (R, C): the inputs broadcast at stride 0
        xs, v = [full[0][:, :1], full[1][:1, :]], vfull
        xs_d, v_d = [dev[0][:, :1], dev[1][:1, :]], dev[2]
    axis = None if layout == "offset" else (1,)
    idx, _ = xh.bin_index(*xs_d, bins=edges)
    mo.assert_bits(_np(idx), mo.index(xs, edges), layout)
    want_shape = np.broadcast_shapes(*[a.shape for a in xs])
    m = 1 if axis is None else want_shape[0]
    table = table_of(rng, m, 600).reshape(((m,) if axis else ()) + (30, 20))
    look, _ = xh.histogram_lookup(*xs_d, table=torch.as_tensor(table).cuda(), bins=edges, axis=axis)
    mo.assert_bits(_np(look), mo.lookup(xs, edges, table, axis), layout)
    an, _ = xh.histogram_anomaly(*xs_d, values=v_d, bins=edges, axis=axis)
    mo.assert_bits(_np(an), mo.anomaly(xs, edges, v, mo.exact_mean(xs, edges, v, axis), None, axis), layout)


@pytest.mark.parametrize("dom", ["int32", "dt", "mixed", "f32"])
def test_public_api_sample_types(xh, dom):
    """int32 samples on float64 edges, datetime64 samples (numpy in: torch holds none), an int64 input next to a float64 one,
    and float32 samples with float32 values: index, lookup and anomaly against the oracle"""
    rng = np.random.default_rng(500 + ["int32", "dt", "mixed", "f32"].index(dom))
    shape = (3, 1201)
    if dom == "int32":
        edges = [np.linspace(-40.0, 40.0, 17)]
        xs = [int_grid(float_samples([np.linspace(-4.0, 4.0, 9)], *shape, F64, 5)[0])]
    elif dom == "f32":
        edges = [edges_of("k2", 60, seed=4)]
        xs = float_samples(edges, *shape, F32, 6)
    else:
        edges = _domain_edges(dom, 25, rng)
        xs = samples(edges, *shape, None, 7)
    v = vx.grid(rng, shape, F32 if dom == "f32" else np.int32 if dom == "dt" else F64)
    host = dom == "dt"
    xs_d = xs if host else [torch.as_tensor(a).cuda() for a in xs]
    v_d = v if host else torch.as_tensor(v).cuda()
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    idx, be = xh.bin_index(*xs_d, bins=edges)
    mo.assert_bits(_np(idx), mo.index(xs, edges), dom)
    h, _ = xh.histogram(*xs_d, bins=edges)
    np.testing.assert_array_equal(np.bincount(_np(idx)[_np(idx) >= 0], minlength=n_bins).reshape(_np(h).shape), _np(h))
    table = table_of(rng, shape[0], n_bins).reshape((shape[0],) + tuple(len(e) - 1 for e in edges))
    look, _ = xh.histogram_lookup(*xs_d, table=table, bins=edges, axis=1)
    mo.assert_bits(_np(look), mo.lookup(xs, edges, table, 1), dom)
    an, _ = xh.histogram_anomaly(*xs_d, values=v_d, bins=edges, axis=1)
    mo.assert_bits(_np(an), mo.anomaly(xs, edges, v, mo.exact_mean(xs, edges, v, 1), None, 1), dom)


def test_public_api_edges_from_a_bin_count(xh):
    """bins=int: the edges are those of the unweighted histogram call, made on the device for resident samples"""
    rng = np.random.default_rng(600)
    x = rng.uniform(-3.0, 5.0, (4, 513))
    xd = torch.as_tensor(x).cuda()
    h, e = xh.histogram(xd, bins=12)
    idx, be = xh.bin_index(xd, bins=12)
    np.testing.assert_array_equal(np.asarray(be[0]), np.asarray(e[0]))
    mo.assert_bits(_np(idx), mo.index([x], [np.asarray(e[0])]), "bins=12")
    assert (_np(idx) >= 0).all()  # (the range is the data's own: nothing falls outside)
    np.testing.assert_array_equal(np.bincount(_np(idx).reshape(-1), minlength=12), _np(h))


@pytest.mark.parametrize("backend", ["torch", "numpy"])
def test_a_plan_without_bins_still_writes_every_element(xh, backend):
    """one edge, no bin: histogram counts nothing, so every index is -1 and every lookup and anomaly NaN, written by the library
    itself (through Plan.execute_map too: the guard bands hold)"""
    from xhistogram_amd import _native as native

    rng = np.random.default_rng(650)
    x = rng.uniform(-1.0, 1.0, (3, 515))
    v = vx.grid(rng, x.shape, F64)
    edges = [np.array([0.25])]
    xd, vd = (torch.as_tensor(a).cuda() for a in (x, v)) if backend == "torch" else (x, v)
    h, _ = xh.histogram(xd, bins=edges, axis=1)
    assert _np(h).shape == (3, 0)
    idx, _ = xh.bin_index(xd, bins=edges)
    assert _np(idx).dtype == np.int64 and _np(idx).shape == x.shape and (_np(idx) == -1).all()
    look, _ = xh.histogram_lookup(xd, table=np.zeros((3, 0)), bins=edges, axis=1)
    an, _ = xh.histogram_anomaly(xd, values=vd, bins=edges, axis=1, standardize=True)
    for out in (look, an):
        assert _np(out).dtype == F64 and _np(out).shape == x.shape and np.isnan(_np(out)).all()
    x_t = torch.as_tensor(x).cuda()
    plan = _plan_for(xh, [x_t], edges)
    got = guarded_map(native, plan, "index", [native.make_view(x_t.data_ptr(), native.F64, 515, 1)], None, 3, 515)
    assert (got == -1).all()


def test_torch_results_follow_the_current_stream(xh):
    """torch in -> torch out, queued on the current stream: on a side stream the result is complete once that stream is"""
    rng = np.random.default_rng(700)
    x = rng.uniform(-1.0, 1.0, 40_000)
    edges = [np.linspace(-1.0, 1.0, 101)]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xd = torch.as_tensor(x).cuda()
        idx, _ = xh.bin_index(xd, bins=edges)
        s.synchronize()
        got = idx.cpu().numpy()
    mo.assert_bits(got, mo.index([x], edges), "side stream")


# ---------------------------------------------------------------------------------------------------------------------
# 5. errors
# ---------------------------------------------------------------------------------------------------------------------
def test_python_front_rejects_before_any_device_work(xh, monkeypatch):
    x = np.zeros((4, 6))
    edges = [np.linspace(0.0, 1.0, 4)]
    xd = torch.zeros((4, 6), dtype=torch.float64)  # a CPU tensor
    monkeypatch.setattr(xh, "_upload_host", lambda *a, **k: pytest.fail("device work"))
    monkeypatch.setattr(xh, "_value_views", lambda *a, **k: pytest.fail("device work"))
    with pytest.raises(ValueError, match=r"table has shape \(4, 4\), but histogram gives \(4, 3\)"):
        xh.histogram_lookup(x, table=np.zeros((4, 4)), bins=edges, axis=1)
    with pytest.raises(ValueError, match=r"table has shape \(4, 3\), but histogram gives \(3,\)"):
        xh.histogram_lookup(x, table=np.zeros((4, 3)), bins=edges)
    with pytest.raises(ValueError, match="table has shape"):
        xh.histogram_lookup(x, table=np.zeros((4, 4)), bins=5, axis=1)  # (a bin count: the shape is known before the edges are)
    with pytest.raises(TypeError, match="complex values have no order: histogram_lookup takes real values"):
        xh.histogram_lookup(x, table=np.zeros((4, 3), np.complex128), bins=edges, axis=1)
    with pytest.raises(TypeError, match="histogram_lookup takes real values, got dtype"):
        xh.histogram_lookup(x, table=np.zeros((4, 3), "U1"), bins=edges, axis=1)
    with pytest.raises(ValueError, match=r"table has shape \(2, 2\), but histogram gives \(4, 3\)"):
        xh.histogram_lookup(x, table=[[0.0, 1.0], [2.0, 3.0]], bins=edges, axis=1)
    with pytest.raises(TypeError, match="histogram_lookup needs a table"):
        xh.histogram_lookup(x, table=None, bins=edges, axis=1)
    with pytest.raises(TypeError, match="histogram_anomaly needs values"):
        xh.histogram_anomaly(x, values=None, bins=edges)
    with pytest.raises(TypeError, match="complex values have no order"):
        xh.histogram_anomaly(x, values=np.zeros((4, 6), np.complex64), bins=edges)
    with pytest.raises(ValueError, match="ddof must be an integer >= 0"):
        xh.histogram_anomaly(x, values=x, bins=edges, ddof=-1)
    with pytest.raises(TypeError, match="standardize must be a bool"):
        xh.histogram_anomaly(x, values=x, bins=edges, standardize=1)
    with pytest.raises(TypeError, match="bin_index needs at least one array"):
        xh.bin_index(bins=edges)
    for call in (lambda: xh.bin_index(xd, bins=edges), lambda: xh.histogram_lookup(xd, table=np.zeros((4, 3)), bins=edges, axis=1),
                 lambda: xh.histogram_anomaly(xd, values=xd, bins=edges)):
        with pytest.raises(RuntimeError, match="torch inputs must live on an MI355X"):
            call()


def test_c_abi_rejects_bad_calls_and_a_valid_call_still_runs(xh):
    """xhist_plan_execute_map's own argument checks, as tests/test_gpu_values_errors.py holds the statistics': every rejected
    call returns XHIST_ERR_INVALID before any launch with the whole message, zero rows are no error and leave describe() alone,
    and the valid call after them gives the oracle's bits"""
    from xhistogram_amd import _native as native

    edges = np.array([0.0, 1.0, 2.0, 3.0, 4.0])
    x = np.array([[0.5, 1.5, 0.5, 2.5, 4.0, 3.5, -1.0, np.nan]])
    v = np.array([[1.0, 3.0, 2.0, -2.0, 4.0, 6.0, 5.0, 7.0]])
    mean = np.array([[1.5, 3.0, -2.0, 5.0]])
    x_t, v_t, c_t = (torch.as_tensor(a).cuda() for a in (x, v, mean))
    out = torch.full((1, 8), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    plan = native.Plan([edges], native.CMP_F64, 0)
    lib = native.load()
    view = lambda t: native.make_view(t.data_ptr(), native.F64, 8, 1)  # noqa: E731
    null = C.POINTER(native.XhistArray)()
    args = dict(plan=plan._h, samples=(native.XhistArray * 1)(view(x_t)), values=C.pointer(view(v_t)), n_rows=1, n_cols=8,
                op=native.MAP_ANOMALY, centre=C.c_void_p(c_t.data_ptr()), scale=C.c_void_p(0), out=C.c_void_p(out.data_ptr()),
                mem_kind=native.MEM_DEVICE, stream=C.c_void_p(0))

    def rejected(message, **changed):
        rc = lib.xhist_plan_execute_map(*dict(args, **changed).values())
        assert (rc, lib.xhist_last_error().decode()) == (native.ERR_INVALID, message), changed

    before = plan.describe()
    rejected("unknown map op 3", op=3)
    rejected("values are required", values=null)
    rejected("only XHIST_MAP_ANOMALY takes values", op=native.MAP_TAKE)
    rejected("only XHIST_MAP_ANOMALY takes values", op=native.MAP_INDEX)
    rejected("XHIST_MAP_INDEX takes no table", op=native.MAP_INDEX, values=null)
    rejected("XHIST_MAP_TAKE takes no scale table", op=native.MAP_TAKE, values=null, scale=C.c_void_p(c_t.data_ptr()))
    rejected("the table (centre) is NULL", centre=C.c_void_p(0))
    rejected("out is NULL", out=C.c_void_p(0))
    rejected("xhist_plan_execute_map takes DEVICE arrays (mem_kind XHIST_MEM_DEVICE); upload host data first", mem_kind=native.MEM_HOST)
    assert lib.xhist_plan_execute_map(*dict(args, n_rows=0).values()) == native.OK
    torch.cuda.synchronize()
    assert plan.describe() == before and bool((out == -7.0).all())

    assert lib.xhist_plan_execute_map(*args.values()) == native.OK, lib.xhist_last_error()
    torch.cuda.synchronize()
    assert plan.describe() == "map op=anomaly family=fast table=lds scan=1 cmp=0 segs=1 block=256 lds_bytes=%d tables_in_lds=1 scale=0 D=1" % (
        mo.predict("anomaly", 256, [edges], 0, F64, F64, 1, 8)["lds_bytes"])
    mo.assert_bits(out.cpu().numpy(), np.array([[-0.5, 0.0, 0.5, 0.0, -1.0, 1.0, np.nan, np.nan]]), "the valid call")
    plan.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. xarray and dask
# ---------------------------------------------------------------------------------------------------------------------
def test_xarray_wrappers(xh, monkeypatch):
    try:
        import xarray as xr
    except ImportError:
        monkeypatch.syspath_prepend(os.path.join(ROOT, "tests", "doubles"))
        import xarray as xr
    from xhistogram_amd import xarray as xhx

    rng = np.random.default_rng(800)
    edges = np.linspace(-1.0, 1.0, 9)
    x, v = pow2_data(rng, (4, 60), edges, (1,))
    temp = xr.DataArray(x, dims=("time", "x"), coords={"time": np.arange(4.0)}, name="temp")
    oxy = xr.DataArray(v, dims=("time", "x"), name="oxygen")
    idx = xhx.bin_index(temp, bins=[edges])
    assert (idx.name, tuple(idx.dims)) == ("temp_bin_index", ("time", "x"))
    mo.assert_bits(np.asarray(idx.data), mo.index([x], [edges]), "xarray bin_index")
    np.testing.assert_array_equal(np.asarray(idx["time"].data), np.arange(4.0))
    cnt, mean, var = xhx.histogram_mean_var(temp, values=oxy, bins=[edges], dim=["x"])
    look = xhx.histogram_lookup(temp, table=mean, bins=[edges], dim=["x"])
    assert (look.name, tuple(look.dims)) == ("oxygen_mean_lookup", ("time", "x"))
    mo.assert_bits(np.asarray(look.data), mo.lookup([x], [edges], np.asarray(mean.data), (1,)), "xarray lookup")
    swapped = xhx.histogram_lookup(temp, table=mean.transpose("temp_bin", "time"), bins=[edges], dim=["x"])
    mo.assert_bits(np.asarray(swapped.data), np.asarray(look.data), "table dims in another order")
    an = xhx.histogram_anomaly(temp, values=oxy, bins=[edges], dim=["x"])
    assert (an.name, tuple(an.dims)) == ("oxygen_anomaly", ("time", "x"))
    mo.assert_bits(np.asarray(an.data), v - np.asarray(look.data), "xarray anomaly")
    z = xhx.histogram_anomaly(temp, values=oxy, bins=[edges], dim=["x"], standardize=True)
    sd = xhx.histogram_lookup(temp, table=xr.DataArray(np.sqrt(np.asarray(var.data)), dims=var.dims, name="sd"), bins=[edges], dim=["x"])
    with np.errstate(invalid="ignore", divide="ignore"):
        mo.assert_bits(np.asarray(z.data), (v - np.asarray(look.data)) / np.asarray(sd.data), "xarray z-score")
    with pytest.raises(ValueError, match="table has dims"):
        xhx.histogram_lookup(temp, table=mean, bins=[edges])
    with pytest.raises(TypeError, match="accepts only xarray.DataArray"):
        xhx.histogram_lookup(temp, table=np.asarray(mean.data), bins=[edges], dim=["x"])


def test_dask_branch(monkeypatch):
    """several chunks along kept and reduced axes give what the numpy call gives, bit for bit: tests/map_dask_script.py in the
    interpreter that has dask, started as tests/test_dask_branch.py starts its own script"""
    import test_dask_branch as tdb

    if not tdb._have_dask_python():
        pytest.skip("no interpreter with dask in this image")
    monkeypatch.setattr(tdb, "SCRIPT", os.path.join(ROOT, "tests", "map_dask_script.py"))
    assert "MAP-DASK-OK" in tdb._run("map")
