"""histogram_extrema on the MI355X: both outputs bit for bit against tests/extrema_oracle.py over sample and value dtypes,
D = 1..3, edge kinds, LDS and beyond-LDS homes, row shapes and views, special values, accumulation, the three in-memory
backends, the counting property, a 10^9-sample case against a torch restatement, and dask in the conda interpreter.  Between
them the cases select every kernel of xhist_extrema.hip (the census of the -m gpu session holds them to that)."""
import os
import subprocess

import numpy as np
import pytest

import extrema_oracle as eo

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from xhistogram_amd import _native

    if _native.device_count() < 1:
        pytest.skip("no MI355X visible")


def _core():
    from xhistogram_amd import core

    return core


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _same(got, want):
    got, want = np.asarray(_np(got), np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64))


def _check(args, values, bins, axis=None, **kw):
    vmin, vmax, edges = _core().histogram_extrema(*args, values=values, bins=bins, axis=axis, **kw)
    want = eo.histogram_extrema(*[_np(a) for a in args], values=_np(values), bins=[_np(e) for e in edges], axis=axis)
    _same(vmin, want[0])
    _same(vmax, want[1])
    return vmin, vmax, edges


SPECIAL = np.array([-np.inf, -1e300, -5e-324, -0.0, 0.0, 5e-324, 2.2e-308, 1e300, np.inf, np.nan])


def _values(rng, shape, dtype=np.float64):
    v = rng.standard_normal(shape)
    if np.dtype(dtype).kind == "f":
        flat = v.reshape(-1)
        sel = rng.random(flat.size) < 0.05
        flat[sel] = SPECIAL[rng.integers(0, len(SPECIAL), int(sel.sum()))]
        with np.errstate(over="ignore"):  # (float32: +-1e300 become +-inf, as intended)
            return flat.reshape(shape).astype(dtype)
    if np.dtype(dtype) == np.bool_:
        return rng.random(shape) < 0.5
    return (v * 1000).astype(dtype)


def _samples(rng, shape, edges, dtype=np.float64):
    lo, hi = float(edges[0]), float(edges[-1])
    x = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), shape)
    flat = x.reshape(-1)
    sel = rng.random(flat.size) < 0.02
    flat[sel] = np.asarray(edges, np.float64)[rng.integers(0, len(edges), int(sel.sum()))]  # on every edge, the last included
    if np.dtype(dtype).kind == "f":
        flat[rng.random(flat.size) < 0.01] = np.nan
    return flat.reshape(shape).astype(dtype)


LIN = np.linspace(-2.0, 3.0, 101)
TWO = np.sort(np.r_[np.linspace(-2.0, 3.0, 81), 0.0001])  # one bucket with two edges: the two-edge scan
ARANGE = np.arange(-2, 32, 0.1)
GEOM = np.geomspace(0.01, 30.0, 64)


# ---- the vector fast path: float32 / float64 samples and values, one or two inputs, every digitize form ------------------
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["one", "two", "arith"])
@pytest.mark.parametrize("D", [1, 2])
def test_fast_path_forms(dt, kind, D):
    rng = np.random.default_rng(100 * (dt == np.float32) + 10 * ["one", "two", "arith"].index(kind) + D)
    if kind == "arith":  # linspace edges whose tables do not fit LDS next to the slots: the table-free digitize
        nb = (7000 if dt == np.float64 else 15000) if D == 1 else (3000 if dt == np.float64 else 6500)
        edges = [np.linspace(-1.0, 2.0, nb + 1)] if D == 1 else [np.linspace(-1.0, 2.0, 4), np.linspace(-1.0, 2.0, nb + 1)]
    else:
        # (two inputs, float64: 100 x 100 bins of 16-byte slots would leave no room for the tables — 100 x 40)
        edges = ([LIN] * D if D == 1 or dt == np.float32 else [LIN, np.linspace(-2.0, 3.0, 41)]) if kind == "one" else [TWO] * D
    n = 1_000_003
    x = [torch.as_tensor(_samples(rng, n, e, dt)).cuda() for e in edges]
    v = torch.as_tensor(_values(rng, n, dt)).cuda()
    _check(x, v, edges)
    # several rows, one kept axis
    x2 = [torch.as_tensor(_samples(rng, (7, 30001), e, dt)).cuda() for e in edges]
    v2 = torch.as_tensor(_values(rng, (7, 30001), dt)).cuda()
    _check(x2, v2, edges, axis=1)


@pytest.mark.parametrize("sdt", [np.float64, np.float32, np.float16, np.int32, np.int64, np.uint64])
@pytest.mark.parametrize("vdt", [np.float64, np.float32, np.int32, np.bool_])
def test_dtypes_numpy(sdt, vdt):
    rng = np.random.default_rng(11)
    if np.dtype(sdt).kind in "iu":
        edges = [np.arange(0, 200, 7).astype(sdt)]
        x = rng.integers(0, 210, 200_001).astype(sdt)
    else:
        edges = [ARANGE]
        x = _samples(rng, 200_001, ARANGE, sdt)
    v = _values(rng, x.shape, vdt)
    _check([x], v, edges)


def test_mixtures_and_three_inputs():
    rng = np.random.default_rng(12)
    n = 300_007
    e = [LIN, GEOM, ARANGE]
    x = [_samples(rng, n, e[0], np.float32), _samples(rng, n, e[1], np.float64), _samples(rng, n, e[2], np.float16)]
    v = _values(rng, n)
    _check(x[:2], v, e[:2])
    _check(x, v, e)
    _check([torch.as_tensor(a).cuda() for a in x], torch.as_tensor(v).cuda(), e)
    # random sorted edges (crowded buckets: the binary search)
    er = np.sort(rng.uniform(-2, 3, 300))
    _check([_samples(rng, n, er)], v, [er])


def test_datetime_and_per_input_domains():
    rng = np.random.default_rng(13)
    n = 100_003
    t = (np.datetime64("2020-01-01") + rng.integers(0, 400, n).astype("timedelta64[D]")).astype("datetime64[s]")
    te = np.arange(np.datetime64("2020-01-01"), np.datetime64("2021-02-01"), np.timedelta64(10, "D")).astype("datetime64[s]")
    v = _values(rng, n)
    _check([t], v, [te])  # the int64 domain, slots in LDS
    y = _samples(rng, n, LIN)
    _check([t, y], v, [te, LIN])  # per-input domains
    # beyond LDS: int64 domain and per-input domains with their keys in global memory
    big_t = np.arange(np.datetime64("2020-01-01"), np.datetime64("2020-01-01") + np.timedelta64(1100, "D")).astype("datetime64[s]")
    big_t = big_t[:1025]
    t2 = (np.datetime64("2020-01-01") + rng.integers(0, 1030, n).astype("timedelta64[D]")).astype("datetime64[s]")
    i2 = rng.integers(0, 1030, n)
    _check([t2, i2.astype(np.int64)], v, [big_t, np.arange(1025, dtype=np.int64)])
    _check([t2, _samples(rng, n, np.linspace(0, 1, 1025))], v, [big_t, np.linspace(0, 1, 1025)])


def test_beyond_lds_homes():
    rng = np.random.default_rng(14)
    n = 2_000_003
    e = [np.linspace(-4, 4, 1025)] * 2
    x = [torch.randn(n, dtype=torch.float64, device="cuda") for _ in range(2)]
    v = torch.as_tensor(_values(rng, n)).cuda()
    _check(x, v, e)  # float64 samples + values, 1024 x 1024 bins: keys in global memory
    _check([a.float() for a in x], torch.as_tensor(_values(rng, n, np.int32)).cuda(), e)


def test_row_shapes_and_views():
    rng = np.random.default_rng(15)
    a = _samples(rng, (6, 50, 40), LIN)
    v = _values(rng, (6, 50, 40))
    for axis in (None, (1, 2), (2,), (0,), (1,), (0, 2)):
        _check([a], v, [LIN], axis=axis)  # flattened, kept leading axis, leading-axis reduction, grouped middle axis
        _check([torch.as_tensor(a).cuda()], torch.as_tensor(v).cuda(), [LIN], axis=axis)
    vb = _values(rng, (1, 50, 1))  # values broadcast with stride 0
    _check([a], vb, [LIN], axis=(1, 2))
    _check([torch.as_tensor(a).cuda()], torch.as_tensor(vb).cuda(), [LIN], axis=(1, 2))
    t = torch.as_tensor(a).cuda()
    _check([t.transpose(0, 2)], torch.as_tensor(v).cuda().transpose(0, 2), [LIN], axis=(0,))  # non-contiguous views
    _check([t[:, ::2, :]], torch.as_tensor(v).cuda()[:, ::2, :], [LIN], axis=(1, 2))


def test_special_values_and_empty_inputs():
    e = np.array([0.0, 1.0, 2.0, 3.0])
    x = np.array([0.5, 0.5, 1.5, 1.5, 3.0, 3.0, np.nan, 0.0])
    v = np.array([0.0, -0.0, np.nan, np.nan, 5e-324, -np.inf, 1.0, np.inf])
    for dt in (np.float64, np.float32):
        vmin, vmax, _ = _check([x.astype(dt)], v.astype(dt), [e])
        assert np.signbit(vmin[0]) and not np.signbit(vmax[0])
        assert np.isnan(vmin[1]) and np.isnan(vmax[1])
    vmin, vmax, _ = _check([np.zeros(0)], np.zeros(0), [e])
    assert np.isnan(vmin).all() and vmin.shape == (3,)
    vmin, vmax, _ = _check([np.zeros((0, 5))], np.zeros((0, 5)), [e], axis=1)
    assert vmin.shape == (0, 3)


def test_accumulate_equals_one_call_over_the_concatenation():
    from xhistogram_amd import _native, core

    rng = np.random.default_rng(16)
    for dt, edges in ((torch.float64, [LIN]), (torch.float32, [LIN, TWO]), (torch.float64, [np.linspace(-4, 4, 1025)] * 2)):
        D = len(edges)
        n = 500_001
        xs = [torch.as_tensor(_samples(rng, 2 * n, e)).to(dt).cuda() for e in edges]
        v = torch.as_tensor(_values(rng, 2 * n)).to(dt).cuda()
        plan = core._get_plan(edges, _native.CMP_F64, 0)
        out = torch.empty((2, plan.n_bins), dtype=torch.float64, device="cuda")
        tag = _native.F64 if dt == torch.float64 else _native.F32
        stream = torch.cuda.current_stream().cuda_stream
        for part, acc in ((slice(0, n), False), (slice(n, 2 * n), True)):
            views = [_native.make_view(x[part].data_ptr(), tag, 0, 1) for x in xs]
            plan.execute_extrema(views, _native.make_view(v[part].data_ptr(), tag, 0, 1), 1, n, out.data_ptr(),
                                 out.data_ptr() + plan.n_bins * 8, accumulate=acc, stream=stream)
        want = eo.histogram_extrema(*[_np(x) for x in xs], values=_np(v), bins=edges)
        _same(out[0].reshape(want[0].shape), want[0])
        _same(out[1].reshape(want[1].shape), want[1])


def test_backends_and_counting_property():
    from xhistogram_amd import core
    from xhistogram_amd.devicearray import DeviceArray

    rng = np.random.default_rng(17)
    x = _samples(rng, (4, 100_000), LIN)
    v = rng.standard_normal((4, 100_000))  # no NaN values
    a = _check([x], v, [LIN], axis=1)
    b = _check([torch.as_tensor(x).cuda()], torch.as_tensor(v).cuda(), [LIN], axis=1)
    c = _check([DeviceArray.from_numpy(x)], DeviceArray.from_numpy(v), [LIN], axis=1)
    assert isinstance(a[0], np.ndarray) and isinstance(c[0], np.ndarray) and b[0].is_cuda
    _same(_np(b[0]), a[0])
    counts, _ = core.histogram(x, bins=[LIN], axis=1)
    np.testing.assert_array_equal(np.isnan(a[0]), counts == 0)
    np.testing.assert_array_equal(np.isnan(a[1]), counts == 0)
    # int / estimator bins: the edges of the unweighted histogram
    xc = np.where(np.isnan(x), 0.5, x)  # (numpy's range detection refuses NaN)
    for bins in (50, "sturges"):
        vmin, _, edges = _check([xc], v, bins)
        _, want = core.histogram(xc, bins=bins)
        np.testing.assert_array_equal(edges[0], want[0])


def test_a_billion_float64_samples_against_torch():
    from xhistogram_amd import core

    n = 1_000_000_000
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    x = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
    v = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
    vmin, vmax, edges = core.histogram_extrema(x, values=v, bins=[LIN])
    e = torch.as_tensor(edges[0], device="cuda")
    idx = torch.bucketize(x, e, right=True) - 1
    idx = torch.where(x == e[-1], torch.full_like(idx, len(LIN) - 2), idx)
    ok = (x >= e[0]) & (x <= e[-1]) & ~torch.isnan(v)
    del x
    bits = v.view(torch.int64)
    keys = bits ^ ((bits >> 63) & 0x7FFFFFFFFFFFFFFF)  # signed keys, ordered like the unsigned ones
    del bits
    idx, keys = idx[ok], keys[ok]
    del ok
    lo = torch.zeros(len(LIN) - 1, dtype=torch.int64, device="cuda").scatter_reduce(0, idx, keys, "amin", include_self=False)
    hi = torch.zeros(len(LIN) - 1, dtype=torch.int64, device="cuda").scatter_reduce(0, idx, keys, "amax", include_self=False)
    unkey = lambda k: (k ^ ((k >> 63) & 0x7FFFFFFFFFFFFFFF)).view(torch.float64)  # noqa: E731
    torch.testing.assert_close(vmin, unkey(lo), rtol=0, atol=0)
    torch.testing.assert_close(vmax, unkey(hi), rtol=0, atol=0)


PY39 = "/opt/conda/bin/python3.9"
SCRIPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "extrema_dask_script.py")


def _have_dask_python():
    return os.path.exists(PY39) and subprocess.run([PY39, "-c", "import dask.array, numpy"], capture_output=True).returncode == 0


@pytest.mark.skipif(not _have_dask_python(), reason="no interpreter with dask in this image")
@pytest.mark.parametrize("exchange", [None, "rccl"])
def test_dask_chunked_equals_unchunked(exchange):
    env = dict(os.environ)
    if exchange:
        env["XHIST_AMD_DASK_EXCHANGE"] = exchange
    sys_cxx = "/usr/lib/x86_64-linux-gnu/libstdc++.so.6"  # (as tests/test_dask_branch.py: conda's libstdc++ is older)
    if os.path.exists(sys_cxx):
        env["LD_PRELOAD"] = (sys_cxx + ":" + env["LD_PRELOAD"]) if env.get("LD_PRELOAD") else sys_cxx
    r = subprocess.run([PY39, "-W", "ignore", SCRIPT], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "EXTREMA-DASK-OK" in r.stdout
