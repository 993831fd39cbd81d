"""histogram_quantile on the MI355X, bit for bit against tests/quantile_oracle.py (np.nanquantile per bin): both families (the
radix select of long rows, the LDS sort of short rows, on both sides of the threshold), every digitize form of the fast family
in both of its passes (window and digits), the generic family's three compare domains with slots in LDS and counters in
global memory, rows / axes / grouped rows / broadcast values, row chunks of the radix scratch, hard data (ties, +-0, +-inf,
NaN values, keys sharing 50+ leading bits), q in {0, 1, 0.5, five quantiles} x numpy's five methods, and the numpy, torch and
DeviceArray backends.  Between them the cases select every kernel of xhist_quantile.hip (the census of the -m gpu session
holds them to that); describe() shows the family, home, d, passes and chunks reached."""
import os
import subprocess

import numpy as np
import pytest

import quantile_oracle as qo

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

METHODS = ("linear", "lower", "higher", "midpoint", "nearest")
QS = (0.0, 1.0, 0.5, [0.1, 0.25, 0.5, 0.75, 0.9])


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from xhistogram_amd import _native

    if _native.device_count() < 1:
        pytest.skip("no MI355X visible")


DESCS = []


@pytest.fixture(autouse=True)
def _record_describe(monkeypatch):
    """the describe() line of the plan after every execute_quantile, for the path assertions"""
    from xhistogram_amd import _native

    orig = _native.Plan.execute_quantile

    def wrapped(self, *a, **kw):
        orig(self, *a, **kw)
        DESCS.append(self.describe())

    monkeypatch.setattr(_native.Plan, "execute_quantile", wrapped)
    DESCS.clear()
    yield


def _core():
    from xhistogram_amd import core

    return core


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _check(args, values, bins, q=0.5, method="linear", axis=None, path=()):
    got, edges = _core().histogram_quantile(*args, values=values, q=q, bins=bins, axis=axis, method=method)
    want = qo.histogram_quantile(*[_np(a) for a in args], values=_np(values), q=q, bins=[_np(e) for e in edges], axis=axis,
                                 method=method)
    g = _np(got)
    assert g.dtype == np.float64 and g.shape == want.shape, (g.shape, want.shape)
    np.testing.assert_array_equal(g, want, err_msg="%s q=%r %s" % (method, q, DESCS[-1:] if DESCS else ""))
    for p in path:
        assert DESCS and p in DESCS[-1], (p, DESCS[-1:] if DESCS else None)
    return got


def _inside(edges, n, rng):
    """n samples spread over the edges' range, some on the edges themselves"""
    e = np.asarray(edges, np.float64)
    x = rng.uniform(e[0], e[-1], n)
    on = rng.random(n) < 0.05
    x[on] = e[rng.integers(0, len(e), on.sum())]
    return x


def _case(rng, edges, n, sdt=np.float64, vdt=np.float64, shape=None):
    """samples inside the edges (2 % outside, 1 % NaN), values with ties, +-0, +-inf and 1 % NaN"""
    shape = shape or (n,)
    sdts = sdt if isinstance(sdt, (list, tuple)) else [sdt] * len(edges)
    xs = []
    for e, dt in zip(edges, sdts):
        x = _inside(e, int(np.prod(shape)), rng).reshape(shape)
        if np.dtype(dt).kind == "f":
            x[rng.random(shape) < 0.02] = np.asarray(e, np.float64)[-1] + 1.0
            x[rng.random(shape) < 0.01] = np.nan
        xs.append(x.astype(dt))
    v = np.round(rng.standard_normal(shape) * 4.0, 1)
    sp = rng.random(shape)
    v[sp < 0.01] = -0.0
    v[(sp >= 0.01) & (sp < 0.015)] = np.inf
    v[(sp >= 0.015) & (sp < 0.02)] = -np.inf
    if np.dtype(vdt).kind == "f":
        v[(sp >= 0.02) & (sp < 0.03)] = np.nan
        v = v.astype(vdt)
    else:
        v = np.nan_to_num(v, posinf=7.0, neginf=-7.0).astype(vdt)
    return xs, v


def _cuda(a):
    return torch.as_tensor(a).cuda()


LIN = np.linspace(-2.0, 3.0, 101)
TWO = np.sort(np.r_[np.linspace(-2.0, 3.0, 81), 0.0001])  # one bucket with two edges: the two-edge scan
L5 = np.linspace(-2.0, 3.0, 5)
LONG = 6000  # columns of a radix-family row (the short-row family takes rows of at most 4096)


# ---- 1. the fast family: every digitize form in both passes -------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["one", "two"])
@pytest.mark.parametrize("D", [1, 2])
def test_fast_table_forms(dt, kind, D):
    rng = np.random.default_rng(10 * D + (dt == np.float32) + 3 * (kind == "two"))
    first = LIN if kind == "one" else TWO
    edges = [first] if D == 1 else [first, L5]
    xs, v = _case(rng, edges, 3 * LONG, sdt=dt, vdt=dt)
    scan = 1 if kind == "one" else 2
    for q in (0.5, [0.1, 0.25, 0.5, 0.75, 0.9]):
        _check([_cuda(x) for x in xs], _cuda(v), edges, q=q, path=("family=radix", "window=fast/lds", "digits=fast/lds",
                                                                    "scan=%d/%d" % (scan, scan)))
    # several rows, one kept axis
    xr_, vr = _case(rng, edges, 0, sdt=dt, vdt=dt, shape=(3, LONG))
    _check([_cuda(x) for x in xr_], _cuda(vr), edges, q=[0.25, 0.75], method="midpoint", axis=1, path=("family=radix", "window=fast"))


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("D", [1, 2])
def test_fast_arith_forms(dt, D):
    """arithmetic edges whose tables do not fit LDS next to the slots: 1800 bins (the digit pass: 88-byte slots at d = 4) and
    4000 bins (the window pass: 36-byte slots; the digits then count in global memory)"""
    rng = np.random.default_rng(40 + D + (dt == np.float32))
    e1800 = [np.linspace(-1.0, 2.0, 1801)] if D == 1 else [np.linspace(-1.0, 2.0, 4), np.linspace(-1.0, 2.0, 601)]
    xs, v = _case(rng, e1800, 8 * LONG, sdt=dt, vdt=dt)
    _check([_cuda(x) for x in xs], _cuda(v), e1800, q=0.5, path=("family=radix", "digits=fast/lds", "scan=", "/5", "d=4"))
    e4000 = [np.linspace(-1.0, 2.0, 4001)] if D == 1 else [np.linspace(-1.0, 2.0, 5), np.linspace(-1.0, 2.0, 1001)]
    xs, v = _case(rng, e4000, 8 * LONG, sdt=dt, vdt=dt)
    _check([_cuda(x) for x in xs], _cuda(v), e4000, q=0.5, method="nearest", path=("family=radix", "window=fast/lds", "scan=5/",
                                                                                   "digits=generic/global"))


# ---- 2. the generic family: compare domains, LDS and global homes -----------------------------------------------------------
@pytest.mark.parametrize("dom", ["f64", "i64", "mixed"])
def test_generic_domains_lds_and_global(dom):
    rng = np.random.default_rng(50 + ["f64", "i64", "mixed"].index(dom))
    if dom == "f64":  # float64 samples, float32 values: the generic family in the float64 domain
        small, big = [LIN], [np.linspace(-2.0, 3.0, 1025)] * 2
        sdt, vdt = np.float64, np.float32
    elif dom == "i64":
        small = [np.arange(0, 2000, 17, dtype=np.int64)]
        big = [np.arange(0, 2050, 2, dtype=np.int64), np.arange(0, 1025, dtype=np.int64)]
        sdt, vdt = np.int64, np.float64
    else:
        small, big = [LIN, np.arange(0, 100, 9, dtype=np.int64)], [np.linspace(-2.0, 3.0, 1025), np.arange(0, 1025, dtype=np.int64)]
        sdt, vdt = [np.float32, np.int64], np.int32
    xs, v = _case(rng, small, 2 * LONG, sdt=sdt, vdt=vdt)
    _check(xs, v, small, q=[0.1, 0.5, 0.9], path=("family=radix", "window=generic/lds", "digits=generic/lds"))
    # 1024 x 1024 bins: windows and counters in global memory
    xs, v = _case(rng, big, 2 * LONG, sdt=sdt, vdt=vdt)
    _check(xs, v, big, q=0.5, path=("family=radix", "window=generic/global", "digits=generic/global"))
    # the short-row family in the same domain
    xs, v = _case(rng, small, 0, sdt=sdt, vdt=vdt, shape=(7, 900))
    _check(xs, v, small, q=[0.25, 0.75], method="higher", axis=1, path=("family=short",))


def test_datetime_samples():
    rng = np.random.default_rng(60)
    te = np.arange(np.datetime64("2020-01-01"), np.datetime64("2021-02-01"), np.timedelta64(10, "D")).astype("datetime64[s]")
    t = te[0] + (rng.uniform(0, 1, 2 * LONG) * (te[-1] - te[0]).astype(np.int64)).astype("timedelta64[s]")
    v = np.round(rng.standard_normal(2 * LONG), 2)
    _check([t], v, [te], q=[0.1, 0.5, 0.9], path=("family=radix", "cmp=1"))


# ---- 3. hard data, every q and method, both families ---------------------------------------------------------------------
def _hard(n_cols, rng):
    """one row of n_cols samples over 10 bins of [0, 10): bin 0 every value equal, bin 1 one value, bin 2 two, bin 3 empty,
    bin 4 +-0 mixed, bin 5 +-inf with finite values, bin 6 values 1 + k ulp, bin 7 keys sharing 52 leading bits, bin 8 heavy
    ties, bin 9 random; NaN values everywhere, NaN and out-of-range samples"""
    x = np.empty(n_cols)
    v = np.empty(n_cols)
    nb = [0] * 10
    rest = n_cols - 3
    per = rest // 7
    layout = [(0, per), (1, 1), (2, 2), (4, per), (5, per), (6, per), (7, per), (8, per), (9, rest - 6 * per)]
    i = 0
    for b, k in layout:
        x[i:i + k] = b + rng.uniform(0.0, 0.999, k)
        nb[b] += k
        if b == 0:
            v[i:i + k] = 2.5
        elif b == 1:
            v[i:i + k] = -3.0
        elif b == 2:
            v[i:i + k] = [np.inf, np.inf]
        elif b == 4:
            v[i:i + k] = np.where(rng.random(k) < 0.5, -0.0, 0.0)
        elif b == 5:
            v[i:i + k] = rng.choice([-np.inf, np.inf, 1.0, -2.0], k)
        elif b == 6:
            v[i:i + k] = np.nextafter(1.0, 2.0) ** rng.integers(0, 9, k)
        elif b == 7:
            v[i:i + k] = (np.float64(1.5).view(np.uint64) + rng.integers(0, 1 << 11, k).astype(np.uint64)).view(np.float64)
        elif b == 8:
            v[i:i + k] = rng.integers(-2, 3, k).astype(np.float64)
        else:
            v[i:i + k] = rng.standard_normal(k)
        i += k
    nanv = rng.random(n_cols) < 0.03
    nanv[:5] = False
    v[nanv & (x >= 3)] = np.nan
    x[rng.random(n_cols) < 0.02] = 11.0
    x[rng.random(n_cols) < 0.01] = np.nan
    p = rng.permutation(n_cols)
    return x[p], v[p]


@pytest.mark.parametrize("n_cols,family", [(LONG, "radix"), (3000, "short")])
@pytest.mark.parametrize("method", METHODS)
def test_hard_data_every_q_and_method(n_cols, family, method):
    rng = np.random.default_rng(70 + n_cols)
    x, v = _hard(n_cols, rng)
    e = np.arange(11.0)
    for q in QS:
        _check([_cuda(x)], _cuda(v), [e], q=q, method=method, path=("family=" + family,))
    # float32 values of the same data
    _check([_cuda(x.astype(np.float32))], _cuda(v.astype(np.float32)), [e], q=[0.0, 0.5, 1.0], method=method, path=("family=" + family,))


def test_all_values_equal_and_empty_bins():
    rng = np.random.default_rng(80)
    x = rng.uniform(0, 4, LONG)
    e = np.linspace(0, 8, 9)  # bins 4..7 empty
    for v in (np.full(LONG, 7.25), np.full(LONG, -0.0), np.full(LONG, np.nan)):
        for m in METHODS:
            _check([x], v, [e], q=[0.0, 0.5, 1.0], method=m, path=("family=radix",))


# ---- 4. rows, axes, grouped rows, broadcast values, the threshold, row chunks --------------------------------------------
def test_rows_axes_and_views():
    rng = np.random.default_rng(90)
    x = rng.uniform(-2.2, 3.2, (3, LONG, 4))
    v = np.round(rng.standard_normal((3, LONG, 4)), 1)
    _check([_cuda(x)], _cuda(v), [LIN], q=[0.25, 0.5], axis=1, path=("family=radix",))  # a middle axis: grouped rows
    _check([_cuda(x)], _cuda(v), [LIN], q=0.5, axis=(0, 1), path=("family=radix",))
    _check([x], v, [LIN], q=0.9, axis=None, path=("family=radix",))
    # a leading (time) axis: the short-row family, several rows per workgroup
    xt = rng.uniform(-2.2, 3.2, (365, 12, 30)).astype(np.float32)
    vt = np.round(rng.standard_normal((365, 12, 30)), 1).astype(np.float32)
    _check([_cuda(xt)], _cuda(vt), [np.linspace(-2, 3, 51)], q=[0.1, 0.5, 0.9], axis=0, path=("family=short", "rows_per_wg=11"))
    # values broadcast along the rows
    vb = np.round(rng.standard_normal(LONG), 1)
    _check([_cuda(x[:, :, 0])], _cuda(vb), [LIN], q=0.5, axis=1, path=("family=radix",))


@pytest.mark.parametrize("n_cols,family", [(4096, "short"), (4097, "radix")])
def test_short_row_threshold(n_cols, family):
    rng = np.random.default_rng(100 + n_cols)
    x = rng.uniform(-2.2, 3.2, (5, n_cols))
    v = np.round(rng.standard_normal((5, n_cols)), 2)
    for m in METHODS:
        _check([_cuda(x)], _cuda(v), [LIN], q=[0.1, 0.5, 0.9], method=m, axis=1, path=("family=" + family,))


def test_row_chunks():
    """9000 rows of 4200 values, 100 bins, two quantiles: the radix scratch (712 bytes per (row, bin): two targets at d = 5)
    takes three chunks of 3770 rows;
    the rows at both chunk borders and at the ends against the oracle, the others by the histogram's counts"""
    rng = np.random.default_rng(110)
    x = rng.uniform(-2.2, 3.2, (9000, 4200)).astype(np.float32)
    v = np.round(rng.standard_normal((9000, 4200)), 1).astype(np.float32)
    got, _ = _core().histogram_quantile(_cuda(x), values=_cuda(v), q=[0.25, 0.5], bins=[LIN], axis=1)
    assert "family=radix" in DESCS[-1] and "group=2" in DESCS[-1] and "chunks=3 " in DESCS[-1], DESCS[-1]
    g = _np(got)
    for r0 in (0, 3720, 7490, 8900):
        want = qo.histogram_quantile(x[r0:r0 + 100], values=v[r0:r0 + 100], q=[0.25, 0.5], bins=[LIN], axis=1)
        np.testing.assert_array_equal(g[:, r0:r0 + 100], want)
    counts, _ = _core().histogram(_cuda(x), bins=[LIN], axis=1)
    np.testing.assert_array_equal(np.isnan(g[0]), _np(counts) == 0)


# ---- 5. many q values: groups of targets ------------------------------------------------------------------------------------
def test_many_q_groups():
    rng = np.random.default_rng(120)
    x = rng.uniform(-2.2, 3.2, 3 * LONG)
    v = np.round(rng.standard_normal(3 * LONG), 2)
    q = np.linspace(0, 1, 11)
    _check([_cuda(x)], _cuda(v), [LIN], q=q, path=("family=radix",))
    assert int(DESCS[-1].split("groups=")[1].split()[0]) >= 2
    _check([_cuda(x[:3000])], _cuda(v[:3000]), [LIN], q=q, method="midpoint", path=("family=short", "groups=2"))


# ---- 6. backends --------------------------------------------------------------------------------------------------------------
def test_backends():
    from xhistogram_amd import core
    from xhistogram_amd.devicearray import DeviceArray

    rng = np.random.default_rng(130)
    x = rng.uniform(-2.2, 3.2, (4, LONG))
    v = np.round(rng.standard_normal(x.shape), 1)
    a, ea = core.histogram_quantile(x, values=v, q=[0.25, 0.75], bins=[LIN], axis=1)
    b, _ = core.histogram_quantile(_cuda(x), values=_cuda(v), q=[0.25, 0.75], bins=[LIN], axis=1)
    c, _ = core.histogram_quantile(DeviceArray.from_numpy(x), values=DeviceArray.from_numpy(v), q=[0.25, 0.75], bins=[LIN], axis=1)
    assert isinstance(a, np.ndarray) and isinstance(c, np.ndarray) and b.is_cuda and b.dtype == torch.float64
    assert a.shape == (2, 4, 100)
    np.testing.assert_array_equal(_np(b), a)
    np.testing.assert_array_equal(c, a)
    np.testing.assert_array_equal(a, qo.histogram_quantile(x, values=v, q=[0.25, 0.75], bins=[LIN], axis=1))
    m, _ = core.histogram_quantile(x, values=v, q=0.5, bins=[LIN], axis=1)
    assert m.shape == (4, 100)
    # torch on a side stream: asynchronous, the result follows the stream's order
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t, _ = core.histogram_quantile(_cuda(x), values=_cuda(v), q=0.5, bins=[LIN], axis=1)
    s.synchronize()
    np.testing.assert_array_equal(_np(t), m)
    # int / estimator bins: the edges of the unweighted histogram
    _, e2 = core.histogram_quantile(x, values=v, q=0.5, bins=20)
    np.testing.assert_array_equal(e2[0], np.histogram_bin_edges(x, bins=20))


# ---- 7. dask ------------------------------------------------------------------------------------------------------------------
PY39 = "/opt/conda/bin/python3.9"
SCRIPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "quantile_dask_script.py")


def _have_dask_python():
    return os.path.exists(PY39) and subprocess.run([PY39, "-c", "import dask.array, numpy"], capture_output=True).returncode == 0


@pytest.mark.skipif(not _have_dask_python(), reason="no interpreter with dask in this image")
def test_dask_blocks_complete_along_the_reduced_axes():
    env = dict(os.environ)
    sys_cxx = "/usr/lib/x86_64-linux-gnu/libstdc++.so.6"  # (as tests/test_dask_branch.py: conda's libstdc++ is older)
    if os.path.exists(sys_cxx):
        env["LD_PRELOAD"] = (sys_cxx + ":" + env["LD_PRELOAD"]) if env.get("LD_PRELOAD") else sys_cxx
    r = subprocess.run([PY39, "-W", "ignore", SCRIPT], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "QUANTILE-DASK-OK" in r.stdout
