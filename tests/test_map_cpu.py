"""tests/map_oracle.py held to what it restates, where no GPU is needed: its index against the golden hot-path vectors and
against np.digitize on edges and special values, its lookup and anomaly on a case small enough to write down, the borders of
the restated kernel choice, and that every case table of tests/map_cases.py (the GPU module's) lands on the kernel it is meant for.  Also the
Python front's surface: the symbol, the Plan method, the public functions and their checks before any device work.  Last, what
tests/test_gpu_map_properties.py relies on: the conditions of its 120 replayed cases and drawn tables (tallies printed), the
interval of the standardized anomaly, the closed form of the row-chunk test against the oracle, and the 8-input case."""
import os

import numpy as np
import pytest

import map_cases as mc
import map_oracle as mo
from conftest import MANIFEST, assert_hist_equal
from map_oracle import last as _last, table_bytes

F64, F32 = np.float64, np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256
LDS = mo.LDS_MAX


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's results
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MANIFEST["hotpath"]))
def test_bincount_of_the_index_is_the_golden_histogram(golden, name):
    samples, edges, w, out = golden.hotpath_case(name)
    idx = mo.index(samples, edges)
    assert idx.shape == samples[0].shape and idx.dtype == np.int64
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    assert idx.max(initial=-1) < n_bins and idx.min(initial=0) >= -1
    rows = []
    for r in range(idx.shape[0]):
        ok = idx[r] >= 0
        rows.append(np.bincount(idx[r][ok], weights=None if w is None else np.asarray(w[r], F64)[ok], minlength=n_bins))
    got = np.array(rows).reshape(out.shape)
    assert_hist_equal(got if w is not None else got.astype(np.int64), out, w is not None)


@pytest.mark.parametrize("dt", [F64, F32])
def test_index_against_np_digitize_on_edges_and_specials(dt):
    edges = np.sort(np.random.default_rng(3).uniform(-4.0, 4.0, 13))
    e = edges.astype(dt).astype(F64) if dt == F32 else edges
    x = np.concatenate([e, np.nextafter(e.astype(dt), dt(np.inf)), np.nextafter(e.astype(dt), dt(-np.inf)),
                        [np.nan, np.inf, -np.inf, 0.0, -0.0, edges[-1], edges[0]]]).astype(dt)
    idx = mo.index([x], [edges])
    d = np.digitize(x.astype(F64), edges)  # i: edges[i - 1] <= x < edges[i]; 0 below; E at and above the last edge, and NaN
    want = np.where((d >= 1) & (d <= 12), d - 1, -1)
    want[x.astype(F64) == edges[-1]] = 11  # the last bin is closed on the right
    np.testing.assert_array_equal(idx, want)
    assert idx[np.isnan(x)].tolist() == [-1] and (idx[np.isinf(x)] == -1).all()
    zero = mo.index([np.array([0.0, -0.0])], [np.array([0.0, 1.0])])
    assert zero.tolist() == [0, 0]  # (-0.0 == 0.0: on the first edge)


def test_pairs_drop_a_sample_out_of_range_in_either_dimension():
    e = [np.array([0.0, 1.0, 2.0]), np.array([0.0, 1.0, 2.0, 3.0])]
    x = np.array([0.5, 1.5, 2.0, -0.1, 0.5, np.nan, 1.0])
    y = np.array([2.5, 0.0, 3.0, 1.0, 3.1, 1.0, np.nan])
    assert mo.index([x, y], e).tolist() == [2, 3, 5, -1, -1, -1, -1]
    assert mo.index([x, y], e).tolist() == [int(np.ravel_multi_index((a, b), (2, 3))) if ok else -1
                                            for a, b, ok in [(0, 2, 1), (1, 0, 1), (1, 2, 1), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)]]


def test_lookup_and_anomaly_written_down():
    edges = [np.array([0.0, 1.0, 2.0])]
    x = np.array([[0.5, 1.5, 2.5], [1.0, np.nan, 0.0]])
    table = np.array([[10.0, 20.0], [30.0, 40.0]])
    out = mo.lookup([x], edges, table, axis=1)
    mo.assert_bits(out, np.array([[10.0, 20.0, np.nan], [40.0, np.nan, 30.0]]))
    v = np.array([[1.0, 2.0, 3.0], [np.nan, 5.0, 6.0]])
    an = mo.anomaly([x], edges, v, table, np.array([[2.0, 0.0], [4.0, 8.0]]), axis=1)
    mo.assert_bits(an, np.array([[-4.5, -np.inf, np.nan], [np.nan, np.nan, -6.0]]))
    full = mo.lookup([x], edges, np.array([7.0, 9.0]))
    mo.assert_bits(full, np.array([[7.0, 9.0, np.nan], [9.0, np.nan, 7.0]]))
    with pytest.raises(AssertionError):
        mo.assert_bits(np.array([0.0]), np.array([-0.0]))
    with pytest.raises(AssertionError):
        mo.assert_bits(np.array([np.nan, 1.0]), np.array([1.0, np.nan]))


def test_lookup_over_a_leading_and_a_split_axis():
    rng = np.random.default_rng(0)
    edges = [np.linspace(0, 1, 5)]
    x = rng.uniform(-0.1, 1.1, (3, 4, 5))
    for axis, kept in (((0,), (4, 5)), ((0, 2), (4,)), ((1,), (3, 5))):
        table = rng.standard_normal(kept + (4,))
        out = mo.lookup([x], edges, table, axis)
        idx = mo.index([x], edges)
        for pos in np.ndindex(*x.shape):
            k = tuple(p for i, p in enumerate(pos) if i not in axis)
            want = table[k + (idx[pos],)] if idx[pos] >= 0 else np.nan
            assert (np.isnan(want) and np.isnan(out[pos])) or out[pos] == want


def test_exact_mean_is_the_sum_over_the_count():
    rng = np.random.default_rng(1)
    import values_exact as vx

    edges = [np.linspace(-1, 1, 6)]
    x = rng.uniform(-1.1, 1.1, (2, 300))
    v = vx.grid(rng, (2, 300))
    w = rng.integers(0, 8, (2, 300)).astype(F64)
    idx = mo.index([x], edges)
    mean, wmean = mo.exact_mean([x], edges, v, (1,)), mo.exact_mean([x], edges, v, (1,), w)
    for r in range(2):
        for b in range(5):
            sel = idx[r] == b
            assert mean[r, b] == v[r][sel].sum() / sel.sum()
            assert wmean[r, b] == (w[r][sel] * v[r][sel]).sum() / w[r][sel].sum()


# ---------------------------------------------------------------------------------------------------------------------
# the restated choice: its borders
# ---------------------------------------------------------------------------------------------------------------------
def _lin(nb):
    return [np.linspace(-4.0, 4.0, nb + 1)]


def _fam(op, nb, st, scale=False, fine=1, arith=True, vdt="same"):
    vdt = (st if op == "anomaly" else None) if vdt == "same" else vdt
    p = mo.predict(op, CUS, _lin(nb), 0, st, vdt, 1, 1, scale=scale, fine=fine, arith=arith)
    return p["family"], p["table"], p["scan"]


def test_table_bytes_is_the_statistics_census_statement():
    """the restated table sizes against tests/test_gpu_values_census.py's, where that module can be imported (it needs torch)"""
    pytest.importorskip("torch")
    import test_gpu_values_census as vc

    assert mo.LDS_MAX == vc.LDS_MAX
    for which in ("native", "fine64", "fine32"):
        for ns in ((2,), (9,), (101,), (301,), (2_304,), (12_001,), (30_001,), (70_000,), (25, 31), (4, 19_001)):
            e = [np.zeros(n) for n in ns]
            assert mo.table_bytes(e, which) == vc.table_bytes(e, which), (which, ns)


def test_slots():
    assert [mo.slot_bytes(op) for op in mo.OPS] == [0, 8, 8] and mo.slot_bytes("anomaly", True) == 16 and mo.slot_bytes("index", True) == 0


@pytest.mark.parametrize("st,which", [(F64, "fine64"), (F32, "fine32")])
def test_fast_borders(st, which):
    """the last bin count whose fine tables fit LDS next to the table rows, per slot size; beyond it arithmetic edges run
    table-free up to 160 KiB of rows, and everything else falls to the generic family"""
    for op, scale, slot in (("index", False, 0), ("take", False, 8), ("anomaly", False, 8), ("anomaly", True, 16)):
        last_fine = _last(lambda n: table_bytes([np.zeros(n + 1)], which) + n * slot <= LDS)
        assert _fam(op, last_fine, st, scale) == ("fast", "none" if op == "index" else "lds", 1)
        assert _fam(op, last_fine + 1, st, scale)[:1] + _fam(op, last_fine + 1, st, scale)[2:] == ("fast", 5)
        assert _fam(op, last_fine + 1, st, scale, arith=False)[0] == "generic"
        if slot:
            last_arith = LDS // slot
            assert last_arith == {8: 20_480, 16: 10_240}[slot]
            assert _fam(op, last_arith, st, scale) == ("fast", "lds", 5)
            assert _fam(op, last_arith + 1, st, scale)[:2] == ("generic", "global")
    assert _fam("anomaly", 100, st, vdt=F32 if st == F64 else F64)[0] == "generic"  # values of another type
    assert mo.predict("take", CUS, _lin(100), 0, st, None, 1, 100, layout_fast=False)["family"] == "generic"
    assert mo.predict("take", CUS, _lin(100), 1, st, None, 1, 100)["family"] == "generic"  # another compare domain


def test_generic_table_homes():
    for slot, op, scale in ((8, "take", False), (16, "anomaly", True)):
        last = _last(lambda n: table_bytes([np.zeros(n + 1)], "native") + n * slot <= LDS)
        for nb, home in ((last, "lds"), (last + 1, "global")):
            p = mo.predict(op, CUS, _lin(nb), 0, np.int32, F64 if op == "anomaly" else None, 1, 1, scale=scale, fine=False)
            assert (p["family"], p["table"], p["tables_in_lds"]) == ("generic", home, 1)
    last_t = _last(lambda n: table_bytes([np.zeros(n + 1)], "native") + 1024 <= LDS)
    for op in mo.OPS:
        for nb, til in ((last_t, 1), (last_t + 1, 0)):
            p = mo.predict(op, CUS, _lin(nb), 0, np.int32, F64 if op == "anomaly" else None, 1, 1, fine=False)
            assert (p["family"], p["tables_in_lds"]) == ("generic", til)
            assert p["table"] == ("none" if op == "index" else "global")
            assert p["lds_bytes"] == (table_bytes(_lin(nb), "native") if til else 0)


def test_geometry():
    assert [mo.tile_of(F64, 1), mo.tile_of(F64, 2), mo.tile_of(F32, 1), mo.tile_of(F32, 2)] == [2048, 2048, 4096, 2048]
    p = mo.predict("take", CUS, _lin(50), 0, F64, None, 3, 2 * 2048 + 5)
    assert (p["block"], p["segs"]) == (256, 3)
    p = mo.predict("take", CUS, _lin(50), 0, np.int32, None, 3, 1500, fine=False)
    assert (p["block"], p["segs"]) == (512, 3)
    p = mo.predict("index", CUS, _lin(50), 0, F32, None, 1, 10 ** 9)
    assert p["segs"] == CUS * 8  # every resident workgroup: 8 blocks of 256 lanes per CU


# ---------------------------------------------------------------------------------------------------------------------
# the GPU module's case tables land where they are meant to
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("st", [F64, F32])
@pytest.mark.parametrize("form", list(mc.FAST_FORMS))
@pytest.mark.parametrize("op", mo.OPS)
def test_fast_cases_are_predicted_fast(op, form, st, D):
    cols = [c for _, c in mc.fast_shapes(st, D)]
    t = mo.tile_of(st, D)
    assert cols == [1, 3, t - 1, t, t + 1, 2 * t + 5]
    for scale in (False, True) if op == "anomaly" else (False,):
        kind, nbs, fine, arith = mc.fast_form(form, op, st, D, scale)
        edges = [np.linspace(-4.0, 4.0, nb + 1) for nb in nbs]  # (the choice reads the number of edges only)
        p = mo.predict(op, CUS, edges, 0, st, st if op == "anomaly" else None, 3, cols[-1], scale=scale, fine=fine, arith=arith)
        assert p["family"] == "fast" and p["scan"] == (5 if form == "arith" else fine), (p, scale)
        assert p["segs"] == 3


@pytest.mark.parametrize("home", list(mc.HOMES))
def test_generic_cases_are_predicted_home(home):
    nb, scale = mc.HOMES[home]
    for op in mo.OPS:
        if scale and op != "anomaly":
            continue
        p = mo.predict(op, CUS, _lin(nb), 0, np.int32, F64 if op == "anomaly" else None, 3, 1500, scale=scale, fine=False)
        assert p["family"] == "generic" and p["tables_in_lds"] == (0 if home == "global_l2" else 1)
        assert p["table"] == ("none" if op == "index" else "lds" if home == "lds" else "global")
    assert [c for _, c in mc.GENERIC_SHAPES] == [511, 512, 513, 1500]


def test_pow2_data_has_power_of_two_counts():
    rng = np.random.default_rng(2)
    edges = np.linspace(-1.0, 1.0, 9)
    for axis in mc.AXES:
        x, v = mc.pow2_data(rng, (5, 37, 11), edges, axis)
        assert x.shape == v.shape == (5, 37, 11)
        idx = mo.index([x], [edges])
        i2, _, _ = mo._rows(idx, axis, 3)
        for row in i2:
            cnt = np.bincount(row[row >= 0], minlength=8)
            assert set(cnt.tolist()) <= {0, 1, 2, 4, 8, 16} and cnt.sum() > 0  # (rows shorter than the bins leave some empty)
        import values_exact as vx
        assert vx.on_grid(v)


# ---------------------------------------------------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------------------------------------------------
def test_symbol_header_and_plan_method():
    from xhistogram_amd import _native

    assert "xhist_plan_execute_map" in _native.EXPORTS
    header = open(os.path.join(ROOT, "include", "xhist_amd.h")).read()
    assert "xhist_plan_execute_map(" in header
    for name, code in (("XHIST_MAP_INDEX", 0), ("XHIST_MAP_TAKE", 1), ("XHIST_MAP_ANOMALY", 2)):
        assert "#define %s %d" % (name, code) in header
    assert (_native.MAP_INDEX, _native.MAP_TAKE, _native.MAP_ANOMALY) == (0, 1, 2)
    lib = _native.load()
    assert len(lib.xhist_plan_execute_map.argtypes) == 11
    assert callable(getattr(_native.Plan, "execute_map"))


def test_public_functions_check_before_any_device_work(monkeypatch):
    from xhistogram_amd import core, xarray as xhx

    for fn in ("bin_index", "histogram_lookup", "histogram_anomaly"):
        assert callable(getattr(core, fn)) and fn in xhx.__all__
    monkeypatch.setattr(core, "_upload_host", lambda *a, **k: pytest.fail("device work"))
    x = np.zeros((4, 6))
    edges = [np.linspace(0.0, 1.0, 4)]
    with pytest.raises(ValueError, match=r"table has shape \(4, 4\), but histogram gives \(4, 3\)"):
        core.histogram_lookup(x, table=np.zeros((4, 4)), bins=edges, axis=1)
    with pytest.raises(ValueError, match=r"table has shape \(6, 3\), but histogram gives \(4, 3\)"):
        core.histogram_lookup(x, table=np.zeros((6, 3)), bins=edges, axis=-1)
    with pytest.raises(TypeError, match="complex values have no order: histogram_lookup takes real values"):
        core.histogram_lookup(x, table=np.zeros((4, 3), np.complex128), bins=edges, axis=1)
    with pytest.raises(TypeError, match="histogram_anomaly needs values"):
        core.histogram_anomaly(x, values=None, bins=edges)
    with pytest.raises(ValueError, match="bins must be provided"):
        core.bin_index(x)


def test_values_call_without_values_keeps_the_samples():
    from xhistogram_amd import core

    x, y = np.zeros((2, 3)), np.zeros((1, 3))
    e = [np.linspace(0, 1, 3)] * 2
    backend, arrays, raw, bins, axis, drop = core._values_call((x, y), None, e, None, [1], "bin_index", needs_values=False)
    assert backend == "numpy" and len(arrays) == 2 and arrays[1].shape == (2, 3) and axis == [1] and drop == (1,)
    with pytest.raises(TypeError, match="histogram_extrema needs values"):
        core._values_call((x,), None, e[:1], None, None, "histogram_extrema")


# ---------------------------------------------------------------------------------------------------------------------
# what tests/test_gpu_map_properties.py relies on
# ---------------------------------------------------------------------------------------------------------------------
def _replayed(stat):
    """the 60 cases of `stat` as tests/test_gpu_map_properties.py replays them, built, with what the maps must give on them"""
    pytest.importorskip("hypothesis")
    pytest.importorskip("torch")  # (for_each_case lives in a GPU file that imports it; none of this needs a GPU)
    import test_gpu_values_properties as tgp
    import values_cases as vc

    if stat not in _REPLAYED:
        cases = []
        tgp.for_each_case(stat, tgp.EXAMPLES, cases.append)
        assert len(cases) == tgp.EXAMPLES
        _REPLAYED[stat] = [(c, mc.expectations(vc.build(c))) for c in cases]
    return _REPLAYED[stat]


_REPLAYED = {}


def _ieee(w, var=None):
    with np.errstate(invalid="ignore", divide="ignore"):
        return w["anomaly"] / np.sqrt(w["var"] if var is None else var)


@pytest.mark.parametrize("stat", mc.MAP_STATS)
def test_replayed_cases_meet_their_conditions(stat):
    """the conditions under which the comparisons of test_gpu_map_properties.test_random_cases_match_oracle bite; the tallies
    are those of that file's docstring (pytest -s prints them)"""
    import collections

    t = collections.Counter()
    largest = 0
    for case, w in _replayed(stat):
        n = int(np.prod(case["shape"]))
        largest = max(largest, n)
        t["without an element"] += n == 0
        t["a finite mean"] += bool(np.isfinite(w["mean"]).any())
        t["a finite positive variance"] += bool((np.isfinite(w["var_table"]) & (w["var_table"] > 0)).any())
        n_exact, n_bracket = mo.assert_standardized(_ieee(w), w["anomaly"], w["var"], w["bound"], repr(case))
        t["bit-for-bit branch"] += n_exact > 0
        t["bracket branch"] += n_bracket > 0
        spec, buf, view, image = mc.table_draw(case)
        kept, bins = mc.table_shape(case)
        assert view.shape == image.shape == kept + bins and view.dtype == np.dtype(spec["dtype"])
        assert np.array_equal(np.asarray(view, F64), image) and image.flags.c_contiguous
        for k in ("dtype", "container", "laid"):
            t["%s %s" % (k, spec[k])] += 1
        if view.ndim > 1 and min(view.shape) > 1:
            assert view.flags.c_contiguous == (spec["laid"] == "contiguous"), spec
            t["tables that are not one contiguous block"] += not view.flags.c_contiguous
        if spec["laid"] == "broadcast":
            assert not view.flags.writeable and 0 in view.strides
        if spec["container"] == "list":
            assert np.shape(view.tolist()) == view.shape
    print("\n%s: largest case %d elements; %s" % (stat, largest, ", ".join("%s %d" % kv for kv in sorted(t.items()))))
    assert t["a finite mean"] >= 55 and t["a finite positive variance"] >= 40 and t["without an element"] <= 5
    assert t["bit-for-bit branch"] >= 10 and t["bracket branch"] >= 10
    for k, options in (("dtype", mc.TABLE_DTYPES), ("container", mc.TABLE_CONTAINERS), ("laid", mc.TABLE_LAYOUTS)):
        for o in options:
            assert t["%s %s" % (k, o)] >= 2, (k, o)


@pytest.mark.parametrize("stat", mc.MAP_STATS)
def test_bracket_holds_what_it_must_and_rejects_a_float32_root(stat):
    """map_oracle.standardized_bracket on the replayed cases: it contains fl(a / sqrt(var)) for var*, var* + b and var* - b
    (the variances the project's bounds allow the kernels), and a result made with a float32 square root falls outside
    wherever that root is not the float64 one to nine digits"""
    rejected = should = 0
    for case, w in _replayed(stat):
        a, var, b = w["anomaly"], w["var"], w["bound"]
        for v in (var, var + b, np.maximum(var - b, 0.0)):
            mo.assert_standardized(_ieee(w, v), a, var, b, repr(case))
        with np.errstate(invalid="ignore", divide="ignore"):
            root32 = np.sqrt(var.astype(F32)).astype(F64)
            off = np.isfinite(a) & (a != 0) & (var > 0) & (np.abs(root32 - np.sqrt(var)) > 1e-9 * np.sqrt(var))
            z32 = a / root32
        if off.any():
            should += 1
            with pytest.raises(AssertionError):
                mo.assert_standardized(z32, a, var, b)
            rejected += 1
    print("\n%s: a float32 square root rejected in %d cases of %d" % (stat, rejected, should))
    assert rejected >= 10


def test_bracket_written_down():
    nan, inf = np.nan, np.inf
    a = np.array([3.0, -3.0, 0.0, 0.0, 2.0, -2.0, 0.0, nan, 1.0])
    var = np.array([4.0, 4.0, 0.0, 4.0, 1e-30, 1e-30, 1e-30, 1.0, nan])
    b = np.array([0.0, 1.0, 0.0, 1.0, 1e-29, 1e-29, 1e-29, 0.0, nan])
    k = mo.standardized_bracket(a, var, b)
    assert k["must_nan"].tolist() == [0, 0, 0, 0, 0, 0, 0, 1, 1] and k["exact"].tolist() == [1, 0, 1, 0, 0, 0, 0, 0, 0]
    assert k["want"][0] == 1.5 and np.isnan(k["want"][2])  # (0 / 0 is IEEE's NaN, bit-for-bit branch)
    assert k["lo"][1] < -3.0 / np.sqrt(3.0) and k["hi"][1] > -3.0 / np.sqrt(5.0) and k["hi"][1] < -1.34
    assert (k["lo"][3], k["hi"][3]) == (0.0, 0.0)
    assert k["hi"][4] == inf and 1e14 < k["lo"][4] <= 2.0 / np.sqrt(1.1e-29) and k["lo"][5] == -inf and k["hi"][5] < 0
    assert k["nan_ok"].tolist() == [0, 0, 0, 0, 0, 0, 1, 0, 0]
    good = np.array([1.5, -1.5, nan, 0.0, 1e20, -inf, nan, nan, nan])
    assert mo.assert_standardized(good, a, var, b) == (2, 4)
    for i, wrong in ((0, np.nextafter(1.5, 2.0)), (1, -1.3), (2, 0.0), (4, nan), (5, 1.0), (6, 1e-3), (7, 0.0), (3, nan)):
        z = good.copy()
        z[i] = wrong
        with pytest.raises(AssertionError):
            mo.assert_standardized(z, a, var, b)


@pytest.mark.parametrize("block", [256, 512])
def test_rows_closed_form_is_the_oracle(block):
    """map_cases.rows_expected, the expectation of test_more_rows_than_one_launch, against map_oracle run by brute force on the
    rows themselves: the first 4096 rows, 2048 on each side of the first launch's last row, and the last 4096"""
    chunk = mc.launch_rows(block, 1)
    assert chunk == {256: 16_777_215, 512: 8_388_607}[block]
    n_rows = chunk + mc.ROWS_EXTRA
    windows = [np.arange(0, 4096), np.arange(chunk - 2048, chunk + 2048), np.arange(n_rows - 4096, n_rows)]
    for family, op in mc.ROW_CASES:
        if (family == "fast") != (block == 256):
            continue
        edges, xs, vs = mc.rows_data(family, op)
        assert xs.shape == (mc.P_S, mc.ROWS_COLS) and len(edges[0]) - 1 == mc.ROWS_BINS
        bin_base = mo.index([xs], edges)
        assert 0.25 < (bin_base < 0).mean() < 0.45 and set(np.unique(bin_base)) == {-1, 0, 1}
        if xs.dtype.kind == "f":
            assert np.isnan(xs).sum() >= 10
        v_base = None if vs is None else vs.astype(F64)
        for rows in windows:
            x_rows = xs[rows % mc.P_S]
            b = np.arange(mc.ROWS_BINS)[None, :]
            centre = mc.centre_of(np, rows[:, None], b)
            scale = mc.scale_of(np, rows[:, None], b, mc.SCALE_LUT)
            assert centre.shape == scale.shape == (len(rows), mc.ROWS_BINS) and centre.dtype == scale.dtype == F64
            if op == "index":
                want = mo.index([x_rows], edges)
            elif op == "take":
                want = mo.lookup([x_rows], edges, centre, axis=1)
            else:
                want = mo.anomaly([x_rows], edges, vs[rows % mc.P_V], centre, scale, axis=1)
            got = mc.rows_expected(np, op, rows, bin_base, v_base, mc.SCALE_LUT if op == "anomaly" else None)
            mo.assert_bits(got, want, "%s %s rows %d.." % (family, op, rows[0]))


def test_row_tables_make_the_arithmetic_exact():
    """centre is a multiple of 2^-3 that depends on the row and on the bin, scale a power of two that depends on both, the
    periods are coprime, and v - centre and its division by scale are exact: against fractions.Fraction"""
    import math
    from fractions import Fraction

    assert math.gcd(mc.P_S, mc.P_V) == 1 and mc.ROWS_COLS != mc.ROWS_BINS and min(mc.ROWS_COLS, mc.ROWS_BINS) > 1
    r = np.arange(0, 5000)[:, None]
    b = np.arange(mc.ROWS_BINS)[None, :]
    c, s = mc.centre_of(np, r, b), mc.scale_of(np, r, b, mc.SCALE_LUT)
    assert np.all(c * 8 == np.round(c * 8)) and np.all(np.abs(c) < 1024)
    assert np.all(np.frexp(s)[0] == 0.5)  # powers of two
    for t in (c, s):
        assert (t[:, 0] != t[:, 1]).all() and (t[:-1] != t[1:]).all()  # (it depends on the bin, and on the row)
    rng = np.random.default_rng(7)
    for family, op in (("fast", "anomaly"), ("generic", "anomaly")):
        _, _, vs = mc.rows_data(family, op)
        v = vs.astype(F64).reshape(-1)
        v = v[~np.isnan(v)]
        for _ in range(150):
            vi, ri, bi = float(rng.choice(v)), int(rng.integers(0, 1 << 24)), int(rng.integers(0, 2))
            ci = float(mc.centre_of(np, np.array(ri), np.array(bi)))
            si = float(mc.scale_of(np, np.array(ri), np.array(bi), mc.SCALE_LUT))
            assert Fraction(vi - ci) == Fraction(vi) - Fraction(ci)
            assert Fraction((vi - ci) / si) == (Fraction(vi) - Fraction(ci)) / Fraction(si)


def test_joint_inputs_straddle_32_bits():
    edges, xs = mc.joint_inputs()
    assert len(xs) == len(edges) == 8 and all(x.shape == (4099,) and x.dtype == F64 for x in xs)
    assert int(np.prod([len(e) - 1 for e in edges], dtype=object)) == 17 ** 8 == 6_975_757_441
    ok, bins = mo.per_input_bins(xs, edges)
    idx = mo.index(xs, edges)
    assert idx[:4].tolist() == [(1 << 32) - 1, 1 << 32, 0, 17 ** 8 - 1]
    assert (idx >= 1 << 32).sum() > 1000 and ((idx >= 0) & (idx < 1 << 32)).sum() > 1000
    want = np.where(ok, np.ravel_multi_index([np.where(ok, b, 0) for b in bins], (17,) * 8), -1)
    np.testing.assert_array_equal(idx, want)
    for d in range(8):  # every input drops samples that every other input counts
        others = np.ones(4099, bool)
        for k in range(8):
            if k != d:
                others &= mo.per_input_bins([xs[k]], [edges[k]])[0]
        dropped = ~mo.per_input_bins([xs[d]], [edges[d]])[0]
        assert (dropped & others).sum() >= 20 and np.isnan(xs[d]).sum() >= 8
