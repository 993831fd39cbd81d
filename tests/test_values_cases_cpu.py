"""What tests/test_gpu_values_properties.py relies on, checked where no GPU is needed: the conditions the random cases of
tests/values_cases.py must meet for that file's comparisons to bite.  Each statistic's examples are replayed here exactly as the
GPU test draws them (for_each_case: derandomised, no database) and held to this:
  - no case is left out: the statistic's oracle and core._compare_domain take every drawn case, and so does the GPU test's own
    comparison (run here on the oracle's results in the place of the library's);
  - at most one case in ten counts no sample, and at least half have a bin with two or more counted values;
  - every enumerated choice is drawn at least once per statistic (the tallies are printed: pytest -s);
  - every built array equals its contiguous copy by value;
  - the reference is plain: on the cases made all float64 without special values, the oracles agree with
    scipy.stats.binned_statistic_dd (count, min, max, mean), np.nanquantile per bin and fractions.Fraction arithmetic;
  - the edge-relative samples of tests/test_gpu_properties.py leave at most one case in ten empty (N(0, 2) samples left 31 %)."""
import collections
import functools
import warnings
from fractions import Fraction

import numpy as np
import pytest

import cov_oracle as co
import cov_weighted_oracle as cwo
import extrema_oracle as eo
import meanvar_oracle as mo
import meanvar_weighted_oracle as mwo
import skew_kurt_oracle as so
import values_cases as vc
from oracle import oracle_np as onp

hyp = pytest.importorskip("hypothesis")
torch = pytest.importorskip("torch")  # (the GPU files' helpers import it; none of this needs a GPU)
from hypothesis import HealthCheck, given, settings  # noqa: E402

import test_gpu_properties as tp  # noqa: E402
import test_gpu_values_properties as tgp  # noqa: E402


@functools.lru_cache(maxsize=None)
def drawn(stat, n=tgp.EXAMPLES):
    out = []
    tgp.for_each_case(stat, n, out.append)
    assert len(out) == n
    return out


@functools.lru_cache(maxsize=None)
def built(stat, i):
    return vc.build(drawn(stat)[i])


def counted(b):
    """(histogram's counts of the case, the counts of the samples whose values are not NaN)"""
    case = b.case
    samples = b.host[:b.d]
    kw = dict(bins=b.edges if b.d > 1 else b.edges[0], axis=case["axis"])
    if 0 in case["shape"]:  # (nothing to count; oracle_np.histogram raises ValueError for arrays without elements, as the reference does)
        return np.zeros(1, np.int64), np.zeros(1)
    hist, _ = onp.histogram(*samples, **kw)
    vals = b.host[b.d:b.d + (2 if case["stat"] in vc.PAIRS else 1)]
    has = np.ones(case["shape"], bool)
    for v in vals:
        if v.dtype.kind == "f":
            has &= ~np.isnan(v)
    with_value, _ = onp.histogram(*samples, weights=has.astype(np.float64), **kw)
    return hist, with_value


def oracle_got(b, params=None):
    """the oracle's results in the form tests/test_gpu_values_properties.compare takes the library's"""
    case = b.case
    stat, axis, edges = case["stat"], case["axis"], b.edges
    params = case["params"] if params is None else params
    got = {"outs": list(vc.oracle(stat, b.host, edges, axis, params))}
    samples = b.host[:b.d]
    if stat == "mean_var":
        got["ext"] = eo.histogram_extrema(*samples, values=b.host[b.d], bins=edges, axis=axis)
        got["hist"] = (np.zeros(got["outs"][0].shape, np.int64) if 0 in case["shape"] else
                       onp.histogram(*samples, bins=edges if b.d > 1 else edges[0], axis=axis)[0])
    if stat in vc.NARROW:
        rows = tgp._rows(b.host, case["shape"], axis)
        moms = list(so.moments_rows(rows[:b.d], edges, rows[b.d], rows[b.d + 1] if stat == "skew_kurt_w" else None))
        if stat == "skew_kurt":
            moms[0] = moms[0].astype(np.int64)
        got["moms"] = moms
    return got


@pytest.mark.parametrize("stat", vc.STATS)
def test_no_case_is_left_out(stat):
    """every drawn case goes through the oracle, core._compare_domain and the GPU test's comparison; the cases whose blocks (b)
    cuts (another number of examples draws other cases) go through the oracle and core._compare_domain"""
    from xhistogram_amd import core

    for i, case in enumerate(drawn(stat)):
        b = built(stat, i)
        core._compare_domain([np.dtype(t) for t in case["sample_dtypes"]], b.edges)
        tgp.compare(stat, b.host, b.edges, case["axis"], case["params"], oracle_got(b))
    for case in drawn(stat, tgp.BLOCK_EXAMPLES):
        b = vc.build(case)
        core._compare_domain([np.dtype(t) for t in case["sample_dtypes"]], b.edges)
        vc.oracle(stat, b.host, b.edges, case["axis"], case["params"])


@pytest.mark.parametrize("stat", vc.STATS)
def test_built_arrays_equal_their_contiguous_copies(stat):
    for i, case in enumerate(drawn(stat)):
        b = built(stat, i)
        assert len(b.views) == len(b.host) == len(case["layouts"])
        for a, h, lay, buf in zip(b.views, b.host, case["layouts"], b.bufs):
            assert h.flags.c_contiguous and h.shape == case["shape"]
            full = np.broadcast_to(a, case["shape"])
            assert full.dtype == h.dtype and np.array_equal(full, h, equal_nan=h.dtype.kind == "f"), (lay, case)
            if a.size:  # what the GPU backends are handed: offset and strides in elements, every element inside the allocation
                item = a.itemsize
                off = (a.__array_interface__["data"][0] - buf.__array_interface__["data"][0]) // item
                reach = [(n - 1) * (st // item) for n, st in zip(a.shape, a.strides)]
                assert 0 <= off + sum(r for r in reach if r < 0) and off + sum(r for r in reach if r > 0) < buf.size
            if lay["kind"] == "negative" and min(case["shape"]) > 1:
                assert min(a.strides) < 0
            if lay["kind"] == "broadcast" and a.shape == case["shape"]:
                assert all(a.strides[k] == 0 or a.shape[k] == 1 for k in lay["axes"])
            if lay["kind"] == "offset" and a.size:
                assert a.__array_interface__["data"][0] - buf.__array_interface__["data"][0] == a.itemsize


def tally(stat):
    t = collections.Counter()
    for i, case in enumerate(drawn(stat)):
        b = built(stat, i)
        ndim = len(case["shape"])
        hist, with_value = counted(b)
        t["empty"] += int(hist.sum() == 0)
        t["two or more"] += int(with_value.max(initial=0) >= 2)
        t["backend " + case["backend"]] += 1
        red = set(vc.reduced_axes(case))
        for lay in case["layouts"]:
            t["layout " + lay["kind"]] += 1
        t["stride-0 reduced axis"] += int(any(lay["kind"] == "broadcast" and any(k in red and case["shape"][k] > 1 for k in lay["axes"])
                                              for lay in case["layouts"]))
        for k in case["values"]:
            t["values " + k] += 1
        for k in case["sample_dtypes"]:
            t["samples " + k] += 1
        if case["weights"]:
            t["weights " + case["weights"]] += 1
        ax = case["axis"]
        t["axis None"] += int(ax is None)
        if ax is not None:
            norm = [a % ndim for a in ax]
            t["axis out of order"] += int(norm != sorted(norm))
            t["axis negative"] += int(any(a < 0 for a in ax))
        t["ndim %d" % ndim] += 1
        t["D %d" % b.d] += 1
        t["extent 0"] += int(0 in case["shape"])
        for name in ("ddof", "method", "bias", "fisher"):
            if name in case["params"]:
                t["%s %s" % (name, case["params"][name])] += 1
        if "q" in case["params"]:
            q = np.atleast_1d(case["params"]["q"])
            t["q scalar" if np.ndim(case["params"]["q"]) == 0 else "q list"] += 1
            t["q holds 0 or 1"] += int(((q == 0) | (q == 1)).any())
    return t


@pytest.mark.parametrize("stat", vc.STATS)
def test_every_choice_is_drawn_and_the_cases_count_something(stat):
    t = tally(stat)
    n = len(drawn(stat))
    print("\n%s: %s" % (stat, ", ".join("%s %d" % kv for kv in sorted(t.items()))))
    assert t["empty"] * 10 <= n, "%d of %d cases count no sample" % (t["empty"], n)
    assert t["two or more"] * 2 >= n, "only %d of %d cases have a bin with two counted values" % (t["two or more"], n)
    need = ["backend " + k for k in vc.BACKENDS] + ["layout " + k for k in vc.LAYOUTS] + ["values " + k for k in vc.VALUE_KINDS[stat]]
    need += ["samples " + k for k in vc.SAMPLE_DTYPES] + ["axis None", "axis out of order", "axis negative", "stride-0 reduced axis", "extent 0"]
    need += ["ndim %d" % k for k in (1, 2, 3, 4)] + ["D %d" % k for k in (1, 2, 3)]
    if stat in vc.WEIGHTED:
        need += ["weights " + k for k in vc.WEIGHT_DTYPES]
    if stat in vc.WITH_DDOF:
        need += ["ddof %d" % k for k in (0, 1, 2)]
    if stat in vc.NARROW:
        need += ["bias True", "bias False", "fisher True", "fisher False"]
    if stat == "quantile":
        need += ["method " + m for m in vc.METHODS]
    if stat in ("quantile", "quantile_w"):
        need += ["q scalar", "q list", "q holds 0 or 1"]
    missing = [k for k in need if not t[k]]
    assert not missing, "never drawn for %s: %s" % (stat, missing)


def test_the_examples_do_not_depend_on_who_draws_them():
    """for_each_case seeds from its own inner function: a second replay, from another caller, draws the same cases"""
    again = []
    tgp.for_each_case("cov_w", 12, lambda case: again.append(case))
    assert repr(again) == repr(drawn("cov_w")[:12])
    blocks = []
    tgp.for_each_case("cov_w", tgp.BLOCK_EXAMPLES, blocks.append)
    assert repr(blocks[:12]) == repr(again)


def test_partials_without_rows_merge_to_nothing():
    """a kept axis of extent 0 (a drawn block case of tests/test_gpu_values_properties.py): the dask steps give empty results"""
    from xhistogram_amd import core

    z = np.zeros((2, 3, 0, 5))
    for out in (core.combine_mean_var(z, z, z, axis=(0,)), core.combine_skew_kurt(z, z, z, z, z, axis=(0, 1)),
                core.combine_weighted_cov(z, z, z, z, z, z, axis=1)):
        assert all(o.shape[2] == 0 and o.size == 0 for o in out)
    assert core._skew_kurt_reduce(np.zeros((5, 2, 3, 0, 4)), axis=(1,), keepdims=True).shape == (5, 1, 3, 0, 4)
    assert core._extrema_pair_reduce(np.zeros((2, 2, 3, 0, 4)), axis=(1,), keepdims=True).shape == (2, 1, 3, 0, 4)


# ---------------------------------------------------------------------------------------------------------------------
# the reference is plain
# ---------------------------------------------------------------------------------------------------------------------
def plain_cases(stat, n=12):
    """the first n drawn cases with strictly increasing edges and some elements, made all float64 without special values"""
    out = []
    for case in drawn(stat):
        if 0 in case["shape"] or any(np.any(np.diff(e) <= 0) for e in case["edges"]):
            continue
        out.append(vc.build(vc.plain(case)))
        if len(out) == n:
            break
    assert len(out) == n
    return out


def scipy_rows(b, statistic, values=None):
    """scipy.stats.binned_statistic_dd row by row: [rows, bins...] of `statistic`, and the flat bin number of every sample
    inside the edges (-1: outside)"""
    from scipy import stats

    case = b.case
    rows = tgp._rows(b.host, case["shape"], case["axis"])
    xs = rows[:b.d]
    v = rows[b.d] if values is None else values
    nbs = [len(e) - 1 for e in b.edges]
    out = np.full((xs[0].shape[0],) + tuple(nbs), np.nan)
    for r in range(xs[0].shape[0]):
        res = stats.binned_statistic_dd(np.stack([x[r] for x in xs], axis=1), v[r], statistic=statistic, bins=b.edges)
        out[r] = res.statistic
    return out


@pytest.mark.parametrize("stat", ["extrema", "mean_var"])
def test_oracles_agree_with_scipy_binned_statistic(stat):
    for b in plain_cases(stat):
        case = b.case
        want = vc.oracle(stat, b.host, b.edges, case["axis"], dict(case["params"], ddof=0) if stat == "mean_var" else {})
        shape = want[0].shape
        count = scipy_rows(b, "count").reshape(shape)
        hist, _ = onp.histogram(*b.host[:b.d], bins=b.edges if b.d > 1 else b.edges[0], axis=case["axis"])
        np.testing.assert_array_equal(count, hist)
        if stat == "extrema":
            for name, w in zip(("min", "max"), want):
                got = scipy_rows(b, name).reshape(shape)
                got = np.where(count == 0, np.nan, got)  # (older scipy fills empty bins with 0 here)
                np.testing.assert_array_equal(got, w)
        else:
            np.testing.assert_array_equal(count, want[0])
            mean = scipy_rows(b, "mean").reshape(shape)
            ok = count > 0
            assert np.isnan(want[1][~ok]).all()
            # scipy's mean is a float64 bincount sum over the count; on the grid that sum is exact, so the bits agree
            np.testing.assert_array_equal(mean[ok], want[1][ok])


def bin_lists(b):
    """(row, flat bin) -> indices of the counted columns, from the oracle's own digitize on [rows, columns]"""
    case = b.case
    rows = tgp._rows(b.host, case["shape"], case["axis"])
    ok, flat, nbs = mo._flat_bins(rows[:b.d], b.edges)
    groups = collections.defaultdict(list)
    for r, c in zip(*np.nonzero(ok)):
        groups[(int(r), int(flat[r, c]))].append(int(c))
    return rows, groups, int(np.prod(nbs))


@pytest.mark.parametrize("method", vc.METHODS)
def test_quantile_oracle_is_nanquantile_per_bin(method):
    for b in plain_cases("quantile", 6):
        case = b.case
        q = np.atleast_1d(case["params"]["q"])
        want = vc.oracle("quantile", b.host, b.edges, case["axis"], dict(q=list(q), method=method))[0]
        rows, groups, n_bins = bin_lists(b)
        got = np.full((len(q), rows[0].shape[0], n_bins), np.nan)
        for (r, k), cols in groups.items():
            got[:, r, k] = np.nanquantile(rows[b.d][r, cols].astype(np.float64), q, method=method)
        np.testing.assert_array_equal(got.reshape(want.shape), want)


def _fraction_moments(vals, w=None):
    """(x, mean, M2, M3, M4) of one bin in rational arithmetic, each rounded once"""
    v = [Fraction(float(t)) for t in vals]
    u = [Fraction(1)] * len(v) if w is None else [Fraction(float(t)) for t in w]
    x = sum(u)
    mean = sum(a * t for a, t in zip(u, v)) / x
    return (float(x), float(mean)) + tuple(float(sum(a * (t - mean) ** j for a, t in zip(u, v))) for j in (2, 3, 4))


def _is_pow2(x, top):
    return x >= 2 and x <= top and float(x).is_integer() and (int(x) & (int(x) - 1)) == 0


@pytest.mark.parametrize("stat", ["mean_var", "mean_var_w", "cov", "cov_w", "skew_kurt", "skew_kurt_w"])
def test_exact_mode_is_fraction_arithmetic_on_power_of_two_counts(stat):
    """M2, C_ab, M3 and M4 of the oracles' exact mode (the sums a kernel forms, in float64) against fractions.Fraction on the
    grid values, bit for bit where the count (the sum of the integer weights) is a power of two: there every term is exact"""
    checked = 0
    for b in plain_cases(stat):
        rows, groups, n_bins = bin_lists(b)
        d = b.d
        xs, a = rows[:d], rows[d]
        w = rows[-1] if stat in vc.WEIGHTED else None
        if stat in ("mean_var", "mean_var_w"):
            res = mo.mean_var_rows(xs, b.edges, a, exact=True) if w is None else mwo.mean_var_w_rows(xs, b.edges, a, w, exact=True)
        elif stat in vc.PAIRS:
            res = co.cov_rows(xs, b.edges, a, rows[d + 1], exact=True) if w is None else cwo.cov_w_rows(xs, b.edges, a, rows[d + 1], w, exact=True)
        else:
            res = so.moments_rows(xs, b.edges, a, w)
        res = [np.asarray(r).reshape(xs[0].shape[0], n_bins) for r in res]
        top = 1 << 9 if w is None else 1 << 8
        if stat in vc.NARROW:
            top = 32
        for (r, k), cols in groups.items():
            wk = None if w is None else w[r, cols]
            x = len(cols) if w is None else float(wk.sum())
            if not _is_pow2(x, top):
                continue
            fa = _fraction_moments(a[r, cols], wk)
            assert res[0][r, k] == fa[0] and res[1][r, k] == fa[1]
            if stat in vc.PAIRS:  # (x, mean_a, mean_b, M2_a, M2_b, C_ab)
                bb = rows[d + 1][r, cols]
                fb = _fraction_moments(bb, wk)
                u = [Fraction(1)] * len(cols) if wk is None else [Fraction(float(t)) for t in wk]
                ma, mb = Fraction(fa[1]), Fraction(fb[1])
                cab = float(sum(t * (Fraction(float(p)) - ma) * (Fraction(float(q)) - mb) for t, p, q in zip(u, a[r, cols], bb)))
                assert (res[2][r, k], res[3][r, k], res[4][r, k], res[5][r, k]) == (fb[1], fa[2], fb[2], cab)
            elif stat in vc.NARROW:
                assert tuple(res[j][r, k] for j in (2, 3, 4)) == fa[2:]
            else:
                assert res[2][r, k] == fa[2]
            checked += 1
    assert checked >= 20, checked


# ---------------------------------------------------------------------------------------------------------------------
# the strategies of tests/test_gpu_properties.py
# ---------------------------------------------------------------------------------------------------------------------
def _replay(strategy, n):
    out = []

    @settings(max_examples=n, deadline=None, derandomize=True, database=None, suppress_health_check=list(HealthCheck))
    @given(strategy)
    def examples(case):
        out.append(case)

    examples()
    return out


@pytest.fixture
def no_local_constants(monkeypatch):
    """hypothesis hands out, now and then, the number constants it finds in whatever project modules are imported, so a replay
    of strategies that draw integers and floats depends on the tests that ran before it (18 to 28 empty cases of 300 here).  For
    a replay that is the same every time that pool is emptied, through the provider's own names where this hypothesis has them."""
    providers = pytest.importorskip("hypothesis.internal.conjecture.providers")
    if not all(hasattr(providers, name) for name in ("_get_local_constants", "Constants", "CONSTANTS_CACHE")):
        yield
        return
    empty = providers.Constants()
    monkeypatch.setattr(providers, "_get_local_constants", lambda: empty)
    providers.CONSTANTS_CACHE.cache.clear()
    yield
    providers.CONSTANTS_CACHE.cache.clear()  # (what was cached here knows no local constants: later tests look again)


def test_histogram_property_cases_count_something(no_local_constants):
    """test_random_cases_match_oracle and test_mixed_dtypes_and_big_histograms_match_oracle of tests/test_gpu_properties.py: with
    samples drawn about the edges at most one case in ten compares nothing but zeros (N(0, 2) samples: 92 of 300)"""
    empty = 0
    cases = _replay(tp.cases(), 300)
    for d, shape, axis, dtype, edges, wshape, density, seed, resident, override in cases:
        args = tp.random_samples(np.random.default_rng(seed), shape, dtype, edges)
        hist, _ = onp.histogram(*args, bins=edges if d > 1 else edges[0], axis=axis)
        empty += int(hist.sum() == 0)
    print("\ntest_random_cases_match_oracle: %d of %d cases count no sample" % (empty, len(cases)))
    assert empty * 10 <= len(cases)
    empty = 0
    cases = _replay(tp.mixed_cases(), 250)
    for case in cases:
        args, edges = tp.mixed_samples_and_edges(np.random.default_rng(case[8]), case)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            hist, _ = onp.histogram(*args, bins=edges if len(edges) > 1 else edges[0], axis=case[7])
        empty += int(hist.sum() == 0)
    print("test_mixed_dtypes_and_big_histograms_match_oracle: %d of %d cases count no sample" % (empty, len(cases)))
    assert empty * 10 <= len(cases)
