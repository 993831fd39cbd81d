"""The host merge of dask partials without a GPU: core.combine_mean_var, core.combine_weighted_mean_var and core.combine_cov
against Chan's pairwise merge restated as a plain loop over parts and bins with Python floats, bit for bit, in the documented
expression order

    tot = cx + xb,  mean = cm + d * xb / tot,  moment = cq + qb + d_i * d_j * cx * xb / tot   (left to right)

and the dask steps built on it: every reduce and aggregate object pickles, which dask's distributed schedulers need."""
import pickle

import numpy as np
import pytest

from xhistogram_amd import core

NAN = float("nan")
N_BINS = 6  # bin 5 is empty in every part


def _counted(x):
    return x > 0


def _weighed(x):
    return x != 0  # (NaN != 0: a NaN part is taken)


def _merge_bin(parts, pairs, present):
    """one bin's parts [(x, [means], [moments])] merged one after another: (x, [means], [moments]) as Python floats"""
    n_means = 1 + max(max(p) for p in pairs)
    cx, cm, cq = 0.0, [NAN] * n_means, [NAN] * len(pairs)
    for xb, mb, qb in parts:
        if not present(xb):
            continue
        tot = cx + xb
        if present(cx):
            d = [b - c for b, c in zip(mb, cm)]
            cq = [c + q + d[i] * d[j] * cx * xb / tot for c, q, (i, j) in zip(cq, qb, pairs)]
            cm = [c + di * xb / tot for c, di in zip(cm, d)]
        else:
            cm, cq = list(mb), list(qb)
        cx = tot
    return cx, cm, cq


def _merge(x, means, moments, pairs, present):
    """[parts, bins] arrays merged over the parts by _merge_bin: (x, means..., moments...) as [bins] float64 arrays"""
    cols = []
    for b in range(x.shape[1]):
        parts = [(float(x[k, b]), [float(m[k, b]) for m in means], [float(q[k, b]) for q in moments]) for k in range(x.shape[0])]
        cx, cm, cq = _merge_bin(parts, pairs, present)
        cols.append([cx] + cm + cq)
    return [np.array(c, np.float64) for c in zip(*cols)]


def _same_bits(got, want):
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    assert got.shape == want.shape
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64))


def _partials(rng, n_parts, empty, n_means, n_moments, weighted=False):
    """[parts, bins] partials as the library emits them: x, then means around 50 (|mean| >> std, so the last bits matter), then
    moments; a part in `empty`, and bin 5 of every part, holds nothing (x 0, the rest NaN).  The last moment of three is a
    co-moment, negative in about half of the bins."""
    x = rng.uniform(0.25, 40.0, (n_parts, N_BINS)) if weighted else rng.integers(1, 300, (n_parts, N_BINS)).astype(np.float64)
    means = [50 + 3 * rng.standard_normal((n_parts, N_BINS)) for _ in range(n_means)]
    moments = [x * rng.uniform(0.5, 9.0, (n_parts, N_BINS)) for _ in range(n_moments)]
    if n_moments == 3:
        moments[2] = moments[2] * rng.choice([-1.0, 1.0], (n_parts, N_BINS))
    for a in [x] + means + moments:
        a[sorted(empty)] = NAN
        a[:, 5] = NAN
    x[np.isnan(x)] = 0.0
    return x, means, moments


# parts, and which of them are empty: none, at the start, in the middle, at the end, and several at once
CASES = [(1, ()), (1, (0,)), (2, (0,)), (2, (1,)), (3, (1,)), (4, (0, 3)), (5, (2, 3)), (6, (0, 2, 5)), (7, ()), (7, (0, 1, 3, 6))]


@pytest.mark.parametrize("n_parts,empty", CASES)
def test_combine_mean_var_bit_for_bit(n_parts, empty):
    rng = np.random.default_rng(100 + 10 * n_parts + len(empty))
    x, (mean,), (m2,) = _partials(rng, n_parts, empty, 1, 1)
    got = core.combine_mean_var(x, mean, m2, axis=0)
    assert all(g.shape == (1, N_BINS) and g.dtype == np.float64 for g in got)
    for g, w in zip(got, _merge(x, [mean], [m2], [(0, 0)], _counted)):
        _same_bits(g, w)
    assert got[0][0, 5] == 0 and np.isnan(got[1][0, 5]) and np.isnan(got[2][0, 5])


@pytest.mark.parametrize("n_parts,empty", CASES)
def test_combine_weighted_mean_var_bit_for_bit(n_parts, empty):
    rng = np.random.default_rng(200 + 10 * n_parts + len(empty))
    x, (mean,), (m2,) = _partials(rng, n_parts, empty, 1, 1, weighted=True)
    got = core.combine_weighted_mean_var(x, mean, m2, axis=0)
    for g, w in zip(got, _merge(x, [mean], [m2], [(0, 0)], _weighed)):
        _same_bits(g, w)
    assert got[0][0, 5] == 0 and np.isnan(got[1][0, 5]) and np.isnan(got[2][0, 5])


def test_combine_weighted_nan_spreads_and_zero_sums_are_skipped():
    """bin 0: part 1 has a NaN W, which makes the bin NaN from there on; bin 1: parts 0 and 2 have weights that sum to 0 (the
    library gives W 0, mean and M2 NaN) and are skipped, so the bin is parts 1 and 3 merged; bin 2: every W is 0"""
    rng = np.random.default_rng(7)
    x, (mean,), (m2,) = _partials(rng, 4, (), 1, 1, weighted=True)
    x[1, 0] = mean[1, 0] = m2[1, 0] = NAN
    for k in (0, 2):
        x[k, 1], mean[k, 1], m2[k, 1] = 0.0, NAN, NAN
    x[:, 2], mean[:, 2], m2[:, 2] = 0.0, NAN, NAN
    got = core.combine_weighted_mean_var(x, mean, m2, axis=0)
    want = _merge(x, [mean], [m2], [(0, 0)], _weighed)
    for g, w in zip(got, want):
        _same_bits(g, w)
    assert all(np.isnan(g[0, 0]) for g in got)
    two = _merge(x[[1, 3]], [mean[[1, 3]]], [m2[[1, 3]]], [(0, 0)], _weighed)
    assert all(g[0, 1] == t[1] for g, t in zip(got, two)) and not np.isnan(got[1][0, 1])
    assert got[0][0, 2] == 0 and np.isnan(got[1][0, 2]) and np.isnan(got[2][0, 2])


COV_PAIRS = [(0, 0), (1, 1), (0, 1)]  # M2_a, M2_b, C_ab: combine_cov's argument and return order


def _cov_case(n_parts, empty):
    rng = np.random.default_rng(300 + 10 * n_parts + len(empty))
    x, means, moments = _partials(rng, n_parts, empty, 2, 3)
    got = core.combine_cov(x, *means, *moments, axis=0)
    assert len(got) == 6 and all(g.shape == (1, N_BINS) and g.dtype == np.float64 for g in got)
    return got, _merge(x, means, moments, COV_PAIRS, _counted)


@pytest.mark.parametrize("n_parts,empty", CASES)
def test_combine_cov_count_and_means_bit_for_bit(n_parts, empty):
    got, want = _cov_case(n_parts, empty)
    for g, w in zip(got[:3], want[:3]):
        _same_bits(g, w)
    assert got[0][0, 5] == 0 and np.isnan(got[1][0, 5]) and np.isnan(got[2][0, 5])


@pytest.mark.parametrize("n_parts,empty", CASES)
def test_combine_cov_moments_bit_for_bit(n_parts, empty):
    got, want = _cov_case(n_parts, empty)
    for g, w in zip(got[3:], want[3:]):  # M2_a, M2_b, C_ab
        _same_bits(g, w)
    assert all(np.isnan(g[0, 5]) for g in got[3:])


def test_combine_cov_negative_co_moment():
    """the co-moments of the parts and the cross term are all negative: b falls where a rises, within the parts and between"""
    x = np.array([[3.0], [5.0], [2.0]])
    ma, mb = np.array([[1.0], [4.0], [9.5]]), np.array([[8.0], [2.5], [-1.0]])
    qa, qb, cc = np.array([[2.0], [1.5], [0.7]]), np.array([[1.0], [2.5], [0.3]]), np.array([[-1.1], [-1.9], [-0.4]])
    got = core.combine_cov(x, ma, mb, qa, qb, cc, axis=0)
    for g, w in zip(got, _merge(x, [ma, mb], [qa, qb, cc], COV_PAIRS, _counted)):
        _same_bits(g, w)
    assert got[5][0, 0] < cc.sum() < 0 and got[3][0, 0] > qa.sum() and got[4][0, 0] > qb.sum()


@pytest.mark.parametrize("which", ["mean_var", "mean_var_w", "cov"])
def test_two_axes_merge_in_c_order(which):
    """[2, rows, 3, bins] partials over axes (0, 2): the six parts of a row in C order, the kept row axis between them"""
    rng = np.random.default_rng({"mean_var": 41, "mean_var_w": 42, "cov": 43}[which])
    n_means, n_moments = (2, 3) if which == "cov" else (1, 1)
    rows = [_partials(rng, 6, (1, 4), n_means, n_moments, weighted=which == "mean_var_w") for _ in range(2)]

    def shaped(i):  # array i of (x, means..., moments...) as [2, rows, 3, bins]
        flat = [[r[0]] + r[1] + r[2] for r in rows]
        return np.stack([f[i].reshape(2, 3, N_BINS) for f in flat], axis=1)

    arrays = [shaped(i) for i in range(1 + n_means + n_moments)]
    fn, pairs, present = {"mean_var": (core.combine_mean_var, [(0, 0)], _counted),
                          "mean_var_w": (core.combine_weighted_mean_var, [(0, 0)], _weighed),
                          "cov": (core.combine_cov, COV_PAIRS, _counted)}[which]
    got = fn(*arrays, axis=(0, 2))
    assert all(g.shape == (1, 2, 1, N_BINS) for g in got)
    for r, (x, means, moments) in enumerate(rows):
        for g, w in zip(got, _merge(x, means, moments, pairs, present)):
            _same_bits(g[0, r, 0], w)


# ---------------------------------------------------------------------------------------------------------------------
# the dask steps
# ---------------------------------------------------------------------------------------------------------------------
def _aggregates(monkeypatch):
    """the `aggregate` objects that histogram_mean_var, histogram_cov and histogram_skew_kurt (unweighted, weighted) hand to
    dask, caught at _value_stat"""
    caught = {}

    def fake(stat, args, values, bins, range, axis, name, aggregate=None, *extras, weights=None, **params):
        assert len(extras) + (weights is not None) == core._VALUE_STATS[stat].extras and not params
        caught[stat] = aggregate
        return "dask", [np.zeros(1)] * core._VALUE_STATS[stat].k, bins, ()

    monkeypatch.setattr(core, "_value_stat", fake)
    x, e = np.zeros(4), np.linspace(0, 1, 3)
    for w in (None, x):
        core.histogram_mean_var(x, values=x, bins=e, ddof=1, weights=w)
        core.histogram_skew_kurt(x, values=x, bins=e, ddof=1, bias=False, weights=w)
    core.histogram_cov(x, values=(x, x), bins=e, ddof=1)
    core.histogram_weighted_cov(x, values=(x, x), weights=x, bins=e, ddof=1)
    assert sorted(caught) == ["cov", "cov_w", "mean_var", "mean_var_w", "skew_kurt", "skew_kurt_w"]
    return caught


def _entry_partials(rng, stat, n_parts, empty):
    """[k, parts, bins] partials shaped as the table entry's dask step takes them: (min, max) pairs for the one step that is no
    moment merge, else Chan's (x, means..., one moment per pair) or, where the step has pairs=None, Pébay's (x, mean, M2, M3,
    M4); x is a sum of weights where the step says a partial is present when x != 0"""
    st = core._VALUE_STATS[stat]
    if st.reduce is core._extrema_pair_reduce:
        _, (lo,), (span,) = _partials(rng, n_parts, empty, 1, 1)
        return np.stack([lo, lo + span])
    assert st.reduce.func is core._moment_reduce
    pairs = st.reduce.keywords.get("pairs", ((0, 0),))
    n_means, n_moments = (1, 3) if pairs is None else (st.k - 1 - len(pairs), len(pairs))
    x, means, moments = _partials(rng, n_parts, empty, n_means, n_moments, weighted=st.reduce.keywords["present"] is core._weighed)
    return np.stack([x] + means + moments)


def test_reduce_and_aggregate_objects_pickle(monkeypatch):
    rng = np.random.default_rng(5)
    steps = {"reduce " + name: st.reduce for name, st in core._VALUE_STATS.items() if st.reduce is not None}
    assert sorted(steps) == ["reduce " + n for n in ("cov", "cov_w", "extrema", "mean_var", "mean_var_w", "skew_kurt", "skew_kurt_w")]
    steps.update(("aggregate " + name, f) for name, f in _aggregates(monkeypatch).items())
    assert len(steps) == 7 + 6
    for name, f in steps.items():
        g = pickle.loads(pickle.dumps(f))
        stat = name.split()[1]
        block = _entry_partials(rng, stat, 4, (2,))[:, :, None, :]  # [k, parts, a kept axis, bins]
        a, b = f(block, axis=(1,), keepdims=False), g(block, axis=(1,), keepdims=False)
        assert a.shape == (core._VALUE_STATS[stat].k, 1, N_BINS), name
        _same_bits(a, b)


# the public merge of each entry that has a dask step, and where each of its results lies in the library's order of outputs
COMBINE = {
    "extrema": (core.combine_extrema, (0, 1)),
    "mean_var": (core.combine_mean_var, (0, 1, 2)),
    "mean_var_w": (core.combine_weighted_mean_var, (0, 1, 2)),
    "cov": (core.combine_cov, (0, 1, 2, 3, 5, 4)),
    "cov_w": (core.combine_weighted_cov, (0, 1, 2, 3, 5, 4)),
    "skew_kurt": (core.combine_skew_kurt, (0, 1, 2, 3, 4)),
    "skew_kurt_w": (core.combine_weighted_skew_kurt, (0, 1, 2, 3, 4)),
}


@pytest.mark.parametrize("stat", sorted(core._VALUE_STATS))
def test_every_table_entry_is_wired_and_its_step_is_the_public_merge(stat):
    from xhistogram_amd import _native

    st = core._VALUE_STATS[stat]
    assert callable(getattr(_native.Plan, st.method))
    k = st.k if st.k is not None else 3  # (one output per element of q: any number of them)
    assert (st.k is None) == ("q" in st.tail) and set(st.tail) <= {"q", "code"}
    assert st.ptrs and st.ptrs[0] == 0 and list(st.ptrs) == sorted(set(st.ptrs)) and st.ptrs[-1] < k
    assert all(0 <= i < k for i in st.ints) and st.extras in (0, 1, 2)
    back = pickle.loads(pickle.dumps(st))
    assert back[:5] == st[:5] and back[6:] == st[6:] and (back.reduce is None) == (st.reduce is None)
    if st.reduce is None:
        assert stat not in COMBINE and st.noun
        return
    combine, order = COMBINE[stat]
    block = _entry_partials(np.random.default_rng(sorted(core._VALUE_STATS).index(stat)), stat, 2, ())
    for step in (st.reduce, back.reduce):
        out = step(block, axis=(1,), keepdims=True)
        assert out.shape == (k, 1, N_BINS) and out.dtype == np.float64
        want = combine(*[block[i] for i in order], axis=0)
        assert len(want) == k
        for i, w in zip(order, want):
            _same_bits(out[i], w)


def test_cov_step_keeps_the_library_order(monkeypatch):
    """blocks are (n, mean_a, mean_b, M2_a, C_ab, M2_b); the last step divides the three moments by n - ddof"""
    rng = np.random.default_rng(6)
    x, (ma, mb), (qa, qb, cc) = _partials(rng, 5, (0,), 2, 3)
    block = np.stack([x, ma, mb, qa, cc, qb])
    n, wa, wb, wqa, wqb, wcc = core.combine_cov(x, ma, mb, qa, qb, cc, axis=0)
    out = core._VALUE_STATS["cov"].reduce(block, axis=(1,), keepdims=True)
    for o, w in zip(out, (n, wa, wb, wqa, wcc, wqb)):
        _same_bits(o, w)
    last = _aggregates(monkeypatch)["cov"](block, axis=(1,), keepdims=True)
    for o, w in zip(last[:3], (n, wa, wb)):
        _same_bits(o, w)
    for o, w in zip(last[3:], (wqa, wcc, wqb)):
        _same_bits(o, core._var_of(n, w, 1))
