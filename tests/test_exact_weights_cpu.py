"""The claims tests/exact_weights.py rests on, checked on the CPU: the generators' sums do not depend on the order of the
float64 additions (nor on 36-bit packed records), and the comparisons reject what a subtly wrong kernel would produce — weights
rounded to float32, float32 accumulation, packed records of float32's precision, one lost weight in a bin of 10^7 — while the float64 bound
accepts float64 sums taken in another order."""
import numpy as np
import pytest

import exact_weights as ew


def _pack(w, keep):
    """round float64 weights to `keep` stored mantissa bits (nearest, ties to even) on their bit patterns — the packed records'
    rounding (36 bits: 16 low bits cleared) and coarser ones.  The exact float64 weights have 24 stored bits (25 significant):
    a record that kept 24 would still carry them exactly, one of float32's precision (23 stored) does not."""
    drop = 52 - keep
    b = w.view(np.uint64)
    half = np.uint64((1 << (drop - 1)) - 1)
    r = b + half + ((b >> np.uint64(drop)) & np.uint64(1))
    return (r & ~np.uint64((1 << drop) - 1)).view(np.float64)


def _case(rng, n, nb, w):
    idx = rng.integers(0, nb, n)
    return idx, np.bincount(idx, weights=w.astype(np.float64), minlength=nb)


def _f32_accumulate(idx, w, nb):
    acc = np.zeros(nb, np.float32)
    np.add.at(acc, idx, w.astype(np.float32))
    return acc.astype(np.float64)


GENS = {
    "f64_one": lambda rng, n: ew.f64(rng, n),
    "f64_both": lambda rng, n: ew.f64(rng, n, signs="both"),
    "f64_subnormal": lambda rng, n: ew.f64(rng, n, scale_log2=-1040),
    "f64_subnormal_both": lambda rng, n: ew.f64(rng, n, signs="both", scale_log2=-1040),
    "f32_one": lambda rng, n: ew.f32(rng, n).astype(np.float64),
}


def test_generators_have_the_stated_bits():
    rng = np.random.default_rng(0)
    w = ew.f64(rng, 100_000)
    assert w.min() >= 0.5 and w.max() < 1.0
    assert np.all(np.ldexp(w, 25) == np.rint(np.ldexp(w, 25)))
    assert np.mean(w.astype(np.float32).astype(np.float64) != w) > 0.4  # 25 bits: float32 rounds about half of them
    s = ew.f64(rng, 100_000, scale_log2=-1040)
    assert np.all((s > 0) & (s < np.finfo(np.float64).tiny))  # subnormal, every one
    assert np.array_equal(np.ldexp(ew.f64(np.random.default_rng(5), 1000, scale_log2=-1040), 1040), ew.f64(np.random.default_rng(5), 1000))
    b = ew.f64(rng, 100_000, signs="both")
    assert 0.45 < np.mean(b < 0) < 0.55 and np.all(np.abs(b) >= 0.5)
    f = ew.f32(rng, 100_000)
    assert f.dtype == np.float32 and f.min() >= 0.5 and f.max() < 1.0
    fb = ew.f32(rng, 100_000, signs="both")
    assert fb.dtype == np.float32 and 0.45 < np.mean(fb < 0) < 0.55 and np.all(np.abs(fb) >= 0.5)


@pytest.mark.parametrize("gen", sorted(GENS))
def test_sums_do_not_depend_on_the_order_of_additions(gen):
    """np.bincount == shuffled np.add.at == chunked partial sums added up in shuffled order == bincount of the 36-bit packed
    records: the same bits, whatever the order"""
    rng = np.random.default_rng(1)
    n, nb = 400_000, 97
    w = GENS[gen](rng, n)
    idx, want = _case(rng, n, nb, w)
    ew.assert_summable(np.bincount(idx, minlength=nb))
    perm = rng.permutation(n)
    got = np.zeros(nb)
    np.add.at(got, idx[perm], w[perm])
    ew.assert_bits_equal(got, want, "shuffled add.at")
    cuts = np.sort(rng.choice(n, 31, replace=False))
    parts = [np.bincount(i, weights=v, minlength=nb) for i, v in zip(np.split(idx, cuts), np.split(w, cuts))]
    acc = np.zeros(nb)
    for p in rng.permutation(len(parts)):
        acc = acc + parts[p]
    ew.assert_bits_equal(acc, want, "chunked partial sums")
    packed = np.bincount(idx, weights=_pack(w, 36), minlength=nb)
    if "subnormal" in gen:
        # a subnormal weight has fewer significant bits than stored ones: rounding its bit pattern to 36 stored bits keeps 18 of
        # the 25 (the packed records' limit on subnormal weights)
        assert np.count_nonzero(packed != want) > nb // 2
    else:
        ew.assert_bits_equal(packed, want, "36-bit packed records")
    ew.assert_bits_equal(-np.bincount(idx, weights=-w, minlength=nb), want, "negated")


@pytest.mark.parametrize("gen", ["f64_one", "f64_both"])
def test_bits_equal_rejects_what_a_subtly_wrong_kernel_computes(gen):
    """weights rounded to float32, float32 accumulation and packed records of float32's precision each change most bins (and
    records of 24 stored bits would carry these weights exactly)"""
    rng = np.random.default_rng(2)
    n, nb = 400_000, 97
    w = GENS[gen](rng, n)
    idx, want = _case(rng, n, nb, w)
    wrong = {
        "weights rounded to float32": np.bincount(idx, weights=w.astype(np.float32).astype(np.float64), minlength=nb),
        "float32 accumulation": _f32_accumulate(idx, w, nb),
        "23-bit packed records": np.bincount(idx, weights=_pack(w, 23), minlength=nb),
    }
    ew.assert_bits_equal(np.bincount(idx, weights=_pack(w, 24), minlength=nb), want, "24 stored bits")
    for what, got in wrong.items():
        with pytest.raises(AssertionError):
            ew.assert_bits_equal(got, want, what)
        assert np.count_nonzero(got != want) > nb // 2, what


def test_bits_equal_rejects_one_weight_lost_in_a_bin_of_ten_million():
    rng = np.random.default_rng(3)
    n = 10_000_000
    w = ew.f64(rng, n)
    want = np.array([w.sum(), 0.0])  # (pairwise summation: exact all the same)
    assert want[0] == np.bincount(np.zeros(n, np.int64), weights=w)[0]
    lost = np.array([np.bincount(np.zeros(n - 1, np.int64), weights=np.delete(w, 4_321_987))[0], 0.0])
    np.testing.assert_allclose(lost, want, rtol=1e-6)  # (invisible to the old tolerance)
    with pytest.raises(AssertionError):
        ew.assert_bits_equal(lost, want, "one lost weight")
    twice = want + np.array([w[17], 0.0])
    with pytest.raises(AssertionError):
        ew.assert_bits_equal(twice, want, "one weight counted twice")


def test_bits_equal_checks_nan_positions_and_the_sign_of_zero():
    a = np.array([1.0, np.nan, 0.0])
    ew.assert_bits_equal(a.copy(), a)
    with pytest.raises(AssertionError):
        ew.assert_bits_equal(np.array([1.0, np.nan, -0.0]), a)
    with pytest.raises(AssertionError):
        ew.assert_bits_equal(np.array([1.0, 2.0, 0.0]), a)
    with pytest.raises(AssertionError):
        ew.assert_bits_equal(np.array([np.nan, np.nan, 0.0]), a)


def test_summable_guard():
    ew.assert_summable(np.array([5, (1 << 28) - 1]))
    with pytest.raises(AssertionError):
        ew.assert_summable(np.array([1 << 28]))
    ew.assert_summable(np.array([1 << 28]), np.float32)
    with pytest.raises(AssertionError):
        ew.assert_summable(np.array([1 << 29]), np.float32)


def _full_mantissa_case(rng, n, nb, signs):
    w = rng.uniform(0.25, 2.0, n)
    if signs == "both":
        w = np.where(rng.integers(0, 2, n).astype(bool), -w, w)
    idx = rng.integers(0, nb, n)
    want = np.bincount(idx, weights=w, minlength=nb)
    return idx, w, want, np.bincount(idx, weights=np.abs(w), minlength=nb), np.bincount(idx, minlength=nb)


@pytest.mark.parametrize("signs", ["one", "both"])
def test_f64_bound_accepts_other_orders_and_rejects_rounded_weights(signs):
    rng = np.random.default_rng(4)
    n, nb = 300_000, 30_011  # (about 10 samples per bin: a tight bound, so rounding of the weights shows)
    idx, w, want, a, cnt = _full_mantissa_case(rng, n, nb, signs)
    perm = rng.permutation(n)
    got = np.zeros(nb)
    np.add.at(got, idx[perm], w[perm])
    assert np.count_nonzero(got != want) > 0  # (full mantissas: the order does show in the bits)
    ew.assert_within_f64_bound(got, want, a, cnt)
    half = n // 2
    ew.assert_within_f64_bound(np.bincount(idx[half:], weights=w[half:], minlength=nb) + np.bincount(idx[:half], weights=w[:half], minlength=nb),
                               want, a, cnt)
    with pytest.raises(AssertionError):
        ew.assert_within_f64_bound(np.bincount(idx, weights=w.astype(np.float32).astype(np.float64), minlength=nb), want, a, cnt)
    with pytest.raises(AssertionError):
        ew.assert_within_f64_bound(_f32_accumulate(idx, w, nb), want, a, cnt, rounding=2.0 ** -37)
    p36 = np.bincount(idx, weights=_pack(w, 36), minlength=nb)
    with pytest.raises(AssertionError):
        ew.assert_within_f64_bound(p36, want, a, cnt)
    ew.assert_within_f64_bound(p36, want, a, cnt, rounding=2.0 ** -37)
    with pytest.raises(AssertionError):
        ew.assert_within_f64_bound(np.bincount(idx, weights=_pack(w, 24), minlength=nb), want, a, cnt, rounding=2.0 ** -37)


def test_f64_bound_wants_non_finite_bins_exactly():
    want = np.array([np.nan, np.inf, 1.0])
    a = np.array([np.nan, np.inf, 1.0])
    cnt = np.array([2, 1, 1])
    ew.assert_within_f64_bound(want.copy(), want, a, cnt)
    with pytest.raises(AssertionError):
        ew.assert_within_f64_bound(np.array([np.nan, -np.inf, 1.0]), want, a, cnt)
    with pytest.raises(AssertionError):
        ew.assert_within_f64_bound(np.array([1.0, np.inf, 1.0]), want, a, cnt)
    with pytest.raises(AssertionError):
        ew.assert_within_f64_bound(np.array([np.nan, np.inf, np.nan]), want, a, cnt)


def test_records_rounding_reads_the_description():
    assert ew.records_rounding("hist=partitioned records=packed48(+exact if both signs) exchange=no exchange_records=-") == 2.0 ** -37
    assert ew.records_rounding("records=u16+f64 exchange=forced exchange_records=packed8") == 2.0 ** -37
    assert ew.records_rounding("records=u16+f64 exchange=no exchange_records=-") == 0.0
    assert ew.records_rounding("family=fast hist=lds") == 0.0
