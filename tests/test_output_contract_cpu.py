"""tests/output_contract_cases.py held to its conditions, without a GPU: every histogram home of the census has its case for every
(sample dtype, weight dtype, inputs) the census has it for; the count prefill carries out of the low 32 bits in every row; the
weights, the prefill and every P + H are exact (integer arithmetic on units of 2^-25 against the oracle's float64, bit for bit);
the sentinel is no expected element; the cases without an empty bin are the listed ones."""
import numpy as np
import pytest

import exact_weights as ew
import output_contract_cases as occ
from census_inputs import HOMES, _ST, _WT, _cases

I64 = np.int64


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(I64)


def to_units(a, what):
    """float64 multiples of 2^-25 as int64 numbers of them"""
    u = np.ldexp(np.asarray(a, np.float64), -occ.UNIT_LOG2)
    assert np.isfinite(u).all() and (u == np.rint(u)).all() and np.abs(u).max(initial=0) < 2.0 ** 53, "%s: not multiples of 2^-25" % what
    return u.astype(I64)


def sums_per_bin(case, values):
    """int64 sums of `values` [n_rows, n_cols] per (row, bin) over the samples the oracle counts"""
    idx = case.flat_index()
    keep = idx >= 0
    at = (idx + np.arange(case.n_rows, dtype=I64)[:, None] * case.n_bins)[keep]
    acc = np.zeros(case.n_rows * case.n_bins, I64)
    np.add.at(acc, at, values[keep])
    return acc.reshape(case.n_rows, case.n_bins)


def check_case(case):
    """-> whether every bin of the case receives a sample"""
    sentinel = I64(occ.SENTINEL)
    counts = sums_per_bin(case, np.ones((case.n_rows, case.n_cols), I64))
    assert case.n_rows > 0 and case.n_cols > 0 and case.n_bins > 0, case
    if not case.weighted:
        want, P = case.want(), case.prefill()
        assert want.dtype == I64 and P.dtype == I64 and want.shape == P.shape == (case.n_rows, case.n_bins), case
        np.testing.assert_array_equal(want, counts, err_msg=case.name)
        low = P & 0xFFFFFFFF
        np.testing.assert_array_equal(low, np.broadcast_to(0xFFFFFFFF - np.arange(case.n_bins) % 3, low.shape))
        assert len(set((P >> 36).max(axis=1).tolist())) == case.n_rows and ((P >> 36).max(axis=1) == (P >> 36).min(axis=1)).all(), case
        carries = (low + want) >> 32
        assert (carries.max(axis=1) >= 1).all(), "%s: a row without a carry out of the low word" % case.name
        for block in (want, P, P + want):
            assert not (block == sentinel).any(), case
        return bool((counts > 0).all())
    for k, w in enumerate(case.weights()):
        w = np.asarray(w)
        ew.assert_summable(counts, np.float32 if w.dtype == np.float32 else np.float64)
        assert counts.max() < (1 << 27), case
        wu = to_units(w.astype(np.float64), case.name + " weights")
        assert (wu != 0).all(), case
        pu = case.prefill_units(k)
        assert ((np.abs(pu) >= 1) & (np.abs(pu) < (1 << 50))).all(), case
        P, want = case.prefill(k), case.want(k)
        assert P.dtype == want.dtype == np.float64 and P.shape == want.shape == (case.n_rows, case.n_bins), case
        np.testing.assert_array_equal(to_units(P, case.name + " prefill"), pu)
        assert not (P == 0).any() and not np.signbit(P[P == 0]).any(), case
        hu = sums_per_bin(case, wu)
        # whatever the order of the additions, a partial sum stays below |P| + sum |w| < 2^53 units: exact
        assert (np.abs(pu) + sums_per_bin(case, np.abs(wu))).max() < (1 << 53), case
        np.testing.assert_array_equal(bits(want), bits(occ.from_units(hu)), err_msg=case.name + ": H")
        np.testing.assert_array_equal(bits(P + want), bits(occ.from_units(pu + hu)), err_msg=case.name + ": P + H")
        assert (bits(want)[counts == 0] == 0).all(), "%s: an empty bin is +0.0" % case.name
        for block in (want, P, P + want):
            assert not (bits(block) == sentinel).any(), case
    signs = {bool(s) for w in case.weights() for s in np.unique(np.signbit(np.asarray(w, np.float64)))}
    assert signs == {False, True} or case.name in ONE_SIGN or case.family == "mixed", "%s: weights of one sign" % case.name
    return bool((counts > 0).all())


# the cases drawn with weights of one sign on purpose: packed records that are added up as they are
ONE_SIGN = {"%s|f64|2|%s" % (st, home) for st in occ.STS for home in occ.PACKED_HOMES} | {
    "exchange|%d|%s" % (n, tag) for n in occ.EXCHANGE_N for tag in ("packed8_one_sign", "no_budget")}


def check_all(cases):
    n, full = 0, set()
    for case in cases:
        if check_case(case):
            full.add(case.name)
        n += 1
    assert n > 0
    return full


def listed(prefix):
    return {name for name in occ.NO_EMPTY_BIN if name.startswith(prefix)}


@pytest.mark.parametrize("D", occ.DS)
@pytest.mark.parametrize("wt", occ.WTS)
@pytest.mark.parametrize("st", occ.STS)
def test_float_families(st, wt, D):
    """every HOMES key the census has for (st, wt, D), "k1" edges unless ruled out, no digitize-form override"""
    census = {}
    for c in _cases(_ST[st], _WT[wt], D):
        census.setdefault(c["home"], set()).add(c["kind"])
    specs = occ.float_case_specs(st, wt, D)
    assert [c["home"] for _, c in specs] == [h for h in HOMES if h in census]
    for _, c in specs:
        assert c["kind"] == ("k1" if "k1" in census[c["home"]] else "lin") and c["params"] == HOMES[c["home"]]["params"], c
    twins = occ.float_lin_twins(st, wt, D)  # (one input, 12 000 bins or more: "k1" edges do not reach the home, "lin" edges do)
    assert [c["home"] for _, c in twins] == [c["home"] for _, c in specs if D == 1 and c["kind"] == "k1" and c["nbs"][0] >= occ.LIN_TWIN_BINS]
    assert all(c["kind"] == "lin" and c["params"] == HOMES[c["home"]]["params"] for _, c in twins)
    if D == 1:
        assert sum(c["home"].startswith("d1_") for _, c in specs) == 32 == sum(c["home"].startswith("d1_") for _, c in twins)
    assert check_all(occ.float_cases(st, wt, D)) == listed("%s|%s|%d|" % (st, wt, D))


def test_every_home_appears():
    seen = {c["home"] for st in occ.STS for wt in occ.WTS for D in occ.DS for _, c in occ.float_case_specs(st, wt, D)}
    assert seen == set(HOMES)


@pytest.mark.parametrize("dtype", occ.SMALL_DTYPES)
def test_small_samples(dtype):
    cases = list(occ.small_sample_cases(dtype))
    assert {(c.home, c.weighted) for c in cases} == occ._SMALL_PICK
    assert check_all(cases) == listed("small|%s|" % dtype)


def test_integer_domains():
    cases = list(occ.int64_domain_cases())
    assert {(c.home, c.weighted) for c in cases} == {(h, w) for h in ("lds", "global") for w in (False, True)}
    assert check_all(cases) == listed("int64|")
    cases = list(occ.generic_integer_cases())
    assert len(cases) == len(occ._GENERIC_PICK) and {len(c.samples) for c in cases} == {1, 2}
    assert check_all(cases) == listed("generic|")


@pytest.mark.parametrize("D", occ.DS)
def test_mixed_dtypes(D):
    cases = list(occ.mixed_dtype_cases(D))
    assert len(cases) == 4 and all(len(c.samples) == D for c in cases)
    assert check_all(cases) == listed("mixed|%d," % D)


def test_two_weights_and_table_columns():
    for st in occ.STS:
        for wt in ("f32", "f64"):
            for D in occ.DS:
                cases = list(occ.two_weight_cases(st, wt, D))
                assert len(cases) == 1 and cases[0].w2 is not None and len(cases[0].samples) == D
                assert check_all(cases) == listed("two|%s|%s|%d" % (st, wt, D))
    cases = list(occ.table_column_cases())
    assert [c.weighted for c in cases] == [False, True]
    for c in cases:  # what execute_table_columns takes: 1 ... 64 rows that are the contiguous direction, >= 4096 columns
        assert c.lead and 1 <= c.n_rows <= 64 and c.n_cols >= 4096 and c.samples[0].dtype == np.float32
    assert check_all(cases) == listed("table|")


@pytest.mark.parametrize("n", occ.EXCHANGE_N)
def test_exchange(n):
    cases = list(occ.exchange_cases(n))
    assert [c.name.split("|")[2] for c in cases] == list(occ.EXCHANGE_KINDS)
    for c in cases:
        assert c.n_bins == 1024 * 1024 and c.w.dtype == np.float64 and c.params["partition"] == 1
    assert check_all(cases) == set() == listed("exchange|%d|" % n)


def test_host_route_cases():
    cases = list(occ.host_route_cases())
    assert sorted((c.home, c.weighted) for c in cases) == sorted((h, w) for h in ("lds", "global", "lanes", "route") for w in (False, True))


def test_the_listed_cases_exist():
    names = set()
    for st in occ.STS:
        for wt in occ.WTS:
            for D in occ.DS:
                names |= {"%s|%s|%d|%s" % (st, wt, D, c["home"]) for _, c in occ.float_case_specs(st, wt, D)}
    others = {n for n in occ.NO_EMPTY_BIN if n.split("|")[0] not in occ.STS}
    assert occ.NO_EMPTY_BIN - others <= names
    assert all(n.split("|")[0] in ("small", "int64", "generic", "mixed", "two", "table") for n in others)
