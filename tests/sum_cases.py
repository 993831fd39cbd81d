"""Directed data for histogram_sum: one bin's values per case, each built for one clause of the definition, with the total
the clause demands where it can be written down (EXPECT; the others are held to tests/sum_oracle.py and to math.fsum).

`layout()` puts case j into bin j of one histogram, shuffled, so a single call covers them all."""
import math

import numpy as np

F = float(0xFFFFFFFF)
REPEAT = 70_000  # 70 000 * 0xFFFFFFFF > 2^48: every limb sum carries far across 2^32


def _limbs(sign):
    """three values per group whose quanta fill one limb each with 0xFFFFFFFF at U = -20: A = (2^32 - 1) * 2^44 < 2^76, so
    E = 76 and U = E - 96"""
    group = np.array([math.ldexp(F, 44), math.ldexp(F, 12), math.ldexp(F, -20)])
    return sign * np.tile(group, REPEAT)


def _cancel():
    rng = np.random.default_rng(11)
    x = rng.uniform(1e6, 1e7, 500)
    return np.concatenate([x, -x, [1.25]])


def _wide():
    """magnitudes over 2^600: everything below 2^(E - 96) is truncated away, part of the rest loses low bits"""
    rng = np.random.default_rng(12)
    big = rng.uniform(1.0, 2.0, 40) * 2.0 ** 300
    mid = rng.uniform(1.0, 2.0, 200) * 2.0 ** rng.integers(200, 300, 200)
    small = rng.uniform(1.0, 2.0, 200) * 2.0 ** rng.integers(-300, 200, 200)
    return np.concatenate([big, -mid, small]) * rng.choice([-1.0, 1.0], 440)


CASES = {
    "limbs_pos": _limbs(1.0),
    "limbs_neg": _limbs(-1.0),
    "cancel": _cancel(),
    "subnormals": np.array([5e-324, 5e-324, 5e-324]),
    "subnormals_mixed": np.arange(-40, 100, dtype=np.float64) * 5e-324,
    "zeros": np.array([0.0, -0.0, -0.0, 0.0, -0.0]),
    "overflow3": np.array([1.5e308, 1.5e308, -1.5e308]),
    "overflow4": np.array([1.5e308] * 4),
    "overflow4_neg": np.array([-1.5e308] * 4),
    "pinf": np.array([1.0, np.inf, -3.0, np.inf]),
    "ninf": np.array([-np.inf, 2.0, 1e308]),
    "both_inf": np.array([np.inf, 5.0, -np.inf]),
    "pinf_nan": np.array([np.nan, np.inf, np.nan, 7.0]),
    "both_inf_nan": np.array([np.nan, -np.inf, np.inf]),
    "all_nan": np.array([np.nan] * 6),
    "wide": _wide(),
    "tie_even": np.array([2.0 ** 53, 1.0]),
    "tie_sticky": np.array([2.0 ** 53, 1.0, 2.0 ** -40]),
    "tie_odd": np.array([2.0 ** 53 + 2.0, 1.0]),
    "tie_even_neg": np.array([-(2.0 ** 53), -1.0]),
    "offset": 1e8 + 1e3 * np.random.default_rng(13).standard_normal(1000),
}

# (count, total) where the clause itself names the answer
EXPECT = {
    "cancel": (1001, 1.25),
    "subnormals": (3, 1.5e-323),
    "subnormals_mixed": (140, float(sum(range(-40, 100))) * 5e-324),
    "zeros": (5, 0.0),
    "overflow3": (3, 1.5e308),
    "overflow4": (4, math.inf),
    "overflow4_neg": (4, -math.inf),
    "pinf": (4, math.inf),
    "ninf": (3, -math.inf),
    "both_inf": (3, math.nan),
    "pinf_nan": (2, math.inf),
    "both_inf_nan": (2, math.nan),
    "all_nan": (0, 0.0),
    "tie_even": (2, 2.0 ** 53),
    "tie_sticky": (3, 2.0 ** 53 + 2.0),
    "tie_odd": (2, 2.0 ** 53 + 4.0),
    "tie_even_neg": (2, -(2.0 ** 53)),
}
# the limb cases' exact sums are integers times 2^-20: 70 000 * (2^96 - 1) * 2^-20, rounded once
_EXACT_LIMBS = REPEAT * ((1 << 96) - 1)
EXPECT["limbs_pos"] = (3 * REPEAT, _EXACT_LIMBS / (1 << 20))  # (int / int: correctly rounded)
EXPECT["limbs_neg"] = (3 * REPEAT, -_EXACT_LIMBS / (1 << 20))

# cases whose every value is converted exactly: the total is math.fsum's (math.fsum itself refuses overflow3: "intermediate
# overflow")
NARROW = ("limbs_pos", "limbs_neg", "cancel", "subnormals", "subnormals_mixed", "zeros", "tie_even", "tie_sticky",
          "tie_odd", "tie_even_neg", "offset")


def layout(seed=0, names=None):
    """(x, v, edges, names): case j's values at samples inside bin j of edges 0 .. n, in shuffled order"""
    names = list(CASES) if names is None else list(names)
    x = np.concatenate([np.full(len(CASES[n]), j + 0.5) for j, n in enumerate(names)])
    v = np.concatenate([CASES[n] for n in names])
    order = np.random.default_rng(seed).permutation(len(x))
    return x[order], v[order], np.arange(len(names) + 1, dtype=np.float64), names


def same_bits(got, want, what=""):
    """bit for bit, zeros compared by value, NaN where NaN"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape, what)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg="NaN bins differ " + what)
    ok = ~np.isnan(want) & ~((want == 0) & (got == 0))
    bad = got[ok].view(np.uint64) != want[ok].view(np.uint64)
    assert not bad.any(), "%d bins differ %s: first %r != %r" % (bad.sum(), what, got[ok][bad][0], want[ok][bad][0])
