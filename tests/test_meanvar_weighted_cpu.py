"""histogram_mean_var with weights, without a GPU: argument checks before any device work, the C ABI surface, the weighted
oracle on hand-computed cases, and combine_weighted_mean_var (the dask merge) against the one-shot oracle."""
import inspect
import os
import re

import numpy as np
import pytest

import meanvar_weighted_oracle as mwo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_signature_has_weights():
    from xhistogram_amd import core, xarray

    sig = inspect.signature(core.histogram_mean_var)
    assert sig.parameters["weights"].default is None
    assert list(sig.parameters).index("weights") > list(sig.parameters).index("ddof")
    assert inspect.signature(xarray.histogram_mean_var).parameters["weights"].default is None


def test_argument_checks():
    from xhistogram_amd import core

    x = np.zeros((3, 4))
    v = np.ones((3, 4))
    with pytest.raises(ValueError):  # the weights' shape does not broadcast
        core.histogram_mean_var(x, values=v, weights=np.ones(5), bins=[np.linspace(0, 1, 3)])
    with pytest.raises(TypeError, match="complex"):
        core.histogram_mean_var(x, values=v, weights=np.ones((3, 4), complex), bins=[np.linspace(0, 1, 3)])
    with pytest.raises(TypeError):
        core.histogram_mean_var(x, values=v, weights=np.ones((3, 4)), bins=[np.linspace(0, 1, 3)], density=True)
    for ddof in (-1, 0.5, True):
        with pytest.raises(ValueError, match="ddof"):
            core.histogram_mean_var(x, values=v, weights=np.ones((3, 4)), bins=[np.linspace(0, 1, 3)], ddof=ddof)
    with pytest.raises(TypeError, match="weights"):  # histogram_quantile still refuses weights
        core.histogram_quantile(x, values=v, q=0.5, weights=np.ones((3, 4)), bins=[np.linspace(0, 1, 3)])


def test_c_abi_symbol():
    from xhistogram_amd import _native

    header = open(os.path.join(ROOT, "include", "xhist_amd.h")).read()
    assert re.search(r"int xhist_plan_execute_mean_var_weighted\(", header)
    assert "added within ABI v11" in header
    assert "#define XHIST_ABI_VERSION 11" in header
    assert "xhist_plan_execute_mean_var_weighted" in _native.EXPORTS
    lib = _native.load()
    assert len(lib.xhist_plan_execute_mean_var_weighted.argtypes) == 11
    assert len(lib.xhist_plan_execute_mean_var.argtypes) == 10
    assert lib.xhist_abi_version() == 11
    assert hasattr(_native.Plan, "execute_mean_var_weighted")


def _rows(x, v, w, edges):
    return mwo.mean_var_w_rows([np.asarray(x, float)[None]], [np.asarray(edges, float)], np.asarray(v, float)[None],
                               np.asarray(w, float)[None], exact=True)


@pytest.mark.parametrize("exact", [True, False])
def test_oracle_hand_cases(exact):
    edges = [0.0, 1.0, 2.0, 3.0, 4.0]
    x = [0.5, 0.5, 1.5, 1.5, 2.5, 2.5, 3.5, 9.0]
    v = [1.0, 3.0, 2.0, np.nan, 4.0, 8.0, 5.0, 1.0]
    w = [1.0, 3.0, 2.0, 7.0, 0.0, 0.0, np.nan, 1.0]
    W, mean, m2 = mwo.mean_var_w_rows([np.array(x)[None]], [np.array(edges)], np.array(v)[None], np.array(w)[None], exact=exact)
    # bin 0: W = 4, mean = (1 + 9) / 4 = 2.5, M2 = 1 * 2.25 + 3 * 0.25 = 3; bin 1: the NaN value drops its weight 7
    np.testing.assert_array_equal(W[0], [4.0, 2.0, 0.0, np.nan])
    np.testing.assert_array_equal(mean[0], [2.5, 2.0, np.nan, np.nan])
    np.testing.assert_array_equal(m2[0], [3.0, 0.0, np.nan, np.nan])
    np.testing.assert_array_equal(mwo.var_of(W, m2, 1)[0], [1.0, 0.0, np.nan, np.nan])
    # np.average agrees (ddof 0)
    assert mean[0][0] == np.average([1.0, 3.0], weights=[1.0, 3.0])
    assert m2[0][0] / W[0][0] == np.average((np.array([1.0, 3.0]) - 2.5) ** 2, weights=[1.0, 3.0])


def test_oracle_unit_weights_are_the_unweighted_oracle():
    import meanvar_oracle as mo

    rng = np.random.default_rng(2)
    x = rng.standard_normal((3, 500))
    v = np.round(rng.standard_normal((3, 500)) * 1024) / 1024
    edges = [np.linspace(-2, 2, 9)]
    W, mean, m2 = mwo.mean_var_w_rows([x], edges, v, np.ones_like(v), exact=True)
    cnt, mean_u, m2_u = mo.mean_var_rows([x], edges, v, exact=True)
    np.testing.assert_array_equal(W, cnt.astype(float))
    np.testing.assert_array_equal(mean, mean_u)
    np.testing.assert_array_equal(m2, m2_u)


def _partials(x, v, w, edges, cuts):
    parts = [_rows(x[a:b], v[a:b], w[a:b], edges) for a, b in zip(cuts[:-1], cuts[1:])]
    return [np.stack([p[k][0] for p in parts])[:, None] for k in range(3)]  # [blocks, 1, bins]


def test_combine_weighted_mean_var_equals_one_shot():
    from xhistogram_amd import core

    rng = np.random.default_rng(7)
    x = rng.uniform(0, 4, 4000)
    v = 50 + rng.standard_normal(4000)
    w = 10.0 ** rng.uniform(0, 3, 4000)
    edges = [0.0, 1.0, 2.0, 3.0, 4.0]
    W, mean, m2 = core.combine_weighted_mean_var(*_partials(x, v, w, edges, [0, 700, 1500, 1501, 3000, 4000]), axis=0)
    Wf, mf, qf = mwo.mean_var_w_rows([x[None]], [np.array(edges)], v[None], w[None], exact=False)
    np.testing.assert_allclose(W[0, 0], Wf[0], rtol=1e-13)
    np.testing.assert_allclose(mean[0, 0], mf[0], rtol=1e-13)
    np.testing.assert_allclose(m2[0, 0], qf[0], rtol=1e-9)


def test_combine_weighted_nan_and_zero_weight_partials():
    from xhistogram_amd import core

    nan = np.nan
    W = np.array([[0.0, 2.0, 3.0], [0.0, 0.0, nan], [4.0, 0.0, 1.0]])
    mean = np.array([[nan, 1.0, 5.0], [nan, nan, nan], [3.0, nan, 5.0]])
    m2 = np.array([[nan, 0.5, 1.0], [nan, nan, nan], [2.0, nan, 0.0]])
    cw, cm, cq = core.combine_weighted_mean_var(W, mean, m2, axis=0)
    np.testing.assert_array_equal(cw[0], [4.0, 2.0, nan])  # bin 0: the zero-weight partials are skipped; bin 2: NaN spreads
    np.testing.assert_array_equal(cm[0], [3.0, 1.0, nan])
    np.testing.assert_array_equal(cq[0], [2.0, 0.5, nan])
    cw, cm, cq = core.combine_weighted_mean_var(np.zeros((2, 1)), np.full((2, 1), nan), np.full((2, 1), nan), axis=0)
    assert cw[0, 0] == 0 and np.isnan(cm[0, 0]) and np.isnan(cq[0, 0])


def test_combine_weighted_with_unit_weights_is_combine_mean_var():
    from xhistogram_amd import core

    rng = np.random.default_rng(9)
    n = rng.integers(0, 5, (6, 4)).astype(float)
    mean = np.where(n > 0, rng.standard_normal((6, 4)), np.nan)
    m2 = np.where(n > 0, rng.uniform(0, 2, (6, 4)) * (n > 1), np.nan)
    a = core.combine_mean_var(n, mean, m2, axis=0)
    b = core.combine_weighted_mean_var(n, mean, m2, axis=0)
    for p, q in zip(a, b):
        np.testing.assert_array_equal(p, q)
