"""xarray API of the MI355X-native histogram: label handling around ``core.histogram``.

Drop-in for ``xhistogram.xarray.histogram`` (reference: /root/reference/xhistogram/xarray.py:13-201)
with the same signature, output dims / coords / name and errors.  This module does no arithmetic
besides the bin centres; the data arrays (numpy, dask, or GPU-resident) go straight to
:func:`xhistogram_amd.core.histogram`.
"""

from __future__ import annotations

import numpy as np

from .core import histogram as _core_histogram
from .core import histogram_two_weights as _core_histogram_two_weights

__all__ = ["histogram", "histogram_extrema", "histogram_mean_var", "histogram_quantile", "histogram_weighted_quantile",
           "histogram_cov", "histogram_weighted_cov", "histogram_skew_kurt", "histogram_argextrema", "bin_index", "histogram_lookup",
           "histogram_anomaly", "histogram_sum", "bin_order", "bin_sort", "bin_rank", "histogram_mode", "bin_unique", "bin_weighted_unique", "histogram_weighted_mode"]


def _xr():
    try:
        import xarray
    except ImportError as e:  # the reference hard-imports xarray at module import (xarray.py:5)
        raise ImportError("xhistogram_amd.xarray.histogram needs the xarray package") from e
    return xarray


def histogram(*args, bins=None, range=None, dim=None, weights=None, density=False, block_size="auto",
              keep_coords=False, bin_dim_suffix="_bin"):
    """Histogram applied along specified dimensions.

    Parameters (identical to the reference, xarray.py:24-100)
    ----------
    args : xarray.DataArray objects
        Input data; N arguments give an N-dimensional histogram.  All must be named and alignable
        (``join="exact"``); they are broadcast against each other by dimension name.
    bins, range, weights, density, block_size
        As in :func:`xhistogram_amd.core.histogram`.  ``weights`` is a DataArray whose dims are a
        subset of the data's — or (an extension: the reference's TODO at xarray.py:106) a PAIR of
        such DataArrays, binned in one pass over the data; the result is then a pair of
        DataArrays (mean of ``A`` in the bins = ``h[0] / h[1]`` for ``weights=(A * w, w)``).
    dim : tuple of strings, optional
        Dimensions to histogram over; default all.
    keep_coords : bool
        Carry over coordinates compatible with the output dims.
    bin_dim_suffix : str
        Output bin dimensions are named ``<arg name> + bin_dim_suffix``.

    Returns
    -------
    xarray.DataArray named ``histogram_<name0>_<name1>…`` with dims = kept dims + bin dims and the
    bin midpoints as coordinates of the bin dims (carrying the inputs' attrs).
    """
    xr = _xr()
    data_args = list(args)
    n_data = len(data_args)
    for a in data_args:  # xarray.py:109-117
        if not isinstance(a, xr.DataArray):
            raise TypeError(
                "xhistogram.xarray.histogram accepts only xarray.DataArray objects but a %s was provided" % type(a).__name__
            )
    for a in data_args:
        assert a.name is not None, "all arrays must have a name"

    operands = list(data_args)
    if not keep_coords:  # coordinates only get in the way of alignment (xarray.py:119-123)
        operands = [a.reset_coords(drop=True) for a in operands]
    pair = isinstance(weights, (tuple, list))
    if pair:
        if len(weights) != 2:
            raise ValueError("weights must be one DataArray or a pair of them")
        if density:
            raise ValueError("density is not defined for a pair of weights")
    w_ops = list(weights) if pair else ([] if weights is None else [weights])
    operands.extend(w.reset_coords(drop=True) for w in w_ops)
    operands = list(xr.align(*operands, join="exact"))  # xarray.py:126
    first = operands[0]
    first_coords = first.coords

    # broadcast by name: union of dims in first-seen order, missing dims inserted with length 1
    # (the core broadcasts them without copying) — xarray.py:133-150
    dims_order = []
    for a in operands:
        for d in a.dims:
            if d not in dims_order:
                dims_order.append(d)
    lined_up = []
    for a in operands:
        missing = [d for d in dims_order if d not in a.dims]
        if missing:
            a = a.expand_dims({d: 1 for d in missing})
        if tuple(a.dims) != tuple(dims_order):
            a = a.transpose(*dims_order)
        lined_up.append(a)
    arrays = [a.data for a in lined_up]
    w_data = [arrays.pop() for _ in w_ops][::-1]

    if dim is not None:  # xarray.py:157-162
        kept_dims = [d for d in dims_order if d not in dim]
        axis = [lined_up[0].get_axis_num(d) for d in dim]
    else:
        kept_dims = []
        axis = None

    if pair:
        *h_all, edges = _core_histogram_two_weights(
            *arrays, weights=tuple(w_data), bins=bins, range=range, axis=axis, block_size=block_size
        )
    else:
        h_data, edges = _core_histogram(
            *arrays, weights=w_data[0] if w_data else None, bins=bins, range=range, axis=axis, density=density,
            block_size=block_size
        )
        h_all = [h_data]

    # output labels (xarray.py:174-201)
    bin_dims = [a.name + bin_dim_suffix for a in operands[:n_data]]
    out_dims = kept_dims + bin_dims
    coords = {name: first[name] for name in kept_dims if name in first_coords}
    for name, e, a in zip(bin_dims, edges, operands):
        coords[name] = ((name,), 0.5 * (e[:-1] + e[1:]), a.attrs)
    if keep_coords:
        for c in first_coords:
            if c not in coords and set(first[c].dims).issubset(out_dims):
                coords[c] = first[c]
    out_name = "_".join(["histogram"] + [a.name for a in operands[:n_data]])
    out = tuple(xr.DataArray(h, dims=out_dims, coords=coords, name=out_name) for h in h_all)
    return out if pair else out[0]


def histogram_extrema(*args, values, bins=None, range=None, dim=None, block_size="auto", keep_coords=False, bin_dim_suffix="_bin"):
    """Per-bin minimum and maximum of the DataArray ``values`` over the bins of ``args``
    (:func:`xhistogram_amd.core.histogram_extrema` with the labels of :func:`histogram`).

    ``args``, ``bins``, ``range``, ``dim``, ``keep_coords`` and ``bin_dim_suffix`` are those of :func:`histogram`; ``values``
    takes the place of its weights (dims a subset of the data's).  Returns ``(vmin, vmax)``: two DataArrays with the dims and
    coords ``histogram`` gives for the same ``args``, ``bins`` and ``dim``, named ``<values name>_min`` / ``_max`` (``values``
    when the DataArray has no name)."""
    from .core import histogram_extrema as _core_histogram_extrema

    (vmin, vmax), out_dims, coords, base = _values_statistic(
        "histogram_extrema", _core_histogram_extrema, args, values, bins, range, dim, keep_coords, bin_dim_suffix, block_size=block_size)
    xr = _xr()
    return (xr.DataArray(vmin, dims=out_dims, coords=coords, name="%s_min" % base),
            xr.DataArray(vmax, dims=out_dims, coords=coords, name="%s_max" % base))


def histogram_argextrema(*args, values, bins=None, range=None, dim=None, block_size="auto", keep_coords=False, bin_dim_suffix="_bin"):
    """Per-bin minimum and maximum of the DataArray ``values`` over the bins of ``args`` and where they lie
    (:func:`xhistogram_amd.core.histogram_argextrema` with the labels of :func:`histogram`).

    ``args``, ``bins``, ``range``, ``dim``, ``keep_coords``, ``bin_dim_suffix`` and ``values`` are those of
    :func:`histogram_extrema`.  Returns a dict of DataArrays with the dims and coords ``histogram`` gives: ``<values name>_min``
    and ``<values name>_max`` (float64), and for every reduced dim ``d`` ``<values name>_argmin_<d>`` and
    ``<values name>_argmax_<d>``: the int64 index along ``d`` of the first sample that holds the bin's extreme (first in C
    order over the reduced dims as the broadcast data orders them), ``-1`` in empty bins — what ``DataArray.isel`` takes.
    The flat positions are unravelled on the host."""
    from .core import histogram_argextrema as _core_histogram_argextrema

    reduced = []
    (amin, amax, vmin, vmax), out_dims, coords, base = _values_statistic(
        "histogram_argextrema", _core_histogram_argextrema, args, values, bins, range, dim, keep_coords, bin_dim_suffix,
        reduced=reduced, block_size=block_size)
    xr = _xr()
    out = {"%s_min" % base: xr.DataArray(vmin, dims=out_dims, coords=coords, name="%s_min" % base),
           "%s_max" % base: xr.DataArray(vmax, dims=out_dims, coords=coords, name="%s_max" % base)}
    for which, flat in (("argmin", amin), ("argmax", amax)):
        if hasattr(flat, "detach"):
            flat = flat.detach().cpu().numpy()
        empty = flat < 0
        stride = 1
        for d, size in reduced[::-1]:  # (C order: the last reduced dim walks fastest)
            name = "%s_%s_%s" % (base, which, d)
            out[name] = xr.DataArray(np.where(empty, -1, (flat // stride) % size), dims=out_dims, coords=coords, name=name)
            stride *= size
    return out


def histogram_mean_var(*args, values, bins=None, range=None, dim=None, ddof=0, block_size="auto", keep_coords=False,
                       bin_dim_suffix="_bin", weights=None):
    """Per-bin count, mean and variance of the DataArray ``values`` over the bins of ``args``
    (:func:`xhistogram_amd.core.histogram_mean_var` with the labels of :func:`histogram`).

    ``args``, ``bins``, ``range``, ``dim``, ``keep_coords`` and ``bin_dim_suffix`` are those of :func:`histogram`; ``values``
    takes the place of its weights (dims a subset of the data's).  Returns ``(count, mean, var)``: three DataArrays with the
    dims and coords ``histogram`` gives for the same ``args``, ``bins`` and ``dim``, named ``<values name>_count`` / ``_mean``
    / ``_var`` (``values`` when the DataArray has no name).

    ``weights`` (a DataArray whose dims are a subset of the data's, aligned and broadcast as ``values`` is) gives the
    frequency-weighted form: ``(sum_of_weights, mean, var)``, the first named ``<values name>_sum_of_weights``."""
    from .core import histogram_mean_var as _core_histogram_mean_var

    (cnt, mean, var), out_dims, coords, base = _values_statistic(
        "histogram_mean_var", _core_histogram_mean_var, args, values, bins, range, dim, keep_coords, bin_dim_suffix, ddof=ddof,
        block_size=block_size, weights=weights)
    xr = _xr()
    first = "count" if weights is None else "sum_of_weights"
    return tuple(xr.DataArray(a, dims=out_dims, coords=coords, name="%s_%s" % (base, suffix))
                 for a, suffix in ((cnt, first), (mean, "mean"), (var, "var")))


def histogram_sum(*args, values, bins=None, range=None, dim=None, block_size="auto", keep_coords=False, bin_dim_suffix="_bin"):
    """Per-bin count and order-independent sum of the DataArray ``values`` over the bins of ``args``
    (:func:`xhistogram_amd.core.histogram_sum` with the labels of :func:`histogram`).

    ``args``, ``bins``, ``range``, ``dim``, ``keep_coords``, ``bin_dim_suffix`` and ``values`` are those of
    :func:`histogram_mean_var`; there are no ``weights`` (multiply them into ``values``).  Returns ``(count, total)``: two
    DataArrays with the dims and coords ``histogram`` gives for the same ``args``, ``bins`` and ``dim``, named
    ``<values name>_count`` / ``<values name>_sum`` (``values`` when the DataArray has no name)."""
    from .core import histogram_sum as _core_histogram_sum

    (cnt, total), out_dims, coords, base = _values_statistic(
        "histogram_sum", _core_histogram_sum, args, values, bins, range, dim, keep_coords, bin_dim_suffix, block_size=block_size)
    xr = _xr()
    return (xr.DataArray(cnt, dims=out_dims, coords=coords, name="%s_count" % base),
            xr.DataArray(total, dims=out_dims, coords=coords, name="%s_sum" % base))


def histogram_mode(*args, values, bins=None, range=None, dim=None, block_size="auto", keep_coords=False, bin_dim_suffix="_bin"):
    """Per-bin most frequent value of the DataArray ``values`` over the bins of ``args``, how often it occurs and how many
    different values there are (:func:`xhistogram_amd.core.histogram_mode` with the labels of :func:`histogram`).

    ``args``, ``bins``, ``range``, ``dim``, ``keep_coords``, ``bin_dim_suffix`` and ``values`` are those of
    :func:`histogram_mean_var`; there are no ``weights``.  Returns ``(count, nunique, mode, mode_count)``: four DataArrays with
    the dims and coords ``histogram`` gives for the same ``args``, ``bins`` and ``dim``, named ``<values name>_count`` /
    ``_nunique`` / ``_mode`` / ``_mode_count`` (``values`` when the DataArray has no name)."""
    from .core import histogram_mode as _core_histogram_mode

    results, out_dims, coords, base = _values_statistic(
        "histogram_mode", _core_histogram_mode, args, values, bins, range, dim, keep_coords, bin_dim_suffix, block_size=block_size)
    xr = _xr()
    return tuple(xr.DataArray(a, dims=out_dims, coords=coords, name="%s_%s" % (base, suffix))
                 for a, suffix in zip(results, ("count", "nunique", "mode", "mode_count")))


def histogram_weighted_mode(*args, values, weights, bins=None, range=None, dim=None, keep_coords=False, bin_dim_suffix="_bin"):
    """Per-bin value of the DataArray ``values`` that carries the most weight over the bins of ``args``
    (:func:`xhistogram_amd.core.histogram_weighted_mode` with the labels of :func:`histogram`).

    ``weights`` is a DataArray whose dims are a subset of the data's, aligned and broadcast as ``values`` is (cell areas or
    volumes, ``cos(lat)``).  Returns ``(count, nunique, mode, mode_weight)``: four DataArrays with the dims and coords
    ``histogram`` gives, named ``<values name>_count`` / ``_nunique`` / ``_weighted_mode`` / ``_mode_weight`` (``values`` when
    the DataArray has no name)."""
    from .core import histogram_weighted_mode as _core_histogram_weighted_mode

    if weights is None:
        raise TypeError("histogram_weighted_mode needs weights")
    results, out_dims, coords, base = _values_statistic(
        "histogram_weighted_mode", _core_histogram_weighted_mode, args, values, bins, range, dim, keep_coords, bin_dim_suffix,
        weights=weights)
    xr = _xr()
    return tuple(xr.DataArray(a, dims=out_dims, coords=coords, name="%s_%s" % (base, suffix))
                 for a, suffix in zip(results, ("count", "nunique", "weighted_mode", "mode_weight")))


def histogram_skew_kurt(*args, values, bins=None, range=None, dim=None, weights=None, ddof=0, bias=True, fisher=True,
                        block_size="auto", keep_coords=False, bin_dim_suffix="_bin"):
    """Per-bin count, mean, variance, skewness and kurtosis of the DataArray ``values`` over the bins of ``args``
    (:func:`xhistogram_amd.core.histogram_skew_kurt` with the labels of :func:`histogram`).

    ``args``, ``bins``, ``range``, ``dim``, ``keep_coords``, ``bin_dim_suffix``, ``values`` and ``weights`` are those of
    :func:`histogram_mean_var`; ``ddof``, ``bias`` and ``fisher`` those of the core function.  Returns ``(count, mean, var,
    skew, kurt)``: five DataArrays with the dims and coords ``histogram`` gives, named ``<values name>_count`` (with
    ``weights``: ``<values name>_sum_of_weights``) / ``_mean`` / ``_var`` / ``_skew`` / ``_kurt`` (``values`` when the
    DataArray has no name)."""
    from .core import histogram_skew_kurt as _core_histogram_skew_kurt

    results, out_dims, coords, base = _values_statistic(
        "histogram_skew_kurt", _core_histogram_skew_kurt, args, values, bins, range, dim, keep_coords, bin_dim_suffix, ddof=ddof,
        bias=bias, fisher=fisher, block_size=block_size, weights=weights)
    xr = _xr()
    first = "count" if weights is None else "sum_of_weights"
    return tuple(xr.DataArray(a, dims=out_dims, coords=coords, name="%s_%s" % (base, suffix))
                 for a, suffix in zip(results, (first, "mean", "var", "skew", "kurt")))


def _with_quantile_coord(res, q, out_dims, coords, name):
    """the DataArray of per-bin quantiles: a leading ``quantile`` dimension with coordinate ``q`` when ``q`` is 1-D, a scalar
    ``quantile`` coordinate when it is a float (as ``DataArray.quantile`` does)"""
    qa = np.asarray(q, dtype=np.float64)
    if qa.ndim == 0:
        coords = dict(coords, quantile=((), qa))
    else:
        out_dims = ["quantile"] + list(out_dims)
        coords = dict(coords, quantile=(("quantile",), qa))
    return _xr().DataArray(res, dims=out_dims, coords=coords, name=name)


def histogram_quantile(*args, values, q, bins=None, range=None, dim=None, method="linear", block_size="auto", keep_coords=False,
                       bin_dim_suffix="_bin"):
    """Per-bin quantiles of the DataArray ``values`` over the bins of ``args``
    (:func:`xhistogram_amd.core.histogram_quantile` with the labels of :func:`histogram`).

    ``args``, ``bins``, ``range``, ``dim``, ``keep_coords`` and ``bin_dim_suffix`` are those of :func:`histogram`; ``values``
    takes the place of its weights (dims a subset of the data's); ``q`` and ``method`` are those of ``DataArray.quantile``.
    Returns one DataArray named ``<values name>_quantile`` (``values`` when the DataArray has no name) with the dims and coords
    ``histogram`` gives, behind a leading ``quantile`` dimension with coordinate ``q`` when ``q`` is 1-D, or with a scalar
    ``quantile`` coordinate when it is a float (as ``DataArray.quantile`` does)."""
    from .core import histogram_quantile as _core_histogram_quantile

    (res,), out_dims, coords, base = _values_statistic(
        "histogram_quantile", _core_histogram_quantile, args, values, bins, range, dim, keep_coords, bin_dim_suffix, q=q, method=method,
        block_size=block_size)
    return _with_quantile_coord(res, q, out_dims, coords, "%s_quantile" % base)


def histogram_weighted_quantile(*args, values, weights, q, bins=None, range=None, dim=None, method="inverted_cdf", block_size="auto",
                                keep_coords=False, bin_dim_suffix="_bin"):
    """Weighted per-bin quantiles of the DataArray ``values`` over the bins of ``args``
    (:func:`xhistogram_amd.core.histogram_weighted_quantile` with the labels of :func:`histogram_quantile`).

    ``weights`` is a DataArray whose dims are a subset of the data's, aligned and broadcast as ``values`` is (cell areas or
    volumes, ``cos(lat)``); ``method`` accepts only ``"inverted_cdf"``.  Returns one DataArray named
    ``<values name>_weighted_quantile`` with the ``quantile`` dimension or scalar coordinate of :func:`histogram_quantile`."""
    from .core import histogram_weighted_quantile as _core_histogram_weighted_quantile

    (res,), out_dims, coords, base = _values_statistic(
        "histogram_weighted_quantile", _core_histogram_weighted_quantile, args, values, bins, range, dim, keep_coords, bin_dim_suffix,
        q=q, method=method, block_size=block_size, weights=weights)
    return _with_quantile_coord(res, q, out_dims, coords, "%s_weighted_quantile" % base)


def histogram_cov(*args, values, bins=None, range=None, dim=None, ddof=0, block_size="auto", keep_coords=False, bin_dim_suffix="_bin"):
    """Per-bin count, means, variances and covariance of the pair of DataArrays ``values=(A, B)`` over the bins of ``args``
    (:func:`xhistogram_amd.core.histogram_cov` with the labels of :func:`histogram`).

    ``args``, ``bins``, ``range``, ``dim``, ``keep_coords`` and ``bin_dim_suffix`` are those of :func:`histogram`; ``A`` and
    ``B`` are lined up as ``values`` of :func:`histogram_mean_var` (dims a subset of the data's).  Returns a dict of six
    DataArrays with the dims and coords ``histogram`` gives, keyed by their names (``xarray.Dataset(result)`` makes a Dataset
    of it): ``<a>_<b>_count``, ``<a>_mean``, ``<b>_mean``, ``<a>_var``, ``<b>_var``, ``<a>_<b>_cov``, with ``<a>`` / ``<b>``
    the names of the DataArrays (``a`` / ``b`` for a nameless one).  There is no ``weights`` parameter here: the weighted form
    is :func:`histogram_weighted_cov`."""
    from .core import _value_pair, histogram_cov as _core_histogram_cov

    A, B = _value_pair(values, "histogram_cov", "DataArrays")
    results, out_dims, coords, _ = _values_statistic(
        "histogram_cov", _core_histogram_cov, args, (A, B), bins, range, dim, keep_coords, bin_dim_suffix, ddof=ddof,
        block_size=block_size, pair=True)
    xr = _xr()
    a, b = A.name or "a", B.name or "b"
    names = ("%s_%s_count" % (a, b), "%s_mean" % a, "%s_mean" % b, "%s_var" % a, "%s_var" % b, "%s_%s_cov" % (a, b))
    return {n: xr.DataArray(r, dims=out_dims, coords=coords, name=n) for n, r in zip(names, results)}


def histogram_weighted_cov(*args, values, weights, bins=None, range=None, dim=None, ddof=0, block_size="auto", keep_coords=False,
                           bin_dim_suffix="_bin"):
    """Weighted per-bin means, variances and covariance of the pair of DataArrays ``values=(A, B)`` over the bins of ``args``
    (:func:`xhistogram_amd.core.histogram_weighted_cov` with the labels of :func:`histogram_cov`).

    ``weights`` is a DataArray whose dims are a subset of the data's, aligned and broadcast as ``A`` and ``B`` are (cell areas
    or volumes, ``cos(lat)``).  Returns a dict of six DataArrays named like :func:`histogram_cov`'s, with
    ``<a>_<b>_sum_of_weights`` in place of ``<a>_<b>_count``."""
    from .core import _value_pair, histogram_weighted_cov as _core_histogram_weighted_cov

    A, B = _value_pair(values, "histogram_weighted_cov", "DataArrays")
    if weights is None:
        raise TypeError("histogram_weighted_cov needs weights")
    results, out_dims, coords, _ = _values_statistic(
        "histogram_weighted_cov", _core_histogram_weighted_cov, args, (A, B), bins, range, dim, keep_coords, bin_dim_suffix, ddof=ddof,
        block_size=block_size, weights=weights, pair=True)
    xr = _xr()
    a, b = A.name or "a", B.name or "b"
    names = ("%s_%s_sum_of_weights" % (a, b), "%s_mean" % a, "%s_mean" % b, "%s_var" % a, "%s_var" % b, "%s_%s_cov" % (a, b))
    return {n: xr.DataArray(r, dims=out_dims, coords=coords, name=n) for n, r in zip(names, results)}


def _values_statistic(name, core_fn, args, values, bins, range, dim, keep_coords, bin_dim_suffix, weights=None, reduced=None,
                      pair=False, **kw):
    """a per-bin statistic of ``values`` (a DataArray; ``pair``: two of them) with the labels of :func:`histogram`: (core_fn's
    arrays, dims, coords, the first values' name or "values").  The values and then ``weights`` (a DataArray or None) are lined
    up with the data and passed on in this order, as core_fn's values and weights.  ``reduced`` (a list, or None) receives the
    (name, broadcast size) of every reduced dim, in ascending axis number."""
    xr = _xr()
    data_args = list(args)
    n_data = len(data_args)
    extra = (list(values) if pair else [values]) + ([] if weights is None else [weights])
    for a in data_args + extra:
        if not isinstance(a, xr.DataArray):
            raise TypeError(
                "xhistogram.xarray.%s accepts only xarray.DataArray objects but a %s was provided" % (name, type(a).__name__)
            )
    for a in data_args:
        assert a.name is not None, "all arrays must have a name"
    operands = list(data_args) if keep_coords else [a.reset_coords(drop=True) for a in data_args]
    operands += [a.reset_coords(drop=True) for a in extra]
    operands = list(xr.align(*operands, join="exact"))
    first = operands[0]
    first_coords = first.coords
    dims_order = []
    for a in operands:
        for d in a.dims:
            if d not in dims_order:
                dims_order.append(d)
    lined_up = []
    for a in operands:
        missing = [d for d in dims_order if d not in a.dims]
        if missing:
            a = a.expand_dims({d: 1 for d in missing})
        if tuple(a.dims) != tuple(dims_order):
            a = a.transpose(*dims_order)
        lined_up.append(a)
    arrays = [a.data for a in lined_up]
    if weights is not None:
        kw["weights"] = arrays.pop()
    v_data = tuple(arrays[n_data:]) if pair else arrays[n_data]
    del arrays[n_data:]
    if dim is not None:
        kept_dims = [d for d in dims_order if d not in dim]
        axis = [lined_up[0].get_axis_num(d) for d in dim]
    else:
        kept_dims = []
        axis = None
    if reduced is not None:
        reduced.extend((d, max(int(a.sizes[d]) for a in lined_up)) for d in dims_order if d not in kept_dims)
    *results, edges = core_fn(*arrays, values=v_data, bins=bins, range=range, axis=axis, **kw)
    bin_dims = [a.name + bin_dim_suffix for a in operands[:n_data]]
    out_dims = kept_dims + bin_dims
    coords = {name: first[name] for name in kept_dims if name in first_coords}
    for name, e, a in zip(bin_dims, edges, operands):
        coords[name] = ((name,), 0.5 * (e[:-1] + e[1:]), a.attrs)
    if keep_coords:
        for c in first_coords:
            if c not in coords and set(first[c].dims).issubset(out_dims):
                coords[c] = first[c]
    return results, out_dims, coords, extra[0].name or "values"


# ---------------------------------------------------------------------------------------------
# per-sample maps: DataArrays on the broadcast dims of the inputs
# ---------------------------------------------------------------------------------------------
def _lined_up(name, data_args, extra, dim=None):
    """the inputs of a per-sample map (DataArrays: the named samples, then `extra`), aligned exactly and broadcast by
    dimension name as :func:`histogram` does: (their data in one dim order, that order, the kept dims (those not in `dim`;
    none for ``dim=None``), the axes of `dim` in that order (None: all), the samples' coordinates on those dims)"""
    xr = _xr()
    for a in list(data_args) + list(extra):
        if not isinstance(a, xr.DataArray):
            raise TypeError(
                "xhistogram.xarray.%s accepts only xarray.DataArray objects but a %s was provided" % (name, type(a).__name__)
            )
    for a in data_args:
        assert a.name is not None, "all arrays must have a name"
    operands = list(xr.align(*[a.reset_coords(drop=True) for a in list(data_args) + list(extra)], join="exact"))
    dims_order = []
    for a in operands:
        for d in a.dims:
            if d not in dims_order:
                dims_order.append(d)
    arrays = []
    for a in operands:
        missing = [d for d in dims_order if d not in a.dims]
        if missing:
            a = a.expand_dims({d: 1 for d in missing})
        if tuple(a.dims) != tuple(dims_order):
            a = a.transpose(*dims_order)
        arrays.append(a.data)
    kept = [d for d in dims_order if dim is not None and d not in dim]
    axis = None if dim is None else [dims_order.index(d) for d in dim]
    first = operands[0]
    return arrays, dims_order, kept, axis, {d: first[d] for d in dims_order if d in first.coords}


def _row_array(data, kept, coords, last_dim, name):
    """a per-row output: a DataArray on the kept dims, with the samples' coordinates on them, and a new last dim"""
    return _xr().DataArray(data, dims=kept + [last_dim], coords={d: coords[d] for d in kept if d in coords}, name=name)


def bin_index(*args, bins=None, range=None):
    """The bin of every sample (:func:`xhistogram_amd.core.bin_index`): an int64 DataArray on the broadcast dims of ``args``,
    named ``<first arg>_bin_index``, ``-1`` where ``histogram`` drops the sample."""
    from .core import bin_index as _core_bin_index

    arrays, dims_order, _, _, coords = _lined_up("bin_index", args, [])
    out, _ = _core_bin_index(*arrays, bins=bins, range=range)
    return _xr().DataArray(out, dims=dims_order, coords=coords, name="%s_bin_index" % args[0].name)


def histogram_lookup(*args, table, bins=None, range=None, dim=None, bin_dim_suffix="_bin"):
    """A per-bin DataArray read back at every sample (:func:`xhistogram_amd.core.histogram_lookup`).  ``table`` has the dims
    :func:`histogram` gives for the same ``args`` and ``dim`` (kept dims and ``<arg name> + bin_dim_suffix``, in any order).
    Returns a float64 DataArray on the broadcast dims of ``args``, named ``<table name>_lookup`` (``table`` without a name)."""
    from .core import histogram_lookup as _core_histogram_lookup

    xr = _xr()
    if not isinstance(table, xr.DataArray):
        raise TypeError("xhistogram.xarray.histogram_lookup accepts only xarray.DataArray objects but a %s was provided"
                        % type(table).__name__)
    arrays, dims_order, kept, axis, coords = _lined_up("histogram_lookup", args, [], dim)
    want = kept + [a.name + bin_dim_suffix for a in args]
    if set(table.dims) != set(want):
        raise ValueError("table has dims %s, but histogram gives %s for these arguments" % (tuple(table.dims), tuple(want)))
    t = table if tuple(table.dims) == tuple(want) else table.transpose(*want)
    out, _ = _core_histogram_lookup(*arrays, table=t.data, bins=bins, range=range, axis=axis)
    return xr.DataArray(out, dims=dims_order, coords=coords, name="%s_lookup" % (table.name or "table"))


def histogram_anomaly(*args, values, bins=None, range=None, dim=None, weights=None, ddof=0, standardize=False):
    """Every sample's value relative to the mean of its bin (:func:`xhistogram_amd.core.histogram_anomaly`); ``values`` and
    ``weights`` are lined up as :func:`histogram_mean_var` lines them up.  Returns a float64 DataArray on the broadcast dims of
    the inputs, named ``<values name>_anomaly`` (``values`` without a name)."""
    from .core import histogram_anomaly as _core_histogram_anomaly

    if values is None:
        raise TypeError("histogram_anomaly needs values")
    extra = [values] + ([] if weights is None else [weights])
    arrays, dims_order, _, axis, coords = _lined_up("histogram_anomaly", args, extra, dim)
    n = len(args)
    out, _ = _core_histogram_anomaly(*arrays[:n], values=arrays[n], bins=bins, range=range, axis=axis,
                                     weights=arrays[n + 1] if weights is not None else None, ddof=ddof, standardize=standardize)
    return _xr().DataArray(out, dims=dims_order, coords=coords, name="%s_anomaly" % (values.name or "values"))


def bin_order(*args, bins=None, range=None, dim=None):
    """The samples grouped by bin (:func:`xhistogram_amd.core.bin_order`): two int64 DataArrays on the kept dims (those not in
    ``dim``; none for ``dim=None``), ``<first arg>_bin_order`` with a new last dim ``<first arg>_order`` (the positions over the
    dims of ``dim`` in the inputs' broadcast dim order, sorted stably by bin, dropped samples last) and ``<first arg>_bin_offsets``
    with a new last dim ``<first arg>_bin_offset`` (where each bin's run starts; the last entry: where the dropped samples
    start)."""
    from .core import bin_order as _core_bin_order

    arrays, _, kept, axis, coords = _lined_up("bin_order", args, [], dim)
    order, offsets, _ = _core_bin_order(*arrays, bins=bins, range=range, axis=axis)
    name = args[0].name
    return (_row_array(order, kept, coords, "%s_order" % name, "%s_bin_order" % name),
            _row_array(offsets, kept, coords, "%s_bin_offset" % name, "%s_bin_offsets" % name))


def bin_sort(*args, values, bins=None, range=None, dim=None, descending=False):
    """The samples grouped by bin and sorted by value inside each bin (:func:`xhistogram_amd.core.bin_sort`); ``values`` is
    lined up as :func:`histogram_extrema` lines it up.  Two int64 DataArrays on the kept dims (those not in ``dim``; none for
    ``dim=None``): ``<values name>_bin_sort`` with a new last dim ``<values name>_order`` (the positions over the dims of
    ``dim`` in the inputs' broadcast dim order, by bin, then by value, NaN last in its bin, dropped samples last) and
    ``<values name>_bin_offsets`` with a new last dim ``<values name>_bin_offset`` (where each bin's run starts; the last entry:
    where the dropped samples start).  ``values`` without a name is called ``values``."""
    from .core import bin_sort as _core_bin_sort

    if values is None:
        raise TypeError("bin_sort needs values")
    arrays, _, kept, axis, coords = _lined_up("bin_sort", args, [values], dim)
    n = len(args)
    order, offsets, _ = _core_bin_sort(*arrays[:n], values=arrays[n], bins=bins, range=range, axis=axis, descending=descending)
    name = values.name or "values"
    return (_row_array(order, kept, coords, "%s_order" % name, "%s_bin_sort" % name),
            _row_array(offsets, kept, coords, "%s_bin_offset" % name, "%s_bin_offsets" % name))


def bin_rank(*args, values, bins=None, range=None, dim=None, method="average", descending=False, pct=False):
    """The rank of every sample's value among the values of its bin (:func:`xhistogram_amd.core.bin_rank`); ``values`` is lined up
    as :func:`histogram_extrema` lines it up.  Returns a float64 DataArray on the broadcast dims of the inputs, named
    ``<values name>_bin_rank`` (``values`` without a name)."""
    from .core import bin_rank as _core_bin_rank

    if values is None:
        raise TypeError("bin_rank needs values")
    arrays, dims_order, _, axis, coords = _lined_up("bin_rank", args, [values], dim)
    n = len(args)
    out, _ = _core_bin_rank(*arrays[:n], values=arrays[n], bins=bins, range=range, axis=axis, method=method, descending=descending,
                            pct=pct)
    return _xr().DataArray(out, dims=dims_order, coords=coords, name="%s_bin_rank" % (values.name or "values"))


def bin_unique(*args, values, bins=None, range=None, dim=None, size=None, return_inverse=False):
    """The distinct values of every bin and how often each occurs (:func:`xhistogram_amd.core.bin_unique`); ``values`` is lined
    up as :func:`bin_sort` lines it up.  DataArrays on the kept dims (those not in ``dim``; none for ``dim=None``):
    ``<values name>_unique`` (float64) and ``<values name>_unique_counts`` (int64) with a new last dim ``<values name>_unique``
    (a row's entries, bin by bin, ascending inside each bin, then padding), and ``<values name>_unique_offsets`` (int64) with a
    new last dim ``<values name>_bin_offset`` (where each bin's entries start; the last entry: how many there are).  With
    ``return_inverse`` a fourth, ``<values name>_unique_inverse`` (int64) on the broadcast dims of the inputs: every sample's
    entry, ``-1`` where it has none.  ``values`` without a name is called ``values``."""
    from .core import bin_unique as _core_bin_unique

    if values is None:
        raise TypeError("bin_unique needs values")
    arrays, dims_order, kept, axis, coords = _lined_up("bin_unique", args, [values], dim)
    n = len(args)
    res = _core_bin_unique(*arrays[:n], values=arrays[n], bins=bins, range=range, axis=axis, size=size, return_inverse=return_inverse)
    name = values.name or "values"
    out = (_row_array(res[0], kept, coords, "%s_unique" % name, "%s_unique" % name),
           _row_array(res[1], kept, coords, "%s_unique" % name, "%s_unique_counts" % name),
           _row_array(res[2], kept, coords, "%s_bin_offset" % name, "%s_unique_offsets" % name))
    if len(res) == 5:
        out += (_xr().DataArray(res[3], dims=dims_order, coords=coords, name="%s_unique_inverse" % name),)
    return out


def bin_weighted_unique(*args, values, weights, bins=None, range=None, dim=None, size=None, return_inverse=False):
    """The distinct values of every bin, how often each occurs and how much weight each carries
    (:func:`xhistogram_amd.core.bin_weighted_unique`); ``values`` and then ``weights`` (cell areas or volumes, ``cos(lat)``) are
    lined up as :func:`bin_sort` lines its values up.  :func:`bin_unique`'s DataArrays, and behind the counts
    ``<values name>_unique_weight_sums`` (float64) on the same new last dim ``<values name>_unique``: ``(unique, counts,
    weight_sums, offsets)``, with ``return_inverse`` the inverse after them."""
    from .core import bin_weighted_unique as _core_bin_weighted_unique

    if values is None:
        raise TypeError("bin_weighted_unique needs values")
    if weights is None:
        raise TypeError("bin_weighted_unique needs weights")
    arrays, dims_order, kept, axis, coords = _lined_up("bin_weighted_unique", args, [values, weights], dim)
    n = len(args)
    res = _core_bin_weighted_unique(*arrays[:n], values=arrays[n], weights=arrays[n + 1], bins=bins, range=range, axis=axis, size=size,
                                    return_inverse=return_inverse)
    name = values.name or "values"
    out = (_row_array(res[0], kept, coords, "%s_unique" % name, "%s_unique" % name),
           _row_array(res[1], kept, coords, "%s_unique" % name, "%s_unique_counts" % name),
           _row_array(res[2], kept, coords, "%s_unique" % name, "%s_unique_weight_sums" % name),
           _row_array(res[3], kept, coords, "%s_bin_offset" % name, "%s_unique_offsets" % name))
    if len(res) == 6:
        out += (_xr().DataArray(res[4], dims=dims_order, coords=coords, name="%s_unique_inverse" % name),)
    return out
