"""Numpy-style API of the MI355X-native xhistogram hot path.

Drop-in for ``xhistogram.core`` (reference: /root/reference/xhistogram/core.py): ``histogram``
keeps the reference's exact signature and semantics (core.py:250-466) and so do the two internal
layers the reference's dask branch and xarray wrapper call, ``_bincount`` (core.py:197-247) and
``_bincount_2d_vectorized`` (core.py:137-194).  What changes is what runs underneath:
``_bincount_2d_vectorized`` hands strided [rows, cols] views to ``libxhist_amd.so`` and ONE fused HIP
kernel does digitize -> joint index -> scatter-add on the GPU (see csrc/xhist_kernels.hip.h).

Inputs may be numpy arrays (staged to the GPU by the library, result returned as numpy, exactly
like the reference), ``torch`` tensors resident on an MI355X (no copies; result returned as a
torch tensor on the same device) or, when dask is importable, dask arrays (the reference's
blockwise + sum graph, each block computed on the GPU).  There is no CPU implementation in this
package: without the native library and a GPU the compute call raises.
"""

from __future__ import annotations

import math
import os
import re
import threading
from collections import OrderedDict, namedtuple
from collections.abc import Iterable
from functools import partial

import warnings

import numpy as np

from . import _native
from .devicearray import DeviceArray, _nocopy_reshape_strides

# range is a keyword of histogram(), like in the reference
_range = range

__all__ = ["histogram", "histogram_two_weights", "histogram_extrema", "histogram_mean_var", "histogram_quantile",
           "histogram_weighted_quantile", "histogram_cov", "histogram_weighted_cov", "combine_weighted_cov",
           "histogram_skew_kurt", "combine_skew_kurt", "combine_weighted_skew_kurt", "histogram_argextrema", "histogram_sum", "bin_order", "bin_sort", "bin_rank",
           "histogram_mode", "bin_unique", "bin_weighted_unique", "histogram_weighted_mode"]


# ---------------------------------------------------------------------------------------------
# backends: numpy (host memory) and torch (device memory)
# ---------------------------------------------------------------------------------------------
def _is_torch(a):
    return type(a).__module__.split(".")[0] == "torch" and hasattr(a, "data_ptr")


def _is_devarr(a):
    return type(a) is DeviceArray


def _backend_of(arrays):
    """"torch" (GPU tensors), "device" (DeviceArray: GPU memory without torch) or "numpy" (host memory)"""
    if any(_is_torch(a) for a in arrays):
        return "torch"
    return "device" if any(_is_devarr(a) for a in arrays) else "numpy"


def _is_dask(a):
    mod = type(a).__module__.split(".")[0]
    return mod == "dask" and hasattr(a, "chunks")


def _torch():
    import torch

    return torch


_TORCH_TAGS = None


def _torch_tag(dtype):
    global _TORCH_TAGS
    if _TORCH_TAGS is None:
        t = _torch()
        m = {
            t.float64: _native.F64, t.float32: _native.F32, t.float16: _native.F16, t.int64: _native.I64,
            t.int32: _native.I32, t.int16: _native.I16, t.int8: _native.I8, t.uint8: _native.U8, t.bool: _native.BOOL,
        }
        for name, tag in (("uint16", _native.U16), ("uint32", _native.U32), ("uint64", _native.U64)):
            if hasattr(t, name):
                m[getattr(t, name)] = tag
        _TORCH_TAGS = m
    try:
        return _TORCH_TAGS[dtype]
    except KeyError:
        raise TypeError("torch dtype %s is not supported by the MI355X histogram path" % dtype) from None


_TAG_NP = {
    _native.F64: np.float64, _native.F32: np.float32, _native.F16: np.float16, _native.I64: np.int64,
    _native.I32: np.int32, _native.I16: np.int16, _native.I8: np.int8, _native.U64: np.uint64,
    _native.U32: np.uint32, _native.U16: np.uint16, _native.U8: np.uint8, _native.BOOL: np.bool_,
}


# the local rank of a one-process-per-GPU job, as the common launchers export it (torch.distributed.run, srun, Open MPI,
# MVAPICH2 / MPICH-hydra): such a process keeps to ITS GPU instead of spreading over the node's
LOCAL_RANK_VARS = ("XHIST_AMD_DEVICE", "LOCAL_RANK", "SLURM_LOCALID", "OMPI_COMM_WORLD_LOCAL_RANK", "MV2_COMM_WORLD_LOCAL_RANK",
                   "MPI_LOCALRANKID")


def launcher_local_rank():
    """the first of LOCAL_RANK_VARS that is set, as an int; None outside a one-process-per-GPU launcher"""
    for key in LOCAL_RANK_VARS:
        v = os.environ.get(key)
        if v not in (None, ""):
            try:
                return int(v)
            except ValueError:
                continue
    return None


# how many tasks the launcher started on THIS node (torch.distributed.run, Slurm, Open MPI, MVAPICH2, MPICH-hydra)
LOCAL_SIZE_VARS = ("LOCAL_WORLD_SIZE", "SLURM_NTASKS_PER_NODE", "SLURM_STEP_TASKS_PER_NODE", "SLURM_TASKS_PER_NODE",
                   "OMPI_COMM_WORLD_LOCAL_SIZE", "MV2_COMM_WORLD_LOCAL_SIZE", "MPI_LOCALNRANKS")


def _slurm_tasks_of_node(spec, node):
    """this node's entry of Slurm's per-node task list — "4(x2),1" = nodes 0 and 1 run four tasks, node 2 one — or None
    when the list cannot be read or does not reach `node`"""
    counts = []
    for item in spec.strip().split(","):
        m = re.fullmatch(r"\s*(\d+)(?:\(x(\d+)\))?\s*", item)
        if not m:
            return None
        counts += [int(m.group(1))] * int(m.group(2) or 1)
    return counts[node] if 0 <= node < len(counts) else None


def launcher_local_size():
    """tasks of this job on THIS node as the launcher reports them, or None when it does not say.  Slurm's
    SLURM_(STEP_)TASKS_PER_NODE lists every node ("1,4", "1(x2),4"): the entry of $SLURM_NODEID is taken (the
    leading integer is the FIRST node's count); a list of several nodes without a readable node id says nothing."""
    for key in LOCAL_SIZE_VARS:
        v = os.environ.get(key)
        if v in (None, ""):
            continue
        if key in ("SLURM_STEP_TASKS_PER_NODE", "SLURM_TASKS_PER_NODE"):
            try:
                node = int(os.environ.get("SLURM_NODEID", ""))
            except ValueError:
                node = 0 if re.fullmatch(r"\s*\d+\s*", v) else -1  # (one node, one figure: unambiguous without an id)
            n = _slurm_tasks_of_node(v, node)
            if n is not None:
                return n
            continue
        try:
            return int(v.strip())
        except ValueError:
            continue
    return None


def default_device():
    """GPU used for host (numpy) inputs: $XHIST_AMD_DEVICE, else the launcher's local rank ($LOCAL_RANK, $SLURM_LOCALID,
    $OMPI_COMM_WORLD_LOCAL_RANK, …) — taken modulo the number of GPUs this process can see: a task the launcher bound to ONE
    GPU (srun --gpus-per-task=1 / --gpu-bind, ROCR_VISIBLE_DEVICES: every task sees its GPU as device 0) has local rank k
    and device 0 — else 0."""
    explicit = os.environ.get("XHIST_AMD_DEVICE")
    if explicit not in (None, ""):
        try:
            return int(explicit)  # (the user's own choice is not second-guessed: a wrong index fails loudly in require_device)
        except ValueError:
            pass
    r = launcher_local_rank()
    if r is None:
        return 0
    try:
        n = _native.device_count()
    except Exception:
        n = 0
    return r % n if n > 0 else r


_tls = threading.local()


def _torch_device_index(device):
    """(logical) device index of this library for a torch.device: the tensor's own index — except under
    $XHIST_AMD_DEVICE_ALIAS (tests: several logical devices on one GPU), where a thread that multigpu bound to logical
    device k keeps k for the tensors that live on k's physical GPU"""
    idx = device.index if device.index is not None else _torch().cuda.current_device()
    bound = getattr(_tls, "device", None)
    if bound is not None and bound != idx and os.environ.get("XHIST_AMD_DEVICE_ALIAS") and _native.physical_device(bound) == idx:
        return bound
    return idx


def _host_device():
    """GPU the calling thread stages host (numpy) inputs to: the one its multi-GPU driver bound it to
    (multigpu.on_device: a shard worker, or one dask block), else default_device()"""
    d = getattr(_tls, "device", None)
    return default_device() if d is None else d


def _np_dtype_of(a):
    """numpy dtype describing the element type of a numpy array or torch tensor."""
    if _is_torch(a):
        return np.dtype(_TAG_NP[_torch_tag(a.dtype)])
    return a.dtype


# ---------------------------------------------------------------------------------------------
# plan cache (edge tables live on the GPU; building one costs a launch + a sync)
# ---------------------------------------------------------------------------------------------
_plans = OrderedDict()
_areas = OrderedDict()  # device-resident bin areas of the density epilogue, per set of edges
_plans_lock = threading.Lock()
_plan_create_lock = threading.Lock()
_PLAN_CACHE = 32


def _get_plan(edges, cmp_domain, device):
    key = (device, cmp_domain) + tuple((e.dtype.str, e.tobytes()) for e in edges)
    with _plans_lock:
        plan = _plans.get(key)
        if plan is not None:
            _plans.move_to_end(key)
            return plan
    # one creation at a time (and no duplicates): building the tables costs a launch and a device synchronisation, and
    # dask's threaded scheduler sends every block of a fresh graph here at once
    with _plan_create_lock:
        with _plans_lock:
            plan = _plans.get(key)
        if plan is None:
            plan = _native.Plan(edges, cmp_domain, device)
            with _plans_lock:
                _plans[key] = plan
                while len(_plans) > _PLAN_CACHE:
                    _plans.popitem(last=False)
    return plan


def _compare_domain(sample_dtypes, edges):
    """Decide how samples are compared with edges, following numpy's promotion in searchsorted
    (core.py:170): float64 compares unless BOTH sides are integers / datetimes, then exact int64;
    decided per input (CMP_PER_DIM | mask when the inputs differ).
    Returns (cmp_domain, edges converted to the domain's dtype, per-input 'view as int64' flag)."""
    doms = []
    conv = []
    for sd, e in zip(sample_dtypes, edges):
        e = np.asarray(e)
        if e.ndim != 1:
            raise AssertionError("bin edges must be 1-D")  # core.py:148
        if sd.kind in "mM" or e.dtype.kind in "mM":
            common = np.result_type(sd, e.dtype)  # TypeError when only one side is a datetime
            conv.append(e.astype(common).view(np.int64))
            doms.append((_native.CMP_I64, common))
            continue
        if sd.kind == "c" or e.dtype.kind == "c":
            raise TypeError("complex samples / bin edges are not supported")
        if sd.kind not in "fiub" or e.dtype.kind not in "fiub":
            raise TypeError("cannot histogram dtype %s against bin edges of dtype %s" % (sd, e.dtype))
        if sd.itemsize > 8 or e.dtype.itemsize > 8:
            raise TypeError("extended-precision floats are not supported on the GPU path")
        common = np.result_type(sd, e.dtype)
        if common.kind == "f":
            conv.append(e.astype(np.float64))
            doms.append((_native.CMP_F64, None))
        elif common == np.dtype(np.uint64):
            # unsigned on both sides: the int64 domain with the sign bit flipped (CMP_UNSIGNED)
            conv.append(e.astype(np.uint64))
            doms.append((_native.CMP_I64, "unsigned"))
        else:
            conv.append(e.astype(np.int64))
            doms.append((_native.CMP_I64, None))
    # Integer samples of at most 32 bits against integer edges within +-2^53: both sides are exact
    # in float64, so the comparison may run there — which is where the vector kernels are
    # (`bins=np.arange(257)` on uint8 / int32 data: 3-4x the generic int64 family).
    unsigned = [c == "unsigned" for _, c in doms]
    doms = [(d, None if c == "unsigned" else c) for d, c in doms]
    if any(unsigned):
        # one flag per plan: every int64-domain input must then be unsigned
        if any(d == _native.CMP_I64 and not u for (d, _), u in zip(doms, unsigned)):
            raise NotImplementedError("uint64 inputs together with signed 64-bit integer / datetime inputs")
        mask = sum(1 << k for k, (d, _) in enumerate(doms) if d == _native.CMP_I64)
        full = mask == (1 << len(doms)) - 1
        return (_native.CMP_I64 if full else _native.CMP_PER_DIM | mask) | _native.CMP_UNSIGNED, conv, [None] * len(doms)

    def small_exact(k):
        d, common = doms[k]
        e = np.asarray(edges[k])
        return (d == _native.CMP_I64 and common is None and sample_dtypes[k].itemsize <= 4 and
                (e.size == 0 or (int(e.min()) >= -(1 << 53) and int(e.max()) <= (1 << 53))))
    if any(d == _native.CMP_I64 for d, _ in doms) and all(d == _native.CMP_F64 or small_exact(k) for k, (d, _) in enumerate(doms)):
        conv = [np.asarray(e).astype(np.float64) for e in edges]
        return _native.CMP_F64, conv, [None] * len(edges)
    kinds = {d for d, _ in doms}
    if len(kinds) > 1:
        # 64-bit integer / datetime inputs next to float ones (a time axis against a value axis):
        # every input keeps its own domain, as numpy digitizes every argument on its own
        mask = sum(1 << k for k, (d, _) in enumerate(doms) if d == _native.CMP_I64)
        return _native.CMP_PER_DIM | mask, conv, [c for _, c in doms]
    return doms[0][0], conv, [c for _, c in doms]


# ---------------------------------------------------------------------------------------------
# L1: the hot path                                                     (core.py:137-194)
# ---------------------------------------------------------------------------------------------
def _torch_contiguous(a):
    """C-contiguous copy of a GPU tensor: the library's strided-copy kernel (transposing layouts tiled through LDS, 3-5 TB/s
    moved) instead of torch's generic one (~0.5 TB/s for the same layouts); small tensors and dtypes without a tag go to torch"""
    if a.is_contiguous():
        return a
    if a.numel() < (1 << 16) or a.ndim > 8 or not a.is_cuda:
        return a.contiguous()
    try:
        tag = _torch_tag(a.dtype)
    except TypeError:
        return a.contiguous()
    torch = _torch()
    out = torch.empty(a.shape, dtype=a.dtype, device=a.device)
    item = a.element_size()
    dev = _torch_device_index(a.device)
    _native.copy_nd(dev, a.shape, a.data_ptr(), tag, [st * item for st in a.stride()], out.data_ptr(), tag,
                    [st * item for st in out.stride()], torch.cuda.current_stream(a.device).cuda_stream)
    return out


def _strided_view(a2d, backend):
    """(pointer, dtype tag, row stride, col stride, 0, 0, keepalive) of a 2-D array, in elements.
    Falls back to a contiguous copy only for layouts the C ABI does not take (negative strides;
    arrays strided in both directions)."""
    if backend == "torch":
        rs, cs = a2d.stride()
        # A large view strided in BOTH directions (e.g. a reduction over a middle axis) would make
        # every lane touch its own cache line; one copy on the device (the reference makes the
        # same copy on the host, core.py:219-226) and the coalesced kernels is far cheaper.
        # (row stride 1 = reductions over leading axes: the library's row-per-lane kernels take
        # those views as they are)
        if rs < 0 or cs < 0 or (cs > 1 and rs > 1 and a2d.shape[1] > 1 and a2d.numel() >= (1 << 16)):
            a2d = _torch_contiguous(a2d)
            rs, cs = a2d.stride()
        if a2d.shape[0] <= 1:
            rs = 0 if a2d.shape[0] == 0 else rs
        return a2d.data_ptr(), _torch_tag(a2d.dtype), rs, cs, 0, 0, a2d
    if backend == "device":
        item = a2d.itemsize
        if any(st < 0 or st % item for st in a2d.strides) or (
                a2d.strides[0] > item and a2d.strides[1] > item and a2d.shape[1] > 1 and a2d.size >= (1 << 16)):
            a2d = a2d.copy()  # (the same two cases as for torch tensors above)
        rs, cs = (st // item for st in a2d.strides)
        if a2d.shape[0] <= 1:
            rs = 0 if a2d.shape[0] == 0 else rs
        return a2d.ptr, _native.dtype_tag(np.dtype(np.int64) if a2d.dtype.kind in "mM" else a2d.dtype), rs, cs, 0, 0, a2d
    if a2d.dtype.kind in "mM":
        a2d = a2d.view(np.int64)
    item = a2d.dtype.itemsize
    rs, cs = (s // item for s in a2d.strides)
    ok = rs >= 0 and cs in (0, 1) and all(s % item == 0 for s in a2d.strides) and (rs == 0 or rs >= a2d.shape[1] * cs)
    if a2d.shape[1] <= 1 and rs >= 0 and a2d.strides[0] % item == 0:
        ok, cs = True, 1  # (a byte stride that is no multiple of the item size — a field of a packed record — is copied)
    if rs == 1 and cs >= a2d.shape[0] and all(s % item == 0 for s in a2d.strides):
        ok = True  # rows are the contiguous direction (leading-axis reduction): staged as it lies
    if not ok or not a2d.dtype.isnative:
        a2d = np.ascontiguousarray(a2d, dtype=a2d.dtype.newbyteorder("="))
        rs, cs = a2d.shape[1], 1
    return a2d.ctypes.data, _native.dtype_tag(a2d.dtype), rs, cs, 0, 0, a2d


def _execute_views(views, wview, nrows, ncols, sample_dtypes, bins, backend, like, block_size, wview2=None):
    """Hand [rows, cols] views (ptr, tag, row stride, col stride, rows per group, group stride,
    keepalive) to the native library and return the [rows, nb_0, ...] histogram.  With ``wview2``
    (a second weight view): a [2, rows, nb_0, ...] pair from one pass (histogram_two_weights)."""
    cmp_domain, edges, _ = _compare_domain(sample_dtypes, bins)
    weighted = wview is not None
    if backend == "numpy":
        device = _host_device()
        stream = 0
        mem = _native.MEM_HOST
    elif backend == "device":
        device = like.device
        stream = 0
        mem = _native.MEM_DEVICE
    else:
        torch = _torch()
        if like.device.type != "cuda":
            raise RuntimeError("torch inputs must live on an MI355X (device='cuda'); got %s" % like.device)
        device = _torch_device_index(like.device)
        stream = torch.cuda.current_stream(like.device).cuda_stream
        mem = _native.MEM_DEVICE
    _native.require_device(device)
    plan = _get_plan(edges, cmp_domain, device)

    # the library zero-initialises (overwrites) the output itself: no fill here, which for torch
    # would be one more kernel launch per call
    out_shape = ((2,) if wview2 is not None else ()) + (nrows,) + plan.bins_shape
    n_out = int(np.prod(out_shape, dtype=np.int64))
    device_partial = backend != "torch" and getattr(_tls, "device_out", False) and wview2 is None
    if n_out > 0 and (device_partial or backend == "device"):
        # a dask block under the device-resident reduction (multigpu.reduce_partials): only host inputs cross PCIe, the
        # partial histogram stays on its GPU.  (A DeviceArray block outside that reduction: downloaded below.)
        out_dtype = np.float64 if weighted else np.int64
        buf = _native.DeviceBuffer(device, n_out * 8)
        out = _native.DevicePartial(buf, out_shape, out_dtype)
        out_ptr = buf.ptr
        if backend == "numpy":
            mem = _native.MEM_HOST_TO_DEVICE
        empty = False
    elif backend != "torch":
        out = np.empty(out_shape, dtype=np.float64 if weighted else np.int64)
        out_ptr = out.ctypes.data
        empty = out.size == 0
    else:
        out = torch.empty(out_shape, dtype=torch.float64 if weighted else torch.int64, device=like.device)
        out_ptr = out.data_ptr()
        empty = out.numel() == 0
    if empty:
        return out

    grouped = any(v[4] for v in views) or (weighted and wview[4]) or (wview2 is not None and wview2[4])
    if block_size in (None, "auto") or grouped:
        row_blocks = [(0, nrows)]
    else:
        if not isinstance(block_size, (int, np.integer)) or isinstance(block_size, bool):
            raise AssertionError("block_size must be None, 'auto' or an int")  # core.py:116
        if block_size <= 0:
            raise ZeroDivisionError("block_size must be positive")  # core.py:117 raises the same
        row_blocks = [(r, min(r + int(block_size), nrows)) for r in _range(0, nrows, int(block_size))]

    def shifted(view, r0):
        ptr, tag, rs, cs, ir, os_, _keep = view
        return _native.make_view(ptr + r0 * rs * np.dtype(_TAG_NP[tag]).itemsize, tag, rs, cs, ir, os_)

    row_bytes = plan.n_bins * 8
    for r0, r1 in row_blocks:
        if wview2 is not None:
            plan.execute_two_weights(
                [shifted(v, r0) for v in views], shifted(wview, r0), shifted(wview2, r0), r1 - r0, ncols,
                out_ptr + r0 * row_bytes, out_ptr + (nrows + r0) * row_bytes, mem, accumulate=False, stream=stream,
            )
            continue
        plan.execute(
            [shifted(v, r0) for v in views],
            shifted(wview, r0) if weighted else None,
            r1 - r0,
            ncols,
            out_ptr + r0 * row_bytes,
            weighted,
            mem,
            accumulate=False,
            stream=stream,
        )
    if backend == "device" and not device_partial:
        return out.to_numpy()  # DeviceArray in, numpy histogram out (the result is small; the data never moved)
    return out


def _bincount_2d_vectorized(*args, bins=None, weights=None, density=False, right=False, block_size=None):
    """Histogram independently on each row of 2-D arrays — the fused GPU replacement of the
    reference function of the same name (core.py:137-194).

    ``args``: D arrays of equal shape [M, C] (numpy or torch-on-GPU, any strides); ``bins``: D 1-D
    edge arrays; ``weights``: None or [M, C].  Returns [M, nb_0, ..., nb_{D-1}]: int64 counts
    (unweighted) or float64 sums.  ``density`` and ``right`` are accepted and ignored, as in the
    reference (core.py:138).  ``block_size`` (None, "auto" or a positive int) only sets how many
    rows one kernel launch covers: the reference's row blocking (core.py:86-134) bounds numpy
    temporaries that do not exist here, and never changes the result.
    """
    a0 = args[0]
    backend = _backend_of(args)
    for a, b in zip(args, bins):  # core.py:146-151
        assert a.ndim == 2
        assert np.ndim(b) == 1
        assert tuple(a.shape) == tuple(a0.shape)
    if weights is not None:
        assert tuple(weights.shape) == tuple(a0.shape)
    if len(bins) != len(args):
        raise ValueError("one array of bin edges per input array")
    nrows, ncols = (int(s) for s in a0.shape)
    dtypes = [_np_dtype_of(a) for a in args]
    args, weights = _prepare_dtypes(list(args), weights, dtypes, bins, backend)
    views = [_strided_view(a, backend) for a in args]
    wview = _strided_view(weights, backend) if weights is not None else None
    return _execute_views(views, wview, nrows, ncols, dtypes, bins, backend, a0, block_size)


def _prepare_dtypes(args, weights, dtypes, bins, backend):
    """dtype-level preparation shared by every entry: datetime64 inputs are brought to the unit
    they share with their edges (and later viewed as int64), complex weights are rejected like
    numpy's bincount does"""
    if backend in ("numpy", "device"):
        _, _, common = _compare_domain(dtypes, bins)
        if backend == "device" and any(c is not None and a.dtype != c for a, c in zip(args, common)):
            raise TypeError("datetime64 DeviceArrays must already have the unit they share with their bin edges")
        args = [a.astype(c) if c is not None and a.dtype != c else a for a, c in zip(args, common)]
        if weights is not None and weights.dtype.kind == "c":
            raise TypeError("Cannot cast array data from complex to float64 (weights)")  # numpy bincount
    elif weights is not None and weights.dtype.is_complex:
        raise TypeError("complex weights are not supported")
    return args, weights


# ---------------------------------------------------------------------------------------------
# L2: block adapter                                                    (core.py:197-247)
# ---------------------------------------------------------------------------------------------
def _rows_cols(a, axis, do_full_array):
    """[M, C] arrangement of an N-D block: kept axes -> rows, reduced axes (in the order given)
    -> cols (core.py:211-227).  A view whenever the strides allow it — broadcast (stride-0)
    inputs and trailing reduced axes are NOT materialised, unlike the reference's reshape."""
    if _is_torch(a):
        if do_full_array:
            return a.reshape(1, -1)
        moved = a.movedim(tuple(axis), tuple(_range(-len(axis), 0)))
        keep = moved.shape[: moved.ndim - len(axis)]
        m = 1
        for k in keep:
            m *= int(k)
        c = (a.numel() // m) if m else 0
        item = a.element_size()
        if m and c and _nocopy_reshape_strides(tuple(moved.shape), tuple(st * item for st in moved.stride()), (m, c), item) is None:
            moved = _torch_contiguous(moved)  # the reshape needs a copy: ours
        return moved.reshape(m, c)  # (not -1: torch cannot infer the columns of a block without rows)
    if _is_devarr(a):
        if do_full_array:
            return a.reshape(1, -1)
        moved = a.moveaxis(tuple(axis), tuple(_range(-len(axis), 0)))
        m = int(np.prod(moved.shape[: moved.ndim - len(axis)], dtype=np.int64))
        return moved.reshape(m, (a.size // m) if m else 0)  # a view where the strides allow it, else one device copy
    if do_full_array:
        moved, m = a, 1
    else:
        moved = np.moveaxis(a, axis, tuple(_range(-len(axis), 0)))
        m = int(np.prod(moved.shape[: moved.ndim - len(axis)], dtype=np.int64))
    c = (a.size // m) if m else 0
    # (numpy's in-place `view.shape = ...` copies the data BEFORE it refuses a shape that needs a copy: ask the rule itself)
    if _nocopy_reshape_strides(moved.shape, moved.strides, (m, c), moved.itemsize) is None:
        return moved.reshape(m, c)
    v = moved.view()
    v.shape = (m, c)
    return v


def _elem_strides(a):
    """(shape, strides in elements) of a numpy array or torch tensor; None if not element-aligned"""
    if _is_torch(a):
        return tuple(int(s) for s in a.shape), tuple(int(s) for s in a.stride())
    item = a.dtype.itemsize
    if any(st % item for st in a.strides):
        return None
    return tuple(a.shape), tuple(st // item for st in a.strides)


def _merge_dims(dims):
    """merge consecutive (size, stride) dims that walk memory like one dim; size-1 dims vanish"""
    out = []
    for size, stride in dims:
        if size == 1:
            continue
        if out and (out[-1][1] == stride * size or (out[-1][1] == 0 and stride == 0)):
            out[-1] = (out[-1][0] * size, stride)
        else:
            out.append((size, stride))
    return out


def _collapse(a, axis, do_full_array, reduced_order):
    """Describe the [kept, reduced] arrangement of an N-D block (core.py:211-227) by strides
    instead of making it: (rows, cols, row stride, col stride, rows per group, group stride) or None.

    The reduced axes must walk memory as ONE strided dimension (their order inside a row does not
    matter to a histogram, so ``reduced_order`` — chosen once for all inputs — may permute them);
    the kept axes as one or two (kept axes on both sides of the reduced ones: grouped rows)."""
    ss = _elem_strides(a)
    if ss is None:
        return None
    shape, strides = ss
    if any(st < 0 for st in strides):
        return None
    ndim = len(shape)
    red = list(_range(ndim)) if do_full_array else list(reduced_order)
    kept = [] if do_full_array else [i for i in _range(ndim) if i not in red]
    cols = _merge_dims([(shape[i], strides[i]) for i in red])
    rows = _merge_dims([(shape[i], strides[i]) for i in kept])
    if len(cols) > 1 or len(rows) > 2:
        return None
    m = 1
    for i in kept:
        m *= shape[i]
    c = 1
    for i in red:
        c *= shape[i]
    cs = cols[0][1] if cols else 0
    if len(rows) == 2:
        (_, os_), (inner, rs) = rows
        return m, c, rs, cs, inner, os_
    rs = rows[0][1] if rows else 0
    return m, c, rs, cs, 0, 0


def _reduced_order(a, axis):
    """order of the reduced axes that walks ``a`` with decreasing strides (C-like)"""
    ss = _elem_strides(a)
    if ss is None:
        return list(axis)
    return sorted(axis, key=lambda i: -ss[1][i])


def _view_of(a, desc, backend, both_strided_limit=1 << 16):
    """native view tuple of an array described by _collapse, or None when a copy is the better plan"""
    m, c, rs, cs, ir, os_ = desc
    if backend == "torch":
        if rs > 1 and cs > 1 and m * c >= both_strided_limit:
            return None  # strided both ways: every lane would touch its own cache line
        return a.data_ptr(), _torch_tag(a.dtype), rs, cs, ir, os_, a
    if backend == "device":
        if rs > 1 and cs > 1 and m * c >= both_strided_limit:
            return None
        return a.ptr, _native.dtype_tag(np.dtype(np.int64) if a.dtype.kind in "mM" else a.dtype), rs, cs, ir, os_, a
    if not a.dtype.isnative:
        return None
    if a.dtype.kind in "mM":
        a = a.view(np.int64)
    # rows that overlap in memory (sliding windows: row stride below the row's extent) cannot be staged
    # as a pitched 2-D copy; the reference's reshape copies them, and so does the copying route here
    rows_side_by_side = ir if ir else m  # rows that follow each other at stride rs
    if m > 1 and c > 1 and rs != 0 and cs != 0 and ((cs == 1 and rs < c) or (rs == 1 and cs < rows_side_by_side)):
        return None
    if ir == 0 and not (cs in (0, 1) or rs in (0, 1)):
        ir, os_ = m, 0  # one group: makes the library stage the bytes as they lie, strides intact
    return a.ctypes.data, _native.dtype_tag(a.dtype), rs, cs, ir, os_, a


def _beyond_lds(bins, weighted):
    """the histogram is bigger than the LDS of the kernels that take any dtype / stride (uint32 or float64 counters)"""
    n_bins = 1
    for b in bins:
        n_bins *= max(len(b) - 1, 1)
    return n_bins * (8 if weighted else 4) > 144 * 1024


def _promote_for_big_histograms(arrays, w_array, dtypes, bins, backend="torch"):
    """Inputs whose dtype mixture only the generic kernel family takes (float32 next to float64,
    integers in a joint histogram, integer weights) AND whose histogram is beyond its LDS: that family then has
    memory-side atomics only (2 x 10^8 samples, 256 x 256 bins, float32 x float64: 24 ms).  Converting to float64 on
    the device is exact wherever the comparison runs in float64 anyway (numpy promotes the same way inside
    searchsorted, and bincount casts weights to double) and opens the packed / sliced / partitioned modes of the vector
    kernels (1.1 ms).  Small histograms stay as they are: the conversion pass would cost more than it saves."""
    weighted = w_array is not None
    if not _beyond_lds(bins, weighted):
        return arrays, w_array, dtypes
    torch = _torch() if backend == "torch" else None
    fast_floats = (np.dtype(np.float32), np.dtype(np.float64))
    d = len(arrays)
    vector_ok = all(dt == dtypes[0] for dt in dtypes) and dtypes[0] in fast_floats and d <= 3
    w_ok = (not weighted) or _np_dtype_of(w_array) in fast_floats
    if vector_ok and w_ok:
        return arrays, w_array, dtypes
    try:
        cmp_domain, _, _ = _compare_domain(dtypes, bins)
    except (TypeError, NotImplementedError, AssertionError):
        return arrays, w_array, dtypes  # let the regular path raise what it raises
    if cmp_domain != _native.CMP_F64 or d > 3:
        return arrays, w_array, dtypes  # exact int64 / datetime comparisons stay exact
    if backend in ("numpy", "device"):
        # host inputs: the conversion is a host pass (numpy), still far cheaper than ~2.5 x 10^10 atomics per second;
        # DeviceArrays: one strided-copy kernel with the conversion in it (DeviceArray.astype)
        if not vector_ok:
            arrays = [a if a.dtype == np.float64 else a.astype(np.float64) for a in arrays]
            dtypes = [np.dtype(np.float64)] * d
        if weighted and not w_ok:
            w_array = w_array.astype(np.float64)
        return arrays, w_array, dtypes
    if not vector_ok:
        arrays = [a if a.dtype == torch.float64 else a.to(torch.float64) for a in arrays]
        dtypes = [np.dtype(np.float64)] * d
    if weighted and not w_ok:
        w_array = w_array.to(torch.float64)
    return arrays, w_array, dtypes


def _block_placement(all_arrays, multigpu):
    """where one dask block runs: on the GPU its chunks already live on (DeviceArray chunks), else on the least busy one"""
    resident = next((a for a in all_arrays if _is_devarr(a)), None)
    return multigpu.block_device() if resident is None else multigpu.on_device(resident.device)


def _bincount_spread(*all_arrays, **kwargs):
    """One dask block (core.py:429-437): the block adapter on whichever of the node's GPUs has the fewest
    blocks in flight — dask's threaded scheduler runs many blocks at once, and each one is staged over
    its own GPU's PCIe link and binned there (multigpu.block_device)."""
    from . import multigpu

    with _block_placement(all_arrays, multigpu):
        return _bincount(*all_arrays, **kwargs)


def _bincount_partial(*all_arrays, **kwargs):
    """One dask block under the device-resident reduction: as _bincount_spread, but the result is a
    _native.DevicePartial on the block's GPU (only the inputs cross PCIe)."""
    from . import multigpu

    with _block_placement(all_arrays, multigpu):
        prev = getattr(_tls, "device_out", False)
        _tls.device_out = True
        try:
            return _bincount(*all_arrays, **kwargs)
        finally:
            _tls.device_out = prev


def _bincount(*all_arrays, weights=False, axis=None, bins=None, density=None, block_size=None):
    """Block adapter with the reference's contract AND signature (core.py:197-247): N-D block(s) in,
    array of shape kept-axes (1 for each reduced axis) + bin dims out.  Called directly for
    numpy/torch inputs and once per block by the dask branch (core.py:429-437).

    Where the reference moves the reduced axes last and reshapes (a copy for anything but
    trailing axes), the block is DESCRIBED to the native library as a strided [rows, cols] view —
    broadcast inputs, leading-axis and middle-axis reductions included — and only layouts no
    three strides can express fall back to that copy."""
    return _block_adapter(all_arrays, weights, axis, bins, density, block_size, False)


def _bincount_two_weights(*all_arrays, weights=False, axis=None, bins=None, density=None, block_size=None):
    """`_bincount` for histogram_two_weights (an extension, private): the LAST TWO of `all_arrays` are weight
    arrays, the result carries a leading pair axis."""
    return _block_adapter(all_arrays, weights, axis, bins, density, block_size, True)


def _block_adapter(all_arrays, weights, axis, bins, density, block_size, second_weights):
    backend = _backend_of(all_arrays)
    if backend == "device":
        # a dask block: chunks that live on a GPU next to host chunks (weights from a numpy-backed dask array) — the
        # host ones follow the resident ones to their GPU
        dev = next(a.device for a in all_arrays if _is_devarr(a))
        all_arrays = [a.to(dev) if _is_devarr(a) else DeviceArray.from_numpy(a, dev) for a in all_arrays]
    a0 = all_arrays[0]
    ndim = a0.ndim
    do_full_array = (axis is None) or (set(axis) == set(_range(ndim)))
    if do_full_array:
        kept_axes_shape = (1,) * ndim
    else:
        kept_axes_shape = tuple(int(a0.shape[i]) if i not in axis else 1 for i in _range(ndim))

    arrays = list(all_arrays)
    w2_array = arrays.pop() if second_weights else None  # histogram_two_weights (extension)
    w_array = arrays.pop() if weights else None
    n_inputs = len(arrays)
    dtypes = [_np_dtype_of(a) for a in arrays]
    arrays, w_array = _prepare_dtypes(arrays, w_array, dtypes, bins, backend)
    if second_weights and (w2_array.dtype.is_complex if backend == "torch" else w2_array.dtype.kind == "c"):
        raise TypeError("complex weights are not supported")
    if all(dt.kind in "fiub" for dt in dtypes) and (w_array is None or _np_dtype_of(w_array).kind in "fiub"):
        arrays, w_array, dtypes = _promote_for_big_histograms(arrays, w_array, dtypes, bins, backend)
    w_list = ([w_array] if weights else []) + ([w2_array] if second_weights else [])

    counts = None
    order = _reduced_order(arrays[0], list(_range(ndim)) if do_full_array else axis)
    descs = [_collapse(a, axis, do_full_array, order) for a in arrays + w_list]
    if backend != "numpy" and _beyond_lds(bins, weights) and any(d is not None and d[1] > 1 and d[3] != 1 for d in descs):
        # columns that are not unit-stride (strided or broadcast views, leading-axis reductions) go to kernels that
        # keep their histogram in LDS or, beyond it, in memory-side atomics: for a big histogram the reference's
        # copy into [rows, cols] blocks (core.py:211-229), made on the device, is far cheaper than those atomics
        descs = [None]
    if all(d is not None for d in descs) and len({d[:2] for d in descs}) == 1:
        views = [_view_of(a, d, backend) for a, d in zip(arrays + w_list, descs)]
        if all(v is not None for v in views):
            m, c = descs[0][:2]
            try:
                counts = _execute_views(views[:n_inputs], views[n_inputs] if weights else None, int(m), int(c), dtypes, bins,
                                        backend, a0, block_size, wview2=views[n_inputs + 1] if second_weights else None)
            except NotImplementedError:
                counts = None  # e.g. a host view spanning > 2^32 elements: take the copying route
    if counts is None:
        blocks = [_rows_cols(a, axis, do_full_array) for a in arrays + w_list]
        if second_weights:  # the copying route: two passes
            pair = [_bincount_2d_vectorized(*blocks[:n_inputs], bins=bins, weights=wb, block_size=block_size) for wb in blocks[n_inputs:]]
            counts = _torch().stack(pair) if backend == "torch" else np.stack(pair)
        else:
            weights_block = blocks.pop() if weights else None
            counts = _bincount_2d_vectorized(*blocks, bins=bins, weights=weights_block, density=density, block_size=block_size)
    if second_weights:
        return counts.reshape((2,) + kept_axes_shape + tuple(counts.shape[2:]))
    return counts.reshape(kept_axes_shape + tuple(counts.shape[1:]))


# ---------------------------------------------------------------------------------------------
# L3: public API                                                       (core.py:250-466)
# ---------------------------------------------------------------------------------------------
def _ensure_correctly_formatted_bins(bins, N_expected):
    """One bin specification per input array (the reference helper of the same name, core.py:37-48):
    a single int / estimator name / edge array serves every input; a sequence must have one entry
    per input."""
    if bins is None:
        raise ValueError("bins must be provided")
    shared = isinstance(bins, (int, str, np.ndarray))
    per_input = [bins] * N_expected if shared else bins
    if len(per_input) != N_expected:
        raise ValueError("The number of bin definitions doesn't match the number of args")
    return per_input


def _ensure_correctly_formatted_range(range_, N_expected):
    """One (lower, upper) pair — or None — per input array (core.py:51-70): a single pair serves every
    input; a sequence of pairs must have one per input."""
    if range_ is None:
        return [None] * N_expected
    entries_are_sequences = [isinstance(entry, Iterable) for entry in range_]
    if len(range_) == 2 and not all(entries_are_sequences):
        return [range_] * N_expected  # one (lower, upper) pair for all
    if len(range_) != N_expected:
        raise ValueError("The number of ranges doesn't match the number of args")
    if any(len(pair) != 2 for pair in range_):
        raise ValueError(
            "range should be provided as (lower_range, upper_range). In the "
            "case of multiple args, range should be a list of such tuples"
        )
    return range_


def _devarr_as_torch(a):
    """zero-copy torch view of a DeviceArray (the array keeps owning the memory), or None: no torch in this interpreter, no
    GPU visible to it, or a dtype / stride pattern torch's `__cuda_array_interface__` import does not take"""
    try:
        torch = _torch()
        if not torch.cuda.is_available() or a.dtype.kind not in "fiu" or a.dtype == np.float16:
            return None
        return torch.as_tensor(a, device=torch.device("cuda", _native.physical_device(a.device)))
    except Exception:
        return None


def _device_bin_edges(a, b, r, has_weights):
    """np.histogram_bin_edges (core.py:383-388) for a GPU-resident array without moving it:
    explicit edges are validated by numpy; an integer ``bins`` needs only the data's min/max
    (reduced on the GPU, NaN-propagating like numpy) and its dtype; string estimators need the
    data itself and take the slow path through host memory."""
    proto_dtype = _np_dtype_of(a)
    resident = _is_devarr(a)
    if isinstance(b, str):
        if has_weights:
            raise TypeError("Automated estimation of the number of bins is not supported for weighted data")
        edges = _device_estimator_edges(a, b, r, proto_dtype, resident)
        if edges is None:
            edges = _device_quartile_edges(a, b, r, proto_dtype, resident)
        if edges is None:
            edges = _device_doane_stone_edges(a, b, r, proto_dtype, resident)
        if edges is None and resident:
            # a DeviceArray where torch is importable: the order-statistics search and the "doane" / "stone" selectors run on
            # a zero-copy torch view of the same memory (`__cuda_array_interface__`); without torch (the dask interpreter of
            # this image) the host copy below remains
            t = _devarr_as_torch(a)
            if t is not None:
                edges = _device_quartile_edges(t, b, r, proto_dtype, False)
                if edges is None:
                    edges = _device_doane_stone_edges(t, b, r, proto_dtype, False)
                del t
        if edges is not None:
            return edges
        # what is left — a DeviceArray without torch, float16 data, "stone" of more than 1.6 x 10^7 elements, a bin
        # count that hangs on numpy's own summation order ("scott", "doane") — takes numpy's implementation on a host copy
        return np.histogram_bin_edges(a.to_numpy() if resident else a.detach().cpu().numpy(), bins=b, range=r)
    if np.ndim(b) == 0 and r is None:
        if (a.size if resident else a.numel()) == 0:
            return np.histogram_bin_edges(np.zeros(0, proto_dtype), bins=b, range=None)
        flat = a.reshape(1, -1)
        ptr, tag, rs, cs, _ir, _os, keep = _strided_view(flat, "device" if resident else "torch")
        if resident:
            dev, stream = a.device, 0
        else:
            torch = _torch()
            dev = _torch_device_index(a.device)
            stream = torch.cuda.current_stream(a.device).cuda_stream
        lo, hi = _native.minmax(_native.make_view(ptr, tag, rs, cs), 1, flat.shape[1], _native.MEM_DEVICE, dev, stream)
        return np.histogram_bin_edges(np.array([lo, hi]).astype(proto_dtype), bins=b, range=None)
    return np.histogram_bin_edges(np.zeros(0, proto_dtype), bins=b, range=r)


ESTIMATORS_FROM_MOMENTS = ("sqrt", "sturges", "rice", "scott")
ESTIMATORS_FROM_QUARTILES = ("fd", "auto")  # float32 / float64 torch tensors: _device_quartile_edges


def _range_cut(r, proto_dtype):
    """the (lo, hi) the data is cut to before a bin-width selector sees it, as numpy's `keep` mask compares: an empty range
    is widened by half a unit each way first (_get_outer_edges), and float32 data meets the bounds ROUNDED TO float32 —
    numpy compares a float32 array with a Python float in float32 (NEP 50 weak scalars), so an element equal to
    float32(lo) < lo is kept (data clipped to 0.7 with range=(0.7, 1.0): 8 bins, not 1)"""
    lo, hi = (float(r[0]) - 0.5, float(r[1]) + 0.5) if r[0] == r[1] else (float(r[0]), float(r[1]))
    if proto_dtype == np.float32:
        # ... per bound, and only where numpy's promotion stays in float32: Python scalars (weak) and NumPy scalars no wider
        # than float32; an np.float64 / np.int64 bound makes numpy compare in float64, so it is kept as given (ADVICE r4:
        # range=(np.float64(0.7), 1.0) on data clipped to float32(0.7) keeps 322 of 1000 elements, not all of them)
        def narrow(bound, value):
            strong = isinstance(bound, np.generic)  # (np.float64 is a Python float as well: ask numpy first)
            if strong and np.result_type(np.float32, bound.dtype) != np.float32:
                return value
            with np.errstate(over="ignore"):
                return float(np.float32(value))

        lo, hi = narrow(r[0], lo), narrow(r[1], hi)
    return lo, hi


def _estimator_cut(name, r, proto_dtype):
    """(supported, lo_hi): whether `name` is one of the estimators that need only moments of data of this dtype, and the
    range the data is cut to before the selector sees it (None: all of it).  numpy validates the range (its own errors)."""
    if name not in ESTIMATORS_FROM_MOMENTS or proto_dtype.kind not in "fiu" or proto_dtype == np.float16:
        return False, None
    if r is None:
        return True, None
    if np.ndim(r[0]) or np.ndim(r[1]):
        return False, None
    np.histogram_bin_edges(np.zeros(0, proto_dtype), bins=1, range=r)
    return True, _range_cut(r, proto_dtype)


def _device_moments(a, lo_hi, want_m2):
    """(n, min, max, mean, M2) of the elements of a GPU-resident array inside lo_hi (all of them for None): xhist_moments"""
    resident = _is_devarr(a)
    if (a.size if resident else a.numel()) == 0:
        return 0, np.inf, -np.inf, np.nan, np.nan
    flat = a.reshape(1, -1)
    ptr, tag, rs, cs, _ir, _os, keep = _strided_view(flat, "device" if resident else "torch")
    if resident:
        dev, stream = a.device, 0
    else:
        dev = _torch_device_index(a.device)
        stream = _torch().cuda.current_stream(a.device).cuda_stream
    out = _native.moments(_native.make_view(ptr, tag, rs, cs), 1, flat.shape[1], lo_hi[0] if lo_hi else None,
                          lo_hi[1] if lo_hi else None, want_m2, dev, stream)
    del keep
    return out


def combine_moments(parts):
    """moments of the union of disjoint shards from the shards' own (n, min, max, mean, M2) — Chan et al.'s pairwise update"""
    n, mn, mx, mean, m2 = 0, np.inf, -np.inf, 0.0, 0.0
    for pn, pmn, pmx, pmean, pm2 in parts:
        if pn == 0:
            continue
        if pmn != pmn or pmx != pmx:  # a NaN among the kept elements: numpy rejects the range
            mn = mx = np.nan
        tot = n + pn
        d = pmean - mean
        m2 = m2 + (0.0 if pm2 != pm2 else pm2) + d * d * n * pn / tot
        mean = mean + d * pn / tot
        if mn == mn:
            mn, mx = min(mn, pmn), max(mx, pmx)
        n = tot
    return n, mn, mx, (mean if n else np.nan), (m2 if n else np.nan)


def _edges_from_moments(name, r, proto_dtype, size, moments, iqr=None, width_of=None):
    """np.histogram_bin_edges(a, bins=name, range=r) from the moments of the cut data — numpy's `_get_bin_edges` for a string
    `bins` restated (numpy/lib/_histograms_impl.py): outer edges from `range` or the data's min / max (NaN -> numpy's
    ValueError), width from the selector, n = ceil((last - first) / width), and numpy's own linspace for the edges —
    bit-identical to numpy whenever n is.  n depends on the data only through exact quantities, except for "scott", whose
    standard deviation is summed in another order than np.std does: when (last - first) / width lies within 1e-6 of an
    integer, or the data are (nearly) constant, the answer is None and numpy decides on a host copy."""
    if size == 0:
        return np.histogram_bin_edges(np.zeros(0, proto_dtype), bins=name, range=r)
    n, mn, mx, mean, m2 = moments
    as_scalar = proto_dtype.type
    if r is None:
        # (first, last) = (a.min(), a.max()) as numpy scalars of the data's dtype; non-finite -> numpy's ValueError
        np.histogram_bin_edges(np.array([mn, mx]).astype(proto_dtype), bins=1, range=None)
        outer = (as_scalar(mn), as_scalar(mx))
    else:
        outer = (r[0], r[1])  # as the caller gave them: numpy computes with their types (python floats are "weak")
    first, last = outer
    if first == last:  # numpy/lib/_histograms_impl.py::_get_outer_edges
        first, last = first - 0.5, last + 0.5
    if n == 0:
        n_bins = 1
    else:
        if proto_dtype.kind == "f":
            ptp = as_scalar(mx) - as_scalar(mn)  # numpy's _ptp: in the data's own precision
        else:
            ptp = int(mx) - int(mn)
        if name == "sqrt":
            width = ptp / np.sqrt(n)
        elif name == "sturges":
            width = ptp / (np.log2(n) + 1.0)
        elif name == "rice":
            width = ptp / (2.0 * n ** (1.0 / 3))
        elif width_of is not None:  # "doane" / "stone": the caller's selector, given numpy's _ptp of the data
            width = width_of(ptp)
            if width is None:
                return None
        elif name in ESTIMATORS_FROM_QUARTILES:
            width = 2.0 * iqr * n ** (-1.0 / 3.0)  # _hist_bin_fd
            if name == "auto":  # _hist_bin_auto: the smaller of "fd" and "sturges" — "sturges" alone where the quartiles coincide
                sturges = ptp / (np.log2(n) + 1.0)
                width = min(width, sturges) if width else sturges
        else:
            std = np.sqrt(m2 / n)
            if not std > 1e-5 * max(abs(mx), abs(mn)):
                # (nearly) constant data: np.std's own rounding — the mean of equal float32 values is not always that value —
                # decides between one bin and "too many bins"; only numpy's summation order reproduces numpy there
                return None
            if proto_dtype == np.float32:
                std = np.float32(std)  # np.std of float32 data is a float32
            width = (24.0 * np.pi ** 0.5 / n) ** (1.0 / 3.0) * std
        if width:
            clamped = proto_dtype.kind in "iub" and width < 1
            if clamped:
                width = 1
            if np.result_type(first, last).kind in "iub":
                span = int(last) - int(first)  # numpy's _unsigned_subtract: exact for integers
            else:
                span = last - first
            q = span / width
            if not np.isfinite(q):
                return None
            if name == "scott" and not clamped and abs(q - np.rint(q)) <= 1e-6 * max(1.0, abs(q)):
                return None  # a tie at the ceil: np.std's own summation order decides
            if name == "doane" and not clamped and abs(q - np.rint(q)) <= 1e-5 * max(1.0, abs(q)):
                return None  # (likewise: numpy's mean / std / third moment in the data's own precision and order)
            n_bins = int(np.ceil(q))
        else:
            n_bins = 1
    return np.histogram_bin_edges(np.zeros(0, proto_dtype), bins=n_bins, range=outer)


def _device_order_statistics(flat, ranks, mn, mx, n):
    """The elements of a 1-D float GPU tensor (no NaNs; min `mn`, max `mx`, `n` elements) at the given 0-based positions of
    its sorted order, exactly, without sorting or copying it: the interval that holds a rank is narrowed by histograms
    of 32768 bins — this library's own streaming pass, 1.2 ms per 10^9 float64 — until it holds at most 65536
    elements, which are then fetched (a boolean mask on the device, a few KB to the host) and sorted there.
    {rank: value} or None (more than 8 passes: leave it to numpy)."""
    torch = _torch()
    B, small = 1 << 15, 1 << 16
    is32 = flat.dtype == torch.float32
    is_int = not flat.dtype.is_floating_point

    def bounds32(lo, top):  # lo <= x <= top for float32 x, decided exactly by float32 scalars
        lo32, top32 = np.float32(lo), np.float32(top)
        if float(lo32) < lo:
            lo32 = np.nextafter(lo32, np.float32(np.inf))
        if float(top32) > top:
            top32 = np.nextafter(top32, np.float32(-np.inf))
        return float(lo32), float(top32)

    out = {}
    first_pass = None
    for rank in sorted(set(int(r) for r in ranks)):
        lo, top, k = float(mn), float(mx), rank  # the interval [lo, top] holds the element; k = its position among the interval's
        found = None
        for step in _range(8):
            if lo == top:
                found = lo
                break
            edges = np.unique(np.linspace(lo, top, B + 1))
            if len(edges) < 2:
                found = lo
                break
            if step == 0 and first_pass is not None:
                counts = first_pass
            else:
                counts = histogram(flat, bins=edges)[0].cpu().numpy()
                if step == 0:
                    first_pass = counts
            cum = np.cumsum(counts)
            if int(cum[-1]) <= k:
                return None  # (the interval does not hold what the bookkeeping says: never observed; numpy decides)
            j = int(np.searchsorted(cum, k, side="right"))
            k -= int(cum[j - 1]) if j else 0
            lo = float(edges[j])
            top = float(edges[j + 1]) if j + 1 == len(edges) - 1 else float(np.nextafter(edges[j + 1], -np.inf))  # bins are [e_j, e_j+1), the last one closed
            if int(counts[j]) <= small:
                l, t = bounds32(lo, top) if is32 else ((int(np.ceil(lo)), int(np.floor(top))) if is_int else (lo, top))
                vals = np.sort(flat[(flat >= l) & (flat <= t)].cpu().numpy())
                if len(vals) != int(counts[j]):
                    return None
                found = float(vals[k])
                break
        if found is None:
            return None
        out[rank] = found
    return out


def _device_quartile_edges(a, name, r, proto_dtype, resident):
    """np.histogram_bin_edges(a, bins="fd" | "auto", range=r) for a float or integer GPU tensor without a host copy:
    numpy's selectors (numpy/lib/_histograms_impl.py: _hist_bin_fd, _hist_bin_auto) need the data only through its size,
    min, max and the two quartiles, and np.percentile's default method needs four order statistics for those — found
    exactly by _device_order_statistics — and its own interpolation (numpy/lib/_function_base_impl.py: _lerp), restated here
    with numpy's dtypes.  With a range the selector sees the data cut to it.  None: not that case (other estimator, dtype,
    a DeviceArray)."""
    if name not in ESTIMATORS_FROM_QUARTILES or resident or proto_dtype.kind not in "fiu" or proto_dtype == np.float16:
        return None
    size = a.numel()
    if size == 0:
        return np.histogram_bin_edges(np.zeros(0, proto_dtype), bins=name, range=r)
    lo_hi = None
    if r is not None:  # the selector sees the data cut to the range (numpy validates it: its own errors)
        if np.ndim(r[0]) or np.ndim(r[1]):
            return None
        np.histogram_bin_edges(np.zeros(0, proto_dtype), bins=1, range=r)
        lo_hi = _range_cut(r, proto_dtype)
    n, mn, mx, _, _ = _device_moments(a, lo_hi, False)
    n = int(n)
    if n == 0:
        return _edges_from_moments(name, r, proto_dtype, size, (0, mn, mx, np.nan, np.nan), iqr=0.0)
    if not (np.isfinite(mn) and np.isfinite(mx)):
        if r is None:
            np.histogram_bin_edges(np.array([mn, mx]).astype(proto_dtype), bins=1, range=None)  # numpy's ValueError
        return None
    if proto_dtype.kind in "iu" and max(abs(mn), abs(mx)) >= 2.0 ** 53:
        return None  # (integers the float64 edges of the search cannot tell apart)
    q = np.true_divide([75, 25], 100)
    virtual = (n - 1) * q
    previous = np.floor(virtual).astype(np.intp)
    nxt = previous + 1
    above = virtual >= n - 1
    previous[above] = n - 1
    nxt[above] = n - 1
    stats = _device_order_statistics(a.reshape(-1), list(previous) + list(nxt), mn, mx, n)
    if stats is None:
        return None
    lower = np.array([stats[int(i)] for i in previous]).astype(proto_dtype)
    upper = np.array([stats[int(i)] for i in nxt]).astype(proto_dtype)
    gamma = np.asanyarray(virtual - previous, dtype=virtual.dtype)
    diff = np.subtract(upper, lower)
    lerp = np.asanyarray(np.add(lower, diff * gamma))
    np.subtract(upper, diff * (1 - gamma), out=lerp, where=gamma >= 0.5, casting="unsafe", dtype=type(lerp.dtype))
    iqr = np.subtract(*lerp)
    return _edges_from_moments(name, r, proto_dtype, size, (n, mn, mx, np.nan, np.nan), iqr=iqr)


def _device_doane_stone_edges(a, name, r, proto_dtype, resident):
    """np.histogram_bin_edges(a, bins="doane" | "stone", range=r) for a float or integer GPU tensor without a host copy
    (numpy/lib/_histograms_impl.py: _hist_bin_doane, _hist_bin_stone).
    "doane" needs the skewness: mean, standard deviation and third moment are reduced on the device in float64; numpy sums
    them in the data's own precision and order, so a bin count that hangs on the last digits (or nearly constant data) is
    left to numpy, as for "scott".
    "stone" minimises a loss over 1 ... max(100, sqrt(n)) bin counts, each needing the histogram of that many uniform bins:
    those are this library's own kernels — exact counts, hence numpy's very numbers — for up to 4000 candidates
    (n <= 1.6 x 10^7; numpy itself needs n / 4 seconds there)."""
    if name not in ("doane", "stone") or resident or proto_dtype.kind not in "fiu" or proto_dtype == np.float16:
        return None
    size = a.numel()
    if size == 0:
        return np.histogram_bin_edges(np.zeros(0, proto_dtype), bins=name, range=r)
    lo_hi = None
    if r is not None:  # the selector sees the data cut to the range (numpy validates it: its own errors)
        if np.ndim(r[0]) or np.ndim(r[1]):
            return None
        np.histogram_bin_edges(np.zeros(0, proto_dtype), bins=1, range=r)
        lo_hi = _range_cut(r, proto_dtype)
    n, mn, mx, _, _ = _device_moments(a, lo_hi, False)
    n = int(n)
    if n == 0:
        return _edges_from_moments(name, r, proto_dtype, size, (0, mn, mx, np.nan, np.nan), width_of=lambda ptp: 0.0)
    if not (np.isfinite(mn) and np.isfinite(mx)):
        if r is None:
            np.histogram_bin_edges(np.array([mn, mx]).astype(proto_dtype), bins=1, range=None)  # numpy's ValueError
        return None
    if proto_dtype.kind in "iu" and max(abs(mn), abs(mx)) >= 2.0 ** 53:
        return None
    torch = _torch()
    flat = a.reshape(-1)
    if name == "doane":
        def width_of(ptp):
            if n <= 2:
                return 0.0
            sg1 = np.sqrt(6.0 * (n - 2) / ((n + 1.0) * (n + 3)))
            # (float64 temporaries of the whole array live on the GPU here — several times a float32 input; a device that
            # cannot hold them hands the case to numpy on a host copy instead of failing: ADVICE r3)
            try:
                xd = flat.to(torch.float64)
                if lo_hi is not None:
                    xd = xd[(xd >= lo_hi[0]) & (xd <= lo_hi[1])]
                mean = xd.mean()
                xd = xd - mean  # (a tensor of our own from here on — `flat.to` may have returned the caller's — so the division below is in place)
                sigma = float(torch.sqrt((xd ** 2).mean()))
                if not sigma > 1e-5 * max(abs(mx), abs(mn)):
                    return None if sigma > 0.0 or mx != mn else 0.0  # exactly constant data: numpy's 0.0 as well
                xd /= sigma
                g1 = float((xd ** 3).mean())
            except torch.cuda.OutOfMemoryError:
                return None
            return ptp / (1.0 + np.log2(n) + np.log2(1.0 + np.absolute(g1) / sg1))
    else:
        upper = max(100, int(np.sqrt(n)))
        if upper > 4000:
            return None
        as_scalar = proto_dtype.type
        first, last = (as_scalar(mn), as_scalar(mx)) if r is None else (r[0], r[1])  # (numpy hands the selector the OUTER edges)
        if first == last:
            first, last = first - 0.5, last + 0.5

        def width_of(ptp):
            if n <= 1 or ptp == 0:
                return 0

            def jhat(nbins):
                hh = ptp / nbins
                edges = np.histogram_bin_edges(np.zeros(0, proto_dtype), bins=nbins, range=(first, last))
                p_k = histogram(flat, bins=edges)[0].cpu().numpy() / n
                return (2 - (n + 1) * p_k.dot(p_k)) / hh

            nbins = min(_range(1, upper + 1), key=jhat)
            if nbins == upper:
                warnings.warn("The number of bins estimated may be suboptimal.", RuntimeWarning, stacklevel=3)
            return ptp / nbins
    return _edges_from_moments(name, r, proto_dtype, size, (n, mn, mx, np.nan, np.nan), width_of=width_of)


def _device_estimator_edges(a, name, r, proto_dtype, resident):
    """np.histogram_bin_edges(a, bins=name, range=r) for the estimators that need only n, min, max and the standard deviation
    of the data — "sqrt", "sturges", "rice", "scott" — from ONE fused reduction on the GPU (xhist_moments; "scott": two
    passes) instead of a host copy of the array (core.py:383-388).  None: another estimator / dtype, or a case only numpy's
    own summation order decides (_edges_from_moments) — the caller then lets numpy work on a host copy."""
    ok, lo_hi = _estimator_cut(name, r, proto_dtype)
    if not ok:
        return None
    size = a.size if resident else a.numel()
    moments = _device_moments(a, lo_hi, name == "scott") if size else None
    if moments is not None and proto_dtype.kind in "iu" and proto_dtype.itemsize == 8 and int(moments[0]) > 0:
        # the reduction reads every element as float64: 64-bit integers of magnitude 2^53 and more would come back rounded,
        # where numpy's min / max / ptp are exact integer arithmetic — numpy on a host copy decides those
        if not (abs(moments[1]) < 2.0 ** 53 and abs(moments[2]) < 2.0 ** 53):
            return None
    return _edges_from_moments(name, r, proto_dtype, size, moments)


def _density(counts, bins, n_inputs):
    """core.py:444-462.  bin areas are the outer product of the bin widths; the reference's
    ``np.prod(np.ix_(...))`` for three or more inputs (core.py:454) fails on numpy >= 1.24, the
    outer product is what it was meant to compute (and what np.histogramdd does)."""
    widths = [np.diff(b) for b in bins]
    bin_axes = tuple(_range(-n_inputs, 0))
    if _is_torch(counts):
        # the outer product is formed on the device (same float64 products): only the widths travel,
        # and only once per set of edges (a host-to-device copy per call costs more than the epilogue)
        torch = _torch()
        key = (str(counts.device),) + tuple(np.asarray(w, dtype=np.float64).tobytes() for w in widths)
        with _plans_lock:
            areas_t = _areas.get(key)
            if areas_t is not None:
                _areas.move_to_end(key)
        if areas_t is None:
            for w in widths:
                wt = torch.as_tensor(np.asarray(w, dtype=np.float64), device=counts.device)
                areas_t = wt if areas_t is None else areas_t[..., None] * wt
            with _plans_lock:
                _areas[key] = areas_t
                while len(_areas) > 8:
                    _areas.popitem(last=False)
        sums = counts.sum(dim=bin_axes, keepdim=True)
        return counts / areas_t / sums
    areas = widths[0]
    for w in widths[1:]:
        areas = np.multiply.outer(areas, w)
    if _is_dask(counts):
        sums = counts.sum(axis=bin_axes)
        return counts / areas / sums.reshape(sums.shape + n_inputs * (1,))
    sums = counts.sum(axis=bin_axes)
    with np.errstate(divide="ignore", invalid="ignore"):
        return counts / areas / np.reshape(sums, sums.shape + n_inputs * (1,))


def _reduce_in_two_steps(all_arrays, has_weights, drop_axes, bins, block_size, backend):
    """Reduced axes that are NOT adjacent (``axis=(0, 2)`` of a 3-D array) cannot be walked as one strided
    dimension, and the reference's moveaxis + reshape copies everything (core.py:218-226).  Histograms
    add up, so: histogram over the last block of adjacent reduced axes (no copy), then sum the — much
    smaller — result over the remaining reduced axes.  int64 counts stay exact.  None when the reduced
    axes are one block anyway, or the intermediate would not be small next to the data."""
    axes = sorted(int(a) for a in drop_axes)
    if len(axes) < 2 or axes[-1] - axes[0] + 1 == len(axes):
        return None
    last = [axes[-1]]
    while last[0] - 1 in axes:
        last.insert(0, last[0] - 1)
    rest = [a for a in axes if a not in last]
    shape = tuple(int(n) for n in all_arrays[0].shape)
    n_bins = 1
    for b in bins:
        n_bins *= max(len(b) - 1, 0)
    cols = 1
    for ax in last:
        cols *= shape[ax]
    n_in = len(all_arrays) - (1 if has_weights else 0)
    itemsize = sum(_np_dtype_of(a).itemsize for a in all_arrays[:n_in])
    if n_bins * 8 * 4 > cols * itemsize:
        return None
    part = _bincount(*all_arrays, weights=has_weights, axis=last, bins=bins, density=False, block_size=block_size)
    if backend == "torch":
        return part.sum(dim=rest, keepdim=True)
    return part.sum(axis=tuple(rest), keepdims=True)


def _weights_slab(args_b, w_raw, drop_axes, bins, block_size, backend):
    """Device-resident data with weights that vary only along reduced axes and are small next to the data —
    ``cos(lat)`` of shape (1, lat, 1) or cell areas (1, lat, lon) against (time, lat, lon): the reference
    materialises them at full size (``broadcast_arrays`` + reshape, core.py:366 / 211-229), a second array
    as big as the data.  Here only the SLAB they really span — the run of adjacent reduced axes from the
    first axis they vary along to the innermost reduced axis next to it — is written out ((lat, lon): 4 MB
    against 1.5 GB) and handed to the weighted kernels with stride 0 along every other axis; reduced axes
    outside the slab are summed afterwards (histograms add up).  (365, 720, 1440) float32, cos(lat), over
    (lat, lon): 0.54 -> 0.30 ms; over everything: 0.61 -> 0.31.  None when it does not apply."""
    if backend != "torch" or w_raw is None:
        return None
    shape = tuple(int(n) for n in args_b[0].shape)
    nd = len(shape)
    if w_raw.ndim > nd or nd < 2:
        return None
    wstrides = tuple(w_raw.stride())
    for ax in _range(w_raw.ndim):
        if wstrides[ax] == 0 and w_raw.shape[ax] > 1:
            w_raw = w_raw[tuple(slice(0, 1) if k == ax else slice(None) for k in _range(w_raw.ndim))]
    wshape = (1,) * (nd - w_raw.ndim) + tuple(int(n) for n in w_raw.shape)
    if any(wshape[ax] not in (1, shape[ax]) for ax in _range(nd)):
        return None  # (not broadcastable: the regular path raises)
    drop = sorted(int(ax) for ax in drop_axes)
    vary = [ax for ax in _range(nd) if wshape[ax] > 1]
    if not vary or len(vary) == nd or any(ax not in drop for ax in vary):
        return None  # scalar weights, full-size weights, or weights that differ from row to row
    lo, hi = vary[0], vary[-1]
    if any(ax not in drop for ax in _range(lo, hi + 1)):
        return None
    while hi + 1 in drop:
        hi += 1
    lo_far = lo
    while lo_far - 1 in drop:
        lo_far -= 1
    total = 1
    for n in shape:
        total *= n
    itemsize = sum(_np_dtype_of(a).itemsize for a in args_b)
    n_bins = 1
    for b in bins:
        n_bins *= max(len(b) - 1, 0)
    blk = None
    for first in ([lo_far, lo] if lo_far != lo else [lo]):  # the whole run of adjacent reduced axes if its slab is still small
        slab_elems = 1
        for ax in _range(first, hi + 1):
            slab_elems *= shape[ax]
        left_over = any(ax < first or ax > hi for ax in drop)
        if slab_elems * 8 * 8 > total * itemsize or slab_elems == total:
            continue  # the slab is not small next to the data
        if left_over and n_bins * 8 * 4 > slab_elems * itemsize:
            continue  # (as in _reduce_in_two_steps: the intermediate must stay small)
        blk = list(_range(first, hi + 1))
        break
    if blk is None:
        return None
    lo = blk[0]
    rest = [ax for ax in drop if ax not in blk]
    slab = w_raw.reshape(wshape).expand(tuple(shape[ax] if lo <= ax <= hi else 1 for ax in _range(nd))).contiguous()
    part = _bincount(*args_b, slab.expand(shape), weights=True, axis=blk, bins=bins, density=False, block_size=block_size)
    return part.sum(dim=rest, keepdim=True) if rest else part


def _weights_constant_along_reduced(args_b, w_raw, drop_axes, bins, block_size, backend):
    """Weights that do not vary along some of the reduced axes (``cos(lat)`` of shape (1, lat, 1) under a
    reduction over lat and lon; one weight per time step; ...): the reference materialises them at
    full size (``broadcast_arrays`` + reshape, core.py:366 / 211-229).  Here the samples are COUNTED
    over those axes, unweighted, and the weights are applied to the counts:

        sum_{r0, r1} w[r1] [x in bin]  =  sum_{r1} w[r1] * count_{r0}[r1, bin]

    which reads the data once and moves no weight array at all.  Bins nobody fell into get 0 whatever
    their weight (a NaN weight poisons only bins that received a sample, as in np.bincount).
    Returns the ``_bincount``-shaped result, or None when the rewrite does not apply / does not pay."""
    shape = tuple(int(n) for n in args_b[0].shape)
    nd = len(shape)
    if w_raw is None or w_raw.ndim > nd:
        return None
    # weights that arrive already broadcast (stride-0 views: np.broadcast_to, torch.expand, what the
    # xarray wrapper hands over) are as good as size-1 axes
    wstrides = tuple(w_raw.stride()) if backend == "torch" else tuple(w_raw.strides)
    for ax in _range(w_raw.ndim):
        if wstrides[ax] == 0 and w_raw.shape[ax] > 1:
            w_raw = w_raw[tuple(slice(0, 1) if k == ax else slice(None) for k in _range(w_raw.ndim))]
    wshape = (1,) * (nd - w_raw.ndim) + tuple(int(n) for n in w_raw.shape)
    cand = sorted(int(ax) for ax in drop_axes if wshape[ax] == 1 and shape[ax] > 1)
    if not cand:
        return None
    # count over ONE block of adjacent axes (the one ending at the last candidate): adjacent axes walk
    # memory as a single strided dimension, which the counting kernels take without a copy
    r0 = [cand[-1]]
    while r0[0] - 1 in cand:
        r0.insert(0, r0[0] - 1)
    r1 = [int(ax) for ax in drop_axes if int(ax) not in r0]
    n_bins = 1
    for b in bins:
        n_bins *= max(len(b) - 1, 0)
    cols = 1
    for ax in r0:
        cols *= shape[ax]
    itemsize = sum(_np_dtype_of(a).itemsize for a in args_b)
    if n_bins * 8 * 4 > cols * itemsize:  # the intermediate counts must stay small next to the data they summarise
        return None
    counts = _bincount(*args_b, weights=False, axis=sorted(r0), bins=bins, density=False, block_size=block_size)
    tail = (1,) * len(bins)
    if backend == "torch":
        torch = _torch()
        w = w_raw.reshape(wshape + tail).to(torch.float64)
        contrib = torch.where(counts != 0, counts.to(torch.float64) * w, torch.zeros((), dtype=torch.float64, device=counts.device))
        return contrib.sum(dim=r1, keepdim=True) if r1 else contrib
    w = np.asarray(w_raw).reshape(wshape + tail)
    if w.dtype.kind == "c":
        return None  # let the regular path raise numpy's error
    with np.errstate(invalid="ignore", over="ignore"):
        contrib = np.where(counts != 0, counts.astype(np.float64) * w.astype(np.float64), 0.0)
    return contrib.sum(axis=tuple(r1), keepdims=True) if r1 else contrib


def histogram_two_weights(*args, bins=None, range=None, axis=None, weights=None, block_size="auto"):
    """Two weighted histograms of the same data from ONE pass over it (an extension; the reference
    leaves it as a TODO at xarray.py:106 and runs the path once per weight array).

    ``weights`` is a pair ``(wa, wb)``; everything else is as in :func:`histogram`.  Returns
    ``(ha, hb, bins)`` with ``ha == histogram(*args, weights=wa, ...)[0]`` and likewise ``hb``.  The
    idiom: the mean of ``A`` in the bins of ``x`` is ``ha / hb`` for ``wa = A * w``, ``wb = w``.
    Device-resident float32/float64 inputs with histograms that fit LDS share one read and one
    digitize of the samples; every other case degrades to two passes with identical results."""
    if weights is None or len(weights) != 2:
        raise ValueError("weights must be a pair of arrays")
    wa, wb = weights
    if any(_is_dask(a) for a in list(args) + [wa, wb]):
        ha, bins_out = histogram(*args, bins=bins, range=range, axis=axis, weights=wa, block_size=block_size)
        hb, _ = histogram(*args, bins=bins_out, axis=axis, weights=wb, block_size=block_size)
        return ha, hb, bins_out
    ha, bins_out = _histogram(args, bins, range, axis, wa, False, block_size, wb)
    return ha[0], ha[1], bins_out


# ---------------------------------------------------------------------------------------------
# short cut for the plain device-resident call
# ---------------------------------------------------------------------------------------------
# `histogram(x, bins=edges)` on a contiguous GPU tensor spends 9 us in its kernel (10^6 float64 samples) and
# used to spend 42 us in the layers above it: backend detection, broadcasting, numpy's validation of the edges,
# dtype promotion rules, stride analysis, plan lookup.  None of that can change between two calls with the same
# edges and the same kind of input, so the outcome is cached per signature and the call goes straight to the
# plan.  Everything this path does not recognise falls through to the general code below it.
_FAST = OrderedDict()  # (device, bins signature) -> (plan, validated edge arrays, the plan cache's key of that plan)
_FAST_TAGS = None


def _fast_signature(bins, n_inputs):
    """hashable identity of explicit float bin edges (their bytes: in-place edits are seen), or None"""
    if type(bins) is np.ndarray:
        per_input = (bins,) * n_inputs
    elif type(bins) in (list, tuple) and len(bins) == n_inputs:
        per_input = tuple(bins)
    else:
        return None, None
    sig = []
    for b in per_input:
        if type(b) is not np.ndarray or b.ndim != 1 or b.dtype.kind != "f" or b.dtype.itemsize > 8 or b.size < 2:
            return None, None
        sig.append((b.dtype.str, b.tobytes()))
    return tuple(sig), per_input


def _resident_fast_path(args, bins, range_, axis, weights, density, block_size):
    """(hist, edges) for contiguous float32 / float64 GPU tensors of one shape and dtype, explicit float edges,
    full or trailing-axes reduction, optional same-shape float weights — or None (take the general path)."""
    global _FAST_TAGS
    a0 = args[0]
    if type(a0).__module__ != "torch" or range_ is not None or block_size not in ("auto", None) or not 1 <= len(args) <= 3:
        return None
    torch = _torch()
    if _FAST_TAGS is None:
        _FAST_TAGS = {torch.float64: _native.F64, torch.float32: _native.F32}
    tag = _FAST_TAGS.get(a0.dtype)
    if tag is None or not a0.is_cuda or not a0.is_contiguous() or a0.numel() == 0:
        return None
    shape, device, dtype = a0.shape, a0.device, a0.dtype
    for a in args[1:]:
        if type(a) is not type(a0) or a.dtype != dtype or a.shape != shape or a.device != device or not a.is_contiguous():
            return None
    wtag = None
    if weights is not None:
        if type(weights) is not type(a0) or weights.shape != shape or weights.device != device or not weights.is_contiguous():
            return None
        wtag = _FAST_TAGS.get(weights.dtype)
        if wtag is None:
            return None
    ndim = a0.ndim
    leading = False
    if axis is None:
        kept = 0
    else:
        k = len(axis)
        if k == 0:
            return None
        order = sorted(axis)
        if order == list(_range(ndim - k, ndim)):
            kept = ndim - k
        elif order == list(_range(k)):  # the LEADING axes (dim="time" of (time, lat, lon)): rows are the contiguous direction
            leading = True
            kept = k
        else:
            return None  # (reduced axes in the middle or apart have their own view logic)
    sig, per_input = _fast_signature(bins, len(args))
    if sig is None:
        return None
    dev_index = _torch_device_index(device)
    key = (dev_index, sig)
    with _plans_lock:
        hit = _FAST.get(key)
        if hit is not None:
            _FAST.move_to_end(key)
            cur = _plans.get(hit[2])
            if cur is None:  # the plan cache dropped these edges since: back in, so that both caches hold ONE object
                _plans[hit[2]] = hit[0]
                while len(_plans) > _PLAN_CACHE:
                    _plans.popitem(last=False)
            elif cur is not hit[0]:  # ... and rebuilt them
                hit = (cur, hit[1], hit[2])
                _FAST[key] = hit
    if hit is None:
        # first call with these edges: numpy validates them exactly as in the general path
        edges = [np.histogram_bin_edges(np.zeros(0, np.float64), bins=b, range=None) for b in per_input]
        cmp_domain, conv, _ = _compare_domain([np.dtype(np.float64)] * len(args), edges)
        if cmp_domain != _native.CMP_F64:
            return None
        _native.require_device(dev_index)
        plan_key = (dev_index, cmp_domain) + tuple((e.dtype.str, e.tobytes()) for e in conv)  # (_get_plan's key)
        hit = (_get_plan(conv, cmp_domain, dev_index), edges, plan_key)
        with _plans_lock:
            _FAST[key] = hit
            while len(_FAST) > _PLAN_CACHE:
                _FAST.popitem(last=False)
    plan, edges = hit[0], hit[1]
    weighted = weights is not None
    if leading:
        cols = 1
        for n in shape[:kept]:
            cols *= int(n)
        rows = a0.numel() // cols
        rs, cs, kept_shape = 1, rows, tuple(shape[kept:])
    else:
        rows = 1
        for n in shape[:kept]:
            rows *= int(n)
        cols = a0.numel() // rows
        rs, cs, kept_shape = cols, 1, tuple(shape[:kept])
    out = torch.empty((rows,) + plan.bins_shape, dtype=torch.float64 if weighted else torch.int64, device=device)
    if out.numel():
        views = [_native.make_view(a.data_ptr(), tag, rs, cs) for a in args]
        wview = _native.make_view(weights.data_ptr(), wtag, rs, cs) if weighted else None
        plan.execute(views, wview, rows, cols, out.data_ptr(), weighted, _native.MEM_DEVICE, accumulate=False,
                     stream=torch.cuda.current_stream(device).cuda_stream)
    h = out.reshape(kept_shape + plan.bins_shape)
    if density:
        h = _density(h, edges, len(args))
    return h, list(edges)


def _normalise_axis(axis, ndim):
    """None, or the list of non-negative axis numbers to histogram over (core.py:346-355)"""
    if axis is None:
        return None
    requested = np.atleast_1d(axis)
    assert requested.ndim == 1
    out = []
    for ax in requested:
        ax = int(ax)
        if ax < 0:
            ax += ndim
        assert ax < ndim, "axis must be less than ndim"
        out.append(ax)
    return out


def _counts_one_device(all_arrays, w_raw, n_inputs, has_weights, two, drop_axes, bins, bincount_kwargs, backend):
    """Partial / full histogram of numpy or torch inputs on ONE GPU, reduced axes kept as size-1 dims
    (+ a leading pair axis for two weight arrays): the block adapter, or one of the rewrites around it."""
    block_size = bincount_kwargs["block_size"]
    counts = None
    if not two and has_weights:
        counts = _weights_slab(all_arrays[:n_inputs], w_raw, drop_axes, bins, block_size, backend)
        if counts is None:
            counts = _weights_constant_along_reduced(all_arrays[:n_inputs], w_raw, drop_axes, bins, block_size, backend)
    if counts is None and not two:
        counts = _reduce_in_two_steps(all_arrays, has_weights, drop_axes, bins, block_size, backend)
    if counts is None:
        counts = (_bincount_two_weights if two else _bincount)(*all_arrays, **bincount_kwargs)
    return counts


def _dask_graph(all_arrays, has_weights, drop_axes, bins, bincount_kwargs):
    """The lazy graph of the reference's dask branch (core.py:403-439): ONE block-adapter task per block of
    the (rechunk-aligned) inputs, whose output block keeps every input axis — reduced ones as single-element
    chunks — and appends one unchunked axis per bin dimension; then a sum over the reduced axes adds the
    partial histograms of the blocks that share output rows.  What differs from the reference is where a
    block runs: `_bincount_spread` puts it on the least busy of the node's GPUs."""
    import dask.array as dsa

    ndim = all_arrays[0].ndim
    data_index = tuple(_range(ndim))
    bin_index = tuple(_range(ndim, ndim + len(bins)))
    operands = [item for arr in all_arrays for item in (arr, data_index)]
    from . import multigpu

    on_gpus = multigpu.dask_exchange() == "rccl"
    out_dtype = np.dtype("i8" if not has_weights else all_arrays[-1].dtype)
    partials = dsa.blockwise(
        _bincount_partial if on_gpus else _bincount_spread,
        data_index + bin_index,
        *operands,
        new_axes={ax: len(b) - 1 for ax, b in zip(bin_index, bins)},
        adjust_chunks={ax: (lambda extent: 1) for ax in drop_axes},
        meta=np.array((), out_dtype),
        **bincount_kwargs,
    )
    if not on_gpus:
        return partials.sum(drop_axes)
    # the partial histograms stay on the GPUs that computed them; one task per output chunk adds up the partials of each
    # GPU there and the GPUs' sums with ONE RCCL all-reduce (multigpu.reduce_partials), instead of dask's tree of host sums
    kept_index = tuple(i for i in data_index if i not in drop_axes)
    return dsa.blockwise(
        multigpu.reduce_partials,
        kept_index + bin_index,
        partials,
        data_index + bin_index,
        concatenate=False,
        meta=np.array((), out_dtype),
        dtype=out_dtype,
        drop_axes=tuple(int(a) for a in drop_axes),
        out_dtype=out_dtype.str,
    )


def histogram(*args, bins=None, range=None, axis=None, weights=None, density=False, block_size="auto"):
    """Histogram applied along specified axis / axes, computed on an MI355X.

    Same signature, argument meaning, return value and error behaviour as
    ``xhistogram.core.histogram`` (core.py:250-466):

    args : array_like
        Input data; N arguments give an N-dimensional histogram.  numpy arrays, GPU-resident
        torch tensors or dask arrays; all broadcast against each other.
    bins : int, str, array, or a list with one of those per argument
        Number of bins, a ``numpy.histogram_bin_edges`` estimator name, or the bin edges.  All
        but the last bin are half-open ``[left, right)``; the last bin includes both edges.
        With dask inputs, bins must be arrays of edges (TypeError otherwise).
    range : (float, float) or a list of such pairs, optional
        Outer edges for integer / string ``bins``; default ``(arg.min(), arg.max())``.
    axis : None, int or tuple of ints
        Axes to histogram over; default all (flattened).
    weights : array_like, optional
        Weights broadcastable to the data; each sample contributes its weight.  A NaN weight
        turns its own bin into NaN.
    density : bool
        Normalise so that the integral over the range is 1 (per kept row).
    block_size : int or 'auto'
        Number of rows (non-histogram positions) handled per kernel launch; results never
        depend on it.  (The reference's 'auto' heuristic divides by zero above 10^7 samples per
        row, core.py:114-117; here 'auto' and None mean one launch.)

    Returns ``(hist, bin_edges)``: ``hist`` has the kept axes followed by one axis per argument;
    int64 counts, or float64 when weighted / density.  numpy in -> numpy out, torch in -> torch
    out (same device), dask in -> lazy dask array.
    """
    return _histogram(args, bins, range, axis, weights, density, block_size, None)


def _histogram(args, bins, range, axis, weights, density, block_size, _second_weights):
    """body of :func:`histogram`; `_second_weights` is histogram_two_weights' second weight array (private: the public
    functions keep the reference's exact signatures, core.py:250-258 and :197-199)"""
    n_inputs = len(args)
    axis = _normalise_axis(axis, args[0].ndim if hasattr(args[0], "ndim") else np.ndim(args[0]))  # (np.ndim would compute a dask array)
    if _second_weights is None:
        fast = _resident_fast_path(args, bins, range, axis, weights, density, block_size)
        if fast is not None:
            return fast
    has_weights = weights is not None
    two = _second_weights is not None  # histogram_two_weights: the second weight array rides along
    all_arrays = list(args) + ([weights] if has_weights else []) + ([_second_weights] if two else [])

    # ---- one backend for every input, then broadcast against each other (core.py:366) -----------
    w_raw = None
    if any(_is_dask(a) for a in all_arrays):
        import dask.array as dsa

        backend = "dask"
        all_arrays = list(dsa.broadcast_arrays(*[a if _is_dask(a) else dsa.asarray(np.asarray(a)) for a in all_arrays]))
    elif any(_is_torch(a) for a in all_arrays):
        torch = _torch()
        backend = "torch"
        dev = next((a.device for a in all_arrays if _is_torch(a) and a.device.type == "cuda"), None)
        if dev is None:
            raise RuntimeError("torch inputs must live on an MI355X (device='cuda'); every tensor given is on the CPU")
        all_arrays = [a.to(dev) if _is_torch(a) else torch.as_tensor(np.asarray(a)).to(dev) for a in all_arrays]
        w_raw = all_arrays[n_inputs] if has_weights else None  # as given, before broadcasting
        all_arrays = list(torch.broadcast_tensors(*all_arrays))
    elif any(_is_devarr(a) for a in all_arrays):
        backend = "device"
        dev = next(a.device for a in all_arrays if _is_devarr(a))
        all_arrays = [a.to(dev) if _is_devarr(a) else DeviceArray.from_numpy(np.asarray(a), dev) for a in all_arrays]
        w_raw = all_arrays[n_inputs] if has_weights else None
        shape = np.broadcast_shapes(*[a.shape for a in all_arrays])
        all_arrays = [a.broadcast_to(shape) for a in all_arrays]
    else:
        backend = "numpy"
        all_arrays = [np.asarray(a) for a in all_arrays]
        w_raw = all_arrays[n_inputs] if has_weights else None
        all_arrays = list(np.broadcast_arrays(*all_arrays))
    drop_axes = tuple(axis) if axis is not None else tuple(_range(all_arrays[0].ndim))

    # ---- bin edges (core.py:377-388) ---------------------------------------------------------
    bins = _ensure_correctly_formatted_bins(bins, n_inputs)
    range = _ensure_correctly_formatted_range(range, n_inputs)
    if backend == "dask":
        if not all(isinstance(b, np.ndarray) for b in bins):
            raise TypeError("When using dask arrays, bins must be provided as numpy array(s) of edges")
    elif backend in ("torch", "device"):
        bins = [_device_bin_edges(a, b, r, has_weights) for a, b, r in zip(all_arrays, bins, range)]
    else:
        w_for_edges = all_arrays[n_inputs] if has_weights else None
        bins = [np.histogram_bin_edges(a, bins=b, range=r, weights=w_for_edges) for a, b, r in zip(all_arrays, bins, range)]
    bincount_kwargs = dict(weights=has_weights, axis=axis, bins=bins, density=density, block_size=block_size)

    # ---- counts ------------------------------------------------------------------------------
    if backend == "dask":
        bin_counts = _dask_graph(all_arrays, has_weights, drop_axes, bins, bincount_kwargs)
    else:
        bin_counts = None
        if backend == "numpy":
            # host inputs big enough to be worth it are cut into shards, one per visible GPU: every shard is
            # staged over its own GPU's PCIe link by that GPU's host thread, the partials are added up
            from . import multigpu

            bin_counts = multigpu.host_sharded_counts(all_arrays, w_raw, n_inputs, has_weights, two, drop_axes, bins, bincount_kwargs)
        if bin_counts is None:
            bin_counts = _counts_one_device(all_arrays, w_raw, n_inputs, has_weights, two, drop_axes, bins, bincount_kwargs, backend)
        squeeze_axes = tuple(int(i) + (1 if two else 0) for i in drop_axes)  # (two: a leading pair axis)
        if backend == "torch":
            keep = [s for i, s in enumerate(bin_counts.shape) if i not in squeeze_axes]
            bin_counts = bin_counts.reshape(keep)
        else:
            bin_counts = bin_counts.squeeze(squeeze_axes)

    h = _density(bin_counts, bins, n_inputs) if density else bin_counts
    return h, bins


# ---------------------------------------------------------------------------------------------
# per-bin minimum and maximum of a value array
# ---------------------------------------------------------------------------------------------
_ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
_SIGN = np.uint64(1 << 63)


def extrema_keys(a):
    """order-preserving uint64 keys of float64 values, as the GPU kernels make them: unsigned order is the total order of the
    values with -0.0 < +0.0.  NaN has no key of its own (callers map it to an empty marker)."""
    b = np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    return b ^ np.where(b >> np.uint64(63) != 0, _ALL_ONES, _SIGN)


def _extrema_values(k):
    """inverse of extrema_keys"""
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return (k ^ np.where(k >> np.uint64(63) != 0, _SIGN, _ALL_ONES)).view(np.float64)


def combine_extrema(vmin, vmax, axis):
    """Per-bin minimum and maximum over `axis` (kept as axes of extent 1) of partial results, NaN meaning "no value", in the
    order of the GPU's keys: -0.0 < +0.0, and a bin is NaN only where every partial is.  The reduction of dask's partials."""
    vmin, vmax = np.asarray(vmin, np.float64), np.asarray(vmax, np.float64)
    kmin = np.where(np.isnan(vmin), _ALL_ONES, extrema_keys(vmin)).min(axis=axis, keepdims=True)
    kmax = np.where(np.isnan(vmax), np.uint64(0), extrema_keys(vmax)).max(axis=axis, keepdims=True)
    lo = np.where(kmin == _ALL_ONES, np.nan, _extrema_values(kmin))
    hi = np.where(kmax == np.uint64(0), np.nan, _extrema_values(kmax))
    return lo, hi


def _extrema_pair_reduce(x, axis=None, keepdims=True, **_):
    """dask.array.reduction step over [2, ...] blocks of (min, max) partials"""
    ax = tuple(int(a) for a in (axis if isinstance(axis, tuple) else (axis,)))
    lo, hi = combine_extrema(x[0], x[1], tuple(a - 1 for a in ax))
    out = np.stack([lo, hi])
    return out if keepdims else out.squeeze(ax)


def _check_values_dtype(values, name="histogram_extrema"):
    """TypeError, before any device work, for values that have no order or no float64 image"""
    if _is_torch(values):
        if values.dtype.is_complex:
            raise TypeError("complex values have no order: %s takes real values" % name)
        _torch_tag(values.dtype)
        return
    dt = np.dtype(values.dtype) if hasattr(values, "dtype") else np.asarray(values).dtype
    if dt.kind == "c":
        raise TypeError("complex values have no order: %s takes real values" % name)
    if dt.kind not in "fiub":
        raise TypeError("%s takes real values, got dtype %s" % (name, dt))


def _upload_host(args, values, bins, *extras):
    """host (numpy) samples and values (and the arrays after them: weights or a second value array, then the weights of a pair
    of values; None: not given) as DeviceArrays on the calling thread's GPU, broadcast there (stride 0, not copied)"""
    args = [np.asarray(a) for a in args]
    args, _ = _prepare_dtypes(args, None, [a.dtype for a in args], bins, "numpy")
    dev = _host_device()
    _native.require_device(dev)
    # (values None: a call that reads the samples alone, bin_index and histogram_lookup)
    arrays = [DeviceArray.from_numpy(a, dev)
              for a in args + [np.asarray(v) for v in (values,) if v is not None] + [np.asarray(e) for e in extras if e is not None]]
    shape = np.broadcast_shapes(*[a.shape for a in arrays])
    return [a.broadcast_to(shape) for a in arrays]


# What one launch over [rows, cols] views needs, as _value_views makes it:
#   plan        the Plan of the edges on the samples' device
#   nv          the native views (samples..., values[, weights or second values[, weights]])
#   keep        the views they were made of: their copies, if any, must outlive the kernels (_launch_outputs holds them)
#   m, c        rows and columns
#   kept_shape  the sample shape with the reduced extents 1 (the kept axes stay in place; then come the bin axes)
#   red, kept   the reduced axes in ascending number and the kept axes
#   device, stream, backend ("torch" or "device")
#   like        the first array of samples: what outputs look like (shape, torch device)
_Launch = namedtuple("_Launch", "plan nv keep m c kept_shape red kept device stream backend like")


def _value_views(args, values, axis, bins, backend, *extras, ordered=False):
    """the [rows, cols] views of broadcast torch tensors or DeviceArrays and of their values (and of the arrays after them, as
    _upload_host takes them), for a per-bin statistic of the values or a per-sample output: a _Launch.  The views are those
    of _bincount's block adapter; layouts no three strides describe are copied.  `ordered`: the columns of a row are the
    reduced axes in ascending axis number, C order (a statistic that reports positions inside the row); otherwise any order
    that walks memory as one strided dimension will do, and layouts that need a permutation for that are not copied."""
    a0 = args[0]
    ndim = a0.ndim
    do_full_array = (axis is None) or (set(axis) == set(_range(ndim)))
    if do_full_array:
        red, kept, kept_axes_shape = tuple(_range(ndim)), (), (1,) * ndim
    else:
        red = tuple(sorted(axis))
        kept = tuple(i for i in _range(ndim) if i not in red)
        kept_axes_shape = tuple(1 if i in red else int(a0.shape[i]) for i in _range(ndim))
    dtypes = [_np_dtype_of(a) for a in args]
    cmp_domain, edges, common = _compare_domain(dtypes, bins)
    if backend == "device" and any(c is not None and a.dtype != c for a, c in zip(args, common)):
        raise TypeError("datetime64 DeviceArrays must already have the unit they share with their bin edges")
    arrays = list(args) + [a for a in (values,) + extras if a is not None]  # (values None: the samples alone)
    if ordered:
        axis = axis if do_full_array else list(red)
        order = list(red)
    else:
        order = _reduced_order(arrays[0], list(_range(ndim)) if do_full_array else axis)
    descs = [_collapse(a, axis, do_full_array, order) for a in arrays]
    views = None
    if all(d is not None for d in descs) and len({d[:2] for d in descs}) == 1:
        views = [_view_of(a, d, backend) for a, d in zip(arrays, descs)]
        m, c = (int(n) for n in descs[0][:2])
        if any(v is None for v in views):
            views = None
    if views is None:
        blocks = [_rows_cols(a, axis, do_full_array) for a in arrays]
        m, c = (int(n) for n in blocks[0].shape)
        views = [_strided_view(b, backend) for b in blocks]
    if backend == "device":
        device, stream = a0.device, 0
    else:
        torch = _torch()
        if a0.device.type != "cuda":
            raise RuntimeError("torch inputs must live on an MI355X (device='cuda'); got %s" % a0.device)
        device = _torch_device_index(a0.device)
        stream = torch.cuda.current_stream(a0.device).cuda_stream
    _native.require_device(device)
    plan = _get_plan(edges, cmp_domain, device)
    nv = [_native.make_view(*v[:6]) for v in views]
    return _Launch(plan, nv, views, m, c, kept_axes_shape, red, kept, device, stream, backend, a0)


def _launch_outputs(rec, blocks, run):
    """The outputs of one launch: `blocks` is a list of (shape, np.int64 or np.float64), and `run(pointers)` has the kernels
    write each dense block at its pointer; it is called exactly when the blocks hold any element at all (a plan without bins
    counts no sample: the library itself then fills the blocks).  torch: one tensor per block on the samples' device,
    asynchronous on the call's stream.  Otherwise: one DeviceBuffer and one download for all blocks, and the blocks are views
    of that one host array.  The kernels are handed these blocks themselves, never a view of something else: a copied
    output would be lost.  `rec`, and with it the keep-alive copies of the views, lives until the launch is enqueued (torch)
    or the download has waited for the kernels."""
    if rec.backend == "torch":
        torch = _torch()
        device = rec.like.device
        outs = [torch.empty(shape, dtype=torch.int64 if dt is np.int64 else torch.float64, device=device) for shape, dt in blocks]
        if any(0 not in shape for shape, _ in blocks):  # (a block holds an element unless one of its extents is 0)
            run([o.data_ptr() for o in outs])
        return outs
    cuts = [0]
    for shape, _ in blocks:
        cuts.append(cuts[-1] + math.prod(shape))
    host = np.empty(cuts[-1], np.int64)
    if cuts[-1] > 0:
        buf = _native.DeviceBuffer(rec.device, host.nbytes)
        run([buf.ptr + 8 * at for at in cuts[:-1]])
        buf.download(host)
    return [(host[a:b] if dt is np.int64 else host[a:b].view(np.float64)).reshape(shape)
            for a, b, (shape, dt) in zip(cuts, cuts[1:], blocks)]


# What the one path below (_value_rows, _value_block, _value_stat) needs of a per-bin statistic of values, an entry of
# _VALUE_STATS:
#   k        the number of outputs, each [rows, bins]; None: one per element of the call's `q`
#   ints     the outputs that are int64 (all others are float64)
#   method   the Plan method that fills them
#   ptrs     the outputs whose pointers the method is given: the outputs are contiguous, in order, so a pointer may stand for
#            a block of several
#   extras   how many arrays it reads after the values (weights; a second value array; a second value array, then weights)
#   reduce   the dask step that merges the partials of blocks that share output rows.  None: they cannot be merged, and every
#            reduced axis must be one chunk
#   tail     the names of the per-call parameters the method takes after the pointers
#   ordered  whether it reports positions inside the row (_value_views, ordered)
#   noun     what the refusal of several chunks calls the partials that cannot be merged
#   max_cols the reduced extent per output row it refuses (NotImplementedError, before any device work); None: no limit
#   max_bins the number of bins beyond which it refuses, in the same way and only next to max_cols; None: no limit
_ValueStat = namedtuple("_ValueStat", "k ints method ptrs extras reduce tail ordered noun max_cols max_bins",
                        defaults=((), False, None, None, None))

# the limits of the sorted order: samples per output row, and bins (B + 1 keys in 32 bits)
_ORDER_MAX_COLS = 1 << 31
_SORT_MAX_BINS = (1 << 32) - 1


def _value_rows(st, args, values, axis, bins, backend, *extras, **params):
    """the statistic's outputs of broadcast torch tensors (torch out) or DeviceArrays (numpy out) as one float64 block
    [k, kept axes (reduced ones of extent 1), bins...], its int64 outputs as the bits they are"""
    rec = _value_views(args, values, axis, bins, backend, *extras, ordered=st.ordered)
    n = rec.m * rec.plan.n_bins
    k = st.k or len(params["q"])

    def run(ptrs):
        getattr(rec.plan, st.method)(rec.nv[:len(args)], *rec.nv[len(args):], rec.m, rec.c, *[ptrs[0] + i * n * 8 for i in st.ptrs],
                                     *[params[p] for p in st.tail], stream=rec.stream)

    return _launch_outputs(rec, [((k,) + rec.kept_shape + rec.plan.bins_shape, np.float64)], run)[0]


def _value_block(*all_arrays, stat=None, axis=None, bins=None, **params):
    """one dask block (samples..., values, the statistic's extras): its outputs as _value_rows gives them.  Counts that the
    dask step merges become float64 by value; int64 outputs that are never merged stay the bits they are."""
    st = _stat_entry(stat)
    n = len(all_arrays) - 1 - st.extras
    arrays = _upload_host(all_arrays[:n], all_arrays[n], bins, *all_arrays[n + 1:])
    out = _value_rows(st, arrays[:n], arrays[n], axis, bins, "device", *arrays[n + 1:], **params)
    if st.reduce is not None:
        for i in st.ints:
            out[i] = out[i].view(np.int64)
    return out


def _resident(backend, raw, all_arrays, n_inputs, bins):
    """the arrays _value_views takes, and the backend it takes them as: numpy inputs (`raw`: samples..., then the values and
    what follows them, if any) uploaded to the calling thread's GPU ("device"), torch tensors and DeviceArrays as they are"""
    if backend == "numpy":
        rest = raw[n_inputs:] or [None]
        return _upload_host(raw[:n_inputs], rest[0], bins, *rest[1:]), "device"
    return all_arrays, backend


def _check_sizes(name, shape, drop_axes, bins, max_cols, max_bins=None):
    """NotImplementedError for `max_cols` samples or more per output row and for more than `max_bins` bins (None: no bound),
    from the broadcast shape and the edges alone: (samples per output row, number of bins)"""
    cols = math.prod(int(shape[ax]) for ax in drop_axes)
    if cols >= max_cols:
        raise NotImplementedError("%s takes fewer than 2^31 = %d samples per output row, got %d: split the reduced axes"
                                  % (name, max_cols, cols))
    n_bins = math.prod(max(len(b) - 1, 0) for b in bins)
    if max_bins is not None and n_bins > max_bins:
        raise NotImplementedError("%s takes at most 2^32 - 1 = %d bins, got %d" % (name, max_bins, n_bins))
    return cols, n_bins


def _check_one_chunk(noun, all_arrays, drop_axes):
    """ValueError for dask inputs whose reduced axes are cut, where there is no merge of the partials (`noun`) of the chunks"""
    if any(len(a.chunks[ax]) > 1 for a in all_arrays for ax in drop_axes):
        raise ValueError("%s of several chunks cannot be merged: rechunk the reduced axes of every input into "
                         "one chunk (e.g. arr.rechunk({axis: -1}))" % noun)


def _drop_axes(a, axes, backend):
    """_value_rows' output without its reduced axes (of extent 1)"""
    if backend == "torch":
        return a.reshape([s for i, s in enumerate(a.shape) if i not in axes])
    return a.squeeze(axes)


def _value_stat(stat, args, values, bins, range, axis, name, aggregate=None, *extras, weights=None, **params):
    """the backends of the per-bin statistic _VALUE_STATS[stat] of values: (backend, the outputs with the shape ``histogram``
    gives, bin edges, reduced axes).  `extras` are the arrays it reads after the values, in its order, `weights` (None: not
    given) the last of them, and `params` its per-call parameters.  The outputs are a list of k arrays; the quantiles stay one
    array behind their q axis.  dask: lazy arrays, the partials merged by the statistic's dask step and the last step by
    `aggregate`.  The entry's size limits are refused before any device work on the samples."""
    backend, all_arrays, raw, bins, axis, drop_axes = _values_call(args, values, bins, range, axis, name, *extras, weights)
    n_inputs = len(args)
    st = _stat_entry(stat)
    k = st.k or len(params["q"])
    if st.max_cols is not None:
        _check_sizes(name, all_arrays[0].shape, drop_axes, bins, st.max_cols, st.max_bins)
    merged = backend == "dask" and st.reduce is not None
    if backend == "dask":
        if not merged:
            _check_one_chunk(st.noun, all_arrays, drop_axes)
        res = _values_blockwise(partial(_value_block, stat=stat, **params), k, all_arrays, bins, axis, drop_axes)
        if merged:
            import dask.array as dsa

            res = dsa.reduction(res, st.reduce, aggregate or st.reduce, combine=st.reduce,
                                axis=tuple(ax + 1 for ax in drop_axes), keepdims=False, dtype=np.float64, concatenate=True,
                                meta=np.array((), np.float64))
        else:
            res = res[(slice(None),) + tuple(0 if i in drop_axes else slice(None) for i in _range(all_arrays[0].ndim))]
    else:
        arrays, on = _resident(backend, raw, all_arrays, n_inputs, bins)
        res = _value_rows(st, arrays[:n_inputs], arrays[n_inputs], axis, bins, on, *arrays[n_inputs + 1:], **params)
        res = _drop_axes(res, tuple(a + 1 for a in drop_axes), backend)
    if st.k is not None:
        res = list(res.unbind(0) if backend == "torch" else res)
        for i in st.ints:  # (counts that the dask step merged come back by value, every other int64 output as the bits it is)
            res[i] = res[i].astype(np.int64) if merged else res[i].view(_torch().int64 if backend == "torch" else np.int64)
    return backend, res, bins, drop_axes


def histogram_extrema(*args, values, bins=None, range=None, axis=None, block_size="auto"):
    """Per-bin minimum and maximum of ``values``, computed on an MI355X: the extreme value in each bin, as
    ``scipy.stats.binned_statistic`` gives it with ``statistic="min"`` / ``"max"``.

    ``args``, ``bins``, ``range`` and ``axis`` are those of :func:`histogram`, and the samples that count are exactly the ones
    ``histogram`` counts (same digitize, last bin closed on the right, NaN and out-of-range samples dropped, the same
    broadcasting).  The edges are those the unweighted ``histogram`` call gives: estimator names are allowed.  ``values``
    (any real dtype, converted like ``astype(np.float64)``; broadcast like weights) is what each counted sample contributes.
    NaN values are ignored (``np.fmin`` / ``np.fmax``), values are ordered totally with ``-0.0 < +0.0``, and a bin that got no
    value is NaN in both outputs.  The results are exact.  ``block_size`` is accepted and changes nothing.

    Returns ``(vmin, vmax, bin_edges)``: float64, with the shape ``histogram`` gives (kept axes, then bin axes).  numpy in ->
    numpy out, torch in -> torch out on the same device, DeviceArray in -> numpy out, dask in -> lazy dask arrays."""
    # dask: one task per block with its (min, max) pair on a leading axis; the pairs of the blocks that share output rows meet
    # in the key-ordered combine on the host (also under XHIST_AMD_DASK_EXCHANGE=rccl: the exchange adds only)
    _, (vmin, vmax), bins, _ = _value_stat("extrema", args, values, bins, range, axis, "histogram_extrema")
    return vmin, vmax, bins


def histogram_argextrema(*args, values, bins=None, range=None, axis=None, block_size="auto"):
    """Where each bin's minimum and maximum of ``values`` lie, computed on an MI355X: the position of the first sample that
    holds the bin's extreme, what ``scipy.stats.binned_statistic`` users get from ``statistic=np.argmin`` as a Python callable
    on the host.  A position indexes every other field: the depth, the oxygen and the date of each class's coldest sample.

    ``args``, ``bins``, ``range``, ``axis`` and ``values`` are those of :func:`histogram_extrema`, and so are the samples that
    count, the NaN-value rule and the total order (``-0.0 < +0.0``); ``vmin`` and ``vmax`` equal its outputs bit for bit.

    ``argmin`` / ``argmax`` hold the position of the FIRST counted sample whose value (as float64) is the bin's minimum /
    maximum, and ``-1`` where the bin is empty.  A position is the C-order flat index over the reduced axes taken in ascending
    axis number, in the broadcast shape, whatever order ``axis`` lists them in:
    ``np.unravel_index(argmin, [shape[i] for i in sorted(axis)])`` gives per-axis indices; with ``axis=None`` it is the flat
    index into the broadcast array.  "First" means smallest position.  The result departs from ``np.nanargmin`` of the bin's
    values only where the total order does: among ``+0.0`` and ``-0.0`` the minimum is a ``-0.0``.  Exact and deterministic:
    one pass finds the extremes, a second one takes the smallest position among the samples that equal them.
    ``block_size`` is accepted and changes nothing.

    Returns ``(argmin, argmax, vmin, vmax, bin_edges)``: int64 and float64 with the shape ``histogram`` gives (kept axes, then
    bin axes).  numpy in -> numpy out, torch in -> torch out on the same device (asynchronous on the current stream),
    DeviceArray in -> numpy out, dask in -> lazy dask arrays, one task per block: every reduced axis must then be a single
    chunk (positions of several chunks are not merged)."""
    # one block of four outputs, (vmin, vmax, argmin, argmax): a position is the column of the row the library saw, and those
    # columns are the reduced axes in ascending axis number (the entry is `ordered`)
    _, (vmin, vmax, amin, amax), bins, _ = _value_stat("argextrema", args, values, bins, range, axis, "histogram_argextrema")
    return amin, amax, vmin, vmax, bins


def histogram_sum(*args, values, bins=None, range=None, axis=None, weights=None, block_size="auto"):
    """Per-bin count and sum of ``values``, computed on an MI355X with integer arithmetic: ``scipy.stats.binned_statistic``'s
    ``"sum"`` (NaN-ignoring), the same bits for any order of the samples, any chunking into rows, any launch geometry and any
    run.  Volumes, heat content or tracer mass per class can then be compared bit for bit across restarts.

    ``args``, ``bins``, ``range``, ``axis``, ``values`` (any real dtype, taken as float64), the samples that count, the NaN-value
    rule (a counted sample contributes when its value is not NaN), the broadcasting and the backends are those of
    :func:`histogram_mean_var`; ``count`` is its int64 count.  ``block_size`` is accepted and changes nothing.

    ``total`` is defined per (row, bin), on integers only:

    1. ``A`` is the largest ``|v|`` of the bin (``max(|vmin|, |vmax|)`` of :func:`histogram_extrema`, which is the first of the
       two passes).  An empty bin, or ``A == 0``, gives ``+0.0``.
    2. ``E`` is ``frexp(A)``'s exponent (``|v| < 2**E``), ``U = max(E - 96, -1074)``; the unit is ``2**U``.
    3. A value ``v = s * m * 2**e`` (``m`` the 53-bit integer significand, ``e = -1074`` for subnormals) becomes
       ``q = m << (e - U)``, or ``m >> (U - e)`` truncated towards zero where ``e < U`` (0 once the shift reaches 64).
       ``q < 2**96`` is split into three unsigned 32-bit limbs, and ``s * limb_j`` is added into three int64 accumulators.
    4. A row has fewer than 2^31 samples, so ``S = L0 + L1 * 2**32 + L2 * 2**64`` fits a signed 128-bit integer.
    5. ``total = RN_even(S * 2**U)``: one rounding, in integer arithmetic, overflowing to ``+-inf`` as IEEE does; a zero
       result is ``+0.0``.
    6. A bin that holds an infinity gives that infinity, or NaN where it holds both; its finite values are skipped.

    Values whose lowest set bit lies at or above ``2**U`` are converted exactly: every value within a factor ``2**43`` of its
    bin's largest magnitude, and every value where ``E - 96 <= -1074`` (subnormals are exact).  A bin of such values gets the
    correctly rounded exact sum, ``math.fsum`` bit for bit.  In general ``|total - exact| <= ulp(total) / 2 + n * 2**(E - 96)``,
    the second term below ``2**-12`` ulp of the bin's largest magnitude.  No intermediate overflows:
    ``[1.5e308, 1.5e308, -1.5e308]`` gives ``1.5e308``.  ``histogram_sum(x, values=w)[1]`` is a reproducible weighted histogram
    that ignores NaN weights instead of letting them poison the bin.

    ``weights`` is refused (``TypeError``): the product of two float64 numbers is not a float64 number, so multiply them into
    ``values``.  A reduced extent of 2^31 samples or more per output row is a ``NotImplementedError``.  Both, and complex
    values, are refused before any device work.

    Returns ``(count, total, bin_edges)``: count int64, total float64, with the shape ``histogram`` gives (kept axes, then bin
    axes).  numpy in -> numpy out, torch in -> torch out on the same device (asynchronous on the current stream), DeviceArray
    in -> numpy out, dask in -> lazy dask arrays, one task per block: every reduced axis must then be a single chunk (the
    integer accumulators of several chunks are not merged)."""
    if weights is not None:
        raise TypeError("histogram_sum does not take weights: multiply them into values (the product of two float64 numbers is "
                        "not a float64 number, so the weighted sum is another statistic)")
    _, (count, total), bins, _ = _value_stat("sum", args, values, bins, range, axis, "histogram_sum")
    return count, total, bins


def _values_call(args, values, bins, range, axis, name, *extras, needs_values=True):
    """the front of a per-bin statistic of values: argument checks before any device work, the backend, the broadcast
    arrays (samples..., values, extras...: the arrays the statistic reads after the values, in its order; None: not given),
    the numpy originals (numpy backend), the edges of the unweighted histogram, the normalised axis and the reduced axes.
    `needs_values` False: a call that reads the samples alone (bin_index, histogram_lookup) passes values None, and the
    arrays are the samples."""
    if values is None and needs_values:
        raise TypeError("%s needs values" % name)
    if not args:
        raise TypeError("%s needs at least one array of samples" % name)
    extras = [x for x in (values,) + extras if x is not None]
    for x in extras:
        _check_values_dtype(x, name)
    n_inputs = len(args)
    axis = _normalise_axis(axis, args[0].ndim if hasattr(args[0], "ndim") else np.ndim(args[0]))
    all_arrays = list(args) + extras
    raw = None
    if any(_is_dask(a) for a in all_arrays):
        import dask.array as dsa

        backend = "dask"
        all_arrays = list(dsa.broadcast_arrays(*[a if _is_dask(a) else dsa.asarray(np.asarray(a)) for a in all_arrays]))
    elif any(_is_torch(a) for a in all_arrays):
        torch = _torch()
        backend = "torch"
        dev = next((a.device for a in all_arrays if _is_torch(a) and a.device.type == "cuda"), None)
        if dev is None:
            raise RuntimeError("torch inputs must live on an MI355X (device='cuda'); every tensor given is on the CPU")
        all_arrays = [a.to(dev) if _is_torch(a) else torch.as_tensor(np.asarray(a)).to(dev) for a in all_arrays]
        all_arrays = list(torch.broadcast_tensors(*all_arrays))
    elif any(_is_devarr(a) for a in all_arrays):
        backend = "device"
        dev = next(a.device for a in all_arrays if _is_devarr(a))
        all_arrays = [a.to(dev) if _is_devarr(a) else DeviceArray.from_numpy(np.asarray(a), dev) for a in all_arrays]
        shape = np.broadcast_shapes(*[a.shape for a in all_arrays])
        all_arrays = [a.broadcast_to(shape) for a in all_arrays]
    else:
        backend = "numpy"
        raw = [np.asarray(a) for a in all_arrays]
        all_arrays = list(np.broadcast_arrays(*raw))
    drop_axes = tuple(axis) if axis is not None else tuple(_range(all_arrays[0].ndim))

    # ---- bin edges: those of the unweighted histogram ------------------------------------------
    bins = _ensure_correctly_formatted_bins(bins, n_inputs)
    range = _ensure_correctly_formatted_range(range, n_inputs)
    if backend == "dask":
        if not all(isinstance(b, np.ndarray) for b in bins):
            raise TypeError("When using dask arrays, bins must be provided as numpy array(s) of edges")
    elif backend in ("torch", "device"):
        bins = [_device_bin_edges(a, b, r, False) for a, b, r in zip(all_arrays[:n_inputs], bins, range)]
    else:
        bins = [np.histogram_bin_edges(a, bins=b, range=r) for a, b, r in zip(all_arrays[:n_inputs], bins, range)]
    return backend, all_arrays, raw, bins, axis, drop_axes


def _values_blockwise(block_fn, k, all_arrays, bins, axis, drop_axes):
    """dask: one task per block of the broadcast (samples..., values[, weights]), each giving k statistics on a leading axis —
    [k, block axes (reduced ones of extent 1), bins...]"""
    import dask.array as dsa

    n_inputs = len(bins)
    ndim = all_arrays[0].ndim
    data_index = tuple(_range(1, ndim + 1))
    bin_index = tuple(_range(ndim + 1, ndim + 1 + n_inputs))
    operands = [item for arr in all_arrays for item in (arr, data_index)]
    return dsa.blockwise(
        block_fn, (0,) + data_index + bin_index, *operands,
        new_axes=dict([(0, k)] + [(ax, len(b) - 1) for ax, b in zip(bin_index, bins)]),
        adjust_chunks={ax + 1: (lambda extent: 1) for ax in drop_axes},
        meta=np.array((), np.float64), axis=axis, bins=bins,
    )


# ---------------------------------------------------------------------------------------------
# per-bin count, mean and variance of a value array
# ---------------------------------------------------------------------------------------------
def _check_ddof(ddof):
    if isinstance(ddof, (bool, np.bool_)) or not isinstance(ddof, (int, np.integer)) or ddof < 0:
        raise ValueError("ddof must be an integer >= 0, got %r" % (ddof,))
    return int(ddof)


def _counted(x):
    """where a partial holds something: a count above 0"""
    return x > 0


def _weighed(x):
    """where a weighted partial holds something: W != 0 (NaN != 0: a NaN partial is taken, and its NaN spreads)"""
    return x != 0


def _merge_partials(update, present, x, rest, axis):
    """The pairwise merge of partial (x, rest...) results over `axis` (kept as axes of extent 1), one partial after another in
    index order (C order over several axes); x is the count or the sum of weights and present(x) says where a partial (or the
    running result) holds something.  Where only the partial does, it is taken as it is; where both do, the running values of
    `rest` become update(cx, xb, tot, running, partial's), with cx and xb the x of the two and tot their sum.  Returns the
    float64 list [x, rest...]."""
    x, *rest = (np.asarray(a, np.float64) for a in [x] + list(rest))
    ax = tuple(sorted(int(a) % x.ndim for a in (axis if isinstance(axis, (tuple, list)) else (axis,))))
    kept = [i for i in _range(x.ndim) if i not in ax]
    keep_shape = tuple(1 if i in ax else x.shape[i] for i in _range(x.ndim))

    def lead(a):
        a = np.transpose(a, ax + tuple(kept))
        return a.reshape((int(np.prod(a.shape[:len(ax)])),) + a.shape[len(ax):])  # (not -1: a kept axis may have extent 0)

    x, rest = lead(x), [lead(a) for a in rest]
    cx = np.zeros(x.shape[1:])
    cur = [np.full(x.shape[1:], np.nan) for _ in rest]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in _range(x.shape[0]):
            xb, part = x[k], [a[k] for a in rest]
            take = present(xb)
            first = take & ~present(cx)
            both = take & present(cx)
            tot = cx + xb
            new = update(cx, xb, tot, cur, part)
            cur = [np.where(first, p, np.where(both, n, c)) for p, n, c in zip(part, new, cur)]
            cx = np.where(take, tot, cx)
    return [a.reshape(keep_shape) for a in [cx] + cur]


def _chan_update(cx, xb, tot, cur, part, pairs=((0, 0),)):
    """Chan's update of running (means..., moments...): pairs[m] = (i, j) names the two means whose deviations multiply into
    moment m's cross term ((0, 0): the M2 of mean 0), so the means are all but the last len(pairs)"""
    n_means = len(cur) - len(pairs)
    d = [m - c for m, c in zip(part[:n_means], cur)]
    return ([c + di * xb / tot for c, di in zip(cur, d)]
            + [c + q + d[i] * d[j] * cx * xb / tot for c, q, (i, j) in zip(cur[n_means:], part[n_means:], pairs)])


# combine_cov's order of moments (M2_a, M2_b, C_ab), and the order of the library's outputs (M2_a, C_ab, M2_b)
_COV_PAIRS = ((0, 0), (1, 1), (0, 1))
_COV_BLOCK_PAIRS = ((0, 0), (0, 1), (1, 1))


def combine_mean_var(n, mean, m2, axis):
    """Merge partial (count, mean, M2) results over `axis` (kept as axes of extent 1) with Chan's pairwise formula, one
    partial after another in index order (C order over several axes):
        n = na + nb,  d = mb - ma,  mean = ma + d * nb / n,  M2 = M2a + M2b + d^2 * na * nb / n.
    Partials with n == 0 are skipped; where every partial is empty, mean and M2 are NaN and n is 0.  The reduction of dask's
    partials.  Returns float64 (n, mean, M2)."""
    return tuple(_merge_partials(_chan_update, _counted, n, [mean, m2], axis))


def combine_weighted_mean_var(w, mean, m2, axis):
    """Merge partial weighted (W, mean, M2) results over `axis` (kept as axes of extent 1) with the weighted form of Chan's
    pairwise formula, one partial after another in index order (C order over several axes):
        W = Wa + Wb,  d = mb - ma,  mean = ma + d * Wb / W,  M2 = M2a + M2b + d^2 * Wa * Wb / W.
    Partials with W == 0 are skipped; a NaN partial (a NaN W among them) makes the bin NaN.  Where every partial has W == 0,
    mean and M2 are NaN and W is 0.  The reduction of dask's weighted partials.  Returns float64 (W, mean, M2)."""
    return tuple(_merge_partials(_chan_update, _weighed, w, [mean, m2], axis))


def _var_of(x, m2, ddof):
    """the variance M2 / (x - ddof) of numpy arrays or torch tensors, x the count or the sum of weights: NaN where x <= ddof"""
    if _is_torch(m2):
        torch = _torch()
        return torch.where(x > ddof, m2 / (x - ddof).to(torch.float64), torch.full_like(m2, float("nan")))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(x > ddof, m2 / (x - ddof), np.nan)


def histogram_mean_var(*args, values, bins=None, range=None, axis=None, ddof=0, weights=None, block_size="auto"):
    """Per-bin count, mean and variance of ``values``, computed on an MI355X: ``scipy.stats.binned_statistic`` with
    ``statistic="count"``, ``"mean"`` and ``"std"`` (squared), NaN-ignoring like ``np.nanmean`` / ``np.nanvar``.

    ``args``, ``bins``, ``range`` and ``axis`` are those of :func:`histogram`, and a sample counts when ``histogram`` counts it
    (same digitize, last bin closed on the right, NaN and out-of-range samples dropped, the same broadcasting) and its value is
    not NaN.  The edges are those the unweighted ``histogram`` call gives: estimator names are allowed.  ``values`` (any real
    dtype, converted like ``astype(np.float64)``; broadcast like weights) is what each counted sample contributes.
    ``block_size`` is accepted and changes nothing.

    Two passes over the data: ``n`` and the float64 sum ``S`` of each bin, ``mean = S / n``; then ``d = v - mean`` in float64
    and the corrected two-pass sum of squared deviations (Chan, Golub & LeVeque) ``M2 = max(0, sum(d**2) - sum(d)**2 / n)``,
    ``var = M2 / (n - ddof)``.  The mean is NaN where ``n == 0``, the variance where ``n <= ddof``; infinite values give what
    ``np.nanmean`` / ``np.nanvar`` give.  Float64 atomics add in arbitrary order, so the last bits of the mean and the
    variance can differ from run to run; data whose sums are exact in any order give the same bits every time.

    Returns ``(count, mean, var, bin_edges)``: count int64, mean and var float64, with the shape ``histogram`` gives (kept
    axes, then bin axes).  numpy in -> numpy out, torch in -> torch out on the same device, DeviceArray in -> numpy out, dask
    in -> lazy dask arrays.

    ``weights`` (any real dtype, converted like ``astype(np.float64)``; broadcast like ``values``) makes them frequency
    weights, the convention of statsmodels' ``DescrStatsW``: each counted sample contributes its pair ``(w, v)``, and
    ``W = sum(w)``, ``mean = sum(w * v) / W``, ``d = v - mean``, ``M2 = max(0, sum(w * d**2) - sum(w * d)**2 / W)``,
    ``var = M2 / (W - ddof)``, all in float64.  With ``ddof=0`` the mean is ``np.average(v, weights=w)`` and the variance
    ``np.average((v - mean)**2, weights=w)``; with ``w == 1`` every output equals the unweighted call's.  The mean and M2 are
    NaN where ``W == 0`` (empty bins and bins whose weights sum to 0), the variance where ``W <= ddof``.  A NaN weight makes
    its bin's W, mean and variance NaN; zero weights contribute nothing (``0 * inf`` is NaN, as in ``np.average``); infinite
    weights give what the formulas give.  Negative weights are not checked: the formulas apply, the clamp of M2 at 0
    included, which is meaningful only for non-negative weights.  Returns ``(sum_of_weights, mean, var, bin_edges)``, all
    three float64 (W, the census of the samples that carry a value, takes the place of the count), with the same shapes and
    backends; dask merges the blocks' partials with :func:`combine_weighted_mean_var`."""
    ddof = _check_ddof(ddof)
    # dask: one task per block with its (n, mean, M2) or (W, mean, M2) on a leading axis; the partials of the blocks that share
    # output rows are merged on the host in block order (Chan), and the last step divides by n - ddof (W - ddof)
    stat, aggregate = ("mean_var", _mean_var_aggregate) if weights is None else ("mean_var_w", _mean_var_w_aggregate)
    backend, (x, mean, m2), bins, _ = _value_stat(stat, args, values, bins, range, axis, "histogram_mean_var",
                                                 partial(aggregate, ddof=ddof), weights=weights)
    return x, mean, (m2 if backend == "dask" else _var_of(x, m2, ddof)), bins


# ---------------------------------------------------------------------------------------------
# per-bin covariance of two value arrays
# ---------------------------------------------------------------------------------------------
def _value_pair(values, name, noun):
    """the (a, b) of ``values=`` in the covariance calls, or their TypeError.  `noun` says what the pair is made of: "arrays"
    here, "DataArrays" in xarray.py, which writes the pair in capitals and whose own type check answers a None"""
    if (isinstance(values, (str, bytes)) or not isinstance(values, (tuple, list)) or len(values) != 2
            or (noun == "arrays" and any(v is None for v in values))):
        raise TypeError("%s needs values=(%s), a pair of %s" % (name, "A, B" if noun == "DataArrays" else "a, b", noun))
    return values


def _cov_call(stat, name, args, a, b, weights, bins, range, axis, ddof):
    """histogram_cov and histogram_weighted_cov behind their own checks: the library's (x, mean_a, mean_b, M2_a, C_ab, M2_b)
    in the order of the public outputs, the moments divided by x - ddof (dask: by the last step of the merge)"""
    ddof = _check_ddof(ddof)
    backend, (x, ma, mb, qa, cc, qb), bins, _ = _value_stat(stat, args, a, bins, range, axis, name,
                                                           partial(_VALUE_STATS[stat].reduce, ddof=ddof), b, weights=weights)
    if backend == "dask":
        return x, ma, mb, qa, qb, cc, bins
    return x, ma, mb, _var_of(x, qa, ddof), _var_of(x, qb, ddof), _var_of(x, cc, ddof), bins


def combine_cov(n, mean_a, mean_b, m2_a, m2_b, c_ab, axis):
    """Merge partial (count, mean_a, mean_b, M2_a, M2_b, C_ab) results over `axis` (kept as axes of extent 1) with Chan's
    pairwise formula extended by the co-moment, one partial after another in index order (C order over several axes):
        n = n1 + n2,  da = mean_a2 - mean_a1,  db = mean_b2 - mean_b1,  mean = mean1 + d * n2 / n,
        M2 = M2_1 + M2_2 + d^2 * n1 * n2 / n,  C = C1 + C2 + da * db * n1 * n2 / n.
    Partials with n == 0 are skipped; where every partial is empty, the means and moments are NaN and n is 0.  The reduction
    of dask's partials.  Returns float64 (n, mean_a, mean_b, M2_a, M2_b, C_ab)."""
    return tuple(_merge_partials(partial(_chan_update, pairs=_COV_PAIRS), _counted, n, [mean_a, mean_b, m2_a, m2_b, c_ab], axis))


def histogram_cov(*args, values, bins=None, range=None, axis=None, ddof=0, block_size="auto"):
    """Per-bin count, means, variances and covariance of a pair of value arrays, computed on an MI355X: how two quantities move
    together inside each class that :func:`histogram` counts.

    ``args``, ``bins``, ``range`` and ``axis`` are those of :func:`histogram_mean_var`, and so are the counted samples and the
    edges (those of the unweighted ``histogram`` call: estimator names are allowed; the same digitize; NaN and out-of-range
    samples dropped).  ``values`` must be a pair ``(a, b)``; each broadcasts like ``values`` of ``histogram_mean_var``, may
    have any real dtype and is taken as float64.  The statistics are pairwise-complete: a counted sample contributes only if
    neither its ``a`` nor its ``b`` is NaN, so ``count`` plus the counted samples with a NaN in either value is ``histogram``'s
    count.  ``block_size`` is accepted and changes nothing.

    Two passes over the three arrays, the corrected two-pass form of ``histogram_mean_var``: ``n``, ``Sa = sum(a)`` and
    ``Sb = sum(b)`` of each bin, ``mean_a = Sa / n``, ``mean_b = Sb / n``; then ``da = a - mean_a``, ``db = b - mean_b`` in
    float64 and ``M2_a = max(0, sum(da**2) - sum(da)**2 / n)``, likewise ``M2_b``, and the co-moment
    ``C_ab = sum(da * db) - sum(da) * sum(db) / n``, which is not clamped: a covariance may be negative.  ``var_a = M2_a / (n -
    ddof)``, ``var_b = M2_b / (n - ddof)``, ``cov_ab = C_ab / (n - ddof)``.  The means are NaN where ``n == 0``, variances and
    covariance where ``n <= ddof``.  The default ``ddof=0`` is that of ``histogram_mean_var``, not ``np.cov``'s 1, so that the
    two calls agree: ``cov_ab`` with ``ddof=1`` is ``np.cov(a_bin, b_bin)[0, 1]``.  The correlation of a bin is ``cov_ab /
    sqrt(var_a * var_b)`` and the slope of the regression of ``b`` on ``a`` is ``cov_ab / var_a``, whatever ``ddof``.  Float64
    atomics add in arbitrary order, so the last bits can differ from run to run; data whose sums are exact in any order give
    the same bits every time.

    There is no ``weights`` parameter here: the weighted covariance is :func:`histogram_weighted_cov`.

    Returns ``(count, mean_a, mean_b, var_a, var_b, cov_ab, bin_edges)``: count int64, the others float64, with the shape
    ``histogram`` gives (kept axes, then bin axes).  numpy in -> numpy out, torch in -> torch out on the same device
    (asynchronous on the current stream), DeviceArray in -> numpy out, dask in -> lazy dask arrays, one task per block, the
    partials merged by :func:`combine_cov`."""
    a, b = _value_pair(values, "histogram_cov", "arrays")
    return _cov_call("cov", "histogram_cov", args, a, b, None, bins, range, axis, ddof)


def combine_weighted_cov(w, mean_a, mean_b, m2_a, m2_b, c_ab, axis):
    """Merge partial weighted (W, mean_a, mean_b, M2_a, M2_b, C_ab) results over `axis` (kept as axes of extent 1) with the
    weighted form of :func:`combine_cov`'s formula, one partial after another in index order (C order over several axes):
        W = W1 + W2,  da = mean_a2 - mean_a1,  db = mean_b2 - mean_b1,  mean = mean1 + d * W2 / W,
        M2 = M2_1 + M2_2 + d^2 * W1 * W2 / W,  C = C1 + C2 + da * db * W1 * W2 / W.
    Partials with W == 0 are skipped; a NaN partial (a NaN W among them) makes the bin NaN.  Where every partial has W == 0,
    the means and moments are NaN and W is 0.  The reduction of dask's weighted partials.  Returns float64 (W, mean_a, mean_b,
    M2_a, M2_b, C_ab)."""
    return tuple(_merge_partials(partial(_chan_update, pairs=_COV_PAIRS), _weighed, w, [mean_a, mean_b, m2_a, m2_b, c_ab], axis))


def histogram_weighted_cov(*args, values, weights, bins=None, range=None, axis=None, ddof=0, block_size="auto"):
    """Weighted per-bin means, variances and covariance of a pair of value arrays, computed on an MI355X: :func:`histogram_cov`
    with a weight per sample, e.g. the volume-weighted covariance of two tracers in each class, an area-weighted eddy flux, or
    the weighted regression slope ``cov_ab / var_a`` of ``b`` on ``a``.

    ``args``, ``bins``, ``range``, ``axis`` and ``values=(a, b)`` are those of :func:`histogram_cov`, and so are the counted
    samples, the edges (those of the unweighted ``histogram`` call) and the broadcasting.  ``weights`` broadcasts like the
    values, may have any real dtype and is taken as float64.  The statistics are pairwise-complete: a counted sample
    contributes its triple ``(w, a, b)`` only if neither ``a`` nor ``b`` is NaN, whatever its weight.  ``block_size`` is accepted
    and changes nothing.

    The weights are frequency weights, as in the weighted :func:`histogram_mean_var`.  Two passes over the four arrays:
    ``W = sum(w)``, ``mean_a = sum(w * a) / W``, ``mean_b = sum(w * b) / W``; then ``da = a - mean_a``, ``db = b - mean_b`` in
    float64 and ``M2_a = max(0, sum(w * da**2) - sum(w * da)**2 / W)``, likewise ``M2_b``, and the co-moment
    ``C_ab = sum(w * da * db) - sum(w * da) * sum(w * db) / W``, which is not clamped.  ``var_a = M2_a / (W - ddof)``,
    ``var_b = M2_b / (W - ddof)``, ``cov_ab = C_ab / (W - ddof)``.  With integer weights and ``ddof=1``, ``cov_ab`` is
    ``np.cov(a_bin, b_bin, fweights=w_bin)[0, 1]``; with any weights and ``ddof=0`` it is
    ``np.cov(a_bin, b_bin, aweights=w_bin, ddof=0)[0, 1]``.  With ``w == 1``, ``W`` is ``histogram_cov``'s count and every
    other output equals that call's.  The means and moments are NaN where ``W == 0`` (empty bins and bins whose weights sum to
    0), variances and covariance where ``W <= ddof``.  A NaN weight on a complete pair makes its bin NaN; on an incomplete pair
    it is dropped with the pair.  Zero weights contribute nothing (``0 * inf`` is NaN, as in ``np.average``).  Negative weights
    are not checked: the formulas apply, the clamp of the M2 at 0 included.  Float64 atomics add in arbitrary order, so the last
    bits can differ from run to run; data whose sums are exact in any order give the same bits every time.

    Returns ``(sum_of_weights, mean_a, mean_b, var_a, var_b, cov_ab, bin_edges)``, all float64, with the shape ``histogram``
    gives (kept axes, then bin axes).  numpy in -> numpy out, torch in -> torch out on the same device (asynchronous on the
    current stream), DeviceArray in -> numpy out, dask in -> lazy dask arrays, one task per block, the partials merged by
    :func:`combine_weighted_cov`."""
    a, b = _value_pair(values, "histogram_weighted_cov", "arrays")
    if weights is None:
        raise TypeError("histogram_weighted_cov needs weights")
    return _cov_call("cov_w", "histogram_weighted_cov", args, a, b, weights, bins, range, axis, ddof)


# ---------------------------------------------------------------------------------------------
# per-bin skewness and kurtosis of a value array
# ---------------------------------------------------------------------------------------------
def _check_flag(name, v):
    if not isinstance(v, (bool, np.bool_)):
        raise TypeError("%s must be a bool, got %r" % (name, v))
    return bool(v)


def _pebay_update(cx, xb, tot, cur, part):
    """Pébay's update of running (mean, M2, M3, M4): mean and M2 by _chan_update's very expressions (so they have its bits), M3
    and M4 by the update of :func:`combine_skew_kurt`"""
    (cm, c2, c3, c4), (mean, m2, m3, m4) = cur, part
    d = mean - cm
    return [cm + d * xb / tot,
            c2 + m2 + d * d * cx * xb / tot,
            (c3 + m3 + d * d * d * cx * xb * (cx - xb) / (tot * tot)
             + 3.0 * d * (cx * m2 - xb * c2) / tot),
            (c4 + m4 + d * d * d * d * cx * xb * (cx * cx - cx * xb + xb * xb) / (tot * tot * tot)
             + 6.0 * d * d * (cx * cx * m2 + xb * xb * c2) / (tot * tot)
             + 4.0 * d * (cx * m3 - xb * c3) / tot)]


def combine_skew_kurt(n, mean, m2, m3, m4, axis):
    """Merge partial (count, mean, M2, M3, M4) results over `axis` (kept as axes of extent 1) with Pébay's pairwise update, one
    partial after another in index order (C order over several axes), as :func:`combine_mean_var` walks them.  With
    ``d = mb - ma`` and ``n = na + nb``: ``mean`` and ``M2`` by :func:`combine_mean_var`'s expressions (bit for bit its
    results), and
        M3 = M3a + M3b + d^3 na nb (na - nb) / n^2 + 3 d (na M2b - nb M2a) / n,
        M4 = M4a + M4b + d^4 na nb (na^2 - na nb + nb^2) / n^3 + 6 d^2 (na^2 M2b + nb^2 M2a) / n^2 + 4 d (na M3b - nb M3a) / n.
    Partials with n == 0 are skipped; where every partial is empty, the mean and the moments are NaN and n is 0.  The reduction
    of dask's partials.  Returns float64 (n, mean, M2, M3, M4)."""
    return tuple(_merge_partials(_pebay_update, _counted, n, [mean, m2, m3, m4], axis))


def combine_weighted_skew_kurt(w, mean, m2, m3, m4, axis):
    """:func:`combine_skew_kurt` for weighted partials (W, mean, M2, M3, M4), W in the place of n: partials with W == 0 are
    skipped; a NaN partial (a NaN W among them) makes the bin NaN, as in :func:`combine_weighted_mean_var`, whose W, mean and M2
    these are bit for bit.  Returns float64 (W, mean, M2, M3, M4)."""
    return tuple(_merge_partials(_pebay_update, _weighed, w, [mean, m2, m3, m4], axis))


def _skew_kurt_of(x, m2, m3, m4, bias, fisher):
    """(skew, kurt) of numpy arrays or torch tensors from the central moments' sums, x the count or the sum of weights:
    g1 = (M3 / x) / (m2 sqrt(m2)), g2 = (M4 / x) / (m2 m2) with m2 = M2 / x, NaN where x == 0 or M2 == 0; bias=False applies
    scipy's sample corrections with x for n, NaN where x <= 2 (skew) and x <= 3 (kurt)"""
    if _is_torch(m2):
        xp = _torch()
        xf = x.to(xp.float64)
    else:
        xp = np
        xf = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nan = xp.full_like(m2, float("nan"))
        v = m2 / xf
        ok = (xf != 0) & (m2 != 0)
        skew = xp.where(ok, (m3 / xf) / (v * xp.sqrt(v)), nan)
        kurt = xp.where(ok, (m4 / xf) / (v * v), nan)
        if not bias:
            skew = xp.where(xf <= 2, nan, xp.sqrt(xf * (xf - 1.0)) / (xf - 2.0) * skew)
            kurt = xp.where(xf <= 3, nan, (xf - 1.0) / ((xf - 2.0) * (xf - 3.0)) * ((xf + 1.0) * kurt - 3.0 * (xf - 1.0)) + 3.0)
        if fisher:
            kurt = kurt - 3.0
    return skew, kurt


def _moment_reduce(x, axis=None, keepdims=True, pairs=((0, 0),), present=_counted, ddof=None, final=None, **_):
    """dask.array.reduction step over stacked blocks of partials in the order the library emits them: x, the means, then the
    moments, `pairs` naming each moment's means as _chan_update reads them; pairs=None: (x, mean, M2, M3, M4), merged by
    _pebay_update.  The last step, here only, has ddof (the moments divided by x - ddof) or, for Pébay's blocks,
    final = (ddof, bias, fisher) (the moments turned into var, skew and kurt)."""
    ax = tuple(int(a) for a in (axis if isinstance(axis, tuple) else (axis,)))
    update = _pebay_update if pairs is None else partial(_chan_update, pairs=pairs)
    out = np.stack(_merge_partials(update, present, x[0], x[1:], tuple(a - 1 for a in ax)))
    out = out if keepdims else out.squeeze(ax)
    moments = _range(len(out) - len(pairs), len(out)) if pairs else (2,)
    if final is not None:
        ddof, bias, fisher = final
        out[3], out[4] = _skew_kurt_of(out[0], out[2], out[3], out[4], bias, fisher)
    if ddof is not None:
        for i in moments:
            out[i] = _var_of(out[0], out[i], ddof)
    return out


def histogram_skew_kurt(*args, values, bins=None, range=None, axis=None, weights=None, ddof=0, bias=True, fisher=True,
                        block_size="auto"):
    """Per-bin count, mean, variance, skewness and kurtosis of ``values``, computed on an MI355X: the shape of the distribution
    inside each class :func:`histogram` counts, as ``scipy.stats.skew`` / ``scipy.stats.kurtosis`` give it for the values of a
    bin (``nan_policy="omit"``).

    The samples, the edges and the broadcasting, the NaN-value rule (a counted sample contributes when its value is not NaN),
    the dtype rules (``values`` and ``weights`` of any real dtype, taken as float64), the backends (numpy in -> numpy out,
    torch in -> torch out on the same device and asynchronous on the current stream, DeviceArray in -> numpy out, dask in ->
    lazy dask arrays) and ``block_size`` (accepted, changes nothing) are those of :func:`histogram_mean_var`.

    Write ``x`` for the count ``n``, or for ``W = sum(w)`` with ``weights`` (frequency weights, as in the weighted
    ``histogram_mean_var``).  Two passes over the data: pass 1 is ``histogram_mean_var``'s (``x`` and ``mean``); pass 2 forms
    ``d = v - mean`` in float64 and the terms ``t1 = d`` (weighted ``w * d``), ``t2 = t1 * d``, ``t3 = t2 * d``, ``t4 = t3 * d``
    in this order of products, and adds ``D = sum(t1)``, ``Q2 = sum(t2)``, ``Q3 = sum(t3)``, ``Q4 = sum(t4)``.  With
    ``delta = D / x`` the corrected two-pass formula carried to the fourth order gives
        M2 = max(0, Q2 - D * D / x)                       (``histogram_mean_var``'s M2, bit for bit on equal sums)
        M3 = Q3 - 3 delta Q2 + 2 x delta^3                (not clamped)
        M4 = max(0, Q4 - 4 delta Q3 + 6 delta^2 Q2 - 3 x delta^4).
    The sums keep the digits that the raw moments ``sum(v^k) / n`` cancel away when ``|mean| >> std``.

    ``var = M2 / (x - ddof)``, NaN where ``x <= ddof``.  With ``m2 = M2 / x``: ``g1 = (M3 / x) / (m2 sqrt(m2))`` and
    ``g2 = (M4 / x) / (m2 m2)``, both NaN where ``x == 0`` or ``M2 == 0`` (a constant bin is ``0 / 0``).  ``skew = g1`` and
    ``kurt = g2 - 3`` (``fisher=False``: ``kurt = g2``).  ``bias=False`` applies scipy's sample corrections with ``x`` in the
    place of ``n``: ``G1 = sqrt(x (x - 1)) / (x - 2) g1`` and ``G2 = (x - 1) / ((x - 2) (x - 3)) ((x + 1) g2 - 3 (x - 1)) + 3``
    (minus 3 under ``fisher``).  scipy keeps the biased value where the count is too small for the correction; here ``G1`` is
    NaN where ``x <= 2`` and ``G2`` where ``x <= 3``, as ``ddof`` gives NaN everywhere in this library.  A NaN weight makes its
    bin NaN; zero weights contribute nothing; negative weights are not checked.  Float64 atomics add in arbitrary order, so the
    last bits can differ from run to run; data whose sums are exact in any order give the same bits every time.

    Returns ``(count, mean, var, skew, kurt, bin_edges)``: count int64, the others float64, with the shape ``histogram`` gives;
    with ``weights`` the first output is the float64 ``sum_of_weights``.  dask merges the blocks' partials with
    :func:`combine_skew_kurt` (:func:`combine_weighted_skew_kurt`)."""
    ddof = _check_ddof(ddof)
    bias = _check_flag("bias", bias)
    fisher = _check_flag("fisher", fisher)
    stat, reduce_ = ("skew_kurt", _skew_kurt_reduce) if weights is None else ("skew_kurt_w", _skew_kurt_w_reduce)
    backend, (x, mean, m2, m3, m4), bins, _ = _value_stat(stat, args, values, bins, range, axis, "histogram_skew_kurt",
                                                         partial(reduce_, final=(ddof, bias, fisher)), weights=weights)
    if backend == "dask":  # (the last step of the merge has turned the moments into var, skew and kurt)
        return x, mean, m2, m3, m4, bins
    skew, kurt = _skew_kurt_of(x, m2, m3, m4, bias, fisher)
    return x, mean, _var_of(x, m2, ddof), skew, kurt, bins


# The dask steps of the moment statistics: partials of a module-level function, so that dask can pickle them.  The blocks of
# the two covariances keep the order of the library's outputs; an aggregate is the last step, (x, mean, var).
_mean_var_reduce = partial(_moment_reduce, present=_counted)
_mean_var_aggregate = partial(_moment_reduce, present=_counted, ddof=0)
_mean_var_w_reduce = partial(_moment_reduce, present=_weighed)
_mean_var_w_aggregate = partial(_moment_reduce, present=_weighed, ddof=0)
_cov_reduce = partial(_moment_reduce, present=_counted, pairs=_COV_BLOCK_PAIRS)
_cov_w_reduce = partial(_moment_reduce, present=_weighed, pairs=_COV_BLOCK_PAIRS)
_skew_kurt_reduce = partial(_moment_reduce, present=_counted, pairs=None)
_skew_kurt_w_reduce = partial(_moment_reduce, present=_weighed, pairs=None)

_VALUE_STATS = {
    "extrema": _ValueStat(2, (), "execute_extrema", (0, 1), 0, _extrema_pair_reduce),
    # (count, total): integer accumulators of several chunks are not kept, so there is no merge
    "sum": _ValueStat(2, (0,), "execute_sum", (0, 1), 0, None, noun="reproducible sums", max_cols=_ORDER_MAX_COLS),
    # (vmin, vmax, argmin, argmax): the library takes the block of values and the block of positions
    "argextrema": _ValueStat(4, (2, 3), "execute_argextrema", (0, 2), 0, None, ordered=True, noun="positions"),
    "mean_var": _ValueStat(3, (0,), "execute_mean_var", (0, 1, 2), 0, _mean_var_reduce),
    "mean_var_w": _ValueStat(3, (), "execute_mean_var_weighted", (0, 1, 2), 1, _mean_var_w_reduce),
    # (x, mean_a, mean_b, M2_a, C_ab, M2_b): the library takes x, the block of means and the block of moments
    "cov": _ValueStat(6, (0,), "execute_cov", (0, 1, 3), 1, _cov_reduce),
    "cov_w": _ValueStat(6, (), "execute_cov_weighted", (0, 1, 3), 2, _cov_w_reduce),
    # (x, mean, M2, M3, M4): the library takes x, the mean and the block of three moments
    "skew_kurt": _ValueStat(5, (0,), "execute_skew_kurt", (0, 1, 2), 0, _skew_kurt_reduce),
    "skew_kurt_w": _ValueStat(5, (), "execute_skew_kurt_weighted", (0, 1, 2), 1, _skew_kurt_w_reduce),
    # one output per element of the call's q, in one block
    "quantile": _ValueStat(None, (), "execute_quantile", (0,), 0, None, ("q", "code"), noun="exact quantiles"),
    "quantile_w": _ValueStat(None, (), "execute_quantile_weighted", (0,), 1, None, ("q",), noun="exact quantiles"),
    # (count, nunique, mode, mode_count): the runs of several chunks are not kept, so there is no merge
    "mode": _ValueStat(4, (0, 1, 3), "execute_mode", (0, 1, 2, 3), 0, None, noun="modes", max_cols=_ORDER_MAX_COLS,
                       max_bins=_SORT_MAX_BINS),
}

# The statistics behind the sorted order that read weights: (count, nunique, mode, mode_weight).  They are entries of the same
# kind and take the same path (_stat_entry looks in both); they are kept beside _VALUE_STATS only because that table's keys and
# its entries with a size limit are pinned by the CPU tests of the earlier statistics, which a new feature leaves as they are.
# Once those tests list the weighted twins, this dict folds into the table above.
_SORTED_WEIGHTED_STATS = {
    "mode_w": _ValueStat(4, (0, 1), "execute_mode_weighted", (0, 1, 2, 3), 1, None, noun="modes", max_cols=_ORDER_MAX_COLS,
                         max_bins=_SORT_MAX_BINS),
}


def _stat_entry(stat):
    return _SORTED_WEIGHTED_STATS[stat] if stat in _SORTED_WEIGHTED_STATS else _VALUE_STATS[stat]


# ---------------------------------------------------------------------------------------------
# per-bin quantiles of a value array
# ---------------------------------------------------------------------------------------------
def _check_quantile_args(q, method):
    """(q as a 1-D float64 array, whether q was a scalar, the method's code), checked as np.nanquantile checks them"""
    if method not in _native.QUANTILE_METHODS:
        raise ValueError("method must be one of %s, got %r" % (", ".join(repr(m) for m in _native.QUANTILE_METHODS), method))
    qa = np.asanyarray(q)
    if qa.dtype.kind == "c" or qa.dtype.kind not in "fiub":
        raise TypeError("q must be a float or a 1-D array-like of floats, got dtype %s" % qa.dtype)
    if qa.ndim > 1:
        raise ValueError("q must be a float or a 1-D array-like, got %d dimensions" % qa.ndim)
    qf = qa.astype(np.float64).ravel()
    if not (np.all(qf >= 0) and np.all(qf <= 1)):  # (NaN fails both)
        raise ValueError("Quantiles must be in the range [0, 1]")
    return qf, qa.ndim == 0, _native.QUANTILE_METHODS.index(method)


def histogram_quantile(*args, values, q, bins=None, range=None, axis=None, method="linear", block_size="auto", weights=None,
                       density=None):
    """Per-bin quantiles of ``values``, computed exactly on an MI355X: every element is what
    ``np.nanquantile(values_in_that_bin.astype(np.float64), q, method=method)`` gives, bit for bit (``method="linear"`` with
    ``q=0.5`` is ``scipy.stats.binned_statistic``'s ``"median"``).  A bin with no non-NaN value gives NaN.

    ``args``, ``bins``, ``range``, ``axis`` and ``values`` are those of :func:`histogram_mean_var`: a sample counts when
    ``histogram`` counts it and its value is not NaN; the edges are those of the unweighted ``histogram``.  ``q`` is a float or a
    1-D array-like in [0, 1] (taken as float64), ``method`` one of ``"linear"``, ``"lower"``, ``"higher"``, ``"midpoint"``,
    ``"nearest"``.  ``weights`` (see :func:`histogram_weighted_quantile`) and ``density`` are not taken.  ``block_size`` is accepted and changes nothing.

    Rows of at most 4096 values are sorted in LDS; longer rows take an exact radix select over order-preserving keys of the
    values in a fixed number of streaming passes (about 9 for float64 values).

    Returns ``(quantiles, bin_edges)``: float64 with the shape ``histogram`` gives (kept axes, then bin axes), behind a leading
    ``len(q)`` axis when ``q`` is 1-D (numpy's convention).  numpy in -> numpy out, torch in -> torch out on the same device
    (asynchronous on the current stream), DeviceArray in -> numpy out, dask in -> a lazy dask array, one task per block: every
    reduced axis must then be a single chunk."""
    if weights is not None:
        raise TypeError("histogram_quantile does not take weights: weighted quantiles are histogram_weighted_quantile's")
    if density is not None:
        raise TypeError("histogram_quantile does not take density")
    qf, scalar, code = _check_quantile_args(q, method)
    _, res, bins, _ = _value_stat("quantile", args, values, bins, range, axis, "histogram_quantile", q=qf, code=code)
    return (res[0] if scalar else res), bins


# ---------------------------------------------------------------------------------------------
# weighted per-bin quantiles of a value array
# ---------------------------------------------------------------------------------------------
def histogram_weighted_quantile(*args, values, weights, q, bins=None, range=None, axis=None, method="inverted_cdf",
                                block_size="auto"):
    """Weighted per-bin quantiles of ``values``, computed on an MI355X: what
    ``np.nanquantile(values_in_that_bin.astype(np.float64), q, weights=weights_in_that_bin, method="inverted_cdf")`` gives.

    ``args``, ``bins``, ``range``, ``axis``, ``values`` and ``q`` are those of :func:`histogram_quantile`: a sample counts when
    ``histogram`` counts it and its value is not NaN; the edges are those of the unweighted ``histogram``.  ``weights`` (any real
    dtype, taken as float64) broadcasts against the inputs as ``values`` does.  ``method`` accepts only ``"inverted_cdf"``, the
    one method numpy defines with weights.  ``block_size`` is accepted and changes nothing.

    Per (row, bin, q): with ``C(x)`` the float64 sum of the weights of the bin's values ``<= x`` (ordered as
    ``histogram_quantile`` orders them, ``-0.0 < +0.0``) and ``W`` the sum of all of them, the result is the smallest value
    ``x`` of the bin with ``C(x) / W >= q`` (one float64 division) and ``C(x) > 0`` — numpy's
    ``cdf /= cdf[-1]; searchsorted(cdf, q, "left")``, which skips leading zero weights at ``q = 0`` — or the largest value of
    positive weight if rounding leaves none.  The value returned always carries positive weight itself.  The result is NaN
    where the bin has no value or ``W`` is not finite and positive, and a weight that is NaN or negative makes its own bin NaN
    (numpy raises for negative weights and gives no meaningful answer for NaN weights or ``W = 0``; device data cannot be
    checked without a synchronisation).  A NaN value contributes nothing, whatever its weight.

    On weights whose float64 sums are exact in any order (fewer than 2^28 samples per bin) every element equals numpy's bit
    for bit; zero results compare by value (numpy keeps the input order of ``-0.0`` and ``+0.0``).  On other weights the
    float64 atomics add in arbitrary order, which moves ``C`` and ``W`` in their last bits: the result may then be a
    neighbouring value of the bin, one whose cdf values bracket ``q`` within ``2 * gamma(n) + 2**-51`` (``gamma(n)`` the
    any-order summation bound of the bin's ``n`` samples), and two runs may differ in the same way.

    Rows of at most 2048 values are sorted in LDS with their weights; longer rows take a radix select over the values' keys
    with per-digit sums of weights, in a fixed number of streaming passes.

    Returns ``(quantiles, bin_edges)``: float64 with the shape ``histogram`` gives (kept axes, then bin axes), behind a leading
    ``len(q)`` axis when ``q`` is 1-D.  numpy in -> numpy out, torch in -> torch out on the same device (asynchronous on the
    current stream), DeviceArray in -> numpy out, dask in -> a lazy dask array, one task per block: every reduced axis must
    then be a single chunk."""
    if method != "inverted_cdf":
        raise ValueError("Only method 'inverted_cdf' supports weights. Got: %s." % (method,))
    if weights is None:
        raise TypeError("histogram_weighted_quantile needs weights")
    qf, scalar, _ = _check_quantile_args(q, "linear")
    _, res, bins, _ = _value_stat("quantile_w", args, values, bins, range, axis, "histogram_weighted_quantile", weights=weights, q=qf)
    return (res[0] if scalar else res), bins


# ---------------------------------------------------------------------------------------------
# per-sample maps: from a per-bin result back to the samples
# ---------------------------------------------------------------------------------------------
def _map_out(rec, has_values, op, centre_ptr, scale_ptr):
    """xhist_plan_execute_map over the `ordered` launch `rec` (samples..., then the values where `has_values`), one element
    per sample"""
    n = rec.plan.n_dims

    def run(ptrs):
        rec.plan.execute_map(rec.nv[:n], rec.nv[n] if has_values else None, rec.m, rec.c, op, centre_ptr, scale_ptr, ptrs[0],
                             stream=rec.stream)

    return _sample_block(rec, np.int64 if op == _native.MAP_INDEX else np.float64, run)


def _sample_block(rec, dtype, run):
    """the [m, c] block that `run([pointer])` has the kernels write, one element per sample of the `ordered` launch `rec`, in
    the broadcast sample shape"""
    return _sample_shape(_launch_outputs(rec, [((rec.m, rec.c), dtype)], run)[0], _shape_of(rec.like), rec.kept, rec.red, rec.backend)


def _sample_shape(out, shape, kept, red, backend):
    """a dense [rows, cols] block, its rows the kept axes in C order and a row's columns the reduced axes in ascending number,
    in the broadcast sample shape `shape`: reshaped, and its axes moved back where the reduced axes are not trailing"""
    ndim = len(shape)
    out = out.reshape([shape[i] for i in kept] + [shape[i] for i in red])
    if kept and tuple(red) != tuple(_range(len(kept), ndim)):
        back = tuple(_range(len(kept), ndim))
        out = out.movedim(back, tuple(red)) if backend == "torch" else np.moveaxis(out, back, red)
    return out


def _table_on_device(table, rows, n_bins, backend, like, device):
    """a per-bin table as contiguous float64 [rows, n_bins] on the samples' device: (what keeps it alive, its pointer)"""
    if backend == "torch":
        torch = _torch()
        t = table if _is_torch(table) else torch.as_tensor(np.array(table, dtype=np.float64, order="C"))  # (a copy: torch takes no read-only arrays)
        t = t.to(device=like.device, dtype=torch.float64).reshape(rows, n_bins).contiguous()
        return t, t.data_ptr()
    if _is_devarr(table):  # (already resident: converted and made contiguous on the device)
        t = table.to(device).astype(np.float64).contiguous().reshape(rows, n_bins)
        return t, t.ptr
    host = table.detach().cpu().numpy() if _is_torch(table) else np.asarray(table)
    host = np.ascontiguousarray(host, np.float64).reshape(rows, n_bins)
    buf = _native.DeviceBuffer(device, max(host.nbytes, 8))
    if host.nbytes:
        buf.upload(host)
    return buf, buf.ptr


def _bins_shape_if_known(bins, n_inputs):
    """the number of bins per input where it can be told before the edges are made (None: an estimator's name)"""
    out = []
    for b in _ensure_correctly_formatted_bins(bins, n_inputs):
        if isinstance(b, str):
            out.append(None)
        elif np.ndim(b) == 0:
            out.append(int(b))
        else:
            out.append(max(len(b) - 1, 0))
    return out


def _check_table_shape(table, sample_shape, drop_axes, n_per_input):
    """ValueError unless `table` has the shape ``histogram`` gives: kept axes, then bin axes (None: any extent)"""
    want = [int(s) for i, s in enumerate(sample_shape) if i not in drop_axes] + list(n_per_input)
    got = _shape_of(table)
    if len(got) != len(want) or any(w is not None and g != w for g, w in zip(got, want)):
        raise ValueError("table has shape %s, but histogram gives %s for these arguments (kept axes, then bin axes)"
                         % (got, tuple("?" if w is None else w for w in want)))


def _shape_of(a):
    return tuple(int(s) for s in (a.shape if hasattr(a, "shape") else np.shape(a)))


# what _sample_call returns: the caller's backend; the broadcast arrays (samples..., values, extras...), resident on a GPU
# unless they are dask arrays; `on`, the backend _value_views takes them as; the edges, the normalised axis and the reduced
# axes; and, for the grouped calls, the samples per output row and the number of bins
_SampleCall = namedtuple("_SampleCall", "backend arrays on bins axis drop_axes cols n_bins")


def _sample_call(name, args, values, bins, range, axis, *extras, needs_values=True, check=None, noun=None, max_bins=None):
    """The front of the functions that return something per sample or per row, all of it before any device work: the caller's
    own `check`, _values_call (`needs_values` False and values None: the samples alone) and, for the calls that group the
    samples by bin (`noun`: what dask chunks of theirs cannot be merged), the refusals of complex samples, of 2^31 samples or
    more per output row, of more than `max_bins` bins (None: no bound here) and of dask inputs whose reduced axes are cut.
    Then numpy inputs are uploaded, once.  Returns a _SampleCall."""
    if check is not None:
        check()
    if noun is not None:
        for a in args:
            dt = a.dtype if hasattr(a, "dtype") else np.asarray(a).dtype
            if getattr(dt, "is_complex", False) or getattr(dt, "kind", "") == "c":
                raise TypeError("complex samples have no order: %s takes real samples" % name)
    if values is not None and not hasattr(values, "dtype"):
        values = np.asarray(values)
    backend, arrays, raw, bins, axis, drop_axes = _values_call(args, values, bins, range, axis, name, *extras, needs_values=needs_values)
    cols = n_bins = None
    if noun is not None:
        cols, n_bins = _check_sizes(name, arrays[0].shape, drop_axes, bins, _ORDER_MAX_COLS, max_bins)
        if backend == "dask":
            _check_one_chunk(noun, arrays, drop_axes)
    on = backend
    if backend != "dask":
        arrays, on = _resident(backend, raw, arrays, len(args), bins)
    return _SampleCall(backend, arrays, on, bins, axis, drop_axes, cols, n_bins)


def _sample_blockwise(block_fn, arrays, dtype, *extra, **params):
    """dask: one task per block of the broadcast `arrays`, each `block_fn`'s output on the samples' own index; `extra` are
    further (operand, index) pairs"""
    import dask.array as dsa

    ind = tuple(_range(arrays[0].ndim))
    return dsa.blockwise(block_fn, ind, *[x for a in arrays for x in (a, ind)], *extra, dtype=dtype, meta=np.array((), dtype),
                         **params)


def _bin_index_block(*blocks, bins=None):
    return bin_index(*blocks, bins=bins)[0]


def bin_index(*args, bins=None, range=None):
    """The bin of every sample, computed on an MI355X: the intermediate ``digitize -> ravel_multi_index`` that ``histogram``
    counts and never shows.

    ``args``, ``bins`` and ``range`` are those of :func:`histogram` (estimator names are allowed: the edges are those of the
    unweighted ``histogram`` call, and they do not depend on the row, so there is no ``axis``).  ``index`` is int64 in the
    broadcast shape of ``args``: for a sample ``histogram`` counts, the C-order flat index over the histogram's bin axes,
    ``np.ravel_multi_index(per-input bins, bins_shape)`` (the same digitize: last bin closed on the right, int64 / datetime
    and mixed compare domains, joint bins of up to 8 inputs); ``-1`` for every sample it does not count (NaN, outside
    ``[e_0, e_last]`` in any input).  So ``np.bincount(index[index >= 0], minlength=n_bins).reshape(bins_shape)`` is
    ``histogram(*args, bins=bins)[0]``, and ``index`` serves ``np.take`` and ``torch.gather`` as the positions of
    :func:`histogram_argextrema` do.

    Returns ``(index, bin_edges)``.  numpy in -> numpy out, torch in -> torch out on the same device (asynchronous on the
    current stream), DeviceArray in -> numpy out, dask in -> a lazy dask array, one task per block (``bins`` must then be
    numpy arrays of edges)."""
    f = _sample_call("bin_index", args, None, bins, range, None, needs_values=False)
    if f.backend == "dask":
        return _sample_blockwise(_bin_index_block, f.arrays, np.int64, bins=f.bins), f.bins
    rec = _value_views(f.arrays, None, None, f.bins, f.on, ordered=True)
    return _map_out(rec, False, _native.MAP_INDEX, 0, 0), f.bins


def _lookup_block(*blocks, axis=None, bins=None):
    return histogram_lookup(*blocks[:-1], table=blocks[-1], bins=bins, axis=axis)[0]


def histogram_lookup(*args, table, bins=None, range=None, axis=None):
    """A per-bin table read back at every sample, computed on an MI355X: ``out[s] = table[kept index of s, bin of s]`` — the
    map of each grid point's class mean, or of any per-bin result of this library.

    ``args``, ``bins``, ``range`` and ``axis`` are those of :func:`histogram`, and the bin of a sample is the one
    :func:`bin_index` gives.  ``table`` (any real dtype, taken as float64) has the shape ``histogram`` gives for these ``args``
    and ``axis``: kept axes, then bin axes.  ``out`` is float64 in the broadcast shape of ``args``; a sample ``histogram`` does
    not count reads NaN.  A table of another shape raises ``ValueError`` and a complex or non-real one ``TypeError``, both
    before any device work.

    Returns ``(out, bin_edges)``.  numpy in -> numpy out, torch in -> torch out on the same device (asynchronous on the current
    stream), DeviceArray in -> numpy out, dask in -> a lazy dask array, one task per block of samples: the table is then a
    dask array chunked like the samples along the kept axes, with every bin axis in one chunk."""
    if table is None:
        raise TypeError("histogram_lookup needs a table")
    if not args:
        raise TypeError("histogram_lookup needs at least one array of samples")
    if not hasattr(table, "shape"):
        table = np.asarray(table)  # (a plain sequence, taken as numpy takes it)
    _check_values_dtype(table, "histogram_lookup")
    ndim = len(np.broadcast_shapes(*[_shape_of(a) for a in args]))
    early_axis = _normalise_axis(axis, ndim)
    _check_table_shape(table, np.broadcast_shapes(*[_shape_of(a) for a in args]),
                       tuple(early_axis) if early_axis is not None else tuple(_range(ndim)), _bins_shape_if_known(bins, len(args)))
    if _is_dask(table) and not any(_is_dask(a) for a in args):
        import dask.array as dsa

        if any(_is_torch(a) or _is_devarr(a) for a in args):
            raise TypeError("a dask table goes with dask or numpy samples: compute the table, or pass the samples as dask arrays")
        args = [dsa.from_array(np.asarray(a), chunks=-1) for a in args]
    f = _sample_call("histogram_lookup", args, None, bins, range, axis, needs_values=False)
    arrays, bins, axis = f.arrays, f.bins, f.axis
    shape = _shape_of(arrays[0])
    _check_table_shape(table, shape, f.drop_axes, [len(b) - 1 for b in bins])
    if f.backend == "dask":
        import dask.array as dsa

        kept = tuple(i for i in _range(len(shape)) if i not in f.drop_axes)
        t_ind = kept + tuple(_range(len(shape), len(shape) + len(bins)))
        # the table's blocks are the sample blocks' along the kept axes, and every bin axis is one chunk
        t_chunks = tuple(arrays[0].chunks[i] for i in kept) + (-1,) * len(bins)
        table = table.rechunk(t_chunks) if _is_dask(table) else dsa.from_array(np.asarray(table), chunks=t_chunks)
        return _sample_blockwise(_lookup_block, arrays, np.float64, table, t_ind, concatenate=True, axis=axis, bins=bins), bins
    rec = _value_views(arrays, None, axis, bins, f.on, ordered=True)
    keep, ptr = _table_on_device(table, rec.m, rec.plan.n_bins, f.on, arrays[0], rec.device)  # (`keep` outlives the launch)
    return _map_out(rec, False, _native.MAP_TAKE, ptr, 0), bins


def histogram_anomaly(*args, values, bins=None, range=None, axis=None, weights=None, ddof=0, standardize=False):
    """Every sample's value relative to the mean of its bin, computed on an MI355X: "oxygen anomaly relative to the mean of
    its T-S class", and with ``standardize=True`` its z-score.

    ``args``, ``values``, ``bins``, ``range``, ``axis``, ``weights`` and ``ddof`` are those of :func:`histogram_mean_var`, whose
    kernels compute ``mean`` and ``var`` here as they do there; the tables stay on the device.  ``anomaly`` is float64 in the
    broadcast shape of the inputs: ``float64(v) - mean[bin]``, one IEEE subtraction, and with ``standardize=True``
    ``(float64(v) - mean[bin]) / sqrt(var[bin])``, an IEEE division.  A sample ``histogram`` does not count gives NaN and a NaN
    value stays NaN; everything else is what IEEE gives (``var = 0``: ``+-inf`` or NaN; a bin whose variance is NaN because
    ``n <= ddof``: NaN).  numpy inputs are uploaded once, for both steps.

    Returns ``(anomaly, bin_edges)``.  numpy in -> numpy out, torch in -> torch out on the same device (asynchronous on the
    current stream), DeviceArray in -> numpy out, dask in -> a lazy dask array: the lazy ``histogram_mean_var`` composed with
    :func:`histogram_lookup`."""
    ddof = _check_ddof(ddof)
    standardize = _check_flag("standardize", standardize)
    n = len(args)
    f = _sample_call("histogram_anomaly", args, values, bins, range, axis, weights)
    arrays, on, bins, axis = f.arrays, f.on, f.bins, f.axis
    if f.backend == "dask":
        import dask.array as dsa

        _, mean, var, _ = histogram_mean_var(*arrays[:n], values=arrays[n], bins=bins, axis=axis, ddof=ddof,
                                             weights=arrays[n + 1] if weights is not None else None)
        out = arrays[n].astype(np.float64) - histogram_lookup(*arrays[:n], table=mean, bins=bins, axis=axis)[0]
        if standardize:
            out = out / histogram_lookup(*arrays[:n], table=dsa.sqrt(var), bins=bins, axis=axis)[0]
        return out, bins
    st = _VALUE_STATS["mean_var" if weights is None else "mean_var_w"]
    rec = _value_views(arrays[:n], arrays[n], axis, bins, on, *arrays[n + 1:], ordered=True)
    plan, nv, m, c, device, stream = rec.plan, rec.nv, rec.m, rec.c, rec.device, rec.stream
    nt = m * plan.n_bins
    # the block (count or sum of weights, mean, M2) of histogram_mean_var's own call, on the device
    if on == "torch":
        torch = _torch()
        stats = torch.empty((3, m, plan.n_bins), dtype=torch.float64, device=arrays[0].device)
        base = stats.data_ptr()
    else:
        stats = _native.DeviceBuffer(device, max(3 * nt * 8, 8))
        base = stats.ptr
    if nt > 0:
        getattr(plan, st.method)(nv[:n], *nv[n:], m, c, base, base + nt * 8, base + 2 * nt * 8, stream=stream)
    scale, scale_ptr = None, 0
    if standardize:
        # sqrt(var) as histogram_mean_var's callers form it; for numpy and DeviceArray inputs the count and M2 tables (bins, not
        # samples) pass through the host for that, the means never leave the device
        if on == "torch":
            x = stats[0].view(torch.int64) if 0 in st.ints else stats[0]
            scale, scale_ptr = _table_on_device(torch.sqrt(_var_of(x, stats[2], ddof)), m, plan.n_bins, on, arrays[0], device)
        else:
            host = np.empty((3, m, plan.n_bins), np.float64)
            if nt > 0:
                stats.download(host)
            x = host[0].view(np.int64) if 0 in st.ints else host[0]
            with np.errstate(invalid="ignore"):
                scale, scale_ptr = _table_on_device(np.sqrt(_var_of(x, host[2], ddof)), m, plan.n_bins, on, arrays[0], device)
    # (`stats` and `scale` outlive the launch)
    return _map_out(rec, True, _native.MAP_ANOMALY, base + nt * 8, scale_ptr), bins


# ---------------------------------------------------------------------------------------------
# histogram_mode: per-bin mode, its count and the number of distinct values
# ---------------------------------------------------------------------------------------------
def histogram_mode(*args, values, bins=None, range=None, axis=None, weights=None, block_size="auto"):
    """Per-bin most frequent value of ``values``, how often it occurs and how many different values there are, computed on an
    MI355X: the statistic of categorical values (water-mass class, land-cover type, cloud regime, a quality flag, any rounded
    field), for which a mean is meaningless.  ``scipy.stats.mode`` or ``np.unique`` on each of ``np.split(v[order], offsets)``
    on the host, ``pandas.Series.groupby(bin).agg(["nunique", mode])``.

    ``args``, ``bins``, ``range``, ``axis`` and ``values`` (any real dtype, taken as float64; a complex dtype is a
    ``TypeError``), the samples that count, the compare domains, the joint bins of up to 8 inputs, the estimator names and the
    broadcasting are those of :func:`histogram_extrema`.  NaN values are ignored (``nan_policy="omit"``), and two values are one
    where IEEE ``==`` says so: ``-0.0`` and ``+0.0`` are one value.  ``block_size`` is accepted and changes nothing.

    Per (kept index, bin), over the ``n`` non-NaN values of the counted samples:

    * ``count`` is ``n``, int64: :func:`histogram_mean_var`'s ``count`` bit for bit;
    * ``nunique`` is the number of distinct values, int64, 0 for an empty bin;
    * ``mode_count`` is the largest number of samples that hold one value, int64, 0 for an empty bin;
    * ``mode`` is that value, float64.  Among several values that occur ``mode_count`` times the smallest wins
      (``scipy.stats.mode``, ``pandas.Series.mode()[0]``).  It is NaN (``0x7ff8000000000000``) where ``n == 0``.  Its bits are
      those of the value's first sample in :func:`bin_sort`'s ascending order: a zero that the bin holds with both signs is
      reported as ``-0.0``.

    So ``nunique`` is the largest ``bin_rank(method="dense")`` of the bin, ``mode_count`` the largest ``max - min + 1`` over its
    ``"max"`` and ``"min"`` ranks, and ``mode == vmin`` of :func:`histogram_extrema` where every value of the bin is distinct.
    Exact and deterministic: the samples are sorted as :func:`bin_sort` sorts them, a value's samples are then one run, and the
    longest run of a bin is an integer maximum that does not depend on the order of arrival.

    ``weights`` is refused (``NotImplementedError``; a weighted mode is another statistic), there is no ``descending``.  A
    reduced extent of 2^31 samples or more per output row, and ``B + 1 > 2**32`` bins, raise ``NotImplementedError``.  All of
    these, and complex values, are refused before any device work.

    Returns ``(count, nunique, mode, mode_count, bin_edges)`` with the shape ``histogram`` gives (kept axes, then bin axes).
    numpy in -> numpy out, torch in -> torch out on the same device (asynchronous on the current stream), DeviceArray in ->
    numpy out, dask in -> lazy dask arrays, one task per block: every reduced axis must then be a single chunk (the modes of
    several chunks are not merged)."""
    if weights is not None:
        raise NotImplementedError("histogram_mode does not take weights: the value with the largest sum of weights is another "
                                  "statistic")
    _, (count, nunique, mode, mode_count), bins, _ = _value_stat("mode", args, values, bins, range, axis, "histogram_mode")
    return count, nunique, mode, mode_count, bins


def histogram_weighted_mode(*args, values, weights, bins=None, range=None, axis=None):
    """Per-bin value of ``values`` that carries the most weight, computed on an MI355X: :func:`histogram_mode` for samples that
    are not equal — the dominant land-cover type of an elevation band by area, the dominant water mass of a T–S class by volume.
    ``pandas.Series(w).groupby([bin, v]).sum()`` and an ``idxmax`` per bin on the host.

    ``args``, ``bins``, ``range``, ``axis`` and ``values`` are :func:`histogram_mode`'s.  ``weights`` broadcasts against the
    inputs as ``values`` does, may have any real dtype and is taken as float64; a complex dtype, ``None`` and a missing
    ``weights`` are a ``TypeError``.  Weights are not checked: a zero weight still counts, negative weights add.

    Per (kept index, bin), with the bin's entries as :func:`bin_weighted_unique` gives them:

    * ``count`` and ``nunique`` are :func:`histogram_mode`'s, bit for bit;
    * ``mode_weight`` is the largest ``weight_sums`` entry of the bin, float64, compared as IEEE compares (``-0.0 == +0.0``);
      bitwise it is the first entry of the segment that holds the maximum;
    * ``mode`` is the value of that entry (its bits are ``uniques``' bits): among equal sums the smallest value wins,
      :func:`histogram_mode`'s rule;
    * if any entry sum of the bin is NaN, both ``mode`` and ``mode_weight`` are NaN (``0x7ff8000000000000``);
    * an empty bin gets ``0``, ``0``, NaN and ``+0.0``.

    With all weights 1, ``mode`` is :func:`histogram_mode`'s ``mode`` by bits and ``mode_weight == mode_count``.  Deterministic:
    the sums are :func:`bin_weighted_unique`'s, a fixed tree of float64 additions per value, and the maximum over them is taken
    with integer atomics on an order-preserving key, which do not depend on the order of arrival.

    There is no ``descending``.  A reduced extent of 2^31 samples or more per output row, and ``B + 1 > 2**32`` bins, raise
    ``NotImplementedError``; all refusals happen before any device work.

    Returns ``(count, nunique, mode, mode_weight, bin_edges)`` with the shape ``histogram`` gives (kept axes, then bin axes).
    numpy in -> numpy out, torch in -> torch out on the same device (asynchronous on the current stream), DeviceArray in ->
    numpy out, dask in -> lazy dask arrays, one task per block: every reduced axis must then be a single chunk."""
    if weights is None:
        raise TypeError("histogram_weighted_mode needs weights")
    _, (count, nunique, mode, mode_weight), bins, _ = _value_stat("mode_w", args, values, bins, range, axis, "histogram_weighted_mode",
                                                                  weights=weights)
    return count, nunique, mode, mode_weight, bins


# ---------------------------------------------------------------------------------------------
# bin_order, bin_sort and bin_rank: the samples grouped by bin, their one call path
# ---------------------------------------------------------------------------------------------
def _row_shape(rec, width):
    """[kept axes, width]: one row of `width` per kept index of the launch `rec`"""
    return tuple(int(rec.like.shape[i]) for i in rec.kept) + (width,)


def _order_offsets_rows(rec, run):
    """(order [kept axes, c], offsets [kept axes, B + 1]), int64, that `run([order_ptr, offsets_ptr])`, the caller's Plan
    method over the `ordered` launch `rec`, has the kernels write"""
    return tuple(_launch_outputs(rec, [(_row_shape(rec, rec.c), np.int64), (_row_shape(rec, rec.plan.n_bins + 1), np.int64)], run))


def _packed_block(order, offsets, like, axis):
    """one dask block of _packed_blockwise: a row's order and its offsets side by side, int64 [kept axes (reduced ones of extent
    1), c + B + 1], for the block `like` of samples"""
    packed = np.concatenate([order, offsets], axis=-1)
    shape = [1 if i in axis else int(s) for i, s in enumerate(like.shape)]
    return packed.reshape(shape + [packed.shape[-1]])


def _packed_blockwise(block_fn, all_arrays, drop_axes, cols, n_bins, **params):
    """dask: one task per block over the kept axes, each `block_fn`'s _packed_block; (order, offsets), lazy"""
    import dask.array as dsa

    ndim = all_arrays[0].ndim
    ind = tuple(_range(ndim))
    packed = dsa.blockwise(block_fn, ind + (ndim,), *[x for a in all_arrays for x in (a, ind)], dtype=np.int64,
                           new_axes={ndim: cols + n_bins + 1}, adjust_chunks={ax: (lambda extent: 1) for ax in drop_axes},
                           axis=list(drop_axes), meta=np.array((), np.int64), **params)
    packed = packed[tuple(0 if i in drop_axes else slice(None) for i in _range(ndim)) + (slice(None),)]
    return packed[..., :cols], packed[..., cols:]


def _bin_order_block(*blocks, axis=None, bins=None):
    """one dask block (samples...)"""
    return _packed_block(*bin_order(*blocks, bins=bins, axis=axis)[:2], blocks[0], axis)


def bin_order(*args, bins=None, range=None, axis=None):
    """The samples grouped by bin, computed on an MI355X: a stable counting sort of the positions by :func:`bin_index`, the CSR
    form (``order`` and ``offsets``) that makes any per-bin function one line of numpy or torch —
    ``np.split(v[order], offsets[1:-1])``, ``np.maximum.reduceat``, ``torch.segment_reduce`` — what
    ``scipy.stats.binned_statistic(statistic=<callable>)`` does on the host.

    ``args``, ``bins``, ``range`` and ``axis`` are those of :func:`histogram`; the samples that count, the digitize, the compare
    domains, the joint bins of up to 8 inputs and the estimator names are those of :func:`bin_index`.  With ``B`` the number of
    bins, ``c`` the product of the reduced extents and ``kept`` the kept axes' shape, ``order`` is int64 ``kept + (c,)`` and
    ``offsets`` int64 ``kept + (B + 1,)``.  A position is what :func:`histogram_argextrema` calls one: the C-order flat index
    over the reduced axes in ascending axis number, whatever order ``axis`` lists them in (``axis=None``: the flat index into the
    broadcast array).  Per kept index, with ``key[p]`` the bin index at position ``p`` and ``-1`` replaced by ``B``:

    * ``order = np.argsort(key, kind="stable")``, a permutation of ``0 .. c - 1``;
    * ``offsets[b] = #{p : key[p] < b}`` for ``b = 0 .. B``;
    * the positions of bin ``b`` are ``order[offsets[b]:offsets[b + 1]]``, ascending, and the samples ``histogram`` drops are
      ``order[offsets[B]:]``, ascending;
    * ``np.diff(offsets)`` reshaped to the bins' shape is ``histogram(...)[0]``.

    A plan without bins (one edge) gives ``offsets == [0]`` and ``order == arange(c)``; ``c == 0`` an empty ``order`` and
    offsets of 0.  Exact and deterministic: nothing depends on the order in which waves arrive.  A reduced extent of 2^31
    samples or more per row, and more than 40 959 bins (one 4-byte counter per bin and one more in the 160 KiB of LDS of a
    workgroup), raise ``NotImplementedError``.

    Returns ``(order, offsets, bin_edges)``.  numpy in -> numpy out, torch in -> torch out on the same device (asynchronous on
    the current stream), DeviceArray in -> numpy out, dask in -> lazy dask arrays, one task per block over the kept axes: every
    reduced axis must then be a single chunk, and ``bins`` numpy arrays of edges."""
    f = _sample_call("bin_order", args, None, bins, range, axis, needs_values=False, noun="group orders")
    if f.backend == "dask":
        return _packed_blockwise(_bin_order_block, f.arrays, f.drop_axes, f.cols, f.n_bins, bins=f.bins) + (f.bins,)
    rec = _value_views(f.arrays, None, f.axis, f.bins, f.on, ordered=True)

    def run(ptrs):
        rec.plan.execute_group(rec.nv, rec.m, rec.c, *ptrs, stream=rec.stream)

    return _order_offsets_rows(rec, run) + (f.bins,)


# ---------------------------------------------------------------------------------------------
# bin_sort: the samples grouped by bin, sorted by value inside each bin
# ---------------------------------------------------------------------------------------------
def _bin_sort_block(*blocks, axis=None, bins=None, descending=False):
    """one dask block (samples..., values)"""
    return _packed_block(*bin_sort(*blocks[:-1], values=blocks[-1], bins=bins, axis=axis, descending=descending)[:2], blocks[0], axis)


def bin_sort(*args, values, bins=None, range=None, axis=None, descending=False):
    """The samples grouped by bin and, inside each bin, sorted by value, computed on an MI355X: :func:`bin_order`'s CSR form
    (``order`` and ``offsets``) with value order inside every segment — the k warmest samples of a class, trimmed and
    winsorized means, ranks and percentile-of-score, quantile mapping, quantiles at many ``q`` at once and run lengths of the
    values are then one line of numpy or torch each.

    ``args``, ``bins``, ``range`` and ``axis``, the samples that count, the compare domains, the joint bins of up to 8 inputs, the
    estimator names and the meaning of a position are :func:`bin_order`'s.  ``values`` broadcasts against the inputs as
    :func:`histogram_extrema`'s does, may have any real dtype and is taken as float64; a complex dtype is a ``TypeError``.
    With ``B`` the number of bins, ``c`` the product of the reduced extents and ``kept`` the kept axes' shape, ``order`` is int64
    ``kept + (c,)`` and ``offsets`` int64 ``kept + (B + 1,)``.  Per kept index, with ``key[p]`` the bin index at position ``p``
    and ``-1`` replaced by ``B``, and ``vk[p]`` the key :func:`extrema_keys` gives ``values[p]`` (the total order of the values
    with ``-0.0 < +0.0``), its bits complemented when ``descending``, and ``2**64 - 1`` for a NaN value in either direction, so
    that NaN is last in its bin either way:

    * ``order = np.lexsort((vk, key))``: by bin, then by value, ties in ascending position;
    * ``offsets[b] = #{p : key[p] < b}`` for ``b = 0 .. B``.

    So, for ``B <= 40959``, ``offsets`` equals :func:`bin_order`'s bit for bit, and ``np.sort(order[offsets[b]:offsets[b + 1]])``
    is its segment; the samples ``histogram`` drops, ``order[offsets[B]:]``, are sorted by value too;
    ``values[order[offsets[b]]]`` of a bin with a non-NaN value is :func:`histogram_extrema`'s ``vmin`` and ``order[offsets[b]]``
    :func:`histogram_argextrema`'s ``argmin`` (``vmax`` and ``argmax`` with ``descending=True``); and with ``n`` non-NaN values in a
    bin, ``values[order[offsets[b] + floor(q * (n - 1))]]`` is ``histogram_quantile(method="lower")``.

    A plan without bins (one edge) gives ``offsets == [0]`` and the whole row sorted by value; ``c == 0`` an empty ``order`` and
    offsets of 0.  Exact and deterministic: a stable radix sort on 8-bit digits whose every placement is a function of the keys
    alone.  There is no bound of 40 959 bins: every pass keeps 256 counters per wave, whatever ``B`` is.  A reduced extent of
    2^31 samples or more per row, and ``B + 1 > 2**32``, raise ``NotImplementedError`` before any device work.  There are no
    ``weights``.

    Returns ``(order, offsets, bin_edges)``.  numpy in -> numpy out, torch in -> torch out on the same device (asynchronous on
    the current stream, no host synchronisation), DeviceArray in -> numpy out, dask in -> lazy dask arrays, one task per block
    over the kept axes: every reduced axis must then be a single chunk, and ``bins`` numpy arrays of edges."""
    f = _sample_call("bin_sort", args, values, bins, range, axis, noun="sorted orders", max_bins=_SORT_MAX_BINS,
                     check=lambda: _check_flag("descending", descending))
    descending = bool(descending)
    if f.backend == "dask":
        return _packed_blockwise(_bin_sort_block, f.arrays, f.drop_axes, f.cols, f.n_bins, bins=f.bins,
                                 descending=descending) + (f.bins,)
    n = len(args)
    rec = _value_views(f.arrays[:n], f.arrays[n], f.axis, f.bins, f.on, ordered=True)

    def run(ptrs):
        rec.plan.execute_sort(rec.nv[:n], rec.nv[n], rec.m, rec.c, descending, *ptrs, stream=rec.stream)

    return _order_offsets_rows(rec, run) + (f.bins,)


# ---------------------------------------------------------------------------------------------
# bin_rank: the rank of each sample's value inside its bin
# ---------------------------------------------------------------------------------------------
def _bin_rank_block(*blocks, axis=None, bins=None, method="average", descending=False, pct=False):
    return bin_rank(*blocks[:-1], values=blocks[-1], bins=bins, axis=axis, method=method, descending=descending, pct=pct)[0]


def bin_rank(*args, values, bins=None, range=None, axis=None, method="average", descending=False, pct=False):
    """The rank of every sample's value among the values of its bin, computed on an MI355X: the per-sample rank,
    percentile-of-score and empirical CDF value inside a class — ``pandas.Series.groupby(bin).rank(...)`` and
    ``scipy.stats.rankdata`` per bin on the host; the input of quantile mapping, of Spearman correlation per class and of
    rank-based outlier masks.

    ``args``, ``bins``, ``range``, ``axis`` and ``values``, the samples that count, the compare domains, the joint bins of up to
    8 inputs, the estimator names, the broadcasting and ``values`` taken as float64 are :func:`bin_sort`'s; a complex dtype is a
    ``TypeError``.  ``rank`` is float64 in the broadcast shape of the inputs, as :func:`histogram_anomaly`'s output is.  It is
    NaN for a sample ``histogram`` does not count (out of range, or NaN in any input) and for a sample whose value is NaN
    (pandas ``na_option="keep"``, scipy ``nan_policy="omit"``).

    Per kept index, let ``S`` be the counted samples of a bin whose value is not NaN and ``n = len(S)``, in ascending order of
    value (descending with ``descending=True``), ties decided by IEEE ``==``, so ``-0.0`` and ``+0.0`` tie.  For a sample with
    value ``v``, with ``lt`` the number of values of ``S`` strictly before ``v`` in that order, ``eq`` the number equal to ``v``,
    ``d`` the number of distinct values up to and including ``v`` and ``D`` the number of distinct values of ``S``:

    * ``"average"``: ``(2 * lt + eq + 1) / 2`` (scipy and pandas ``average``);
    * ``"min"``: ``lt + 1``; ``"max"``: ``lt + eq``; ``"dense"``: ``d``;
    * ``"ordinal"``: its place in :func:`bin_sort`'s segment, ``i - offsets[b] + 1`` for ``order[i] == position`` (scipy
      ``ordinal``, pandas ``first``): ties in ascending position, and ``-0.0`` before ``+0.0`` (after it when descending).

    With ``pct=True`` the rank is divided once, in IEEE float64, by ``n`` (by ``D`` for ``"dense"``), as pandas
    ``rank(pct=True)`` divides.  Every rank is an integer or a half-integer below 2^31, so every result is exact, and the call
    is deterministic.  So ``pct=True, method="max"`` is the bin's empirical CDF at the sample
    (``scipy.stats.percentileofscore(kind="weak") / 100``), ``(min - 1) / n`` is ``kind="strict"`` and ``average / n`` is
    ``kind="rank"``; the samples of ``min`` rank 1 are those whose value ``==`` :func:`histogram_extrema`'s ``vmin`` (``vmax``
    when descending); and the largest ``max`` rank of a bin is :func:`histogram_mean_var`'s ``count``.

    A plan without bins (one edge) counts no sample: all NaN.  Extents of 0 give empty outputs.  An unknown ``method`` raises
    ``ValueError``; a reduced extent of 2^31 samples or more per row, and ``B + 1 > 2**32``, raise ``NotImplementedError``; all
    before any device work.  There are no ``weights``.

    Returns ``(rank, bin_edges)``.  numpy in -> numpy out (uploaded once), torch in -> torch out on the same device
    (asynchronous on the current stream, no host synchronisation), DeviceArray in -> numpy out, dask in -> a lazy dask array,
    one task per block over the kept axes: every reduced axis must then be a single chunk, and ``bins`` numpy arrays of
    edges."""
    def check():
        if not isinstance(method, str) or method not in _native.RANK_METHODS:
            raise ValueError("unknown rank method %r: one of %s" % (method, ", ".join(_native.RANK_METHODS)))
        _check_flag("descending", descending)
        _check_flag("pct", pct)

    f = _sample_call("bin_rank", args, values, bins, range, axis, noun="ranks", max_bins=_SORT_MAX_BINS, check=check)
    descending, pct = bool(descending), bool(pct)
    n = len(args)
    if f.backend == "dask":
        return _sample_blockwise(_bin_rank_block, f.arrays, np.float64, axis=list(f.drop_axes), bins=f.bins, method=method,
                                 descending=descending, pct=pct), f.bins
    rec = _value_views(f.arrays[:n], f.arrays[n], f.axis, f.bins, f.on, ordered=True)

    def run(ptrs):
        rec.plan.execute_rank(rec.nv[:n], rec.nv[n], rec.m, rec.c, _native.RANK_METHODS[method], descending, pct, ptrs[0],
                              stream=rec.stream)

    return _sample_block(rec, np.float64, run), f.bins


# ---------------------------------------------------------------------------------------------
# bin_unique: each bin's distinct values and their counts (CSR)
# ---------------------------------------------------------------------------------------------
def _check_size(size):
    """ValueError unless `size` is None or an integer >= 0 (a bool is not one)"""
    if size is None:
        return
    if isinstance(size, (bool, np.bool_)) or not isinstance(size, (int, np.integer)) or size < 0:
        raise ValueError("size must be None or an integer >= 0, got %r" % (size,))


def _bin_unique_block(*blocks, axis=None, bins=None, size=None):
    """one dask block (samples..., values): uniques (as the bits they are) and counts side by side, then the offsets"""
    uniques, counts, offsets, _ = bin_unique(*blocks[:-1], values=blocks[-1], bins=bins, axis=axis, size=size)
    return _packed_block(np.concatenate([np.ascontiguousarray(uniques).view(np.int64), counts], axis=-1), offsets, blocks[0], axis)


def _bin_unique_inverse_block(*blocks, axis=None, bins=None):
    return bin_unique(*blocks[:-1], values=blocks[-1], bins=bins, axis=axis, size=0, return_inverse=True)[3]


def _float64_bits(block):
    return np.ascontiguousarray(block).view(np.float64)


def bin_unique(*args, values, bins=None, range=None, axis=None, size=None, return_inverse=False):
    """The distinct values of every bin and how often each occurs, in CSR form, computed on an MI355X:
    ``np.unique(v_bin, return_counts=True, return_inverse=True)`` per bin, ``pandas.groupby(bin).value_counts()`` — the census
    of each class, the composition of each band, a contingency table whose categories are not known in advance, per-bin
    entropy, and the code of every sample for a later :func:`histogram_lookup`.

    ``args``, ``bins``, ``range``, ``axis`` and ``values`` (any real dtype, taken as float64; a complex dtype is a
    ``TypeError``), the samples that count, the compare domains, the joint bins of up to 8 inputs, the estimator names and the
    broadcasting are those of :func:`histogram_mode`; the meaning of a position and the two size limits are
    :func:`bin_sort`'s.  NaN values are ignored, and two values are one where IEEE ``==`` says so: ``-0.0`` and ``+0.0`` are one
    value.

    With ``B`` the number of bins, ``c`` the reduced samples per kept index, ``kept`` the kept axes' shape and ``W`` the output
    width (``c`` when ``size is None``, else ``size``), per kept index:

    * ``offsets``, int64 ``kept + (B + 1,)``: ``offsets[b]`` is the number of distinct non-NaN values in the bins below ``b``;
      ``np.diff(offsets)`` is :func:`histogram_mode`'s ``nunique`` bit for bit and ``U = offsets[B]`` the row's number of
      distinct (bin, value) pairs.  ``offsets`` always tells the truth, whatever ``size`` is.
    * ``uniques``, float64 ``kept + (W,)``: ``uniques[offsets[b]:offsets[b + 1]]`` are bin ``b``'s distinct values, ascending.
      The bits of an entry are those of the value's first sample in :func:`bin_sort`'s ascending order: a zero the bin holds
      with both signs reads ``-0.0``, as :func:`histogram_mode` reports it.
    * ``counts``, int64 ``kept + (W,)``: ``counts[u]`` is the number of counted samples of that bin whose value ``==``
      ``uniques[u]``.
    * Entries ``min(U, W) <= u < W`` are padding: NaN (``0x7ff8000000000000``) in ``uniques`` and ``0`` in ``counts``.
    * ``inverse``, only with ``return_inverse=True``: int64 in the broadcast shape of the inputs, as :func:`bin_rank`'s output
      is.  The index ``u`` into the row's ``uniques`` for a counted sample with a non-NaN value, ``-1`` for every other sample;
      the true index even where ``u >= W``.

    ``size`` exists because ``c`` is the only bound known without a host synchronisation, and categorical data has
    ``U << c``.  With ``size=k`` entries ``u >= k`` are written nowhere: silent truncation, as ``jnp.unique(size=)`` does, which
    the caller sees as ``offsets[..., B] > k``.  There is no synchronisation and no error from the device.

    So, per kept index: the segment sums of ``counts`` are :func:`histogram_mode`'s ``count``; a segment's largest count is its
    ``mode_count`` and the first entry that holds it its ``mode``, by bits; ``uniques[offsets[b]]`` ``==``
    :func:`histogram_extrema`'s ``vmin`` and the segment's last entry ``==`` its ``vmax``; on counted non-NaN samples
    ``inverse == offsets[bin_index] + bin_rank(method="dense") - 1`` and ``uniques[inverse] == values``; and
    ``np.bincount(inverse[inverse >= 0], minlength=U) == counts[:U]``.  Exact and deterministic: the samples are sorted as
    :func:`bin_sort` sorts them, and every output is an integer or the bits of an input value.

    A plan without bins (one edge) gives ``offsets == [0]``, padding only and an ``inverse`` of ``-1``; ``c == 0`` gives empty or
    all-padding outputs and offsets of 0.  ``size`` is ``None`` or an integer ``>= 0`` (anything else, a bool included, is a
    ``ValueError``); there are no ``weights`` and no ``descending``.  A reduced extent of 2^31 samples or more per row, and
    ``B + 1 > 2**32``, raise ``NotImplementedError``.  All refusals happen before any device work.

    Returns ``(uniques, counts, offsets, bin_edges)``, with ``return_inverse`` ``(uniques, counts, offsets, inverse,
    bin_edges)``.  numpy in -> numpy out (uploaded once, one download), torch in -> torch out on the same device (asynchronous
    on the current stream, no host synchronisation), DeviceArray in -> numpy out, dask in -> lazy dask arrays, one task per
    block over the kept axes: every reduced axis must then be a single chunk, and ``bins`` numpy arrays of edges."""
    return _bin_unique("bin_unique", args, values, None, bins, range, axis, size, return_inverse)


def _bin_unique(name, args, values, weights, bins, range, axis, size, return_inverse):
    """bin_unique (`weights` None) and bin_weighted_unique: the outputs without weight_sums, or with it behind counts"""
    def check():
        _check_size(size)
        _check_flag("return_inverse", return_inverse)

    weighted = weights is not None
    f = _sample_call(name, args, values, bins, range, axis, *((weights,) if weighted else ()), noun="distinct values",
                     max_bins=_SORT_MAX_BINS, check=check)
    bins, return_inverse = f.bins, bool(return_inverse)
    size = None if size is None else int(size)
    n = len(args)
    if f.backend == "dask":
        width = f.cols if size is None else size
        k = 3 if weighted else 2
        both, offsets = _packed_blockwise(_bin_weighted_unique_block if weighted else _bin_unique_block, f.arrays, f.drop_axes, k * width,
                                          f.n_bins, bins=bins, size=width)
        floats = [both[..., i * width:(i + 1) * width].map_blocks(_float64_bits, dtype=np.float64, meta=np.array((), np.float64))
                  for i in ((0, 2) if weighted else (0,))]
        out = (floats[0], both[..., width:2 * width]) + tuple(floats[1:]) + (offsets,)
        if return_inverse:
            out += (_sample_blockwise(_bin_unique_inverse_block, f.arrays[:n + 1], np.int64, axis=list(f.drop_axes), bins=bins),)
        return out + (bins,)
    rec = _value_views(f.arrays[:n], f.arrays[n], f.axis, bins, f.on, *f.arrays[n + 1:], ordered=True)
    width = rec.c if size is None else size
    # (a call without an inverse: its block has no column, and the library is told so with a NULL pointer)
    blocks = [(_row_shape(rec, width), np.float64), (_row_shape(rec, width), np.int64)]
    blocks += [(_row_shape(rec, width), np.float64)] if weighted else []
    blocks += [(_row_shape(rec, rec.plan.n_bins + 1), np.int64), ((rec.m, rec.c if return_inverse else 0), np.int64)]

    def run(ptrs):
        method = rec.plan.execute_unique_weighted if weighted else rec.plan.execute_unique
        method(rec.nv[:n], *rec.nv[n:], rec.m, rec.c, width, *ptrs[:-1], ptrs[-1] if return_inverse else None, stream=rec.stream)

    *out, inverse = _launch_outputs(rec, blocks, run)
    out = tuple(out)
    if return_inverse:
        out += (_sample_shape(inverse, _shape_of(rec.like), rec.kept, rec.red, rec.backend),)
    return out + (bins,)


def _bin_weighted_unique_block(*blocks, axis=None, bins=None, size=None):
    """one dask block (samples..., values, weights): uniques, counts and weight_sums (the float64 ones as the bits they are) side
    by side, then the offsets"""
    uniques, counts, sums, offsets, _ = bin_weighted_unique(*blocks[:-2], values=blocks[-2], weights=blocks[-1], bins=bins, axis=axis,
                                                            size=size)
    bits = [np.ascontiguousarray(a).view(np.int64) for a in (uniques, sums)]
    return _packed_block(np.concatenate([bits[0], counts, bits[1]], axis=-1), offsets, blocks[0], axis)


def bin_weighted_unique(*args, values, weights, bins=None, range=None, axis=None, size=None, return_inverse=False):
    """The distinct values of every bin, how often each occurs and how much weight each carries, in CSR form, computed on an
    MI355X: :func:`bin_unique` for samples that are not equal — a land-cover composition by area per elevation band, a water-mass
    census by volume per T–S class.  ``pandas.Series(w).groupby([bin, v]).sum()``, or :func:`bin_sort`, a gather of the weights
    and ``np.add.reduceat`` over the run starts on the host.

    Every argument but ``weights`` is :func:`bin_unique`'s, and ``uniques``, ``counts``, ``offsets`` and ``inverse`` are its
    outputs bit for bit, with every ``size``, padding and truncation rule.  ``weights`` broadcasts against the inputs as
    ``values`` does, may have any real dtype and is taken as float64; a complex dtype, ``None`` and a missing ``weights`` are a
    ``TypeError``.

    ``weight_sums`` is float64 ``kept + (W,)``: ``weight_sums[u]`` is the float64 sum of the weights of the counted samples of
    that bin whose value ``==`` ``uniques[u]``, the samples ``counts[u]`` counts.  A counted sample with a NaN value belongs to
    no entry, whatever its weight.  Padding entries ``min(U, W) <= u < W`` are ``+0.0``; entries ``u >= W`` are stored nowhere.
    Weights are not checked: a zero weight still counts in ``counts``, negative weights add, a NaN weight makes its own entry's
    sum NaN and no other, ``+inf`` and ``-inf`` in one entry give NaN.

    The order of the additions is part of the interface.  The samples of an entry are one run of :func:`bin_sort`'s order, in
    ascending position; the run is summed over a fixed tree that depends only on where its first and last sorted position lie
    against the words of 64 positions and the tiles of 65 536 positions of the row.  There is no floating-point atomic.  So
    ``weight_sums`` has the same bits run to run, on any stream, however the rows are batched, with and without an inverse, for
    any ``size``, and :func:`histogram_weighted_mode`'s ``mode_weight`` is bitwise the first maximal entry of its segment.  On
    weights whose partial sums are all exact in float64 every sum equals ``math.fsum``; otherwise it is within
    ``2 * gamma(n) * sum(abs(w))`` of it, ``n`` the entry's count.

    So, per kept index: with all weights 1 ``weight_sums == counts``; on exactly summable weights
    ``np.bincount(inverse[inverse >= 0], weights=w[inverse >= 0], minlength=U) == weight_sums[:U]``, and the segment sums of
    ``weight_sums`` are ``histogram(..., weights=w)`` where no value is NaN.

    The refusals and the empty cases are :func:`bin_unique`'s, all before any device work; there is no ``descending``.

    Returns ``(uniques, counts, weight_sums, offsets, bin_edges)``, with ``return_inverse`` ``(uniques, counts, weight_sums,
    offsets, inverse, bin_edges)``.  numpy in -> numpy out (uploaded once, one download), torch in -> torch out on the same
    device (asynchronous on the current stream, no host synchronisation), DeviceArray in -> numpy out, dask in -> lazy dask
    arrays, one task per block over the kept axes: every reduced axis must then be a single chunk, and ``bins`` numpy arrays of
    edges."""
    if weights is None:
        raise TypeError("bin_weighted_unique needs weights")
    if not hasattr(weights, "dtype"):
        weights = np.asarray(weights)
    return _bin_unique("bin_weighted_unique", args, values, weights, bins, range, axis, size, return_inverse)
