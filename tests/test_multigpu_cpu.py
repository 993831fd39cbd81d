"""In-call multi-GPU path (xhistogram_amd.multigpu) on the CPU: shard planning, block -> GPU assignment, the
per-GPU host threads and the reduce logic run here with the rank-local compute swapped for the oracle (a test
double for `core._bincount`; the product default is the HIP path, covered by the gpu-marked tests) and with
"virtual" device numbers — nothing below touches a GPU."""
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

from oracle import oracle_np as onp
from xhistogram_amd import _native, core, multigpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle_bincount(seen):
    def fn(*all_arrays, weights=False, axis=None, bins=None, density=None, block_size=None):
        arrays = [a.numpy() if hasattr(a, "numpy") else np.asarray(a) for a in all_arrays]
        w = arrays.pop() if weights else None
        nd = arrays[0].ndim
        ax = tuple(range(nd)) if axis is None else tuple(int(a) for a in axis)
        seen.append((core._host_device(), threading.current_thread().name, tuple(arrays[0].shape)))
        h, _ = onp.histogram(*arrays, bins=bins if len(arrays) > 1 else bins[0], weights=w, axis=ax)
        kept = tuple(1 if i in ax else arrays[0].shape[i] for i in range(nd))
        return np.asarray(h).reshape(kept + tuple(len(b) - 1 for b in bins))

    return fn


def test_plan_shards_prefers_kept_axes_then_reduced_ones():
    # C4: (time, lat, lon) over lat, lon -> rows of the kept time axis, no arithmetic
    mode, ax, b = multigpu.plan_shards((3650, 720, 1440), (1, 2), 8)
    assert (mode, ax) == ("rows", 0) and b[0] == (0, 457) and b[-1][1] == 3650 and len(b) == 8
    assert sum(hi - lo for lo, hi in b) == 3650 and all(b[k][1] == b[k + 1][0] for k in range(7))
    # C2 / C5: one long sample axis, fully reduced -> partial histograms, summed
    mode, ax, b = multigpu.plan_shards((10**9,), (0,), 8)
    assert (mode, ax) == ("sum", 0) and b[3] == (375_000_000, 500_000_000)
    # kept axis too short for the GPUs: the reduced axis takes the shards
    assert multigpu.plan_shards((3, 10**6), (1,), 8)[:2] == ("sum", 1)
    # the outermost long-enough kept axis wins (contiguous shards)
    assert multigpu.plan_shards((4, 100, 200, 50), (3,), 8)[:2] == ("rows", 1)
    # nothing is long enough: as many shards as the longest axis has indices
    mode, ax, b = multigpu.plan_shards((3, 5), (1,), 8)
    assert (mode, ax, len(b)) == ("sum", 1, 5)


CASES = {
    # name: (shape, n_args, kwargs, weights: None | "full" | broadcastable shape)
    "c2_full_reduce_weighted": ((100_003,), 1, dict(bins=np.linspace(-4, 4, 101)), "full"),
    "c3_joint_2d": ((50_001,), 2, dict(bins=[np.sort(np.random.default_rng(5).uniform(-4, 4, 33)), np.linspace(-3, 3, 17)]), None),
    "c4_time_rows": ((23, 18, 36), 1, dict(bins=np.linspace(-4, 4, 51), axis=(1, 2)), None),
    "c4_rows_lat_weights": ((23, 18, 36), 1, dict(bins=np.linspace(-4, 4, 51), axis=(1, 2)), (1, 18, 1)),
    "c4_rows_time_weights": ((23, 18, 36), 1, dict(bins=np.linspace(-4, 4, 11), axis=(1, 2)), (23, 1, 1)),
    "reduced_axis_short_kept": ((2, 4001), 1, dict(bins=np.linspace(-4, 4, 21), axis=1, density=True), "full"),
    "middle_axis_kept": ((6, 9, 7), 1, dict(bins=np.linspace(-4, 4, 9), axis=(0, 2)), None),
    "bins_int_density": ((4001,), 1, dict(bins=13, density=True), None),
}


@pytest.mark.parametrize("n_dev", [2, 3, 8])
@pytest.mark.parametrize("case", sorted(CASES))
def test_host_inputs_sharded_over_virtual_gpus(monkeypatch, case, n_dev):
    shape, n_args, kw, wspec = CASES[case]
    rng = np.random.default_rng(11)
    args = [rng.standard_normal(shape) for _ in range(n_args)]
    if not isinstance(kw["bins"], int):
        args[0].flat[::97] = np.nan  # (an integer `bins` needs finite data, as in numpy)
    w = None if wspec is None else rng.uniform(0.1, 1, shape if wspec == "full" else wspec)
    seen = []
    monkeypatch.setattr(core, "_bincount", _oracle_bincount(seen))
    monkeypatch.setattr(multigpu, "MIN_SHARD_BYTES", 1)
    multigpu.set_devices(list(range(10, 10 + n_dev)))  # virtual device numbers: nothing is launched
    try:
        got, edges = core.histogram(*args, weights=w, **kw)
    finally:
        multigpu.set_devices(None)
    want, wedges = onp.histogram(*args, weights=w, **kw)
    for e, we in zip(edges, wedges):
        np.testing.assert_array_equal(e, we)
    assert got.shape == np.asarray(want).shape and got.dtype == np.asarray(want).dtype
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, equal_nan=True)
    if w is None and not kw.get("density"):
        np.testing.assert_array_equal(got, want)  # int64 counts: exact, whatever the shard layout
    # every shard ran on its own GPU's thread, bound to that GPU
    devs = sorted({d for d, _, _ in seen})
    assert devs == list(range(10, 10 + len(devs))) and len(devs) >= min(n_dev, 2)
    for d, tname, _ in seen:
        assert tname.startswith("xhist-gpu%d" % d)


def test_small_host_inputs_stay_on_one_gpu(monkeypatch):
    seen = []
    monkeypatch.setattr(core, "_bincount", _oracle_bincount(seen))
    multigpu.set_devices([0, 1, 2, 3])
    try:
        x = np.random.default_rng(0).standard_normal(1000)
        got, _ = core.histogram(x, bins=np.linspace(-4, 4, 11))
    finally:
        multigpu.set_devices(None)
    np.testing.assert_array_equal(got, onp.histogram(x, bins=np.linspace(-4, 4, 11))[0])
    assert len(seen) == 1 and not seen[0][1].startswith("xhist-gpu")  # the caller's own thread, default device


def test_a_rank_of_a_launcher_keeps_to_its_gpu(monkeypatch):
    monkeypatch.setattr(_native, "device_count", lambda: 8)  # a node of 8 GPUs, whatever this machine shows
    monkeypatch.setenv("LOCAL_RANK", "3")
    assert multigpu.get_devices() == [3]
    monkeypatch.setenv("XHIST_AMD_DEVICES", "1,2")
    assert multigpu.get_devices() == [1, 2]
    monkeypatch.delenv("LOCAL_RANK")
    monkeypatch.setenv("XHIST_AMD_DEVICES", "5")
    assert multigpu.get_devices() == [5]


def test_block_device_hands_out_the_least_busy_gpu():
    multigpu.set_devices([0, 1, 2, 3])
    try:
        # a serial scheduler (one block at a time) still visits every GPU
        order = []
        for _ in range(8):
            with multigpu.block_device() as d:
                order.append(d)
                assert core._host_device() == d
        assert sorted(order[:4]) == [0, 1, 2, 3] and sorted(order[4:]) == [0, 1, 2, 3]
        assert getattr(core._tls, "device", None) is None
        # concurrent blocks: never two on one GPU while another GPU is idle
        gate, lock, live, worst = threading.Barrier(4), threading.Lock(), {}, [0]

        def block():
            with multigpu.block_device() as d:
                with lock:
                    live[d] = live.get(d, 0) + 1
                    worst[0] = max(worst[0], live[d])
                gate.wait(timeout=30)
                with lock:
                    live[d] -= 1

        ts = [threading.Thread(target=block) for _ in range(4)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        assert worst[0] == 1
        assert all(v == 0 for v in multigpu._inflight.values())
        # a thread that already owns a GPU (a shard worker) keeps it
        with multigpu.on_device(7):
            with multigpu.block_device() as d:
                assert d == 7
    finally:
        multigpu.set_devices(None)


def test_errors_in_one_shard_surface_after_all_threads_finished(monkeypatch):
    def boom(*a, **k):
        if core._host_device() == 21:
            raise RuntimeError("GPU 21 fell over")
        return _oracle_bincount([])(*a, **k)

    monkeypatch.setattr(core, "_bincount", boom)
    monkeypatch.setattr(multigpu, "MIN_SHARD_BYTES", 1)
    multigpu.set_devices([20, 21, 22])
    try:
        with pytest.raises(RuntimeError, match="GPU 21 fell over"):
            core.histogram(np.zeros(3000), bins=np.linspace(-1, 1, 5))
    finally:
        multigpu.set_devices(None)


# ---- device-resident shards (torch): sharding + exchange logic with CPU tensors --------------------
torch = pytest.importorskip("torch")


def _local_oracle(arrays, has_weights, axis, edges, block_size):
    arrs = [a.numpy() if hasattr(a, "numpy") else np.asarray(a) for a in arrays]
    w = arrs.pop() if has_weights else None
    return torch.from_numpy(np.ascontiguousarray(onp.block_adapter(arrs, edges, w, axis)))


def _cpu_shards(a, n, axis):
    parts = [torch.from_numpy(np.ascontiguousarray(multigpu._take(a, axis, *multigpu.shard_bounds(a.shape[axis], n, k)))) for k in range(n)]
    return multigpu.Sharded(parts, axis, devices=list(range(30, 30 + n)))


@pytest.mark.parametrize("case", ["c2_full_reduce_weighted", "c4_time_rows", "reduced_axis_short_kept", "middle_axis_kept", "bins_int_density"])
def test_sharded_tensors_reduce_and_gather_logic(case):
    shape, n_args, kw, wspec = CASES[case]
    rng = np.random.default_rng(21)
    full = [rng.standard_normal(shape) for _ in range(n_args)]
    w = None if wspec is None else rng.uniform(0.1, 1, shape)
    for shard_axis in range(len(shape)):
        if shape[shard_axis] < 3:
            continue
        args = [_cpu_shards(a, 3, shard_axis) for a in full]
        ws = None if w is None else _cpu_shards(w, 3, shard_axis)
        with multigpu._hooks(local=_local_oracle, reduce=lambda parts: sum(parts[1:], parts[0].clone())):
            got, edges = multigpu.histogram(*args, weights=ws, **kw)
        want, _ = onp.histogram(*full, weights=w, **kw)
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-12, equal_nan=True)
        assert tuple(got.shape) == np.asarray(want).shape


def test_sharded_inputs_must_match():
    a = _cpu_shards(np.zeros((6, 4)), 2, 0)
    b = _cpu_shards(np.zeros((6, 4)), 2, 1)
    with pytest.raises(ValueError):
        multigpu.histogram(a, b, bins=[np.arange(3.0)] * 2)
    # sharded weights are cut like the inputs: another axis or other part shapes is an error, not a silent mismatch
    with pytest.raises(ValueError, match="sharded weights"):
        multigpu.histogram(a, bins=[np.arange(3.0)], weights=b)
    c = _cpu_shards(np.zeros((8, 4)), 2, 0)
    with pytest.raises(ValueError, match="sharded weights"):
        multigpu.histogram(a, bins=[np.arange(3.0)], weights=c)
    with pytest.raises(TypeError):
        multigpu.histogram(np.zeros(4), bins=3)


@pytest.mark.parametrize("name", ["sqrt", "sturges", "rice", "scott"])
def test_sharded_inputs_take_the_cheap_bin_estimators(name):
    """f-1 on sharded data: bins="sqrt" | "sturges" | "rice" | "scott" from per-GPU moments combined on the host — the edges of
    np.histogram_bin_edges on the whole array, with and without a range; "fd" & co. still need all the data in one place"""
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((7, 3001)) * 2.5 + 1).astype(np.float64)

    def moments(part, lo_hi, want_m2):
        v = np.asarray(part).ravel().astype(np.float64)
        if lo_hi is not None:
            v = v[(v >= lo_hi[0]) & (v <= lo_hi[1])]
        if v.size == 0:
            return 0, np.inf, -np.inf, np.nan, np.nan
        return v.size, v.min(), v.max(), v.mean(), ((v - v.mean()) ** 2).sum()

    for shard_axis in (0, 1):
        sx = _cpu_shards(x, 3, shard_axis)
        for r in (None, (-2.0, 4.5)):
            with multigpu._hooks(local=_local_oracle, moments=moments, reduce=lambda parts: sum(parts[1:], parts[0].clone())):
                got, edges = multigpu.histogram(sx, bins=name, range=r)
            want_e = np.histogram_bin_edges(x, bins=name, range=r)
            np.testing.assert_array_equal(edges[0], want_e)
            np.testing.assert_array_equal(np.asarray(got), np.histogram(x, bins=want_e)[0])
    with pytest.raises(TypeError, match="estimators"), multigpu._hooks(local=_local_oracle, moments=moments):
        multigpu.histogram(_cpu_shards(x, 2, 0), bins="fd")
    with pytest.raises(TypeError):  # the hooks are not keyword arguments of the public function
        multigpu.histogram(_cpu_shards(x, 2, 0), bins=5, _local=_local_oracle)


# ---- bench.py --gpus N spawns its own ranks -------------------------------------------------------
def test_bench_spawns_its_ranks_and_fails_per_rank_without_gpus():
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        pytest.skip("two GPUs here: the spawn path would run for real")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert "spawning 2 ranks" in r.stderr
    # torch.distributed.run SIGTERMs the surviving rank as soon as the first one exits: either rank's message may be
    # the one that makes it to stderr
    assert re.search(r"rank [01] of 2: needs GPU [01]", r.stderr)
    assert r.stdout.strip() == ""  # stdout carries the JSON line of a successful run, nothing else


@pytest.mark.parametrize("scaling", ["weak", "strong"])
def test_bench_multi_rank_control_flow_selftest(scaling):
    """`bench.py --gpus 2 --selftest`: the N > 1 branches of the harness (rank spawn, rendezvous, both scaling legs,
    per-rank gathers, all-reduce timing, ONE JSON line from rank 0) run on CPU over gloo with a plan double — no kernel, no
    oracle, nothing measured.  The real launch differs only in backend ("nccl"), device and plan."""
    import json

    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--selftest", "--steps", "3", "--warmup", "1",
                        "--scaling", scaling], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    other = "strong" if scaling == "weak" else "weak"
    assert d["metric"].startswith("SELFTEST") and d["n_gpus"] == 2 and d["scaling"] == scaling and d["steps"] == 3
    assert len(d["kernel_ms_per_rank"]) == 2 and d["allreduce_ms_alone"] is not None and "cpu_baseline" not in d
    assert d[other]["samples_total"] == (20_000 if other == "strong" else 40_000)
    assert d["config"]["samples_total"] == (40_000 if scaling == "weak" else 20_000)
    assert len(d[other]["kernel_ms_per_rank"]) == 2
    for key in ("value", "unit", "ms_per_step", "higher_is_better", "vs_baseline", "dtype", "data", "roofline", "overhead_us_per_step"):
        assert key in d
    # the headline's unweighted variant (north_star's target sentence; VERDICT r2 "next" #5) rides along in the same line
    u = d["unweighted"]
    assert u["roofline"]["algorithmic_bytes_per_launch"] * 2 == d["roofline"]["algorithmic_bytes_per_launch"]  # 8 vs 16 B/sample
    for key in ("value", "ms_per_step", "kernel_ms_mean", "overhead_us_per_step"):
        assert u[key] is not None
    assert "overhead_us_per_step" in d[other]
    # who ran it, gathered over the process group itself (VERDICT r5 "next" #4): two ranks, two distinct entries
    rk = d["ranks"]
    assert rk["backend"] == "gloo" and rk["world_size_seen"] == 2 and rk["distinct_devices"] == 2
    assert sorted(e["rank"] for e in rk["devices"]) == [0, 1] and len({e["pid"] for e in rk["devices"]}) == 2
    # the LAST key of the line is the summary (an 8 KB tail of the driver's record still holds it)
    assert list(d.keys())[-1] == "summary" and d["summary"]["n_gpus"] == 2 and d["summary"]["distinct_devices"] == 2
    assert lines[0].rstrip().endswith("}}") and '"summary"' in lines[0][-600:]


def test_blocks_in_flight_per_gpu_are_bounded():
    """dask's threaded scheduler runs os.cpu_count() blocks at once; each holds device memory of its own size"""
    import time

    multigpu.set_devices([0, 1])
    try:
        lock, live, worst = threading.Lock(), {}, {}

        def block():
            with multigpu.block_device() as d:
                with lock:
                    live[d] = live.get(d, 0) + 1
                    worst[d] = max(worst.get(d, 0), live[d])
                time.sleep(0.01)
                with lock:
                    live[d] -= 1

        ts = [threading.Thread(target=block) for _ in range(40)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        assert sorted(worst) == [0, 1] and max(worst.values()) <= multigpu.MAX_BLOCKS_IN_FLIGHT
        assert all(v == 0 for v in multigpu._inflight.values())
    finally:
        multigpu.set_devices(None)


def test_reduce_partials_adds_per_gpu_then_across_gpus():
    """second stage of the dask graph under the device-resident reduction: partials grouped by GPU, added there INTO A BUFFER
    OF THE TASK'S OWN, the GPUs' sums all-reduced over the whole configured group (test seam instead of RCCL), one copy
    back; empty blocks arrive as host arrays.  The upstream partials are neither changed nor freed: running the task twice
    gives the same answer (a retried reduce task must not double-count or read freed memory)."""
    from xhistogram_amd import _native

    log = []

    class FakeBuf:
        def __init__(self, arr, device):
            self.arr, self.device, self.ptr, self.closed = arr.astype(np.float64).ravel().copy(), device, id(self), False

        def upload(self, host):
            assert not self.closed
            self.arr[: host.size] = host.ravel()

        def add(self, other, count, tag):
            assert other.device == self.device and not other.closed and not self.closed
            log.append(("add", self.device))
            self.arr[:count] += other.arr[:count]

        def download(self, out):
            log.append(("download", self.device))
            out[...] = self.arr.reshape(out.shape)

        def close(self):
            self.closed = True

    made = []

    def alloc(device, nbytes):
        made.append(FakeBuf(np.full(nbytes // 8, 123.0), device))  # (garbage: the task must zero it)
        return made[-1]

    rng = np.random.default_rng(3)
    shape = (4, 1, 1, 7)  # a kept-axis chunk of 4 rows, two reduced axes as single-element dims, 7 bins
    blocks = [rng.integers(0, 9, shape).astype(np.float64) for _ in range(7)]
    devs = [2, 0, 2, 1, 0, 2, 1]
    parts = [_native.DevicePartial(FakeBuf(b, d), shape, np.float64) for b, d in zip(blocks, devs)]
    before = [p.buf.arr.copy() for p in parts]
    empty = np.zeros(shape)
    nested = [[parts[0], parts[1], [parts[2]]], [parts[3], empty, parts[4]], [parts[5], parts[6]]]

    def allreduce(sums, count, tag):
        log.append(("allreduce", tuple(s.device for s in sums)))
        tot = sum(s.buf.arr[:count] for s in sums)
        for s in sums:
            s.buf.arr[:count] = tot

    multigpu.set_devices([0, 1, 2, 3])  # GPU 3 holds no partial of this chunk: it joins the exchange with zeros
    try:
        for attempt in range(2):
            del log[:], made[:]
            got = multigpu.reduce_partials(nested, drop_axes=(1, 2), out_dtype="<f8", _allreduce=allreduce, _alloc=alloc)
            np.testing.assert_allclose(got, sum(blocks).squeeze((1, 2)))
            assert got.shape == (4, 7)
            assert [e for e in log if e[0] == "allreduce"] == [("allreduce", (0, 1, 2, 3))]    # ONE exchange, the whole group, in order
            assert sorted(e[1] for e in log if e[0] == "add") == [0, 0, 1, 1, 2, 2, 2]          # every partial added once, on its GPU
            assert [e for e in log if e[0] == "download"] == [("download", 0)]                   # one copy back
            assert len(made) == 4 and all(b.closed for b in made)                                # the task's own buffers, released
            assert not any(p.buf.closed for p in parts)                                          # upstream outputs: not freed ...
            assert all(np.array_equal(p.buf.arr, b) for p, b in zip(parts, before))              # ... and not changed
    finally:
        multigpu.set_devices(None)
    # integer counts; a single GPU needs no exchange (and no group beyond that GPU)
    ip = [_native.DevicePartial(FakeBuf(np.full((2, 1, 3), k), 5), (2, 1, 3), np.int64) for k in (1, 2, 3)]
    got = multigpu.reduce_partials([ip], drop_axes=(1,), out_dtype="<i8", _alloc=alloc,
                                   _allreduce=lambda *a: (_ for _ in ()).throw(AssertionError("no exchange for one GPU")))
    np.testing.assert_array_equal(got, np.full((2, 3), 6))
    assert got.dtype == np.int64


def test_dask_exchange_follows_the_scheduler(monkeypatch):
    """device-resident partials are handed from task to task only when dask's scheduler keeps every task
    in this process; under the multiprocessing scheduler or dask.distributed the reference's host-side sum is the graph"""
    import types

    monkeypatch.delenv("XHIST_AMD_DASK_EXCHANGE", raising=False)
    multigpu.set_dask_exchange(None)
    multigpu.set_devices([0, 1])
    fake_base = types.ModuleType("dask.base")
    fake_dask = types.ModuleType("dask")
    fake_dask.base = fake_base
    monkeypatch.setitem(sys.modules, "dask", fake_dask)
    monkeypatch.setitem(sys.modules, "dask.base", fake_base)

    def getter(module, name):
        def get(*a, **k):
            return None

        get.__module__, get.__name__ = module, name
        return get

    try:
        for module, name, want in [("dask.threaded", "get", "rccl"), ("dask.local", "get_sync", "rccl"),
                                   ("dask.multiprocessing", "get", "host"), ("distributed.client", "get", "host")]:
            fake_base.get_scheduler = lambda g=getter(module, name): g
            assert multigpu.dask_exchange() == want, (module, name)
        fake_base.get_scheduler = lambda: None  # nothing configured: dask arrays default to the threaded scheduler
        assert multigpu.dask_exchange() == "rccl"
        multigpu.set_dask_exchange("rccl")      # an explicit choice wins
        fake_base.get_scheduler = lambda g=getter("dask.multiprocessing", "get"): g
        assert multigpu.dask_exchange() == "rccl"
    finally:
        multigpu.set_dask_exchange(None)
        multigpu.set_devices(None)


def test_dask_exchange_policy(monkeypatch):
    multigpu.set_devices([0])
    try:
        assert multigpu.dask_exchange() == "host"
        multigpu.set_devices([0, 1])
        assert multigpu.dask_exchange() == "rccl"
        monkeypatch.setenv("XHIST_AMD_DASK_EXCHANGE", "host")
        assert multigpu.dask_exchange() == "host"
        multigpu.set_dask_exchange("rccl")
        assert multigpu.dask_exchange() == "rccl"
    finally:
        multigpu.set_dask_exchange(None)
        multigpu.set_devices(None)


def test_bench_default_run_lengths(monkeypatch):
    """20 timed steps after 3 warm-up ones, except the sub-millisecond C4 shard step (200 after 50); explicit flags win"""
    import importlib
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.syspath_prepend(root)
    bench = importlib.import_module("bench")
    for argv, want in (([], (20, 10)), (["--config", "c4"], (200, 50)), (["--config", "c4", "--full"], (20, 10)), (["--config", "c5"], (20, 10)),
                       (["--config", "c4", "--steps", "7"], (7, 50)), (["--steps", "5", "--warmup", "2"], (5, 2))):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
        a = bench.parse()
        assert (a.steps, a.warmup) == want, (argv, a.steps, a.warmup)



@pytest.mark.parametrize("var", ["LOCAL_RANK", "SLURM_LOCALID", "OMPI_COMM_WORLD_LOCAL_RANK", "MV2_COMM_WORLD_LOCAL_RANK", "MPI_LOCALRANKID"])
def test_a_launched_rank_keeps_to_its_gpu(monkeypatch, var):
    """ranks started by srun / mpirun (not only torchrun) must not each grab every GPU of the node"""
    from xhistogram_amd import core

    for k in core.LOCAL_RANK_VARS + ("XHIST_AMD_DEVICES",):
        monkeypatch.delenv(k, raising=False)
    multigpu.set_devices(None)
    monkeypatch.setattr(multigpu, "visible_devices", lambda: [0, 1, 2, 3, 4, 5, 6, 7])
    monkeypatch.setattr(_native, "device_count", lambda: 8)
    assert multigpu.get_devices() == [0, 1, 2, 3, 4, 5, 6, 7]
    monkeypatch.setenv(var, "5")
    assert core.default_device() == 5 and multigpu.get_devices() == [5]
    monkeypatch.setenv("XHIST_AMD_DEVICE", "2")  # the library's own variable wins
    assert multigpu.get_devices() == [2]
    monkeypatch.setenv("XHIST_AMD_DEVICES", "all")  # and an explicit spread wins over both
    assert multigpu.get_devices() == [0, 1, 2, 3, 4, 5, 6, 7]


def test_launcher_rank_is_clamped_to_the_visible_gpus_and_a_lone_task_owns_the_node(monkeypatch):
    """under srun --gpus-per-task=1 / --gpu-bind every task sees ONE GPU (device 0) whatever its local
    rank; and a single task on a node (srun -n1 around a multi-GPU process) must keep every visible GPU"""
    from xhistogram_amd import _native, core

    for k in core.LOCAL_RANK_VARS + core.LOCAL_SIZE_VARS + ("XHIST_AMD_DEVICES",):
        monkeypatch.delenv(k, raising=False)
    multigpu.set_devices(None)
    monkeypatch.setattr(multigpu, "visible_devices", lambda: [0, 1, 2, 3])
    monkeypatch.setenv("SLURM_LOCALID", "3")
    monkeypatch.setattr(_native, "device_count", lambda: 1)
    assert core.default_device() == 0 and multigpu.get_devices() == [0]  # bound to one GPU: local rank 3 is device 0
    monkeypatch.setattr(_native, "device_count", lambda: 4)
    assert core.default_device() == 3 and multigpu.get_devices() == [3]
    monkeypatch.setattr(_native, "device_count", lambda: 2)
    assert core.default_device() == 1  # two GPUs shared by four tasks
    # one task on the node: it is not "a rank that keeps to its GPU"
    monkeypatch.setenv("SLURM_LOCALID", "0")
    monkeypatch.setenv("SLURM_NTASKS_PER_NODE", "1")
    assert multigpu.get_devices() == [0, 1, 2, 3]
    monkeypatch.delenv("SLURM_NTASKS_PER_NODE")
    monkeypatch.setenv("SLURM_TASKS_PER_NODE", "4(x2)")  # Slurm's notation for "4 tasks on each of 2 nodes"
    monkeypatch.setenv("SLURM_NODEID", "1")
    assert core.launcher_local_size() == 4 and multigpu.get_devices() == [0]
    # the list names EVERY node — this node's entry is the one at $SLURM_NODEID, not the leading integer
    for spec, node, want in (("1,4", "0", 1), ("1,4", "1", 4), ("1(x2),4", "2", 4), ("1(x2),4", "1", 1), ("2,1", "5", None)):
        monkeypatch.setenv("SLURM_TASKS_PER_NODE", spec)
        monkeypatch.setenv("SLURM_NODEID", node)
        assert core.launcher_local_size() == want, (spec, node)
    monkeypatch.delenv("SLURM_NODEID")
    assert core.launcher_local_size() is None  # several nodes, no node id: says nothing
    monkeypatch.setenv("SLURM_TASKS_PER_NODE", "4")
    assert core.launcher_local_size() == 4  # one figure is unambiguous
    monkeypatch.delenv("SLURM_TASKS_PER_NODE")
    monkeypatch.delenv("SLURM_LOCALID")
    monkeypatch.setenv("OMPI_COMM_WORLD_LOCAL_RANK", "0")
    monkeypatch.setenv("OMPI_COMM_WORLD_LOCAL_SIZE", "1")
    assert multigpu.get_devices() == [0, 1, 2, 3]
    monkeypatch.setenv("XHIST_AMD_DEVICE", "7")  # explicit: never second-guessed
    assert core.default_device() == 7


def test_device_containers_pickle_through_host_memory_or_fail_loudly():
    """DeviceBuffer / DevicePartial / DeviceArray must never pickle as a bare pointer.  Here (no GPU) the
    serialising side is a double and the receiving side has no device: unpickling raises instead of producing a foreign
    pointer; the GPU round trip is in tests/test_gpu_devicearray.py."""
    import copy
    import pickle

    from xhistogram_amd import _native
    from xhistogram_amd.devicearray import DeviceArray

    if torch.cuda.is_available():
        pytest.skip("GPU present: the real round trip runs in tests/test_gpu_devicearray.py")
    buf = _native.DeviceBuffer.__new__(_native.DeviceBuffer)
    buf.device, buf.nbytes, buf.ptr = 0, 24, 0xdead0000
    payload = np.arange(3, dtype=np.float64)
    buf.download = lambda host: host.__setitem__(slice(None), payload.view(np.uint8))
    try:
        fn, args = buf.__reduce__()
        assert fn is _native._rebuild_buffer and args[0] == 0 and args[1] == 24
        np.testing.assert_array_equal(args[2].view(np.float64), payload)  # the BYTES travel, not the pointer
        blob = pickle.dumps(_native.DevicePartial(buf, (3,), np.float64))
        assert b"dead0000" not in blob and str(0xdead0000).encode() not in blob
        with pytest.raises(RuntimeError):  # no GPU on the receiving side: loud, no CPU stand-in
            pickle.loads(blob)
        with pytest.raises(RuntimeError):
            copy.deepcopy(buf)
        buf.ptr = None
        with pytest.raises(ValueError):
            pickle.dumps(buf)
    finally:
        buf.ptr = None  # (nothing to free)
    arr = DeviceArray(None, 0xbeef0000, (2, 2), (16, 8), np.float64, 0)
    arr_host = np.arange(4.0).reshape(2, 2)
    fn, args = DeviceArray.__reduce__.__get__(type("A", (), {"to_numpy": lambda self: arr_host, "device": 0})())()
    np.testing.assert_array_equal(args[0], arr_host)
    with pytest.raises(RuntimeError):
        fn(*args)


def test_a_failed_exchange_drops_the_communicators_and_the_next_one_rebuilds_them(monkeypatch):
    """after a deadline `xhist_comm_wait` aborts the communicator and every later call on it fails at once; the
    DeviceGroup of a long-lived worker must therefore drop its communicators on a RuntimeError and build new ones for the next
    exchange — one slow peer is one failed call, not a poisoned process.  Communicator doubles; no GPU."""
    made, closed = [], []

    class CommDouble:
        def __init__(self, device, rank, world, uid):
            self.device, self.rank, self.world_size, self.generation = device, rank, world, len(made) // 2
            self.aborted = False
            made.append(self)

        def wait(self, stream=0):
            if self.aborted:
                raise RuntimeError("XHIST_ERR_COMM: communicator was aborted earlier")
            if self.generation == 0 and self.rank == 1:
                self.aborted = True
                raise RuntimeError("XHIST_ERR_COMM: deadline passed with the collective still in flight")

        def close(self):
            closed.append(self)

    monkeypatch.setattr(_native, "Comm", CommDouble)
    monkeypatch.setattr(_native, "comm_unique_id", lambda: b"\0" * 128)
    group = multigpu.DeviceGroup([5, 6])
    try:
        with pytest.raises(RuntimeError, match="deadline"):
            group.exchange(lambda comm, rank, device, item: comm.wait(0), [None, None])
        assert group._comms is None and len(closed) == 2  # dropped and closed, not cached
        assert group.exchange(lambda comm, rank, device, item: (comm.wait(0), comm.generation)[1], [None, None]) == [1, 1]
        assert len(made) == 4 and group._comms is not None  # the second exchange ran on new communicators
        # ANY exception out of an exchange drops them (a MemoryError / NotImplementedError on one rank between two
        # collectives leaves its peers inside the next one) — the following exchange builds the third generation
        with pytest.raises(ValueError):
            group.exchange(lambda comm, rank, device, item: (_ for _ in ()).throw(ValueError("raised on one rank mid-exchange")), [None, None])
        assert group._comms is None and len(closed) == 4
        assert group.exchange(lambda comm, rank, device, item: comm.generation, [None, None]) == [2, 2]
    finally:
        group.close()


def test_a_rendezvous_that_fails_on_one_rank_closes_what_the_other_ranks_built(monkeypatch):
    """`comms()` ran outside the try and kept nothing of a half-built set — the communicators the other ranks'
    threads had created were neither cached nor closed.  Now they are closed on their own GPU threads, and the next exchange
    starts from scratch."""
    made, closed = [], []
    fail_first = [True]

    class CommDouble:
        def __init__(self, device, rank, world, uid):
            if rank == 1 and fail_first[0]:
                fail_first[0] = False
                raise RuntimeError("XHIST_ERR_COMM: rank 1 of 2: the rendezvous deadline passed")
            self.rank = rank
            made.append(self)

        def close(self):
            closed.append(self)

    monkeypatch.setattr(_native, "Comm", CommDouble)
    monkeypatch.setattr(_native, "comm_unique_id", lambda: b"\0" * 128)
    group = multigpu.DeviceGroup([5, 6])
    try:
        with pytest.raises(RuntimeError, match="rendezvous"):
            group.exchange(lambda comm, rank, device, item: rank, [None, None])
        assert group._comms is None and len(made) == 1 and closed == made  # rank 0's communicator was closed, not leaked
        assert group.exchange(lambda comm, rank, device, item: rank, [None, None]) == [0, 1]
        assert len(made) == 3 and group._comms is not None
    finally:
        group.close()
