"""bench.py --dump-outputs: what the main leg's last step computed lands in DIR as float64 .npy files (CPU: the
--selftest plan double stands in for the kernel), and --steps is the number of timed steps the line reports."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_selftest_dumps_the_main_legs_output(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--selftest", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    assert sorted(os.listdir(out)) == ["bin_edges_0.npy", "hist.npy"]
    h = np.load(out / "hist.npy")
    assert h.dtype == np.float64 and h.shape == (100,)
    np.testing.assert_array_equal(h, np.ones(100))  # the plan double's "histogram"
    np.testing.assert_array_equal(np.load(out / "bin_edges_0.npy"), np.linspace(-4.0, 4.0, 101))


@pytest.mark.parametrize("steps", [3, 4])
def test_two_ranks_dump_the_reduced_histogram_of_the_last_step(tmp_path, steps):
    """--gpus 2 --selftest (gloo, CPU): every rank's plan double writes ones, the partials are all-reduced, so the histogram a
    caller receives is 2 everywhere — whichever of the two result buffers the last timed step used (odd and even launch counts)"""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--selftest", "--steps", str(steps), "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][0])
    assert d["steps"] == steps and d["n_gpus"] == 2 and d["allreduce_ms_alone"] is not None
    np.testing.assert_array_equal(np.load(out / "hist.npy"), 2 * np.ones(100))


@pytest.mark.parametrize("bad",[["--steps", "0"], ["--warmup", "-1"]])
def test_step_counts_are_checked(bad):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--selftest"] + bad,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and r.stdout.strip() == ""


def test_large_outputs_are_a_fixed_sample(tmp_path, monkeypatch):
    edges = [np.linspace(0.0, 1.0, 65), np.linspace(0.0, 1.0, 33)]
    hist = torch.arange(64 * 32, dtype=torch.int64).reshape(64, 32)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 8 * (65 + 33 + 200))
    got = []
    for k in range(2):
        bench.dump_outputs(str(tmp_path / str(k)), hist, edges)
        got.append({n: np.load(tmp_path / str(k) / n) for n in sorted(os.listdir(tmp_path / str(k)))})
    a, b = got
    assert sorted(a) == ["bin_edges_0.npy", "bin_edges_1.npy", "hist_sample.npy", "hist_sample_index.npy"]
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_LIMIT_BYTES
    idx = a["hist_sample_index.npy"]
    assert idx.dtype == np.float64 and len(idx) == 100 and np.all(np.diff(idx) > 0)
    np.testing.assert_array_equal(a["hist_sample.npy"], idx)  # hist[i] == i: the values are those of the sampled bins
    for n in a:
        np.testing.assert_array_equal(a[n], b[n])  # the same sample every time
