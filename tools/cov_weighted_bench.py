#!/usr/bin/env python
"""histogram_weighted_cov against histogram_cov (the same passes with one stream fewer), against the weighted
histogram_mean_var (one value array and the weights) and against the three-call workaround cov = (var(a + b) - var(a) -
var(b)) / 2 (the weighted histogram_mean_var of a, of b and of a precomputed a + b) on the same arrays, in the same process:
device-event times after warm-up, the calls alternating, the median and minimum of each, one JSON line per shape (printed, and
written to --out) with the weighted cov call's describe() line.  The bytes each pass reads (samples + both value arrays +
weights) give its streaming rate against 8 TB/s, and the ratio of those bytes over histogram_cov's is what the weighted call
is expected to cost over it: 4/3 for one input, 5/4 for pairs.

    python tools/cov_weighted_bench.py [--reps 20] [--only c2,c4,c4b,d2] [--out profiles/cov_weighted_bench.jsonl]

Per-pass times (covw_sum_* against cov_sum_*, covw_dev_* against cov_dev_*): run this under `rocprofv3 --kernel-trace --stats`,
in a run of its own.

Shapes: C2 (10^9 float64 samples, two float64 value arrays and weights, 100 bins), C4's shard ((456, 720, 1440) float32 over
lat / lon, 50 bins), the shard with (lat, lon) weights broadcast over time (c4b), and 2e8 float64 pairs in 50 x 50 bins (d2: the
fast family's two-input form, five streams, whose passes read a tile in two halves)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xhistogram_amd import _native, core  # noqa: E402

PEAK = 8e12  # bytes / s


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def case(name, args, a, b, w, bins, axis, reps, out, pass_bytes, cov_pass_bytes):
    covw = lambda: core.histogram_weighted_cov(*args, values=(a, b), weights=w, bins=bins, axis=axis)  # noqa: E731
    cov = lambda: core.histogram_cov(*args, values=(a, b), bins=bins, axis=axis)  # noqa: E731
    mvw = lambda: core.histogram_mean_var(*args, values=a, weights=w, bins=bins, axis=axis)  # noqa: E731
    ab = a + b  # (precomputed: the workaround is not charged for forming it)

    def three():
        for v in (a, b, ab):
            core.histogram_mean_var(*args, values=v, weights=w, bins=bins, axis=axis)

    fns = (covw, cov, mvw, three)
    for _ in range(3):
        for f in fns:
            f()
    times = [[] for _ in fns]
    for _ in range(reps):
        for t, f in zip(times, fns):
            t.append(timed(f))
    covw()  # (the plan's describe() line is that of its last call)
    torch.cuda.synchronize()
    edges = [np.asarray(e, np.float64) for e in bins]
    desc = core._get_plan(edges, _native.CMP_F64, torch.cuda.current_device()).describe()
    m = [statistics.median(t) for t in times]
    line = json.dumps({"case": name, "weighted_cov_ms": round(m[0], 4), "cov_ms": round(m[1], 4), "weighted_mean_var_ms": round(m[2], 4),
                       "three_weighted_mean_var_calls_ms": round(m[3], 4), "weighted_cov_over_cov": round(m[0] / m[1], 3),
                       "byte_ratio_over_cov": round(pass_bytes / cov_pass_bytes, 3),
                       "weighted_cov_over_weighted_mean_var": round(m[0] / m[2], 3), "three_calls_over_weighted_cov": round(m[3] / m[0], 3),
                       "weighted_cov_min_ms": round(min(times[0]), 4), "cov_min_ms": round(min(times[1]), 4),
                       "weighted_mean_var_min_ms": round(min(times[2]), 4), "three_weighted_mean_var_calls_min_ms": round(min(times[3]), 4),
                       "pass_bytes": pass_bytes, "call_rate_of_8TBs": round(2 * pass_bytes / (m[0] * 1e-3) / PEAK, 3),
                       "cov_call_rate_of_8TBs": round(2 * cov_pass_bytes / (m[1] * 1e-3) / PEAK, 3), "reps": reps, "describe": desc})
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="c2,c4,c4b,d2")
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    only = set(opt.only.split(","))
    out = open(opt.out, "w") if opt.out else None
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    dev = "cuda"
    if "c2" in only:
        n = 10 ** 9
        x = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        a = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
        b = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
        w = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
        case("c2: 1e9 f64 samples, two value arrays and weights, 100 bins", [x], a, b, w, [np.linspace(-4, 4, 101)], None, opt.reps, out,
             32 * n, 24 * n)
        del x, a, b, w
    if "c4" in only or "c4b" in only:
        shape = (456, 720, 1440)
        n = int(np.prod(shape))
        x = torch.randn(shape, dtype=torch.float32, device=dev, generator=g)
        a = torch.rand(shape, dtype=torch.float32, device=dev, generator=g)
        b = torch.rand(shape, dtype=torch.float32, device=dev, generator=g)
        if "c4" in only:
            w = torch.rand(shape, dtype=torch.float32, device=dev, generator=g)
            case("c4: (456, 720, 1440) f32 over lat/lon, 50 bins", [x], a, b, w, [np.linspace(-4, 4, 51)], (1, 2), opt.reps, out, 16 * n, 12 * n)
            del w
        if "c4b" in only:
            area = torch.rand((720, 1440), dtype=torch.float32, device=dev, generator=g)
            case("c4b: the shard, (lat, lon) weights broadcast over time", [x], a, b, area.expand(shape), [np.linspace(-4, 4, 51)], (1, 2),
                 opt.reps, out, 12 * n + 4 * 720 * 1440, 12 * n)
            del area
        del x, a, b
    if "d2" in only:
        n = 2 * 10 ** 8
        x = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        y = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        a = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
        b = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
        w = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
        case("d2: 2e8 f64 pairs, 50 x 50 bins", [x, y], a, b, w, [np.linspace(-4, 4, 51)] * 2, None, opt.reps, out, 40 * n, 32 * n)
        del x, y, a, b, w
    if out:
        out.close()


if __name__ == "__main__":
    main()
