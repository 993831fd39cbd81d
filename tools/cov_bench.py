#!/usr/bin/env python
"""histogram_cov against the weighted histogram_mean_var (the same three streams and two passes) and against the three-call
workaround cov = (var(a + b) - var(a) - var(b)) / 2 (histogram_mean_var of a, of b and of a precomputed a + b) on the same
arrays, in the same process: device-event times after warm-up, the calls alternating, the median and minimum of each, one JSON
line per shape (printed, and written to --out) with the cov call's describe() line.  The bytes each cov pass reads (samples +
both value arrays) give its streaming rate against 8 TB/s.

    python tools/cov_bench.py [--reps 20] [--only c2,c4,d2,ts] [--out profiles/cov_bench.jsonl]

Per-pass times (cov_sum_* against mvw_sum_*, cov_dev_* against mvw_dev_*): run this under `rocprofv3 --kernel-trace --stats`,
in a run of its own.

Shapes: C2 (10^9 float64 samples and two float64 value arrays, 100 bins), C4's shard ((456, 720, 1440) float32 over lat / lon,
50 bins), 2e8 float64 pairs in 50 x 50 bins (d2: the fast family's two-input form, whose passes read a tile in two halves),
and the tutorial's 279 x 339 T-S bins (ts: 2e8 float64 pairs; beyond LDS, the generic kernels with float64 atomics in L2)."""
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


def case(name, args, a, b, bins, axis, reps, out, pass_bytes):
    cov = lambda: core.histogram_cov(*args, values=(a, b), bins=bins, axis=axis)  # noqa: E731
    mvw = lambda: core.histogram_mean_var(*args, values=a, weights=b, bins=bins, axis=axis)  # noqa: E731
    ab = a + b  # (precomputed: the workaround is not charged for forming it)

    def three():
        for v in (a, b, ab):
            core.histogram_mean_var(*args, values=v, bins=bins, axis=axis)

    for _ in range(3):
        cov()
        mvw()
        three()
    tc, tw, t3 = [], [], []
    for _ in range(reps):
        tc.append(timed(cov))
        tw.append(timed(mvw))
        t3.append(timed(three))
    cov()  # (the plan's describe() line is that of its last call)
    torch.cuda.synchronize()
    edges = [np.asarray(e, np.float64) for e in bins]
    desc = core._get_plan(edges, _native.CMP_F64, torch.cuda.current_device()).describe()
    mc, mw, m3 = statistics.median(tc), statistics.median(tw), statistics.median(t3)
    line = json.dumps({"case": name, "cov_ms": round(mc, 4), "weighted_mean_var_ms": round(mw, 4), "three_mean_var_calls_ms": round(m3, 4),
                       "cov_over_weighted_mean_var": round(mc / mw, 3), "three_calls_over_cov": round(m3 / mc, 3),
                       "cov_min_ms": round(min(tc), 4), "weighted_mean_var_min_ms": round(min(tw), 4),
                       "three_mean_var_calls_min_ms": round(min(t3), 4), "pass_bytes": pass_bytes,
                       "call_rate_of_8TBs": round(2 * pass_bytes / (mc * 1e-3) / PEAK, 3), "reps": reps, "describe": desc})
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="c2,c4,d2,ts")
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
        case("c2: 1e9 f64 samples and two value arrays, 100 bins", [x], a, b, [np.linspace(-4, 4, 101)], None, opt.reps, out, 24 * n)
        del x, a, b
    if "c4" in only:
        shape = (456, 720, 1440)
        n = int(np.prod(shape))
        x = torch.randn(shape, dtype=torch.float32, device=dev, generator=g)
        a = torch.rand(shape, dtype=torch.float32, device=dev, generator=g)
        b = torch.rand(shape, dtype=torch.float32, device=dev, generator=g)
        case("c4: (456, 720, 1440) f32 over lat/lon, 50 bins", [x], a, b, [np.linspace(-4, 4, 51)], (1, 2), opt.reps, out, 12 * n)
        del x, a, b
    if "d2" in only:
        n = 2 * 10 ** 8
        x = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        y = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        a = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
        b = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
        case("d2: 2e8 f64 pairs, 50 x 50 bins", [x, y], a, b, [np.linspace(-4, 4, 51)] * 2, None, opt.reps, out, 32 * n)
        del x, y, a, b
    if "ts" in only:
        n = 2 * 10 ** 8
        t = 15 + 8 * torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        s = 34.5 + torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        a = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
        b = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
        case("ts: 2e8 f64 T-S pairs, 279 x 339 bins", [s, t], a, b, [np.arange(31, 38, .025), np.arange(-2, 32, .1)], None, opt.reps, out,
             32 * n)
        del t, s, a, b
    if out:
        out.close()


if __name__ == "__main__":
    main()
