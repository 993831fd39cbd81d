#!/usr/bin/env python
"""histogram_sum against histogram_mean_var on the same arrays, in the same process: device-event times after warm-up, the two
calls alternating, the median and minimum of each and the ratio of the medians, one JSON line per shape (printed, and written
to --out).  Both move the same bytes, two passes over samples and values; the bar is mean_var's median plus 10 %.

    python tools/sum_bench.py [--reps 20] [--only c2,c4,d2,ts] [--out profiles/sum_bench.jsonl]

Shapes: C2 (10^9 float64 samples and values, 100 bins), C4's shard ((456, 720, 1440) float32 over lat / lon, 50 bins), 2 x 10^8
float64 pairs in 50 x 50 bins (d2), and the tutorial's 279 x 339 T-S bins (ts: 2e8 float64 pairs; 94 581 bins of 32 bytes are
beyond LDS, the generic kernels with 64-bit integer atomics in L2 — recorded, not held to the bar).  The values are 1e8 + 1e3
N(0, 1) for the float64 shapes: offset data, where all three limbs of a value are in use.  Each line also carries the plan's
describe() line: which kernel family ran each pass and where its slots lived."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xhistogram_amd import _native, core  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def case(name, args, values, bins, axis, reps, out):
    sm = lambda: core.histogram_sum(*args, values=values, bins=bins, axis=axis)  # noqa: E731
    mv = lambda: core.histogram_mean_var(*args, values=values, bins=bins, axis=axis)  # noqa: E731
    for _ in range(3):
        sm()
        mv()
    ts, tm = [], []
    for _ in range(reps):
        ts.append(timed(sm))
        tm.append(timed(mv))
    ms, mm = statistics.median(ts), statistics.median(tm)
    sm()  # (the plan's describe() line is that of its last call)
    torch.cuda.synchronize()
    edges = [np.asarray(b, np.float64) for b in bins]
    desc = core._get_plan(edges, _native.CMP_F64, torch.cuda.current_device()).describe()
    line = json.dumps({"case": name, "sum_ms": round(ms, 4), "mean_var_ms": round(mm, 4), "ratio": round(ms / mm, 3),
                       "sum_min_ms": round(min(ts), 4), "mean_var_min_ms": round(min(tm), 4), "reps": reps, "describe": desc})
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def offset_values(shape, dtype, g):
    v = torch.randn(shape, dtype=dtype, device="cuda", generator=g)
    return v.mul_(1e3).add_(1e8) if dtype == torch.float64 else v


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
        v = offset_values(n, torch.float64, g)
        case("c2: 1e9 f64 samples and values, 100 bins", [x], v, [np.linspace(-4, 4, 101)], None, opt.reps, out)
        del x, v
    if "c4" in only:
        shape = (456, 720, 1440)
        x = torch.randn(shape, dtype=torch.float32, device=dev, generator=g)
        v = offset_values(shape, torch.float32, g)
        case("c4: (456, 720, 1440) f32 over lat/lon, 50 bins", [x], v, [np.linspace(-4, 4, 51)], (1, 2), opt.reps, out)
        del x, v
    if "d2" in only:
        n = 2 * 10 ** 8
        x = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        y = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        v = offset_values(n, torch.float64, g)
        case("d2: 2e8 f64 pairs, 50 x 50 bins", [x, y], v, [np.linspace(-4, 4, 51)] * 2, None, opt.reps, out)
        del x, y, v
    if "ts" in only:
        n = 2 * 10 ** 8
        t = 15 + 8 * torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        s = 34.5 + torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        v = offset_values(n, torch.float64, g)
        case("ts: 2e8 f64 T-S pairs, 279 x 339 bins", [s, t], v, [np.arange(31, 38, .025), np.arange(-2, 32, .1)], None, opt.reps, out)
        del t, s, v
    if out:
        out.close()


if __name__ == "__main__":
    main()
