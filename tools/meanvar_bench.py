#!/usr/bin/env python
"""histogram_mean_var against the weighted histogram of the same arrays, in the same process: device-event times after
warm-up, the two calls alternating, the median and minimum of each and the ratio of the medians, one JSON line per shape
(printed, and written to --out).

    python tools/meanvar_bench.py [--reps 20] [--only c2,c4,c3,global] [--out profiles/meanvar_bench.jsonl]

Shapes: C2 (10^9 float64 samples, float64 values, 100 bins), C4's shard ((456, 720, 1440) float32 over lat / lon, 50 bins,
float32 values), C3's 256 x 256 random edges (float64), and 1024 x 1024 bins (sums in global memory).  Each line also carries
the plan's describe() line: which kernel family ran each pass and where its slots lived."""
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
    mv = lambda: core.histogram_mean_var(*args, values=values, bins=bins, axis=axis)  # noqa: E731
    hist = lambda: core.histogram(*args, weights=values, bins=bins, axis=axis)  # noqa: E731
    for _ in range(3):
        mv()
        hist()
    tm, th = [], []
    for _ in range(reps):
        tm.append(timed(mv))
        th.append(timed(hist))
    mm, mh = statistics.median(tm), statistics.median(th)
    mv()  # (the plan's describe() line is that of its last call)
    torch.cuda.synchronize()
    edges = [np.asarray(b, np.float64) for b in bins]
    desc = core._get_plan(edges, _native.CMP_F64, torch.cuda.current_device()).describe()
    line = json.dumps({"case": name, "mean_var_ms": round(mm, 4), "weighted_hist_ms": round(mh, 4), "ratio": round(mm / mh, 3),
                       "mean_var_min_ms": round(min(tm), 4), "weighted_hist_min_ms": round(min(th), 4), "reps": reps,
                       "describe": desc})
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="c2,c4,c3,global")
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    only = set(opt.only.split(","))
    out = open(opt.out, "w") if opt.out else None
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    dev = "cuda"
    if "c2" in only:
        x = torch.randn(10 ** 9, dtype=torch.float64, device=dev, generator=g)
        v = torch.rand(10 ** 9, dtype=torch.float64, device=dev, generator=g)
        case("c2: 1e9 f64, f64 values, 100 bins", [x], v, [np.linspace(-4, 4, 101)], None, opt.reps, out)
        del x, v
    if "c4" in only:
        x = torch.randn((456, 720, 1440), dtype=torch.float32, device=dev, generator=g)
        v = torch.rand((456, 720, 1440), dtype=torch.float32, device=dev, generator=g)
        case("c4: (456, 720, 1440) f32 over lat/lon, 50 bins", [x], v, [np.linspace(-4, 4, 51)], (1, 2), opt.reps, out)
        del x, v
    if "c3" in only:
        rng = np.random.default_rng(3)
        e = [np.sort(rng.uniform(-4, 4, 257)) for _ in range(2)]
        x = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
        y = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
        v = torch.rand(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
        case("c3: 2e8 f64 pairs, 256 x 256 random edges", [x, y], v, e, None, opt.reps, out)
        del x, y, v
    if "global" in only:
        x = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
        y = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
        v = torch.rand(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
        case("global: 2e8 f64 pairs, 1024 x 1024 bins", [x, y], v, [np.linspace(-4, 4, 1025)] * 2, None, opt.reps, out)
        del x, y, v
    if out:
        out.close()


if __name__ == "__main__":
    main()
