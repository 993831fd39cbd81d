#!/usr/bin/env python
"""histogram_extrema against the weighted histogram of the same arrays, in the same process: device-event times after
warm-up, the two calls alternating, the median of each and their ratio, one JSON line per shape.

    python tools/extrema_bench.py [--reps 20] [--only c2,c4,c3,global,adversarial]

Shapes: C2 (10^9 float64 samples, float64 values, 100 bins), C4's shard ((456, 720, 1440) float32 over lat / lon, 50 bins,
float32 values), C3's 256 x 256 random edges (float64), 1024 x 1024 bins (keys in global memory), and an adversarial case
whose values increase with position, so that every sample improves its bin's maximum."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xhistogram_amd import core  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def case(name, args, values, bins, axis, reps):
    ext = lambda: core.histogram_extrema(*args, values=values, bins=bins, axis=axis)  # noqa: E731
    hist = lambda: core.histogram(*args, weights=values, bins=bins, axis=axis)  # noqa: E731
    for _ in range(3):
        ext()
        hist()
    te, th = [], []
    for _ in range(reps):
        te.append(timed(ext))
        th.append(timed(hist))
    me, mh = statistics.median(te), statistics.median(th)
    print(json.dumps({"case": name, "extrema_ms": round(me, 4), "weighted_hist_ms": round(mh, 4), "ratio": round(me / mh, 3),
                      "extrema_min_ms": round(min(te), 4), "weighted_hist_min_ms": round(min(th), 4), "reps": reps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="c2,c4,c3,global,adversarial")
    opt = ap.parse_args()
    only = set(opt.only.split(","))
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    dev = "cuda"
    if "c2" in only:
        x = torch.randn(10 ** 9, dtype=torch.float64, device=dev, generator=g)
        v = torch.rand(10 ** 9, dtype=torch.float64, device=dev, generator=g)
        case("c2: 1e9 f64, f64 values, 100 bins", [x], v, [np.linspace(-4, 4, 101)], None, opt.reps)
        del x, v
    if "c4" in only:
        x = torch.randn((456, 720, 1440), dtype=torch.float32, device=dev, generator=g)
        v = torch.rand((456, 720, 1440), dtype=torch.float32, device=dev, generator=g)
        case("c4: (456, 720, 1440) f32 over lat/lon, 50 bins", [x], v, [np.linspace(-4, 4, 51)], (1, 2), opt.reps)
        del x, v
    if "c3" in only:
        rng = np.random.default_rng(3)
        e = [np.sort(rng.uniform(-4, 4, 257)) for _ in range(2)]
        x = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
        y = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
        v = torch.rand(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
        case("c3: 2e8 f64 pairs, 256 x 256 random edges", [x, y], v, e, None, opt.reps)
        del x, y, v
    if "global" in only:
        x = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
        y = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
        v = torch.rand(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
        case("global: 2e8 f64 pairs, 1024 x 1024 bins", [x, y], v, [np.linspace(-4, 4, 1025)] * 2, None, opt.reps)
        del x, y, v
    if "adversarial" in only:
        x = torch.randn(10 ** 9, dtype=torch.float64, device=dev, generator=g)
        v = torch.arange(10 ** 9, dtype=torch.float64, device=dev)
        case("adversarial: 1e9 f64, values increasing with position, 100 bins", [x], v, [np.linspace(-4, 4, 101)], None, opt.reps)


if __name__ == "__main__":
    main()
