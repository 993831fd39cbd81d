#!/usr/bin/env python
"""histogram_mean_var with weights against the unweighted call and the two-weights idiom (mean only) on the same arrays, in
the same process: device-event times after warm-up, the three calls alternating, the median and minimum of each, one JSON
line per shape (printed, and written to --out) with the weighted call's describe() line.  The bytes each weighted pass reads
(samples + values + weights) give its streaming rate against 8 TB/s.

    python tools/meanvar_weighted_bench.py [--reps 20] [--only c2,c4,c4b,d2,ts] [--out profiles/meanvar_weighted_bench.jsonl]

Shapes: C2 (10^9 float64 samples, values and weights, 100 bins), C4's shard ((456, 720, 1440) float32 over lat / lon, 50
bins), the shard with (lat, lon) weights broadcast over time (c4b), 2e8 float64 pairs in 50 x 50 bins (d2: the fast family's
two-input form, whose weighted passes read a tile in two halves), and the tutorial's 279 x 339 T-S bins (ts: 2e8 float64
pairs; beyond LDS, the generic kernels with float64 atomics in L2)."""
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


def case(name, args, values, weights, bins, axis, reps, out, pass_bytes):
    mvw = lambda: core.histogram_mean_var(*args, values=values, weights=weights, bins=bins, axis=axis)  # noqa: E731
    mv = lambda: core.histogram_mean_var(*args, values=values, bins=bins, axis=axis)  # noqa: E731
    vw = values * weights
    two = lambda: core.histogram_two_weights(*args, weights=(vw, weights.expand_as(values)), bins=bins, axis=axis)  # noqa: E731
    for _ in range(3):
        mvw()
        mv()
        two()
    tw, tu, tt = [], [], []
    for _ in range(reps):
        tw.append(timed(mvw))
        tu.append(timed(mv))
        tt.append(timed(two))
    mvw()  # (the plan's describe() line is that of its last call)
    torch.cuda.synchronize()
    edges = [np.asarray(b, np.float64) for b in bins]
    desc = core._get_plan(edges, _native.CMP_F64, torch.cuda.current_device()).describe()
    mw, mu, mt = statistics.median(tw), statistics.median(tu), statistics.median(tt)
    line = json.dumps({"case": name, "weighted_mean_var_ms": round(mw, 4), "mean_var_ms": round(mu, 4), "two_weights_ms": round(mt, 4),
                       "weighted_over_unweighted": round(mw / mu, 3), "weighted_min_ms": round(min(tw), 4), "mean_var_min_ms": round(min(tu), 4),
                       "two_weights_min_ms": round(min(tt), 4), "pass_bytes": pass_bytes,
                       "call_rate_of_8TBs": round(2 * pass_bytes / (mw * 1e-3) / PEAK, 3), "reps": reps, "describe": desc})
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="c2,c4,c4b,d2,ts")
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
        v = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
        w = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
        case("c2: 1e9 f64 samples, values, weights, 100 bins", [x], v, w, [np.linspace(-4, 4, 101)], None, opt.reps, out, 24 * n)
        del x, v, w
    if "c4" in only or "c4b" in only:
        shape = (456, 720, 1440)
        n = int(np.prod(shape))
        x = torch.randn(shape, dtype=torch.float32, device=dev, generator=g)
        v = torch.rand(shape, dtype=torch.float32, device=dev, generator=g)
        if "c4" in only:
            w = torch.rand(shape, dtype=torch.float32, device=dev, generator=g)
            case("c4: (456, 720, 1440) f32 over lat/lon, 50 bins", [x], v, w, [np.linspace(-4, 4, 51)], (1, 2), opt.reps, out, 12 * n)
            del w
        if "c4b" in only:
            area = torch.rand((720, 1440), dtype=torch.float32, device=dev, generator=g)
            case("c4b: the shard, (lat, lon) weights broadcast over time", [x], v, area.expand(shape), [np.linspace(-4, 4, 51)], (1, 2),
                 opt.reps, out, 8 * n + 4 * 720 * 1440)
            del area
        del x, v
    if "d2" in only:
        n = 2 * 10 ** 8
        x = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        y = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        v = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
        w = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
        case("d2: 2e8 f64 pairs, 50 x 50 bins", [x, y], v, w, [np.linspace(-4, 4, 51)] * 2, None, opt.reps, out, 32 * n)
        del x, y, v, w
    if "ts" in only:
        n = 2 * 10 ** 8
        t = 15 + 8 * torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        s = 34.5 + torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        o2 = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
        dv = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
        case("ts: 2e8 f64 T-S pairs, 279 x 339 bins", [s, t], o2, dv, [np.arange(31, 38, .025), np.arange(-2, 32, .1)], None, opt.reps, out,
             32 * n)
        del t, s, o2, dv
    if out:
        out.close()


if __name__ == "__main__":
    main()
