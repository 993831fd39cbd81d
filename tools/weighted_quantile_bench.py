#!/usr/bin/env python
"""histogram_weighted_quantile against histogram_quantile(method="lower") and the weighted histogram_mean_var of the same
arrays, in the same process: device-event times after warm-up, the three calls alternating, the median and minimum of each and
the ratios of the medians, one JSON line per shape (printed, and written to --out).

    python tools/weighted_quantile_bench.py [--reps 10] [--only c2,c2q,c4,c4area,time,edge] [--out profiles/weighted_quantile_bench.jsonl]

Shapes: C2 (10^9 float64 samples, values and weights, 100 bins) median and quartiles, C4's shard ((456, 720, 1440) float32 over
lat / lon, 50 bins) median with weights of full shape and with (lat, lon) weights broadcast over time, (365, 720, 1440) float32
over time with 50 bins (the short-row family), and the short-row bound: 2000 rows of 2048 values (short) against 2049 (radix).
Each line carries the plan's describe() line of the weighted call: the family, the kernel family and home of each pass, d, the
passes and chunks.  Under a profiler (--only one shape, --no-unweighted) the kernel times of the passes stand next to mvw_sum_*
of the same arrays in the same run."""
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


def case(name, args, values, weights, bins, axis, q, reps, out, unweighted=True):
    wq = lambda: core.histogram_weighted_quantile(*args, values=values, weights=weights, q=q, bins=bins, axis=axis)  # noqa: E731
    uq = lambda: core.histogram_quantile(*args, values=values, q=q, bins=bins, axis=axis, method="lower")  # noqa: E731
    mv = lambda: core.histogram_mean_var(*args, values=values, weights=weights, bins=bins, axis=axis)  # noqa: E731
    calls = [wq, mv] + ([uq] if unweighted else [])
    for _ in range(2):
        for f in calls:
            f()
    t = [[] for _ in calls]
    for _ in range(reps):
        for ts, f in zip(t, calls):
            ts.append(timed(f))
    med = [statistics.median(ts) for ts in t]
    wq()  # (the plan's describe() line is that of its last call)
    torch.cuda.synchronize()
    edges = [np.asarray(b, np.float64) for b in bins]
    desc = core._get_plan(edges, _native.CMP_F64, torch.cuda.current_device()).describe()
    rec = {"case": name, "weighted_quantile_ms": round(med[0], 4), "weighted_mean_var_ms": round(med[1], 4),
           "ratio_to_weighted_mean_var": round(med[0] / med[1], 3), "weighted_quantile_min_ms": round(min(t[0]), 4), "reps": reps}
    if unweighted:
        rec.update({"quantile_lower_ms": round(med[2], 4), "ratio_to_quantile_lower": round(med[0] / med[2], 3),
                    "quantile_lower_min_ms": round(min(t[2]), 4)})
    m = [f for f in desc.split() if f.startswith("passes=")]
    if m and "family=radix" in desc:
        rec["streams_launched"] = int(m[0].split("=")[1]) + 1  # pass 0 and the digit passes
    rec["describe"] = desc
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def exact_weights(shape, dtype, dev, g):
    """tests/exact_weights.py on the device: (2^24 + k) * 2^-25 (float32: (2^23 + k) * 2^-24)"""
    bits = 23 if dtype == torch.float32 else 24
    k = torch.randint(0, 1 << bits, shape, dtype=torch.int64, device=dev, generator=g)
    return ((k + (1 << bits)).to(torch.float64) * 2.0 ** -(bits + 1)).to(dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="c2,c2q,c4,c4area,time,edge")
    ap.add_argument("--no-unweighted", action="store_true", help="skip histogram_quantile (profiler passes)")
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    only = set(opt.only.split(","))
    out = open(opt.out, "w") if opt.out else None
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    dev = "cuda"
    unw = not opt.no_unweighted
    if "c2" in only or "c2q" in only:
        x = torch.randn(10 ** 9, dtype=torch.float64, device=dev, generator=g)
        v = torch.rand(10 ** 9, dtype=torch.float64, device=dev, generator=g)
        w = exact_weights((10 ** 9,), torch.float64, dev, g)
        e = [np.linspace(-4, 4, 101)]
        if "c2" in only:
            case("c2: 1e9 f64, f64 values and weights, 100 bins, median", [x], v, w, e, None, 0.5, opt.reps, out, unw)
        if "c2q" in only:
            case("c2: 1e9 f64, f64 values and weights, 100 bins, quartiles", [x], v, w, e, None, [0.25, 0.75], opt.reps, out, unw)
        del x, v, w
    if "c4" in only or "c4area" in only:
        x = torch.randn((456, 720, 1440), dtype=torch.float32, device=dev, generator=g)
        v = torch.rand((456, 720, 1440), dtype=torch.float32, device=dev, generator=g)
        e = [np.linspace(-4, 4, 51)]
        if "c4" in only:
            w = exact_weights((456, 720, 1440), torch.float32, dev, g)
            case("c4: (456, 720, 1440) f32 over lat/lon, full weights, 50 bins, median", [x], v, w, e, (1, 2), 0.5, opt.reps, out, unw)
            del w
        if "c4area" in only:
            w = exact_weights((720, 1440), torch.float32, dev, g)
            case("c4: (456, 720, 1440) f32 over lat/lon, (lat, lon) weights, 50 bins, median", [x], v, w, e, (1, 2), 0.5, opt.reps, out, unw)
            del w
        del x, v
    if "time" in only:
        x = torch.randn((365, 720, 1440), dtype=torch.float32, device=dev, generator=g)
        v = torch.rand((365, 720, 1440), dtype=torch.float32, device=dev, generator=g)
        w = exact_weights((365, 720, 1440), torch.float32, dev, g)
        case("time: (365, 720, 1440) f32 over time, 50 bins, median", [x], v, w, [np.linspace(-4, 4, 51)], (0,), 0.5, opt.reps, out, unw)
        del x, v, w
    if "edge" in only:
        for cols in (2048, 2049):
            x = torch.randn((2000, cols), dtype=torch.float32, device=dev, generator=g)
            v = torch.rand((2000, cols), dtype=torch.float32, device=dev, generator=g)
            w = exact_weights((2000, cols), torch.float32, dev, g)
            case("edge: 2000 rows x %d f32, 100 bins, median" % cols, [x], v, w, [np.linspace(-4, 4, 101)], (1,), 0.5, opt.reps, out, unw)
            del x, v, w
    if out:
        out.close()


if __name__ == "__main__":
    main()
