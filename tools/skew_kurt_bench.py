#!/usr/bin/env python
"""histogram_skew_kurt, unweighted and weighted, against histogram_mean_var (the same pass 1; pass 2 adds two sums on a 24-byte
slot where skew_kurt adds four on a 40-byte one) and against histogram_cov (five sums on a 56-byte slot, one stream more) on the
same arrays, in the same process: device-event times after warm-up, the calls alternating, the median and minimum of each, one
JSON line per shape (printed, and written to --out) with the describe() lines of the two skew_kurt calls.  `in_bracket` says
whether the unweighted call's median lies between mean_var's and cov's.

    python tools/skew_kurt_bench.py [--reps 20] [--only c2,c4,d2,ts] [--out profiles/skew_kurt_bench.jsonl]

Per-pass times (sk_dev_* against mv_dev_* and cov_dev_*): run this under `rocprofv3 --kernel-trace --stats`, in a run of its own.

Shapes: C2 (10^9 float64 samples and values, 100 bins), C4's shard ((456, 720, 1440) float32 over lat / lon, 50 bins), 2e8
float64 pairs in 50 x 50 bins (d2) and the tutorial's 279 x 339 T-S bins (ts: 2e8 float64 pairs; 94 581 bins of 40 bytes are
beyond LDS, so the sums are global atomics)."""
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


def case(name, args, v, b, w, bins, axis, reps, out):
    edges = [np.asarray(e, np.float64) for e in bins]
    plan = core._get_plan(edges, _native.CMP_F64, torch.cuda.current_device())
    fns = {
        "skew_kurt": lambda: core.histogram_skew_kurt(*args, values=v, bins=bins, axis=axis),
        "skew_kurt_w": lambda: core.histogram_skew_kurt(*args, values=v, weights=w, bins=bins, axis=axis),
        "mean_var": lambda: core.histogram_mean_var(*args, values=v, bins=bins, axis=axis),
        "mean_var_w": lambda: core.histogram_mean_var(*args, values=v, weights=w, bins=bins, axis=axis),
        "cov": lambda: core.histogram_cov(*args, values=(v, b), bins=bins, axis=axis),
    }
    desc = {}
    for _ in range(3):
        for k, f in fns.items():
            f()
            torch.cuda.synchronize()
            desc[k] = plan.describe()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            times[k].append(timed(f))
    m = {k: statistics.median(t) for k, t in times.items()}
    rec = {"case": name}
    for k in fns:
        rec[k + "_ms"] = round(m[k], 4)
        rec[k + "_min_ms"] = round(min(times[k]), 4)
    rec.update({"skew_kurt_over_mean_var": round(m["skew_kurt"] / m["mean_var"], 3), "skew_kurt_over_cov": round(m["skew_kurt"] / m["cov"], 3),
                "skew_kurt_w_over_mean_var_w": round(m["skew_kurt_w"] / m["mean_var_w"], 3),
                "in_bracket": bool(m["mean_var"] <= m["skew_kurt"] <= m["cov"]), "reps": reps,
                "describe": desc["skew_kurt"], "describe_w": desc["skew_kurt_w"]})
    line = json.dumps(rec)
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

    def rand(shape, dt):
        return torch.rand(shape, dtype=dt, device=dev, generator=g)

    if "c2" in only:
        n = 10 ** 9
        x = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        v, b, w = (rand(n, torch.float64) for _ in range(3))
        case("c2: 1e9 f64 samples and values, 100 bins", [x], v, b, w, [np.linspace(-4, 4, 101)], None, opt.reps, out)
        del x, v, b, w
    if "c4" in only:
        shape = (456, 720, 1440)
        x = torch.randn(shape, dtype=torch.float32, device=dev, generator=g)
        v, b, w = (rand(shape, torch.float32) for _ in range(3))
        case("c4: (456, 720, 1440) f32 over lat/lon, 50 bins", [x], v, b, w, [np.linspace(-4, 4, 51)], (1, 2), opt.reps, out)
        del x, v, b, w
    if "d2" in only:
        n = 2 * 10 ** 8
        x = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        y = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        v, b, w = (rand(n, torch.float64) for _ in range(3))
        case("d2: 2e8 f64 pairs, 50 x 50 bins", [x, y], v, b, w, [np.linspace(-4, 4, 51)] * 2, None, opt.reps, out)
        del x, y, v, b, w
    if "ts" in only:
        n = 2 * 10 ** 8
        t = 15 + 8 * torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        s = 34.5 + torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        v, b, w = (rand(n, torch.float64) for _ in range(3))
        case("ts: 2e8 f64 T-S pairs, 279 x 339 bins", [s, t], v, b, w, [np.arange(31, 38, .025), np.arange(-2, 32, .1)], None, opt.reps, out)
        del t, s, v, b, w
    if out:
        out.close()


if __name__ == "__main__":
    main()
