#!/usr/bin/env python
"""histogram_argextrema against histogram_extrema on the same arrays, in the same process: device-event times after warm-up,
the two calls alternating, the median of each and their ratio, one JSON line per shape.  The expectation is bytes moved: two
passes over the streams histogram_extrema reads once, so twice its time.

    python tools/argextrema_bench.py [--reps 20] [--only c2,c4,d2,ts,ties] [--out FILE]

Shapes: C2 (10^9 float64 samples and values, 100 bins), C4's shard ((456, 720, 1440) float32 over lat / lon, 50 bins), 2e8
float64 pairs in 50 x 50 bins (d2), the tutorial's 279 x 339 T-S bins (ts: 2e8 float64 pairs; 94 581 bins of 32 bytes are
beyond LDS, the generic kernels on global memory), and C2's shape with constant values (ties: every counted sample holds its
bin's minimum and its maximum, so every sample reaches the position filter)."""
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
    arg = lambda: core.histogram_argextrema(*args, values=values, bins=bins, axis=axis)  # noqa: E731
    ext = lambda: core.histogram_extrema(*args, values=values, bins=bins, axis=axis)  # noqa: E731
    plan = core._get_plan([np.asarray(b, np.float64) for b in bins], _native.CMP_F64, 0)
    for _ in range(3):
        ext()
        arg()
    torch.cuda.synchronize()
    desc = plan.describe()
    ta, te = [], []
    for _ in range(reps):
        ta.append(timed(arg))
        te.append(timed(ext))
    ma, me = statistics.median(ta), statistics.median(te)
    line = json.dumps({"case": name, "argextrema_ms": round(ma, 4), "extrema_ms": round(me, 4), "ratio": round(ma / me, 3),
                       "argextrema_min_ms": round(min(ta), 4), "extrema_min_ms": round(min(te), 4), "reps": reps, "describe": desc})
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="c2,c4,d2,ts,ties")
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    only = set(opt.only.split(","))
    out = open(opt.out, "w") if opt.out else None
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    dev = "cuda"
    if "c2" in only or "ties" in only:
        n = 10 ** 9
        x = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        if "c2" in only:
            v = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
            case("c2: 1e9 f64 samples and values, 100 bins", [x], v, [np.linspace(-4, 4, 101)], None, opt.reps, out)
            del v
        if "ties" in only:
            v = torch.full((n,), 1.5, dtype=torch.float64, device=dev)
            case("ties: c2's shape, constant values", [x], v, [np.linspace(-4, 4, 101)], None, opt.reps, out)
            del v
        del x
    if "c4" in only:
        shape = (456, 720, 1440)
        x = torch.randn(shape, dtype=torch.float32, device=dev, generator=g)
        v = torch.rand(shape, dtype=torch.float32, device=dev, generator=g)
        case("c4: (456, 720, 1440) f32 over lat/lon, 50 bins", [x], v, [np.linspace(-4, 4, 51)], (1, 2), opt.reps, out)
        del x, v
    if "d2" in only:
        n = 2 * 10 ** 8
        x = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        y = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        v = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
        case("d2: 2e8 f64 pairs, 50 x 50 bins", [x, y], v, [np.linspace(-4, 4, 51)] * 2, None, opt.reps, out)
        del x, y, v
    if "ts" in only:
        n = 2 * 10 ** 8
        t = 15 + 8 * torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        s = 34.5 + torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        v = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
        case("ts: 2e8 f64 T-S pairs, 279 x 339 bins", [s, t], v, [np.arange(31, 38, .025), np.arange(-2, 32, .1)], None, opt.reps, out)
        del t, s, v
    if out:
        out.close()


if __name__ == "__main__":
    main()
