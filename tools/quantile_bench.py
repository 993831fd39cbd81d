#!/usr/bin/env python
"""histogram_quantile against the weighted histogram of the same arrays, in the same process: device-event times after
warm-up, the two calls alternating, the median and minimum of each and the ratio of the medians, one JSON line per shape
(printed, and written to --out).  Where memory allows, a torch restatement by sorting (values sorted, then stably by (row, bin))
is timed too, for context.

    python tools/quantile_bench.py [--reps 10] [--only c2,c2q,c4,time,global,edge] [--out profiles/quantile_bench.jsonl]

Shapes: C2 (10^9 float64 samples, float64 values, 100 bins) median and quartiles, C4's shard ((456, 720, 1440) float32 over
lat / lon, 50 bins) median, (365, 720, 1440) float32 over time with 50 bins (the short-row family), 1024 x 1024 bins (2 x 10^8
float64 pairs, counters in global memory), and the short-row threshold: 2000 rows of 4096 values (short) against 4097 (radix).
Each line carries the plan's describe() line: the family, the kernel family and home of each pass, d, the passes and chunks."""
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


def sort_quantile(x, v, edges, q, axis):
    """a torch restatement by sorting (linear method): each value's (row, bin), values sorted, then stably by (row, bin); the
    two order statistics of each target gathered and interpolated"""
    e = torch.as_tensor(edges, device=x.device, dtype=torch.float64)
    nb = len(edges) - 1
    if axis is not None:
        keep = [i for i in range(x.ndim) if i not in axis]
        x = x.permute(*keep, *axis).reshape(int(np.prod([x.shape[i] for i in keep])), -1)
        v = v.permute(*keep, *axis).reshape(x.shape)
    else:
        x, v = x.reshape(1, -1), v.reshape(1, -1)
    rows = x.shape[0]
    b = torch.bucketize(x.to(torch.float64), e, right=True) - 1
    b = torch.where(x.to(torch.float64) == e[-1], nb - 1, b)
    ok = (b >= 0) & (b < nb) & ~torch.isnan(v)
    key = (torch.arange(rows, device=x.device)[:, None] * nb + b)[ok]
    vals = v[ok].to(torch.float64)
    vals, o = torch.sort(vals)
    key = key[o]
    key, o = torch.sort(key, stable=True)
    vals = vals[o]
    n = torch.bincount(key, minlength=rows * nb)
    start = torch.cumsum(n, 0) - n
    out = []
    for qq in q:
        vi = (n - 1).to(torch.float64) * qq
        lo = torch.floor(vi).clamp(min=0).to(torch.int64)
        hi = torch.minimum(lo + 1, (n - 1).clamp(min=0))
        a = vals[(start + lo).clamp(max=len(vals) - 1)]
        c = vals[(start + hi).clamp(max=len(vals) - 1)]
        out.append(torch.where(n > 0, torch.lerp(a, c, vi - torch.floor(vi)), torch.nan))
    return torch.stack(out)


def case(name, args, values, bins, axis, q, reps, out, sort_ok=True):
    qt = lambda: core.histogram_quantile(*args, values=values, q=q, bins=bins, axis=axis)  # noqa: E731
    hist = lambda: core.histogram(*args, weights=values, bins=bins, axis=axis)  # noqa: E731
    for _ in range(2):
        qt()
        hist()
    tq, th = [], []
    for _ in range(reps):
        tq.append(timed(qt))
        th.append(timed(hist))
    mq, mh = statistics.median(tq), statistics.median(th)
    qt()  # (the plan's describe() line is that of its last call)
    torch.cuda.synchronize()
    edges = [np.asarray(b, np.float64) for b in bins]
    dom = _native.CMP_F64
    desc = core._get_plan(edges, dom, torch.cuda.current_device()).describe()
    rec = {"case": name, "quantile_ms": round(mq, 4), "weighted_hist_ms": round(mh, 4), "ratio": round(mq / mh, 3),
           "quantile_min_ms": round(min(tq), 4), "weighted_hist_min_ms": round(min(th), 4), "reps": reps, "describe": desc}
    m = [f for f in desc.split() if f.startswith("passes=")]
    if m and "family=radix" in desc:
        # streaming passes: pass 0, the digit passes, the successor — the ratio per pass against one weighted histogram
        streams = int(m[0].split("=")[1]) + 2
        rec["streams_launched"] = streams
    if sort_ok and len(args) == 1:
        try:
            qq = [q] if np.ndim(q) == 0 else list(q)
            sort_quantile(args[0], values, bins[0], qq, axis)
            ts = [timed(lambda: sort_quantile(args[0], values, bins[0], qq, axis)) for _ in range(3)]
            rec["torch_sort_ms"] = round(statistics.median(ts), 4)
        except torch.cuda.OutOfMemoryError:
            rec["torch_sort_ms"] = None
        torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="c2,c2q,c4,time,global,edge")
    ap.add_argument("--no-sort", action="store_true", help="skip the torch sort restatement (profiler passes)")
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    only = set(opt.only.split(","))
    out = open(opt.out, "w") if opt.out else None
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    dev = "cuda"
    srt = not opt.no_sort
    if "c2" in only or "c2q" in only:
        x = torch.randn(10 ** 9, dtype=torch.float64, device=dev, generator=g)
        v = torch.rand(10 ** 9, dtype=torch.float64, device=dev, generator=g)
        e = [np.linspace(-4, 4, 101)]
        if "c2" in only:
            case("c2: 1e9 f64, f64 values, 100 bins, median", [x], v, e, None, 0.5, opt.reps, out, srt)
        if "c2q" in only:
            case("c2: 1e9 f64, f64 values, 100 bins, quartiles", [x], v, e, None, [0.25, 0.75], opt.reps, out, srt)
        del x, v
    if "c4" in only:
        x = torch.randn((456, 720, 1440), dtype=torch.float32, device=dev, generator=g)
        v = torch.rand((456, 720, 1440), dtype=torch.float32, device=dev, generator=g)
        case("c4: (456, 720, 1440) f32 over lat/lon, 50 bins, median", [x], v, [np.linspace(-4, 4, 51)], (1, 2), 0.5, opt.reps, out, srt)
        del x, v
    if "time" in only:
        x = torch.randn((365, 720, 1440), dtype=torch.float32, device=dev, generator=g)
        v = torch.rand((365, 720, 1440), dtype=torch.float32, device=dev, generator=g)
        case("time: (365, 720, 1440) f32 over time, 50 bins, median", [x], v, [np.linspace(-4, 4, 51)], (0,), 0.5, opt.reps, out, srt)
        del x, v
    if "global" in only:
        x = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
        y = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
        v = torch.rand(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
        case("global: 2e8 f64 pairs, 1024 x 1024 bins, median", [x, y], v, [np.linspace(-4, 4, 1025)] * 2, None, 0.5, opt.reps, out, srt)
        del x, y, v
    if "edge" in only:
        for cols in (4096, 4097):
            x = torch.randn((2000, cols), dtype=torch.float32, device=dev, generator=g)
            v = torch.rand((2000, cols), dtype=torch.float32, device=dev, generator=g)
            case("edge: 2000 rows x %d f32, 100 bins, median" % cols, [x], v, [np.linspace(-4, 4, 101)], (1,), 0.5, opt.reps, out, srt)
            del x, v
    if out:
        out.close()


if __name__ == "__main__":
    main()
