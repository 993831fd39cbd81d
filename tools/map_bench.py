#!/usr/bin/env python
"""bin_index, histogram_lookup and histogram_anomaly against two yardsticks on the same arrays, in the same process:
`histogram` (the same reads and the same digitize, no per-sample writes) and a plain device copy, `Tensor.copy_`, sized to move
as many bytes as the call reads and writes.  Device-event times after warm-up, the calls alternating, the median and minimum of
each, one JSON line per op and shape (printed, and written to --out).

    python tools/map_bench.py [--reps 20] [--only c2,c4,pairs,tutorial] [--out profiles/map_bench.jsonl]

Shapes: C2 (10^9 float64 samples, 100 bins), C4's shard ((456, 720, 1440) float32 over lat / lon, 50 bins), 2 * 10^8 float64
pairs in 50 x 50 bins, and the tutorial's 279 x 339 bins, whose table row does not fit LDS (table home "global").

Bytes of a call: bin_index and histogram_lookup read the samples once and write 8 bytes per sample; histogram_anomaly reads
samples and values three times (histogram_mean_var's two passes, then the map) and writes 8 bytes per sample.  The copy moves
half of that sum in and half out.  The bar is the copy's time plus 10 %, the margin the project gave histogram_weighted_cov
over its byte ratio: `over_copy` above 1.10 calls for per-kernel times (rocprofv3 --kernel-trace --stats, a run of its own)."""
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
    n = args[0].numel()
    item = args[0].element_size()
    edges = [np.asarray(b, np.float64) for b in bins]
    hist = lambda: core.histogram(*args, bins=bins, axis=axis)  # noqa: E731
    table = hist()[0].to(torch.float64)
    ops = {
        "bin_index": (lambda: core.bin_index(*args, bins=bins), len(args) * item * n + 8 * n),
        "histogram_lookup": (lambda: core.histogram_lookup(*args, table=table, bins=bins, axis=axis), len(args) * item * n + 8 * n),
        "histogram_anomaly": (lambda: core.histogram_anomaly(*args, values=values, bins=bins, axis=axis),
                              3 * (len(args) + 1) * item * n + 8 * n),
        "histogram_anomaly_z": (lambda: core.histogram_anomaly(*args, values=values, bins=bins, axis=axis, standardize=True),
                                3 * (len(args) + 1) * item * n + 8 * n),
    }
    for op, (fn, nbytes) in ops.items():
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=args[0].device)
        dst = torch.empty_like(src)
        copy = lambda: dst.copy_(src)  # noqa: E731
        for _ in range(3):
            fn()
            hist()
            copy()
        to, th, tc = [], [], []
        for _ in range(reps):
            to.append(timed(fn))
            th.append(timed(hist))
            tc.append(timed(copy))
        mo_, mh, mc = statistics.median(to), statistics.median(th), statistics.median(tc)
        fn()  # (the plan's describe() line is that of its last call)
        torch.cuda.synchronize()
        desc = core._get_plan(edges, _native.CMP_F64, torch.cuda.current_device()).describe()
        line = json.dumps({"case": name, "op": op, "ms": round(mo_, 4), "histogram_ms": round(mh, 4), "copy_ms": round(mc, 4),
                           "bytes": nbytes, "over_copy": round(mo_ / mc, 3), "over_histogram": round(mo_ / mh, 3),
                           "tb_per_s": round(nbytes / mo_ / 1e9, 3), "min_ms": round(min(to), 4), "histogram_min_ms": round(min(th), 4),
                           "copy_min_ms": round(min(tc), 4), "reps": reps, "describe": desc})
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        del src, dst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="c2,c4,pairs,tutorial")
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
        case("c2: 1e9 f64, 100 bins", [x], v, [np.linspace(-4, 4, 101)], None, opt.reps, out)
        del x, v
    if "c4" in only:
        x = torch.randn((456, 720, 1440), dtype=torch.float32, device=dev, generator=g)
        v = torch.rand((456, 720, 1440), dtype=torch.float32, device=dev, generator=g)
        case("c4: (456, 720, 1440) f32 over lat/lon, 50 bins", [x], v, [np.linspace(-4, 4, 51)], (1, 2), opt.reps, out)
        del x, v
    for key, name, nb in (("pairs", "pairs: 2e8 f64 pairs, 50 x 50 bins", (50, 50)),
                          ("tutorial", "tutorial: 2e8 f64 pairs, 279 x 339 bins", (279, 339))):
        if key in only:
            x = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
            y = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
            v = torch.rand(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
            case(name, [x, y], v, [np.linspace(-4, 4, k + 1) for k in nb], None, opt.reps, out)
            del x, y, v
    if out:
        out.close()


if __name__ == "__main__":
    main()
