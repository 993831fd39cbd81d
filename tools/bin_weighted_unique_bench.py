#!/usr/bin/env python
"""bin_weighted_unique against bin_unique and histogram_weighted_mode against histogram_mode, on the same arrays, in the same
process; the unweighted calls come unchanged from the parent commit.  This tool reports what the weights cost, as medians of
device-event times; the bars themselves are read from a kernel trace of C4's lines (profiles/bin_weighted_unique_kernel_stats.txt):

    bin_weighted_unique      wruns_* summed <= 1.1 * (rank_heads + unique_runs)
    histogram_weighted_mode  (wruns_* + wmode_*) - (mode_runs + mode_finish) <= 1.1 * (rank_heads + unique_runs + mode_runs)

Device-event times after warm-up, the calls alternating, the median and minimum of each, one JSON line per (shape, distribution)
(printed, and written to --out).  Before the timing the results are held to each other on the device, and the line says whether
they agree: uniques, counts and offsets of the weighted call are bin_unique's by bits; with the unit weights used for this check
weight_sums == counts, count and nunique are histogram_mode's, mode is its mode by bits and mode_weight == mode_count; and on the
timed weights mode_weight is the largest weight_sums entry of each bin where no row is cut.

    python tools/bin_weighted_unique_bench.py [--reps 20] [--only c2,c4,pairs50,pairs279] [--dist rounded,categories,continuous]
                                              [--out profiles/bin_weighted_unique_bench.jsonl]

Shapes and distributions are tools/bin_unique_bench.py's; the weights are uniform in [0.5, 1) in the samples' dtype.  The width is
ten entries per bin, which holds every entry of the categorical case."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bin_unique_bench import CATEGORIES, timed, values_of  # noqa: E402
from xhistogram_amd import _native, core  # noqa: E402


def same_bits(a, b):
    return bool(torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)))


def checks(args, values, weights, bins, axis, size, n_bins):
    """the results held to each other; every comparison on the device"""
    kw = dict(values=values, bins=bins, axis=axis)
    one = torch.ones((), dtype=weights.dtype, device=weights.device)
    u0, c0, o0 = core.bin_unique(*args, size=size, **kw)[:3]
    u1, c1, s1, o1 = core.bin_weighted_unique(*args, weights=one, size=size, **kw)[:4]
    m0 = core.histogram_mode(*args, **kw)[:4]
    m1 = core.histogram_weighted_mode(*args, weights=one, **kw)[:4]
    out = {"unique_outputs_agree": same_bits(u0, u1) and bool(torch.equal(c0, c1)) and bool(torch.equal(o0, o1)),
           "unit_weight_sums_are_counts": bool(torch.equal(s1, c1.to(torch.float64))),
           "unit_weight_mode_agrees": bool(torch.equal(m0[0], m1[0])) and bool(torch.equal(m0[1], m1[1])) and same_bits(m0[2], m1[2])
           and bool(torch.equal(m0[3].to(torch.float64), m1[3]))}
    del u0, c0, o0, u1, c1, s1, o1, m0, m1
    _, _, sums, offsets = core.bin_weighted_unique(*args, weights=weights, size=size, **kw)[:4]
    mode_weight = core.histogram_weighted_mode(*args, weights=weights, **kw)[3]
    lead = offsets.shape[:-1]
    if int(offsets[..., -1].max()) > sums.shape[-1]:
        out["mode_weight_is_the_largest_sum"] = None  # (a row is cut)
    else:
        pos = torch.arange(sums.shape[-1], device=sums.device).expand(lead + (-1,)).contiguous()
        seg = torch.searchsorted(offsets[..., 1:].contiguous(), pos, right=True)  # the bin of every entry, n_bins: padding
        valid = seg < n_bins
        best = torch.full(lead + (n_bins + 1,), -float("inf"), dtype=torch.float64, device=sums.device)
        best.scatter_reduce_(-1, torch.where(valid, seg, torch.full_like(seg, n_bins)), sums, "amax")
        best = best[..., :n_bins]
        has = offsets[..., 1:] > offsets[..., :-1]
        out["mode_weight_is_the_largest_sum"] = bool(torch.equal(torch.where(has, best, torch.zeros_like(best)), mode_weight.reshape(lead + (n_bins,))))
    return out


def case(name, dist, args, values, weights, bins, axis, reps, out, note=""):
    edges = [np.asarray(b, np.float64) for b in bins]
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    size = CATEGORIES * n_bins
    kw = dict(values=values, bins=bins, axis=axis)
    agree = checks(args, values, weights, bins, axis, size, n_bins)
    torch.cuda.empty_cache()
    calls = [lambda: core.bin_weighted_unique(*args, weights=weights, size=size, **kw)[:4],
             lambda: core.bin_unique(*args, size=size, **kw)[:3],
             lambda: core.histogram_weighted_mode(*args, weights=weights, **kw)[:4],
             lambda: core.histogram_mode(*args, **kw)[:4]]
    calls[0]()
    torch.cuda.synchronize()
    desc = core._get_plan(edges, _native.CMP_F64, torch.cuda.current_device()).describe()
    for _ in range(2):
        for fn in calls:
            fn()
    t = [[] for _ in calls]
    for _ in range(reps):
        for times, fn in zip(t, calls):
            times.append(timed(fn))
    med = [statistics.median(x) for x in t]
    line = {"case": name, "values": dist, "size": size,
            "weighted_unique_ms": round(med[0], 4), "bin_unique_ms": round(med[1], 4), "unique_added_ms": round(med[0] - med[1], 4),
            "unique_ratio": round(med[0] / med[1], 3),
            "weighted_mode_ms": round(med[2], 4), "histogram_mode_ms": round(med[3], 4), "mode_added_ms": round(med[2] - med[3], 4),
            "mode_ratio": round(med[2] / med[3], 3),
            "weighted_unique_min_ms": round(min(t[0]), 4), "bin_unique_min_ms": round(min(t[1]), 4),
            "weighted_mode_min_ms": round(min(t[2]), 4), "histogram_mode_min_ms": round(min(t[3]), 4),
            **agree, "reps": reps, "describe": desc, "note": note}
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        out.write(text + "\n")
        out.flush()


def weights_of(shape, dtype, g):
    return torch.rand(shape, dtype=dtype, device="cuda", generator=g) * 0.5 + 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="c2,c4,pairs50,pairs279")
    ap.add_argument("--dist", default="rounded,categories,continuous")
    ap.add_argument("--c2-n", type=int, default=10 ** 9)
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    only, dists = set(opt.only.split(",")), opt.dist.split(",")
    out = open(opt.out, "a") if opt.out else None
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    dev = "cuda"
    if "c2" in only:
        x = torch.randn(opt.c2_n, dtype=torch.float64, device=dev, generator=g)
        w = weights_of(opt.c2_n, torch.float64, g)
        note = "" if opt.c2_n == 10 ** 9 else "C2 at %d samples instead of 10^9" % opt.c2_n
        for dist in dists:
            v = values_of(dist, opt.c2_n, torch.float64, g)
            case("c2: %.3g f64, f64 values and weights, 100 bins" % opt.c2_n, dist, [x], v, w, [np.linspace(-4, 4, 101)], None, opt.reps, out, note)
            del v
        del x, w
    if "c4" in only:
        x = torch.randn((456, 720, 1440), dtype=torch.float32, device=dev, generator=g)
        w = weights_of((456, 720, 1440), torch.float32, g)
        for dist in dists:
            v = values_of(dist, (456, 720, 1440), torch.float32, g)
            case("c4: (456, 720, 1440) f32 over lat/lon, f32 values and weights, 50 bins", dist, [x], v, w, [np.linspace(-4, 4, 51)], (1, 2),
                 opt.reps, out)
            del v
        del x, w
    for tag, nbs in (("pairs50", (50, 50)), ("pairs279", (279, 339))):
        if tag in only:
            x = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
            y = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
            w = weights_of(2 * 10 ** 8, torch.float64, g)
            for dist in dists:
                v = values_of(dist, 2 * 10 ** 8, torch.float64, g)
                case("%s: 2e8 f64 pairs, f64 values and weights, %d x %d bins" % ((tag,) + nbs), dist, [x, y], v, w,
                     [np.linspace(-4, 4, nb + 1) for nb in nbs], None, opt.reps, out)
                del v
            del x, y, w
    if out:
        out.close()


if __name__ == "__main__":
    main()
