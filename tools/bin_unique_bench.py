#!/usr/bin/env python
"""bin_unique against calls that come unchanged from the parent commit, on the same arrays, in the same process.  The bars:

    without inverse   bin_unique <= 1.1 * (histogram_mode + a Tensor.fill_ of as many bytes as the uniques and counts blocks hold)
    with inverse      bin_unique <= 1.1 * (bin_rank(method="dense") + the same fill)

By bytes the call is the same sort and head pass, then one read of the keys as in mode_runs, then stores of at most the output
bytes; the 10 % is the margin histogram_mode and histogram_sum were given.

Device-event times after warm-up, the calls alternating, the median and minimum of each, one JSON line per (shape,
distribution, size) (printed, and written to --out).  Before the timing the result is held once to histogram_mode on the device:
np.diff(offsets) is its nunique, and the segment sums of counts are its count (where no row is cut: U <= W everywhere; the line
says whether that was so).  The line says whether they agree.

    python tools/bin_unique_bench.py [--reps 20] [--only c2,c4,pairs50,pairs279] [--dist rounded,categories,continuous]
                                     [--out profiles/bin_unique_bench.jsonl]

Shapes: mode_bench's four.  C2 (10^9 float64 samples and values, 100 bins; --c2-n lowers it where memory runs out, and the line
says so), C4's shard ((456, 720, 1440) float32 samples and values over lat / lon, 50 bins), and 2 * 10^8 float64 pairs with
float64 values in 50 x 50 and in 279 x 339 bins.  Distributions of the values: N(0, 1) rounded to two decimals ("rounded"), ten
integer categories ("categories": the intended use) and N(0, 1) as it comes ("continuous": nearly every sample its own entry).
Sizes: None (the width is the samples per row) and ten entries per bin, which holds every entry of the categorical case."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xhistogram_amd import _native, core  # noqa: E402

CATEGORIES = 10


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def agrees(got, mode_out, n_bins):
    """(np.diff(offsets) == nunique, the segment sums of counts == count or None where a row is cut), on the device"""
    _, counts, offsets = got[:3]
    count, nunique = mode_out[0], mode_out[1]
    lead = offsets.shape[:-1]
    diff_ok = bool(torch.equal(offsets[..., 1:] - offsets[..., :-1], nunique.reshape(lead + (n_bins,))))
    if int(offsets[..., -1].max()) > counts.shape[-1]:
        return diff_ok, None
    run = torch.cat([torch.zeros(lead + (1,), dtype=torch.int64, device=counts.device), torch.cumsum(counts, -1)], -1)
    seg = torch.gather(run, -1, offsets[..., 1:]) - torch.gather(run, -1, offsets[..., :-1])
    return diff_ok, bool(torch.equal(seg, count.reshape(lead + (n_bins,))))


def case(name, dist, args, values, bins, axis, cols, rows, reps, out, note=""):
    edges = [np.asarray(b, np.float64) for b in bins]
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    mode = lambda: core.histogram_mode(*args, values=values, bins=bins, axis=axis)[:4]  # noqa: E731
    rank = lambda: core.bin_rank(*args, values=values, bins=bins, axis=axis, method="dense")[0]  # noqa: E731
    mode_out = mode()
    for size in (None, CATEGORIES * n_bins):
        width = cols if size is None else size
        unique = lambda: core.bin_unique(*args, values=values, bins=bins, axis=axis, size=size)[:3]  # noqa: E731
        unique_inv = lambda: core.bin_unique(*args, values=values, bins=bins, axis=axis, size=size, return_inverse=True)[:4]  # noqa: E731
        block = torch.empty(2 * rows * width, dtype=torch.int64, device="cuda")  # as many bytes as uniques and counts hold
        fill = lambda: block.fill_(1)  # noqa: E731
        got = unique_inv()
        torch.cuda.synchronize()
        desc = core._get_plan(edges, _native.CMP_F64, torch.cuda.current_device()).describe()
        cut = bool(int(got[2][..., -1].max()) > width)
        diff_ok, sums_ok = agrees(got, mode_out, n_bins)
        del got
        torch.cuda.empty_cache()
        calls = [unique, mode, fill, unique_inv, rank]
        for _ in range(2):
            for fn in calls:
                fn()
        t = [[] for _ in calls]
        for _ in range(reps):
            for times, fn in zip(t, calls):
                times.append(timed(fn))
        med = [statistics.median(x) for x in t]
        bar, bar_inv = 1.1 * (med[1] + med[2]), 1.1 * (med[4] + med[2])
        line = {"case": name, "values": dist, "size": size, "width": width, "cut": cut,
                "ms": round(med[0], 4), "histogram_mode_ms": round(med[1], 4), "fill_ms": round(med[2], 4), "bar_ms": round(bar, 4),
                "over_bar": round(med[0] / bar, 3), "within_bar": med[0] <= bar,
                "inverse_ms": round(med[3], 4), "bin_rank_dense_ms": round(med[4], 4), "inverse_bar_ms": round(bar_inv, 4),
                "inverse_over_bar": round(med[3] / bar_inv, 3), "inverse_within_bar": med[3] <= bar_inv,
                "min_ms": round(min(t[0]), 4), "histogram_mode_min_ms": round(min(t[1]), 4), "fill_min_ms": round(min(t[2]), 4),
                "inverse_min_ms": round(min(t[3]), 4), "bin_rank_dense_min_ms": round(min(t[4]), 4),
                "offsets_agree_with_nunique": diff_ok, "segment_sums_agree_with_count": sums_ok, "reps": reps, "describe": desc, "note": note}
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            out.write(text + "\n")
            out.flush()
        del block
        torch.cuda.empty_cache()


def values_of(dist, shape, dtype, g):
    if dist == "rounded":
        return torch.round(torch.randn(shape, dtype=dtype, device="cuda", generator=g), decimals=2)
    if dist == "categories":
        return torch.randint(0, CATEGORIES, shape if isinstance(shape, tuple) else (shape,), device="cuda", generator=g).to(dtype)
    if dist == "continuous":
        return torch.randn(shape, dtype=dtype, device="cuda", generator=g)
    raise ValueError(dist)


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
        note = "" if opt.c2_n == 10 ** 9 else "C2 at %d samples instead of 10^9" % opt.c2_n
        for dist in dists:
            v = values_of(dist, opt.c2_n, torch.float64, g)
            case("c2: %.3g f64, f64 values, 100 bins" % opt.c2_n, dist, [x], v, [np.linspace(-4, 4, 101)], None, opt.c2_n, 1, opt.reps, out, note)
            del v
        del x
    if "c4" in only:
        x = torch.randn((456, 720, 1440), dtype=torch.float32, device=dev, generator=g)
        for dist in dists:
            v = values_of(dist, (456, 720, 1440), torch.float32, g)
            case("c4: (456, 720, 1440) f32 over lat/lon, f32 values, 50 bins", dist, [x], v, [np.linspace(-4, 4, 51)], (1, 2), 720 * 1440, 456,
                 opt.reps, out)
            del v
        del x
    for tag, nbs in (("pairs50", (50, 50)), ("pairs279", (279, 339))):
        if tag in only:
            x = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
            y = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
            for dist in dists:
                v = values_of(dist, 2 * 10 ** 8, torch.float64, g)
                case("%s: 2e8 f64 pairs, f64 values, %d x %d bins" % ((tag,) + nbs), dist, [x, y], v,
                     [np.linspace(-4, 4, nb + 1) for nb in nbs], None, 2 * 10 ** 8, 1, opt.reps, out)
                del v
            del x, y
    if out:
        out.close()


if __name__ == "__main__":
    main()
