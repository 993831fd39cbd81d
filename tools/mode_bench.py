#!/usr/bin/env python
"""histogram_mode against bin_rank(method="min") and against bin_sort from the same build, on the same arrays, in the same
process.  The bar: histogram_mode <= bin_rank(method="min") + 10 % on every shape and every distribution of the values.  By
bytes it should cost less: the same sort and head pass, then one read of the keys where bin_rank reads keys and order and
scatters 8 bytes per sample.

Device-event times after warm-up, the calls alternating, the median and minimum of each, one JSON line per (shape,
distribution) (printed, and written to --out).  Before the timing the result is held once to two identities with bin_rank,
taken per bin on the device with scatter_reduce: count is the largest "max" rank, mode_count the largest max - min + 1.  The
line says whether they agree.

    python tools/mode_bench.py [--reps 20] [--only c2,c4,pairs50,pairs279] [--dist rounded,categories,continuous]
                               [--out profiles/mode_bench.jsonl]

Shapes: bin_rank_bench's four.  C2 (10^9 float64 samples and values, 100 bins; --c2-n lowers it where memory runs out, and the
line says so), C4's shard ((456, 720, 1440) float32 samples and values over lat / lon, 50 bins), and 2 * 10^8 float64 pairs with
float64 values in 50 x 50 and in 279 x 339 bins.  Distributions of the values: N(0, 1) rounded to two decimals ("rounded": a few
hundred distinct values), ten integer categories ("categories": long runs, the intended use), and N(0, 1) as it comes
("continuous": nearly every sample is its own run, the most candidates for the atomic maximum)."""
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


def rows_last(t, axis):
    """[kept..., c] with the reduced axes last, as bin_sort numbers its positions"""
    if axis is None:
        return t.reshape(-1)
    kept = [i for i in range(t.ndim) if i not in axis]
    return t.permute(*kept, *sorted(axis)).reshape(*[t.shape[i] for i in kept], -1)


def agrees(args, values, bins, axis, n_bins, got):
    """mode_count against the per-bin maximum of max - min + 1 over bin_rank's ranks, count against the per-bin maximum of the
    max rank: two scatter_reduce calls on the device"""
    count, _, _, mode_count = got
    rmax = rows_last(core.bin_rank(*args, values=values, bins=bins, axis=axis, method="max")[0], axis)
    rmin = rows_last(core.bin_rank(*args, values=values, bins=bins, axis=axis, method="min")[0], axis)
    idx = rows_last(core.bin_index(*args, bins=bins)[0], axis)
    ok = ~torch.isnan(rmax)
    key = torch.where(ok, idx, n_bins)
    del idx
    lead = key.shape[:-1]

    def per_bin(x):
        out = torch.zeros(lead + (n_bins + 1,), dtype=torch.float64, device=x.device)
        return out.scatter_reduce(-1, key, torch.where(ok, x, 0.0), "amax")[..., :n_bins]

    want_count, want_mode_count = per_bin(rmax), per_bin(rmax - rmin + 1)
    return bool(torch.equal(count.reshape(lead + (n_bins,)).to(torch.float64), want_count)
                and torch.equal(mode_count.reshape(lead + (n_bins,)).to(torch.float64), want_mode_count))


def case(name, dist, args, values, bins, axis, reps, out, note=""):
    edges = [np.asarray(b, np.float64) for b in bins]
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    mode = lambda: core.histogram_mode(*args, values=values, bins=bins, axis=axis)[:4]  # noqa: E731
    rank = lambda: core.bin_rank(*args, values=values, bins=bins, axis=axis, method="min")[0]  # noqa: E731
    sort = lambda: core.bin_sort(*args, values=values, bins=bins, axis=axis)  # noqa: E731

    got = mode()
    torch.cuda.synchronize()
    desc = core._get_plan(edges, _native.CMP_F64, torch.cuda.current_device()).describe()
    agree = None
    try:
        agree = agrees(args, values, bins, axis, n_bins, got)
    except RuntimeError as err:  # (out of memory: the line reports the identities as not checked)
        note = (note + " identities: " + str(err).split("\n")[0]).strip()
    del got
    torch.cuda.empty_cache()
    for _ in range(2):
        mode()
        rank()
        sort()
    tm, tr, ts = [], [], []
    for _ in range(reps):
        tm.append(timed(mode))
        tr.append(timed(rank))
        ts.append(timed(sort))
    med = statistics.median
    line = {"case": name, "values": dist, "ms": round(med(tm), 4), "bin_rank_min_ms": round(med(tr), 4), "bin_sort_ms": round(med(ts), 4),
            "over_bin_rank": round(med(tm) / med(tr), 3), "over_bin_sort": round(med(tm) / med(ts), 3), "within_bar": med(tm) <= 1.1 * med(tr),
            "min_ms": round(min(tm), 4), "bin_rank_min_min_ms": round(min(tr), 4), "bin_sort_min_ms": round(min(ts), 4),
            "agrees_with_bin_rank": agree, "reps": reps, "describe": desc, "note": note}
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        out.write(text + "\n")
        out.flush()
    torch.cuda.empty_cache()


def values_of(dist, shape, dtype, g):
    if dist == "rounded":
        return torch.round(torch.randn(shape, dtype=dtype, device="cuda", generator=g), decimals=2)
    if dist == "categories":
        return torch.randint(0, 10, shape if isinstance(shape, tuple) else (shape,), device="cuda", generator=g).to(dtype)
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
            case("c2: %.3g f64, f64 values, 100 bins" % opt.c2_n, dist, [x], v, [np.linspace(-4, 4, 101)], None, opt.reps, out, note)
            del v
        del x
    if "c4" in only:
        x = torch.randn((456, 720, 1440), dtype=torch.float32, device=dev, generator=g)
        for dist in dists:
            v = values_of(dist, (456, 720, 1440), torch.float32, g)
            case("c4: (456, 720, 1440) f32 over lat/lon, f32 values, 50 bins", dist, [x], v, [np.linspace(-4, 4, 51)], (1, 2), opt.reps, out)
            del v
        del x
    for tag, nbs in (("pairs50", (50, 50)), ("pairs279", (279, 339))):
        if tag in only:
            x = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
            y = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
            for dist in dists:
                v = values_of(dist, 2 * 10 ** 8, torch.float64, g)
                case("%s: 2e8 f64 pairs, f64 values, %d x %d bins" % ((tag,) + nbs), dist, [x, y], v,
                     [np.linspace(-4, 4, nb + 1) for nb in nbs], None, opt.reps, out)
                del v
            del x, y
    if out:
        out.close()


if __name__ == "__main__":
    main()
