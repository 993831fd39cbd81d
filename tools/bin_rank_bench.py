#!/usr/bin/env python
"""bin_rank(method="average") against what a user could do without it, on the same arrays, in the same process (the bar, no
margin): bin_sort, then torch ops in the sorted domain,

    order, offsets, _ = bin_sort(*args, values=values)      # the library's own
    vs = values.to(float64).gather(order)                   # the values and the bin keys of the sorted positions
    ks = bin_index(*args).gather(order)
    head = (ks[1:] != ks[:-1]) | ~(vs[1:] == vs[:-1])       # neighbour compares
    s = cummax(where(head, i, 0)); e = the reversed cummin of where(head, i, c), moved one on
    rank = (s + e - 2 * offsets[ks] + 1).to(float64) / 2    # NaN where ks == B or vs is NaN
    out.scatter_(order, rank)

and against bin_sort alone.  Device-event times after warm-up, the calls alternating, the median and minimum of each, one JSON
line per shape (printed, and written to --out).  Before the timing the two results are compared once, bit for bit with NaN
held to its place; the line says whether they agree.

    python tools/bin_rank_bench.py [--reps 20] [--only c2,c4,pairs50,pairs279] [--out profiles/bin_rank_bench.jsonl]

Shapes: C2 (10^9 float64 samples and values, 100 bins; --c2-n lowers it where either side runs out of memory, and the line says
so), C4's shard ((456, 720, 1440) float32 samples and values over lat / lon, 50 bins), and 2 * 10^8 float64 pairs with float64
values in 50 x 50 and in 279 x 339 bins.  The values are N(0, 1) rounded to two decimals: a few hundred distinct values, so
nearly every sample is in a tie run."""
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


def case(name, args, values, bins, axis, reps, out, note=""):
    edges = [np.asarray(b, np.float64) for b in bins]
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    rank = lambda: core.bin_rank(*args, values=values, bins=bins, axis=axis)[0]  # noqa: E731
    sort = lambda: core.bin_sort(*args, values=values, bins=bins, axis=axis)  # noqa: E731

    def workaround():
        """the ranks with the reduced axes last"""
        order, offsets, _ = sort()
        vs = rows_last(values, axis).to(torch.float64).gather(-1, order)
        idx = rows_last(core.bin_index(*args, bins=bins)[0], axis)
        ks = torch.where(idx < 0, n_bins, idx).gather(-1, order)
        del idx
        c = order.shape[-1]
        head = torch.ones_like(ks, dtype=torch.bool)
        head[..., 1:] = (ks[..., 1:] != ks[..., :-1]) | ~(vs[..., 1:] == vs[..., :-1])
        i = torch.arange(c, device=ks.device).expand(ks.shape)
        s = torch.cummax(torch.where(head, i, 0), -1).values
        nxt = torch.cummin(torch.where(head, i, c).flip(-1), -1).values.flip(-1)
        del head
        e = torch.cat([nxt[..., 1:], torch.full_like(nxt[..., :1], c)], -1)
        del nxt
        r = (s + e - 2 * offsets.gather(-1, ks) + 1).to(torch.float64) / 2.0  # (float64 as the ranks are: float32 ends at 2^24)
        del s, e
        r = torch.where((ks < n_bins) & ~torch.isnan(vs), r, float("nan"))
        return torch.empty_like(r).scatter_(-1, order, r)

    got = rank()
    torch.cuda.synchronize()
    desc = core._get_plan(edges, _native.CMP_F64, torch.cuda.current_device()).describe()
    bar_ok, agree = True, None
    try:
        want = workaround()
        got = rows_last(got, axis)
        agree = bool(torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got), torch.nan_to_num(want)))
        del want
    except RuntimeError as err:  # (out of memory: the line reports the workaround as not measured)
        bar_ok, note = False, (note + " workaround: " + str(err).split("\n")[0]).strip()
    del got
    torch.cuda.empty_cache()
    for _ in range(2):
        rank()
        sort()
        if bar_ok:
            workaround()
    tr, ts, tw = [], [], []
    for _ in range(reps):
        tr.append(timed(rank))
        ts.append(timed(sort))
        if bar_ok:
            tw.append(timed(workaround))
    med = statistics.median
    line = {"case": name, "ms": round(med(tr), 4), "workaround_ms": round(med(tw), 4) if bar_ok else None, "bin_sort_ms": round(med(ts), 4),
            "over_workaround": round(med(tr) / med(tw), 3) if bar_ok else None, "over_bin_sort": round(med(tr) / med(ts), 3),
            "min_ms": round(min(tr), 4), "workaround_min_ms": round(min(tw), 4) if bar_ok else None, "bin_sort_min_ms": round(min(ts), 4),
            "agrees_with_workaround": agree, "reps": reps, "describe": desc, "note": note}
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        out.write(text + "\n")
        out.flush()
    torch.cuda.empty_cache()


def tied(shape, dtype, g):
    return torch.round(torch.randn(shape, dtype=dtype, device="cuda", generator=g), decimals=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="c2,c4,pairs50,pairs279")
    ap.add_argument("--c2-n", type=int, default=10 ** 9)
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    only = set(opt.only.split(","))
    out = open(opt.out, "a") if opt.out else None
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    dev = "cuda"
    if "c2" in only:
        x = torch.randn(opt.c2_n, dtype=torch.float64, device=dev, generator=g)
        v = tied(opt.c2_n, torch.float64, g)
        note = "" if opt.c2_n == 10 ** 9 else "C2 at %d samples instead of 10^9" % opt.c2_n
        case("c2: %.3g f64, f64 values, 100 bins" % opt.c2_n, [x], v, [np.linspace(-4, 4, 101)], None, opt.reps, out, note)
        del x, v
    if "c4" in only:
        x = torch.randn((456, 720, 1440), dtype=torch.float32, device=dev, generator=g)
        v = tied((456, 720, 1440), torch.float32, g)
        case("c4: (456, 720, 1440) f32 over lat/lon, f32 values, 50 bins", [x], v, [np.linspace(-4, 4, 51)], (1, 2), opt.reps, out)
        del x, v
    for tag, nbs in (("pairs50", (50, 50)), ("pairs279", (279, 339))):
        if tag in only:
            x = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
            y = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
            v = tied(2 * 10 ** 8, torch.float64, g)
            case("%s: 2e8 f64 pairs, f64 values, %d x %d bins" % ((tag,) + nbs), [x, y], v, [np.linspace(-4, 4, nb + 1) for nb in nbs], None,
                 opt.reps, out)
            del x, y, v
    if out:
        out.close()


if __name__ == "__main__":
    main()
