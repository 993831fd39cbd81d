#!/usr/bin/env python
"""bin_sort against what a user could do without it, on the same arrays, in the same process (the bar, no margin):

    idx = bin_index(*args)                                  # the library's own
    i1 = torch.sort(values as float64, stable=True)         # by value, along the row
    i2 = torch.sort(binkey.gather(i1), stable=True)         # by bin, stable: the value order survives
    order = i1.gather(i2)

and a plain device copy, `Tensor.copy_`, of the bytes the design moves (the floor, not a gate).  Device-event times after
warm-up, the calls alternating, the median and minimum of each, one JSON line per shape (printed, and written to --out).

    python tools/bin_sort_bench.py [--reps 20] [--only c2,c4,pairs50,pairs279] [--out profiles/bin_sort_bench.jsonl]

Shapes: C2 (10^9 float64 samples and values, 100 bins; --c2-n lowers it where either side runs out of memory, and the line says
so), C4's shard ((456, 720, 1440) float32 samples and values over lat / lon, 50 bins), and 2 * 10^8 float64 pairs with float64
values in 50 x 50 and in 279 x 339 bins.

Bytes of a bin_sort call per sample, with P = value passes + bin passes: the samples read once and 8 of bin key written; the
value read and 12 of (key, position) written; per pass 8 read by the count and 12 read and 12 written by the scatter (the last
pass of the value phase writes 4, the last of the call 16); the gather reads 4 + 8 and writes 8; the offsets read 8.  The copy
moves half in, half out; it is timed on at most 16 GiB each way and scaled to the bytes of the call."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xhistogram_amd import _native, core  # noqa: E402


COPY_MAX = 16 << 30  # bytes of the copy's source: the sorts' scratch leaves no room for all the bytes they move


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
    n = args[0].numel()
    edges = [np.asarray(b, np.float64) for b in bins]
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    sort = lambda: core.bin_sort(*args, values=values, bins=bins, axis=axis)  # noqa: E731

    def workaround():
        idx = rows_last(core.bin_index(*args, bins=bins)[0], axis)
        i1 = torch.sort(rows_last(values, axis).to(torch.float64), dim=-1, stable=True).indices
        key = torch.where(idx < 0, n_bins, idx).gather(-1, i1)
        del idx
        i2 = torch.sort(key, dim=-1, stable=True).indices
        return i1.gather(-1, i2)

    sort()
    torch.cuda.synchronize()
    desc = core._get_plan(edges, _native.CMP_F64, torch.cuda.current_device()).describe()
    fields = dict(kv.split("=") for kv in desc.split()[1:])
    passes = int(fields["value_passes"]) + int(fields["bin_passes"])
    per_sample = sum(a.element_size() for a in args) + 8 + values.element_size() + 12 + 32 * passes + 20 + 8
    nbytes = per_sample * n
    half = min(nbytes // 2, COPY_MAX)  # (a copy of more is this copy's time, scaled: it runs at the same rate)
    scale = (nbytes // 2) / half
    src = torch.empty(half, dtype=torch.uint8, device=args[0].device)
    dst = torch.empty_like(src)
    copy = lambda: dst.copy_(src)  # noqa: E731
    sort_ok = True
    try:
        workaround()
    except RuntimeError as err:  # (out of memory: the line reports the workaround as not measured)
        sort_ok, note = False, (note + " workaround: " + str(err).split("\n")[0]).strip()
        torch.cuda.empty_cache()
    for _ in range(2):
        sort()
        copy()
        if sort_ok:
            workaround()
    to, ts, tc = [], [], []
    for _ in range(reps):
        to.append(timed(sort))
        if sort_ok:
            ts.append(timed(workaround))
        tc.append(timed(copy) * scale)
    med = statistics.median
    line = {"case": name, "ms": round(med(to), 4), "workaround_ms": round(med(ts), 4) if sort_ok else None, "copy_ms": round(med(tc), 4),
            "bytes": nbytes, "over_workaround": round(med(to) / med(ts), 3) if sort_ok else None, "over_copy": round(med(to) / med(tc), 3),
            "tb_per_s": round(nbytes / med(to) / 1e9, 3), "min_ms": round(min(to), 4), "workaround_min_ms": round(min(ts), 4) if sort_ok else None,
            "copy_min_ms": round(min(tc), 4), "reps": reps, "describe": desc, "note": note}
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        out.write(text + "\n")
        out.flush()
    del src, dst
    torch.cuda.empty_cache()


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
        v = torch.randn(opt.c2_n, dtype=torch.float64, device=dev, generator=g)
        note = "" if opt.c2_n == 10 ** 9 else "C2 at %d samples instead of 10^9" % opt.c2_n
        case("c2: %.3g f64, f64 values, 100 bins" % opt.c2_n, [x], v, [np.linspace(-4, 4, 101)], None, opt.reps, out, note)
        del x, v
    if "c4" in only:
        x = torch.randn((456, 720, 1440), dtype=torch.float32, device=dev, generator=g)
        v = torch.randn((456, 720, 1440), dtype=torch.float32, device=dev, generator=g)
        case("c4: (456, 720, 1440) f32 over lat/lon, f32 values, 50 bins", [x], v, [np.linspace(-4, 4, 51)], (1, 2), opt.reps, out)
        del x, v
    for tag, nbs in (("pairs50", (50, 50)), ("pairs279", (279, 339))):
        if tag in only:
            x = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
            y = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
            v = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
            case("%s: 2e8 f64 pairs, f64 values, %d x %d bins" % ((tag,) + nbs), [x, y], v, [np.linspace(-4, 4, nb + 1) for nb in nbs], None,
                 opt.reps, out)
            del x, y, v
    if out:
        out.close()


if __name__ == "__main__":
    main()
