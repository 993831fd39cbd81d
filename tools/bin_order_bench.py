#!/usr/bin/env python
"""bin_order against what a user could do without it, on the same arrays, in the same process: `bin_index` followed by
`torch.sort(stable=True)` along the row (the workaround, and the bar: bin_order has no reason to exist on a shape where the
general sort is faster), `bin_index` alone (step 0 of bin_order), and a plain device copy, `Tensor.copy_`, of the bytes the
design moves (the floor, not a gate).  Device-event times after warm-up, the calls alternating, the median and minimum of each,
one JSON line per shape (printed, and written to --out).

    python tools/bin_order_bench.py [--reps 20] [--only c2,c4,time,pairs] [--out profiles/bin_order_bench.jsonl]

Shapes: C2 (10^9 float64 samples, 100 bins; --c2-n lowers it where the sort workaround runs out of memory, and the line says
so), C4's shard ((456, 720, 1440) float32 over lat / lon, 50 bins), (365, 720, 1440) float32 over the leading time axis, 50 bins
(a million short rows), and 2 * 10^8 float64 pairs in 50 x 50 bins.

Bytes of a bin_order call per sample: the samples read once, 8 written and 8 + 8 read again for the keys (count, scatter), 8
written for the order: 40 for a float64 sample, 36 for a float32 one, 48 for a float64 pair.  The copy moves half in, half out."""
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
    """the bin indices as [kept..., c] with the reduced axes last, as bin_order numbers its positions"""
    if axis is None:
        return t.reshape(-1)
    kept = [i for i in range(t.ndim) if i not in axis]
    return t.permute(*kept, *sorted(axis)).reshape(*[t.shape[i] for i in kept], -1)


def case(name, args, bins, axis, reps, out, note=""):
    n = args[0].numel()
    item = args[0].element_size()
    edges = [np.asarray(b, np.float64) for b in bins]
    order = lambda: core.bin_order(*args, bins=bins, axis=axis)  # noqa: E731
    index = lambda: core.bin_index(*args, bins=bins)  # noqa: E731

    def workaround():
        return torch.sort(rows_last(core.bin_index(*args, bins=bins)[0], axis), dim=-1, stable=True)

    nbytes = (len(args) * item + 32) * n
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=args[0].device)
    dst = torch.empty_like(src)
    copy = lambda: dst.copy_(src)  # noqa: E731
    sort_ok = True
    try:
        workaround()
    except RuntimeError as err:  # (out of memory: the line reports the workaround as not measured)
        sort_ok, note = False, (note + " sort workaround: " + str(err).split("\n")[0]).strip()
        torch.cuda.empty_cache()
    for _ in range(2):
        order()
        index()
        copy()
        if sort_ok:
            workaround()
    to, ts, ti, tc = [], [], [], []
    for _ in range(reps):
        to.append(timed(order))
        if sort_ok:
            ts.append(timed(workaround))
        ti.append(timed(index))
        tc.append(timed(copy))
    order()  # (the plan's describe() line is that of its last call)
    torch.cuda.synchronize()
    desc = core._get_plan(edges, _native.CMP_F64, torch.cuda.current_device()).describe()
    med = statistics.median
    line = {"case": name, "ms": round(med(to), 4), "sort_ms": round(med(ts), 4) if sort_ok else None,
            "bin_index_ms": round(med(ti), 4), "copy_ms": round(med(tc), 4), "bytes": nbytes,
            "over_sort": round(med(to) / med(ts), 3) if sort_ok else None, "over_copy": round(med(to) / med(tc), 3),
            "tb_per_s": round(nbytes / med(to) / 1e9, 3), "min_ms": round(min(to), 4), "sort_min_ms": round(min(ts), 4) if sort_ok else None,
            "bin_index_min_ms": round(min(ti), 4), "copy_min_ms": round(min(tc), 4), "reps": reps, "describe": desc, "note": note}
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
    ap.add_argument("--only", default="c2,c4,time,pairs")
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
        note = "" if opt.c2_n == 10 ** 9 else "C2 at %d samples instead of 10^9" % opt.c2_n
        case("c2: %.3g f64, 100 bins" % opt.c2_n, [x], [np.linspace(-4, 4, 101)], None, opt.reps, out, note)
        del x
    if "c4" in only:
        x = torch.randn((456, 720, 1440), dtype=torch.float32, device=dev, generator=g)
        case("c4: (456, 720, 1440) f32 over lat/lon, 50 bins", [x], [np.linspace(-4, 4, 51)], (1, 2), opt.reps, out)
        del x
    if "time" in only:
        x = torch.randn((365, 720, 1440), dtype=torch.float32, device=dev, generator=g)
        case("time: (365, 720, 1440) f32 over the leading axis, 50 bins", [x], [np.linspace(-4, 4, 51)], (0,), opt.reps, out)
        del x
    if "pairs" in only:
        x = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
        y = torch.randn(2 * 10 ** 8, dtype=torch.float64, device=dev, generator=g)
        case("pairs: 2e8 f64 pairs, 50 x 50 bins", [x, y], [np.linspace(-4, 4, 51)] * 2, None, opt.reps, out)
        del x, y
    if out:
        out.close()


if __name__ == "__main__":
    main()
