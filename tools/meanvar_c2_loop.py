"""histogram_mean_var with and without weights at C2's size (10^9 float64 samples, 100 bins), from the package under the
checkout given as the first argument (so that a base revision's build and the working tree's can alternate): device-event
times after warm-up, the median and minimum of 20 calls each, one JSON line per form, printed and written to the second argument.

    python tools/meanvar_c2_loop.py <checkout root> <out.jsonl>"""
import json
import statistics
import sys

root, out = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from xhistogram_amd import core  # noqa: E402

assert core.__file__.startswith(root), core.__file__
g = torch.Generator(device="cuda")
g.manual_seed(0)
x = torch.randn(10 ** 9, dtype=torch.float64, device="cuda", generator=g)
v = torch.rand(10 ** 9, dtype=torch.float64, device="cuda", generator=g)
w = torch.rand(10 ** 9, dtype=torch.float64, device="cuda", generator=g)
e = [np.linspace(-4, 4, 101)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


calls = {"mean_var c2": lambda: core.histogram_mean_var(x, values=v, bins=e),
         "mean_var weighted c2": lambda: core.histogram_mean_var(x, values=v, weights=w, bins=e)}
with open(out, "w") as f:
    for name, fn in calls.items():
        for _ in range(3):
            fn()
        t = [timed(fn) for _ in range(20)]
        line = json.dumps({"case": name, "ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "reps": 20})
        print(line, flush=True)
        f.write(line + "\n")
