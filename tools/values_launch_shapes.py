"""One radix and one short-row call of histogram_quantile and of histogram_weighted_quantile and one call of each
histogram_mean_var form, from the package under the checkout given as the argument; prints the plan's describe() line after
each call.  Run once under a base revision's build and once under the working tree's, each under
`rocprofv3 --kernel-trace --stats -- python tools/values_launch_shapes.py <checkout>`, it shows whether a change of the host
drivers moved a launch: the kernel names, their call counts and the six DESCRIBE lines must be the same.

    python tools/values_launch_shapes.py <checkout root>"""
import sys

root = sys.argv[1]
sys.path.insert(0, root)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from xhistogram_amd import _native, core  # noqa: E402

assert core.__file__.startswith(root), core.__file__
g = torch.Generator(device="cuda")
g.manual_seed(0)
edges = [np.linspace(-4, 4, 101)]


def desc(tag):
    torch.cuda.synchronize()
    print("DESCRIBE", tag, "|", core._get_plan(edges, _native.CMP_F64, torch.cuda.current_device()).describe(), flush=True)


xl = torch.randn((6, 300000), dtype=torch.float64, device="cuda", generator=g)
vl = torch.rand((6, 300000), dtype=torch.float64, device="cuda", generator=g)
wl = torch.rand((6, 300000), dtype=torch.float64, device="cuda", generator=g)
xs = torch.randn((365, 5000), dtype=torch.float32, device="cuda", generator=g)
vs = torch.rand((365, 5000), dtype=torch.float32, device="cuda", generator=g)
ws = torch.rand((365, 5000), dtype=torch.float32, device="cuda", generator=g)
q = [0.1, 0.25, 0.5, 0.75, 0.9, 0.95, 0.99, 0.995, 1.0]  # two groups of targets
core.histogram_quantile(xl, values=vl, q=q, bins=edges, axis=1)
desc("quantile radix")
core.histogram_quantile(xs, values=vs, q=q, bins=edges, axis=0)
desc("quantile short")
core.histogram_weighted_quantile(xl, values=vl, weights=wl, q=q, bins=edges, axis=1)
desc("weighted_quantile radix")
core.histogram_weighted_quantile(xs, values=vs, weights=ws, q=q, bins=edges, axis=0)
desc("weighted_quantile short")
core.histogram_mean_var(xl, values=vl, bins=edges, axis=1)
desc("mean_var")
core.histogram_mean_var(xl, values=vl, weights=wl, bins=edges, axis=1)
desc("mean_var_w")
