"""histogram_weighted_quantile at C2's full size (10^9 float64 samples, values and exactly summable weights, 100 bins), the
quartiles, checked by exact weighted counting on the device: index_add_ of exactly summable weights is exact in any order, so
with L = sum w[v < x], U = sum w[v <= x] and W per bin the result x satisfies L / W < q <= U / W.  The fullest bin holds about
3 * 10^7 samples, below the 2^28 the weights' exactness allows.  (The sums go to 2^16 partial sums per bin, by the sample's
position, and those are then added: 10^9 float64 atomics on 100 addresses take minutes, and the order does not matter.)"""
import numpy as np
import pytest

import exact_weights as xw

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def test_c2_full_size_weighted_quartiles_by_exact_weighted_counting():
    from xhistogram_amd import _native, core

    if _native.device_count() < 1:
        pytest.skip("no MI355X visible")
    g = torch.Generator(device="cuda")
    g.manual_seed(2)
    n = 10 ** 9
    x = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
    v = torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
    # exact_weights.f64 on the device: (2^24 + k) * 2^-25, about 30 % of them zero
    w = torch.randint(0, 1 << 24, (n,), dtype=torch.int64, device="cuda", generator=g).add_(1 << 24).to(torch.float64).mul_(2.0 ** -25)
    w.mul_((torch.rand(n, dtype=torch.float32, device="cuda", generator=g) >= 0.3).to(torch.float64))
    edges = np.linspace(-4, 4, 101)
    q = [0.25, 0.75]
    got, _ = core.histogram_weighted_quantile(x, values=v, weights=w, q=q, bins=[edges])
    assert got.shape == (2, 100) and got.is_cuda
    counts, _ = core.histogram(x, bins=[edges])
    xw.assert_summable(counts.cpu().numpy())
    e = torch.as_tensor(edges, device="cuda")
    b = torch.bucketize(x, e, right=True) - 1
    b = torch.where(x == e[-1], 99, b)
    del x
    ok = (b >= 0) & (b < 100)
    b = torch.where(ok, b, 0)
    w = torch.where(ok, w, torch.zeros((), dtype=torch.float64, device="cuda"))
    del ok
    spread = 1 << 16
    b.mul_(spread).add_(torch.arange(n, dtype=torch.int64, device="cuda").remainder_(spread))

    def per_bin(weights):
        return torch.zeros(100 * spread, dtype=torch.float64, device="cuda").index_add_(0, b, weights).reshape(100, spread).sum(1)

    W = per_bin(w)
    has = W > 0
    assert bool(has.any())
    for i, qq in enumerate(q):
        xb = got[i][b >> 16]
        L = per_bin(torch.where(v < xb, w, torch.zeros_like(w)))
        U = per_bin(torch.where(v <= xb, w, torch.zeros_like(w)))
        del xb
        print("q=%r: L/W in [%r, %r], U/W in [%r, %r]" % (qq, float((L / W)[has].min()), float((L / W)[has].max()),
                                                         float((U / W)[has].min()), float((U / W)[has].max())))
        assert bool(torch.all(~has | ((L / W < qq) & (qq <= U / W)))), qq
        assert bool(torch.all(torch.isnan(got[i]) == ~has))
