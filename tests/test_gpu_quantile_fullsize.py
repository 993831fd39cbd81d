"""histogram_quantile at C2's full size (10^9 float64 samples and values, 100 bins), lower and higher quartiles, checked by
exact counting on the device: the value x of rank r in its bin satisfies #(v < x) <= r < #(v <= x) among the bin's values."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("method", ["lower", "higher"])
def test_c2_full_size_quartiles_by_counting(method):
    from xhistogram_amd import _native, core

    if _native.device_count() < 1:
        pytest.skip("no MI355X visible")
    g = torch.Generator(device="cuda")
    g.manual_seed(2)
    n = 10 ** 9
    x = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
    v = torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
    edges = np.linspace(-4, 4, 101)
    q = [0.25, 0.75]
    got, _ = core.histogram_quantile(x, values=v, q=q, bins=[edges], method=method)
    assert got.shape == (2, 100) and got.is_cuda
    counts, _ = core.histogram(x, bins=[edges])
    e = torch.as_tensor(edges, device="cuda")
    b = torch.bucketize(x, e, right=True) - 1
    b = torch.where(x == e[-1], 99, b)
    del x
    ok = (b >= 0) & (b < 100)
    b = torch.where(ok, b, 0)
    nb = torch.zeros(100, dtype=torch.int64, device="cuda").index_add_(0, b, ok.to(torch.int64))
    np.testing.assert_array_equal(nb.cpu().numpy(), counts.cpu().numpy().astype(np.int64))
    for i, qq in enumerate(q):
        vi = (nb - 1).to(torch.float64) * qq
        r = (torch.floor(vi) if method == "lower" else torch.ceil(vi)).to(torch.int64)
        xb = got[i][b]
        below = torch.zeros(100, dtype=torch.int64, device="cuda").index_add_(0, b, (ok & (v < xb)).to(torch.int64))
        upto = torch.zeros(100, dtype=torch.int64, device="cuda").index_add_(0, b, (ok & (v <= xb)).to(torch.int64))
        del xb
        has = nb > 0
        assert bool(torch.all(~has | ((below <= r) & (r < upto)))), (method, qq)
        assert bool(torch.all(torch.isnan(got[i]) == ~has))
