"""k-means plane path for 64 < K <= 1024 (K-tiled bf16 MFMA assignment, strided re-rank, sliced
movers) against plain f64 references."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,k", [(1000, 65), (3001, 130), (5003, 257), (3001, 520), (3001, 1024)])
def test_largek_step_matches_f64(n, k):
    """Every movers slice width, a ragged last tile, several point blocks.  The assignment may
    differ from the f64 argmin only where the f64 top-2 gap is within the rounding of two f32
    128-term distances (gamma_128 = 128 * 2^-24 on 2 x.c and on |c|^2, two centroids)."""
    from dryad_amd.ops import kmeans as KM
    g = torch.Generator().manual_seed(n + k)
    x = torch.randn((n, KM.DIM), generator=g)
    c = torch.randn((k, KM.DIM), generator=g)
    sums, counts, assign = KM.step(x.cuda(), c.cuda(), planes=True)
    xd, cd = x.double(), c.double()
    d = (cd * cd).sum(1)[None, :] - 2.0 * xd @ cd.T
    top2 = torch.topk(d, 2, dim=1, largest=False)
    cmax = cd.norm(dim=1).max()
    tied = (top2.values[:, 1] - top2.values[:, 0]) <= 5e-5 * (xd.norm(dim=1) + cmax) * cmax
    assert int(tied.sum()) <= 0.005 * n
    a = assign.long().cpu()
    assert int(((a != top2.indices[:, 0]) & ~tied).sum()) == 0
    assert torch.equal(counts.cpu(), torch.bincount(a, minlength=k))
    ref = torch.zeros((k, KM.DIM), dtype=torch.float64).index_add_(0, a, xd)
    torch.testing.assert_close(sums.cpu(), ref, rtol=1e-12, atol=1e-8)


@pytest.mark.parametrize("k", [65, 1024])
def test_largek_sums_exact_on_24bit_points(k):
    """One 24-bit point per cluster: the sums are the points bit for bit, also after every point
    changes cluster (rows are subtracted and added)."""
    from dryad_amd.ops import kmeans as KM
    g = torch.Generator().manual_seed(5)
    x = torch.randint(1 << 23, 1 << 24, (k, KM.DIM), generator=g).float().cuda() * 2.0 ** -20
    ws = KM.KMeansWorkspace(k, k, x.device)
    sums, counts, assign = KM.step(x, x.clone(), ws, planes=True)
    assert torch.equal(assign.long().cpu(), torch.arange(k))
    assert torch.equal(counts, torch.ones(k, dtype=torch.int64, device="cuda"))
    assert torch.equal(sums, x.double())
    perm = torch.randperm(k, generator=g)
    sums, counts, assign = KM.step(x, x[perm.cuda()].clone(), ws, planes=True)
    assert torch.equal(assign.long().cpu(), torch.argsort(perm))
    assert torch.equal(sums, x[perm.cuda()].double())


@pytest.mark.parametrize("k", [65, 130])
def test_largek_near_ties_across_chunks(k):
    """Points just off the bisector of c[0] and c[k - 1] = c[0] + u: best and runner-up live in
    different 64-centroid chunks and only the exact re-rank can order them."""
    from dryad_amd.ops import kmeans as KM
    g = torch.Generator().manual_seed(1)
    c = (torch.rand((k, KM.DIM), generator=g, dtype=torch.float64) * 10 - 5)
    u = torch.randn(KM.DIM, generator=g, dtype=torch.float64)
    u /= u.norm()
    c[k - 1] = c[0] + u
    n = 4096
    eps = (torch.rand(n, generator=g, dtype=torch.float64) - 0.5) * 0.04
    eps[eps.abs() < 0.004] = 0.004
    x = (c[0] + c[k - 1]) / 2 + eps[:, None] * u[None, :]
    xf, cf = x.float().cuda(), c.float().cuda()
    sums, counts, assign = KM.step(xf, cf, planes=True)
    d = ((xf.double()[:, None, :] - cf.double()[None, :, :]) ** 2).sum(-1)
    assert torch.equal(assign.long().cpu(), torch.argmin(d, 1).cpu())
    assert int(counts.sum()) == n


def test_largek_iterations_track_f64_sums():
    """Ten iterations: rows move between the kept sums; every step's sums equal the f64 sums of
    its own assignment up to f64 summation order."""
    from dryad_amd.ops import kmeans as KM
    n, k = 20000, 130
    x = torch.empty((n, KM.DIM), dtype=torch.float32, device="cuda")
    KM.generate(x, 0, blobs=64, seed=11)
    x.add_(1000.0)
    c = x[:k].clone()
    ws = KM.KMeansWorkspace(n, k, x.device)
    for _ in range(10):
        last = c
        s, cnt, a = KM.step(x, c, ws, planes=True)
        assert torch.equal(cnt, torch.bincount(a.long(), minlength=k))
        ref = torch.zeros((k, KM.DIM), dtype=torch.float64, device="cuda").index_add_(0, a.long(), x.double())
        torch.testing.assert_close(s, ref, rtol=1e-12, atol=1e-6)
        c = KM.update(c, s, cnt)
    _rs, _rc, ra, d = KM.step_reference(x, last)
    top2 = torch.topk(d.double(), 2, dim=1, largest=False).values
    cmax = last.double().norm(dim=1).max()
    tied = (top2[:, 1] - top2[:, 0]) <= 5e-5 * (x.double().norm(dim=1) + cmax) * cmax
    assert int(((a.long() != ra.long()) & ~tied).sum()) == 0
