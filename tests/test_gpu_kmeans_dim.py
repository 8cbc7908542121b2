"""k-means plane path for point widths other than 128 (csrc/kernels/kmeans_dim.hip: padded bf16
plane, NS-templated MFMA assignment, f32 re-rank and sliced movers at pitch D) against plain f64
references."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _tied(d, xd, cd):
    """Points whose f64 top-2 gap is within the rounding of two f32 D-term distances (or the
    5e-5 of the large-K test)."""
    top2 = torch.topk(d, 2, dim=1, largest=False).values
    cmax = cd.norm(dim=1).max()
    return (top2[:, 1] - top2[:, 0]) <= max(5e-5, 4 * xd.shape[1] * 2.0 ** -24) * (xd.norm(dim=1) + cmax) * cmax


@pytest.mark.parametrize("n,k,dim", [(1000, 3, 1), (3001, 64, 2), (3001, 17, 3), (3001, 65, 31), (5003, 64, 33),
                                     (2000, 64, 100), (3001, 257, 129), (2000, 64, 256), (1500, 1024, 300),
                                     (3001, 130, 512)])
def test_dim_step_matches_f64(n, k, dim):
    """Odd and unaligned row pitches, a padded width one step past a multiple of 32, every chunk
    geometry, ragged last tiles, one and several chunks, ragged mover slices."""
    from dryad_amd.ops import kmeans as KM
    g = torch.Generator().manual_seed(n + k + dim)
    x = torch.randn((n, dim), generator=g)
    c = torch.randn((k, dim), generator=g)
    sums, counts, assign = KM.step(x.cuda(), c.cuda())
    xd, cd = x.double(), c.double()
    d = (cd * cd).sum(1)[None, :] - 2.0 * xd @ cd.T
    tied = _tied(d, xd, cd)
    a = assign.long().cpu()
    print(f"tied {int(tied.sum())} of {n}, mismatches {int((a != d.argmin(1)).sum())}")
    assert int(tied.sum()) <= 0.01 * n
    assert int(((a != d.argmin(1)) & ~tied).sum()) == 0
    assert torch.equal(counts.cpu(), torch.bincount(a, minlength=k))
    ref = torch.zeros((k, dim), dtype=torch.float64).index_add_(0, a, xd)
    torch.testing.assert_close(sums.cpu(), ref, rtol=1e-12, atol=1e-8)


@pytest.mark.parametrize("n,k,dim", [(700001, 64, 2), (150001, 130, 300)])
def test_dim_workgroups_walk_several_blocks(n, k, dim):
    """More point blocks (128 points each) than resident workgroups, so the assignment kernel's
    block loop, prefetch hand-over and running chunk parity are used; the f64 reference runs on
    the GPU."""
    from dryad_amd.ops import kmeans as KM
    g = torch.Generator().manual_seed(n + k + dim)
    x = torch.randn((n, dim), generator=g).cuda()
    c = torch.randn((k, dim), generator=g).cuda()
    sums, counts, assign = KM.step(x, c)
    xd, cd = x.double(), c.double()
    d = (cd * cd).sum(1)[None, :] - 2.0 * xd @ cd.T
    a = assign.long()
    assert int(((a != d.argmin(1)) & ~_tied(d, xd, cd)).sum()) == 0
    assert torch.equal(counts, torch.bincount(a, minlength=k))
    ref = torch.zeros((k, dim), dtype=torch.float64, device="cuda").index_add_(0, a, xd)
    torch.testing.assert_close(sums, ref, rtol=1e-12, atol=1e-7)


@pytest.mark.parametrize("k,dim", [(5, 3), (65, 33), (64, 300)])
def test_dim_sums_exact_on_24bit_points(k, dim):
    """One 24-bit point per cluster: the sums are the points bit for bit, also after every point
    changes cluster (rows are subtracted and added)."""
    from dryad_amd.ops import kmeans as KM
    g = torch.Generator().manual_seed(5)
    x = torch.randint(1 << 23, 1 << 24, (k, dim), generator=g).float().cuda() * 2.0 ** -20
    ws = KM.KMeansWorkspace(k, k, x.device, dim=dim)
    sums, counts, assign = KM.step(x, x.clone(), ws)
    assert torch.equal(assign.long().cpu(), torch.arange(k))
    assert torch.equal(counts, torch.ones(k, dtype=torch.int64, device="cuda"))
    assert torch.equal(sums, x.double())
    perm = torch.randperm(k, generator=g)
    sums, counts, assign = KM.step(x, x[perm.cuda()].clone(), ws)
    assert torch.equal(assign.long().cpu(), torch.argsort(perm))
    assert torch.equal(sums, x[perm.cuda()].double())


@pytest.mark.parametrize("k,dim", [(64, 2), (130, 33), (65, 200)])
def test_dim_near_ties_need_the_rerank(k, dim):
    """Points just off the bisector of c[0] and c[k - 1] = c[0] + u, |u| = 1, by eps with |eps| in
    [m, 5 m]: the gap 2 eps is at least twice the rounding of the f32 re-rank
    (m = 4 D 2^-24 (|x| + cmax) cmax) and far below the bf16 estimate's bound."""
    from dryad_amd.ops import kmeans as KM
    g = torch.Generator().manual_seed(1)
    c = torch.rand((k, dim), generator=g, dtype=torch.float64) * 2 - 1
    u = torch.randn(dim, generator=g, dtype=torch.float64)
    u /= u.norm()
    c[k - 1] = c[0] + u
    n = 4096
    mid = (c[0] + c[k - 1]) / 2
    cmax = c.norm(dim=1).max()
    m = 4 * dim * 2.0 ** -24 * (mid.norm() + cmax) * cmax
    eps = m * (1 + 4 * torch.rand(n, generator=g, dtype=torch.float64))
    eps *= torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    x = mid + eps[:, None] * u[None, :]
    xf, cf = x.float().cuda(), c.float().cuda()
    sums, counts, assign = KM.step(xf, cf)
    xd, cd = xf.double(), cf.double()
    d = (cd * cd).sum(1)[None, :] - 2.0 * xd @ cd.T
    assert torch.equal(assign.long(), d.argmin(1))
    assert int(counts.sum()) == n


def test_dim_iterations_track_f64_sums():
    """Ten iterations at D = 48: rows move between the kept sums; every step's sums equal the f64
    sums of its own assignment up to f64 summation order."""
    from dryad_amd.ops import kmeans as KM
    n, k, dim = 20000, 20, 48
    x = torch.empty((n, dim), dtype=torch.float32, device="cuda")
    KM.generate(x, 0, blobs=64, seed=11)
    x.add_(1000.0)
    c = x[:k].clone()
    ws = KM.KMeansWorkspace(n, k, x.device, dim=dim)
    for _ in range(10):
        last = c
        s, cnt, a = KM.step(x, c, ws)
        assert torch.equal(cnt, torch.bincount(a.long(), minlength=k))
        ref = torch.zeros((k, dim), dtype=torch.float64, device="cuda").index_add_(0, a.long(), x.double())
        torch.testing.assert_close(s, ref, rtol=1e-12, atol=1e-6)
        c = KM.update(c, s, cnt)
    _rs, _rc, ra, d = KM.step_reference(x, last)
    tied = _tied(d.double(), x.double(), last.double())
    assert int(((a.long() != ra.long()) & ~tied).sum()) == 0


@pytest.mark.parametrize("dim", [1, 48, 300])
def test_dim_generator_matches_numpy_twin(dim):
    from dryad_amd.models.kmeans_cpu import gen_points
    from dryad_amd.ops import kmeans as KM
    whole = KM.generate(torch.empty((3000, dim), dtype=torch.float32, device="cuda"), 0, blobs=7, seed=3)
    assert np.array_equal(whole.cpu().numpy(), gen_points(0, 3000, 7, 3, dim))
    part = KM.generate(torch.empty((1000, dim), dtype=torch.float32, device="cuda"), 2000, blobs=7, seed=3)
    assert torch.equal(part, whole[2000:])


def test_dim_job_through_query_api():
    import dryad_amd as D
    from dryad_amd.models.kmeans import KMeansConfig, KMeansJob, reference
    ctx = D.DryadLinqContext(platform="gpu")
    ctx.PartitionCount = 1
    cfg = KMeansConfig(points_per_partition=20000, k=8, dim=24, blobs=8, iterations=3)
    res = KMeansJob(ctx, cfg, partitions=1).run()
    assert res.centroids.shape == (8, 24)
    np.testing.assert_allclose(res.centroids, reference(cfg, 1), atol=1e-4)
    assert ctx._get_executor().last_result["fallbacks"] == []
