"""k-means for point widths other than 128 on the CPU side: generator twin, gen://points schema and
the LocalDebug job against the numpy reference."""
import numpy as np
import pytest

import dryad_amd as D
from dryad_amd import types as T
from dryad_amd.models.kmeans import KMeansConfig, KMeansJob, reference
from dryad_amd.models.kmeans_cpu import gen_points


@pytest.mark.parametrize("dim", [1, 48, 300])
def test_gen_points_any_dim(dim):
    a = gen_points(5, 40, 7, 3, dim=dim)
    assert a.dtype == np.float32 and a.shape == (40, dim)
    if dim <= 128:   # the formula indexes by dimension
        np.testing.assert_array_equal(a, gen_points(5, 40, 7, 3)[:, :dim])


def test_gen_uri_schema_carries_dim():
    c = D.DryadLinqContext(1)
    c.LocalDebug = True
    q = c.FromStore("gen://points?count=10&partitions=1&blobs=3&seed=1&dim=16")
    assert q.dtype == T.Vector(T.Float32, 16)
    rows = list(q)
    assert len(rows) == 10 and all(len(r) == 16 for r in rows)


def test_kmeans_localdebug_dim16_matches_numpy_reference():
    c = D.DryadLinqContext(1)
    c.LocalDebug = True
    cfg = KMeansConfig(points_per_partition=1500, k=6, dim=16, blobs=6, iterations=2)
    r = KMeansJob(c, cfg, partitions=2).run()
    assert r.centroids.shape == (6, 16)
    np.testing.assert_allclose(r.centroids, reference(cfg, 2, r.iterations), rtol=0, atol=1e-6)
