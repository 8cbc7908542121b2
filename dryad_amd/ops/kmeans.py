"""k-means step on MFMA (HIP kernels in csrc/kernels/kmeans.hip, 128-dim points, and
csrc/kernels/kmeans_dim.hip, any other width from 1 to 512).

K <= 1024 runs on a per-table state (``SplitPoints``, cached per point tensor): the bf16 rounding
of every coordinate and |x| per point, written once, so an iteration's assignment kernel reads
half the bytes of the f32 rows; and the per-cluster sums and counts, kept with the table and
updated only for the points whose cluster changed (their exact f32 rows move from the old
cluster's sums to the new one's).  K <= 64 (the benchmark's K = 64) keeps all centroids in LDS;
64 < K <= 1024 keeps the points in registers and streams the split centroids through LDS in
64-centroid chunks (``dr_kmeans_step_plane``); ``step`` takes that path only on request
(``planes=True``, see ``PLANES_DEFAULT_MAX_K``).  Larger K, or a plane that does not fit in free
HBM, use the f32 kernels.

Points of any other width D in 1 .. ``MAX_DIM`` run the plane path of kmeans_dim.hip for every K
up to 1024: the plane rows are padded to ``padded_dim(D)``, the f32 rows stay at pitch D.  There
are no f32 kernels for those widths, so ``planes=False``, K > 1024 or a plane that does not fit
are errors there.
"""
from __future__ import annotations

import weakref

import torch

from . import _lib
from ._lib import c_i32, c_u64, ptr, stream_of, vp

DIM = 128
MAX_DIM = 512
# plane row widths (bf16 per point) that kmeans_dim.hip instantiates
_PLANE_WIDTHS = (32, 64, 96, 128, 192, 256, 384, 512)

_lib.register_signatures({
    "dr_kmeans_mode": (c_i32, [c_i32]),
    "dr_kmeans_step": (c_i32, [vp, c_u64, c_i32, vp, c_i32, vp, vp, vp, vp, vp, vp]),
    "dr_kmeans_near_workspace": (c_u64, [c_u64]),
    "dr_kmeans_gen": (c_i32, [vp, c_u64, c_i32, c_u64, c_i32, c_u64, vp]),
    "dr_kmeans_hi": (c_i32, [vp, c_u64, vp, vp, vp]),
    "dr_kmeans_step_hi": (c_i32, [vp, vp, vp, c_u64, vp, c_i32, vp, vp, vp, vp, vp, vp, vp]),
    "dr_kmeans_centroid_workspace": (c_u64, [c_i32]),
    "dr_kmeans_step_plane": (c_i32, [vp, vp, vp, c_u64, vp, c_i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "dr_kmeans_dim_padded": (c_i32, [c_i32]),
    "dr_kmeans_dim_plane": (c_i32, [vp, c_u64, c_i32, c_i32, vp, vp, vp]),
    "dr_kmeans_dim_centroid_workspace": (c_u64, [c_i32, c_i32]),
    "dr_kmeans_dim_step": (c_i32, [vp, vp, vp, c_u64, c_i32, vp, c_i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "dr_kmeans_dim_gen": (c_i32, [vp, c_u64, c_i32, c_u64, c_i32, c_u64, vp]),
})

PLANES_MAX_K = 1024
# largest K that step() puts on the plane by itself (planes=None).  Above 64 the plane path is
# opt-in (planes=True): its bf16 estimate cannot order centroids closer than ~8e-3 |x| max|c|, and
# with several centroids per natural cluster every point is re-ranked in f32, which measured 5x
# slower than the f32 kernels at K = 128 .. 1024 (profiles/kmeans_largek_bw.log); it wins only
# when the centroids are that far apart.
PLANES_DEFAULT_MAX_K = 64
# free HBM kept beyond the planes (the step's workspace and whatever the job allocates next)
PLANES_HEADROOM = 4 << 30


def padded_dim(dim: int) -> int:
    """bf16 per plane row for ``dim``-wide points (``dr_kmeans_dim_padded``); 128 stays 128."""
    if not 1 <= dim <= MAX_DIM:
        raise ValueError(f"kmeans: the point dimension must be in 1 .. {MAX_DIM} (D = {dim})")
    return next(w for w in _PLANE_WIDTHS if w >= dim)


class KMeansWorkspace:
    """Per-K scratch buffers reused across iterations (no allocation inside the loop)."""

    def __init__(self, n: int, k: int, device, dim: int = DIM):
        self.k = k
        self.dim = dim
        self.cnorm = torch.empty(k, dtype=torch.float32, device=device)
        self.assign = torch.empty(n, dtype=torch.int32, device=device)
        self.sums = torch.empty((k, dim), dtype=torch.float64, device=device)
        self.counts = torch.empty(k, dtype=torch.int64, device=device)
        # near-tie list of the bf16-MFMA paths (count + (point, estimate) pairs)
        self.near = torch.empty(int(_lib.lib().dr_kmeans_near_workspace(c_u64(n))) if k <= PLANES_MAX_K else 16,
                                dtype=torch.uint8, device=device)
        # split centroids (ch, cm, |c|^2 in 64-centroid chunks) of the 64 < K <= 1024 plane path
        if dim == DIM:
            cbytes = int(_lib.lib().dr_kmeans_centroid_workspace(k)) if 64 < k <= PLANES_MAX_K else 16
        else:
            cbytes = int(_lib.lib().dr_kmeans_dim_centroid_workspace(k, dim)) if k <= PLANES_MAX_K else 16
        self.csplit = torch.empty(max(cbytes, 16), dtype=torch.uint8, device=device)


class SplitPoints:
    """Per-point-table state of the plane path: ``xh`` [n, padded_dim(D)] bf16 (round-to-nearest
    of x, zero in the pad), ``xnorm`` |x| per point, and the running per-cluster state of the last
    step: ``prev`` (final assignment, -1 = none), ``sums`` (K x D f64) and ``counts`` (K i64)."""

    def __init__(self, x: torch.Tensor):
        n, dim = x.shape
        self.n = n
        self.dim = dim
        self.version = x._version
        dp = padded_dim(dim)
        # the plane kernel writes the pad itself
        self.xh = (torch.empty if x.is_cuda else torch.zeros)((n, dp), dtype=torch.bfloat16, device=x.device)
        self.xnorm = torch.empty(n, dtype=torch.float32, device=x.device)
        self.prev = torch.full((n,), -1, dtype=torch.int32, device=x.device)
        self.sums = self.counts = None
        if x.is_cuda and dim == DIM:
            _lib.call("dr_kmeans_hi", ptr(x), c_u64(n), ptr(self.xh), ptr(self.xnorm), stream_of(x))
        elif x.is_cuda:
            _lib.call("dr_kmeans_dim_plane", ptr(x), c_u64(n), dim, dp, ptr(self.xh), ptr(self.xnorm), stream_of(x))
        else:
            self.xh[:, :dim].copy_(x.bfloat16())
            self.xnorm.copy_(x.double().norm(dim=1).float())

    def state_for(self, k: int):
        """The running sums / counts for ``k`` clusters; a new K restarts them (every point moves)."""
        if self.sums is None or self.sums.shape[0] != k:
            self.sums = torch.zeros((k, self.dim), dtype=torch.float64, device=self.xh.device)
            self.counts = torch.zeros(k, dtype=torch.int64, device=self.xh.device)
            self.prev.fill_(-1)
        return self.sums, self.counts


# (device, data_ptr, n, D) -> SplitPoints.  The entry lives as long as the tensor that owns the
# points' memory (the base of whatever view the caller passes: a table column handed out as a new
# view every iteration still hits), and is checked against that owner and its version counter.
_SPLITS: dict = {}


def split_bytes(n: int, dim: int = DIM) -> int:
    return n * (padded_dim(dim) * 2 + 4 + 4)


def split_points(x: torch.Tensor, create: bool = True) -> SplitPoints | None:
    """The cached split of ``x`` (recomputed if ``x`` was modified in place since).  Returns None
    when the planes do not fit in free HBM (the caller then runs the f32 kernels)."""
    base = x if x._base is None else x._base
    key = (str(x.device), x.data_ptr(), x.shape[0], x.shape[1])
    sp = _SPLITS.get(key)
    if sp is not None and sp.owner() is base and sp.version == x._version:
        return sp
    if not create:
        return None
    _SPLITS.pop(key, None)
    if x.is_cuda:
        free, _total = torch.cuda.mem_get_info(x.device)
        cached = torch.cuda.memory_reserved(x.device) - torch.cuda.memory_allocated(x.device)
        if split_bytes(x.shape[0], x.shape[1]) + PLANES_HEADROOM > free + cached:
            return None
    sp = SplitPoints(x)

    def _drop(ref, key=key):
        cur = _SPLITS.get(key)
        if cur is not None and cur.owner is ref:
            del _SPLITS[key]

    sp.owner = weakref.ref(base, _drop)
    _SPLITS[key] = sp
    return sp


def split_reference(x: torch.Tensor):
    """torch twin of kmeans_split_kernel: x = xh + xm + xl, each a round-to-nearest bf16 of the
    remainder so far (exact: the remainders are exact in f32 and 3 x 8 significand bits cover 24;
    for |x| >= 2^-100, where the remainders stay normal numbers)."""
    x = x.float()
    h = x.bfloat16()
    r1 = x - h.float()
    m = r1.bfloat16()
    lo = (r1 - m.float()).bfloat16()
    return h, m, lo


def mode(k: int) -> int:
    """0: centroids + accumulator slab in LDS; 1: streamed centroid tiles + slab; 2: two-pass;
    3: K <= 64 on bf16 MFMA (split-precision distances, exact re-rank of near ties, MFMA sums)."""
    return int(_lib.lib().dr_kmeans_mode(k))


def generate(points: torch.Tensor, first: int = 0, blobs: int = 64, seed: int = 0x6B6D) -> torch.Tensor:
    """Deterministic synthetic Gaussian-blob points (counter based: slices of a global set agree)."""
    _lib.require_gpu_tensor(points, "kmeans.generate")
    assert points.dtype == torch.float32 and points.dim() == 2 and 1 <= points.shape[1] <= MAX_DIM
    assert points.is_contiguous()
    dim = points.shape[1]
    _lib.call("dr_kmeans_gen" if dim == DIM else "dr_kmeans_dim_gen", ptr(points), c_u64(points.shape[0]), dim,
              c_u64(first), int(blobs), c_u64(seed), stream_of(points))
    _lib.written(points)
    return points


def step(points: torch.Tensor, centroids: torch.Tensor, ws: KMeansWorkspace | None = None,
         planes: bool | None = None):
    """One assignment + partial-sum pass.  Returns (sums f64 [K,D], counts i64 [K], assign i32 [n]).

    ``planes``: None = the bf16-plane path with kept sums when K <= 64 and the plane fits (the
    default), False = the f32 kernels, True = the plane path or an error.  Points of a width other
    than 128 (1 .. ``MAX_DIM``) always take the plane path of kmeans_dim.hip, K <= 1024."""
    _lib.require_gpu_tensor(points, "kmeans.step")
    _lib.require_gpu_tensor(centroids, "kmeans.step")
    assert points.dtype == torch.float32 and centroids.dtype == torch.float32
    assert points.dim() == 2 and centroids.dim() == 2 and points.shape[1] == centroids.shape[1]
    if points.shape[1] != DIM:
        return _step_dim(points, centroids, ws, planes)
    if ws is not None and ws.dim != DIM:
        ws = None
    n, k = points.shape[0], centroids.shape[0]
    if ws is None or ws.k != k or ws.assign.shape[0] < n:
        ws = KMeansWorkspace(n, k, points.device)
    ws.sums.zero_()
    ws.counts.zero_()
    sp = None
    if planes is not False and 1 <= k <= (PLANES_MAX_K if planes else PLANES_DEFAULT_MAX_K) and n > 0:
        sp = split_points(points)
        if sp is None and planes:
            raise MemoryError(f"kmeans.step: the bf16 plane of {n} points ({split_bytes(n) >> 20} MiB) does not fit")
    elif planes:
        raise ValueError(f"kmeans.step: the plane path needs 1 <= K <= {PLANES_MAX_K} (K = {k})")
    if sp is not None:
        sums, counts = sp.state_for(k)
        _lib.call("dr_kmeans_step_plane", ptr(sp.xh), ptr(sp.xnorm), ptr(points), c_u64(n), ptr(centroids), k,
                  ptr(ws.cnorm), ptr(ws.assign), ptr(sp.prev), ptr(sums), ptr(counts), ptr(ws.near),
                  ptr(ws.csplit), stream_of(points))
        ws.sums.copy_(sums)
        ws.counts.copy_(counts)
        return ws.sums, ws.counts, ws.assign[:n]
    _lib.call("dr_kmeans_step", ptr(points), c_u64(n), DIM, ptr(centroids), k, ptr(ws.cnorm), ptr(ws.assign),
              ptr(ws.sums), ptr(ws.counts), ptr(ws.near), stream_of(points))
    return ws.sums, ws.counts, ws.assign[:n]


def _step_dim(points: torch.Tensor, centroids: torch.Tensor, ws: KMeansWorkspace | None, planes: bool | None):
    """``step`` for points of a width other than 128 (csrc/kernels/kmeans_dim.hip)."""
    n, d = points.shape
    k = centroids.shape[0]
    if not 1 <= d <= MAX_DIM or not 1 <= k <= PLANES_MAX_K or planes is False:
        raise ValueError(f"kmeans.step: {d}-dim points run on the plane path only (planes is not False), "
                         f"1 <= D <= {MAX_DIM} and 1 <= K <= {PLANES_MAX_K} (K = {k})")
    assert points.is_contiguous() and centroids.is_contiguous() and n < 1 << 32
    if ws is None or ws.k != k or ws.dim != d or ws.assign.shape[0] < n:
        ws = KMeansWorkspace(n, k, points.device, dim=d)
    if n == 0:
        ws.sums.zero_()
        ws.counts.zero_()
        return ws.sums, ws.counts, ws.assign[:0]
    sp = split_points(points)
    if sp is None:
        raise MemoryError(f"kmeans.step: the bf16 plane of {n} {d}-dim points ({split_bytes(n, d) >> 20} MiB) "
                          "does not fit, and there are no f32 kernels for this width")
    sums, counts = sp.state_for(k)
    _lib.call("dr_kmeans_dim_step", ptr(sp.xh), ptr(sp.xnorm), ptr(points), c_u64(n), d, ptr(centroids), k,
              ptr(ws.cnorm), ptr(ws.assign), ptr(sp.prev), ptr(sums), ptr(counts), ptr(ws.near), ptr(ws.csplit),
              stream_of(points))
    ws.sums.copy_(sums)
    ws.counts.copy_(counts)
    return ws.sums, ws.counts, ws.assign[:n]


def update(centroids: torch.Tensor, sums: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
    """New centroids = sums / counts; empty clusters keep their old centre."""
    c = counts.to(torch.float64).unsqueeze(1)
    new = torch.where(c > 0, sums / c.clamp_min(1), centroids.to(torch.float64))
    return new.to(torch.float32)


def step_reference(points: torch.Tensor, centroids: torch.Tensor):
    """Plain PyTorch fp32 reference of the same op (for numerics tests)."""
    d = (centroids * centroids).sum(1)[None, :] - 2.0 * points @ centroids.T
    a = torch.argmin(d, dim=1)
    k = centroids.shape[0]
    sums = torch.zeros((k, points.shape[1]), dtype=torch.float64, device=points.device)
    sums.index_add_(0, a, points.to(torch.float64))
    counts = torch.bincount(a, minlength=k)
    return sums, counts, a.to(torch.int32), d
