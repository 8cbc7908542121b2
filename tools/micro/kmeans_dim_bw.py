"""k-means step at point widths other than 128 (ops/kmeans.step -> csrc/kernels/kmeans_dim.hip)
against the plane's copy_ rate and against the torch reference:

    python tools/micro/kmeans_dim_bw.py [base_points] [dims] [ks]

``base_points`` (default 50e6) 128-dim points' worth of f32 bytes per width: D in
(2, 16, 32, 64, 96, 256, 512) runs base * 128 / D blob points (KM.generate, 64 blobs), halved until
the point table, its plane and the workspaces fit in free HBM (the n used is printed), for K in
(16, 64, 256) with the first K points as centroids.  Per (D, K), min .. max of 3 rounds after a
warm-up round, host clock around one ``KM.step`` that ends in a device synchronise, the three
settings alternating within a round:

    first    every point is new to the kept sums (prev = -1): assignment + movers of all rows
    steady   the step after one centroid update: assignment + movers of the rows that changed
    repeat   the same centroids again: nothing moves, so assignment (estimate, near list, re-rank)
             plus the movers' scan of assign / prev; first - repeat and steady - repeat are the
             movers' share of those two steps

``copy`` is a ``copy_`` of the plane's bytes (read + write) in the same process, the assignment's
memory roof; ``reference`` is ``KM.step_reference`` (matmul, argmin, index_add_), what runs without
these kernels, timed on the first 4M rows of the same tensors and scaled to n (its n x K distance
matrix does not fit at n; a user would chunk it the same way).  The warm-up round also checks the
step's assignment of the first 2M rows against the f64 argmin outside the tests' tied set.  A last
section runs D = 128 through the new kernels and through the existing plane path, alternating,
as a sanity line."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

from dryad_amd.ops import _lib  # noqa: E402
from dryad_amd.ops import kmeans as KM  # noqa: E402
from dryad_amd.ops._lib import c_u64, ptr, stream_of  # noqa: E402

REF_ROWS = 1 << 22


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def span(ts):
    return f"{min(ts):.2f} .. {max(ts):.2f} ms"


def mismatches(x, c, assign, rows=1 << 21):
    """Points of the first ``rows`` whose assignment is not the f64 argmin, outside the tied set."""
    xd, cd = x[:rows].double(), c.double()
    d = (cd * cd).sum(1)[None, :] - 2.0 * xd @ cd.T
    top2 = torch.topk(d, 2, dim=1, largest=False)
    cmax = cd.norm(dim=1).max()
    tied = (top2.values[:, 1] - top2.values[:, 0]) <= max(5e-5, 4 * x.shape[1] * 2.0 ** -24) * (xd.norm(dim=1) + cmax) * cmax
    return int(((assign[:rows].long() != top2.indices[:, 0]) & ~tied).sum()), int(tied.sum()), xd.shape[0]


def fit_points(n, dim):
    """n halved until x, its plane, a plane copy, assign / prev / near and the reference's chunk fit."""
    free, _total = torch.cuda.mem_get_info()
    while n * (dim * 4 + 2 * KM.padded_dim(dim) * 2 + 8 + 16) + (8 << 30) > free:
        n //= 2
    return n


def restart(sp):
    sp.sums = sp.counts = None          # state_for() then zeroes the sums and fills prev with -1


def run_dim(base, dim, ks):
    want = base * 128 // dim
    n = fit_points(want, dim)
    x = torch.empty((n, dim), dtype=torch.float32, device="cuda")
    KM.generate(x, 0, blobs=64, seed=0x6B6D)
    t_plane, sp = clock(lambda: KM.split_points(x))
    assert sp is not None, "the plane does not fit"
    dst = torch.empty_like(sp.xh)
    t_copy = min(clock(lambda: dst.copy_(sp.xh))[0] for _ in range(4))
    del dst
    plane_gb = sp.xh.numel() * 2 / 1e9
    print(f"D = {dim}: n = {n}" + (f" (of {want}: HBM)" if n != want else "") +
          f", f32 rows {n * dim * 4 / 1e9:.1f} GB, plane [n, {sp.xh.shape[1]}] {plane_gb:.1f} GB written in "
          f"{t_plane:.1f} ms, copy_ of the plane {t_copy:.2f} ms ({2 * plane_gb / t_copy * 1e3:.0f} GB/s)", flush=True)
    for k in ks:
        c0 = x[:k].clone()
        ws = KM.KMeansWorkspace(n, k, x.device, dim=dim)
        first, steady, repeat, ref = [], [], [], []
        for rnd in range(4):
            restart(sp)
            t1, (s, cnt, _a) = clock(lambda: KM.step(x, c0, ws))
            c1 = KM.update(c0, s, cnt)
            t2, _ = clock(lambda: KM.step(x, c1, ws))
            t3, (_s, _c, a3) = clock(lambda: KM.step(x, c1, ws))
            t4, _ = clock(lambda: KM.step_reference(x[:REF_ROWS], c1))
            t4 *= n / min(n, REF_ROWS)
            if rnd == 0:                      # warm-up round; also the result check
                bad, tied, rows = mismatches(x, c1, a3)
                print(f"  K = {k}: {bad} of the first {rows} points off the f64 argmin outside the tied set "
                      f"({tied} tied)", flush=True)
                continue
            first.append(t1), steady.append(t2), repeat.append(t3), ref.append(t4)
        a = min(repeat)
        print(f"  K = {k}: first {span(first)}, steady {span(steady)}, repeat {span(repeat)}; movers' share: first "
              f"{min(first) - a:.2f} ms, steady {min(steady) - a:.2f} ms; repeat / copy_ {a / t_copy:.2f}; "
              f"reference {span(ref)} = {min(ref) / min(steady):.2f} x steady, {min(ref) / min(first):.2f} x first",
              flush=True)
        del ws
    del x, sp


def run_sanity(base, ks):
    """D = 128: the kernels of kmeans_dim.hip (raw entry point, same plane) against the existing path."""
    n = fit_points(base, 128)
    x = torch.empty((n, 128), dtype=torch.float32, device="cuda")
    KM.generate(x, 0, blobs=64, seed=0x6B6D)
    sp = KM.split_points(x)
    for k in ks:
        c = x[:k].clone()
        ws = KM.KMeansWorkspace(n, k, x.device)
        cws = torch.empty(int(_lib.lib().dr_kmeans_dim_centroid_workspace(k, 128)), dtype=torch.uint8, device="cuda")

        def new():
            sums, counts = sp.state_for(k)
            _lib.call("dr_kmeans_dim_step", ptr(sp.xh), ptr(sp.xnorm), ptr(x), c_u64(n), 128, ptr(c), k,
                      ptr(ws.cnorm), ptr(ws.assign), ptr(sp.prev), ptr(sums), ptr(counts), ptr(ws.near), ptr(cws),
                      stream_of(x))
            return sums

        def old():
            return KM.step(x, c, ws, planes=True)[0]

        res = {"new": [], "old": []}
        for rnd in range(4):
            for name, fn in (("new", new), ("old", old)) if rnd % 2 == 0 else (("old", old), ("new", new)):
                restart(sp)
                fn()                                  # first step: every row moves
                t, _ = clock(fn)                      # timed: nothing moves
                if rnd:
                    res[name].append(t)
                res[name + "_a"] = ws.assign[:n].clone()
        diff = int((res["new_a"] != res["old_a"]).sum())
        print(f"sanity D = 128, n = {n}, K = {k}: kmeans_dim.hip {span(res['new'])}, kmeans.hip {span(res['old'])} "
              f"(repeat steps; {diff} assignments differ between the two re-ranks)", flush=True)


def main():
    base = int(float(sys.argv[1])) if len(sys.argv) > 1 else 50_000_000
    dims = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [2, 16, 32, 64, 96, 256, 512]
    ks = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [16, 64, 256]
    print(f"{torch.cuda.get_device_name(0)}; base {base} points", flush=True)
    for dim in dims:
        run_dim(base, dim, ks)
    run_sanity(base, [k for k in ks if k >= 64])


if __name__ == "__main__":
    main()
