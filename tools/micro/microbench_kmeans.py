"""Time one k-means step (MFMA kernel) vs the torch (hipBLASLt GEMM + argmin + index_add) path."""
import json
import sys
import time

import os
sys_path = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, sys_path)

import torch  # noqa: E402

from dryad_amd.ops import kmeans as KM  # noqa: E402


def timeit(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    timeit.spread = (max(ts) - min(ts)) * 1e3   # run-to-run noise of the last measurement
    return min(ts) * 1e3


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 50_000_000
    x = torch.empty((n, KM.DIM), dtype=torch.float32, device="cuda")
    blobs = int(sys.argv[3]) if len(sys.argv) > 3 else 64   # >= max K: one centroid per blob (no near ties)
    KM.generate(x, 0, blobs, 1)
    res = {"n": n, "blobs": blobs}
    ks = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [16, 64, 128, 256, 1024]
    for k in ks:
        c = x[:k].clone()
        ws = KM.KMeansWorkspace(n, k, x.device)
        gb = n * KM.DIM * 4 / 1e9
        for tag, pl in (("planes", None if k <= KM.PLANES_DEFAULT_MAX_K else True), ("f32", False)) if k <= KM.PLANES_MAX_K else (("mfma", False),):
            if tag == "planes":
                t0 = time.perf_counter()
                KM.split_points(x)
                torch.cuda.synchronize()
                res["split ms (once)"] = round((time.perf_counter() - t0) * 1e3, 3)
            if tag == "planes":
                # the first step over a table moves every point into the kept sums (one-off): warm
                # the kernels up, restart the table's state, time one step
                KM.step(x, c, ws, planes=pl)
                KM.split_points(x).sums = None
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                KM.step(x, c, ws, planes=pl)
                torch.cuda.synchronize()
                res[f"planes k={k} first step ms"] = round((time.perf_counter() - t0) * 1e3, 3)
                res[f"planes k={k} near-tie re-ranks"] = int(ws.near[:4].view(torch.int32)[0])
            ms = timeit(lambda: KM.step(x, c, ws, planes=pl))
            res[f"{tag} k={k} ms"] = round(ms, 3)
            res[f"{tag} k={k} spread ms"] = round(timeit.spread, 3)
            res[f"{tag} k={k} GB/s"] = round(gb / ms * 1e3, 1)
            res[f"{tag} k={k} TFLOP/s"] = round(2 * n * k * KM.DIM / ms / 1e9, 1)
        if n <= 20_000_000 and os.environ.get("KM_TORCH") == "1":
            res[f"torch k={k} ms"] = round(timeit(lambda: KM.step_reference(x, c), 2), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
