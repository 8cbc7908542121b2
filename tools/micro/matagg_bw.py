"""Low-cardinality GroupBy: the int8 matrix-core aggregation against the LDS hash tables
(ops/matagg.matrix_aggregate, csrc/kernels/matagg.hip; ops/relational.hash_aggregate):

    python tools/micro/matagg_bw.py [rows]

``rows`` (default 1e9) int64 keys uniform in [0, K) for K = 16, 64, 256 with three random int64
value columns; the aggregates are Count + Sum + Min + Max as in benchmarks/groupby.py.  The two
paths are called alternately in one process: min and max of 3 timed calls each after a warm-up,
host clock around a call that ends in a device synchronise (both calls include their sampling of
the keys and their result extraction).  The results are compared (exact) at that size.  GB/s is
the 32 bytes per row both paths read over the call's time."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

from dryad_amd.ops import matagg as MA  # noqa: E402
from dryad_amd.ops import relational as R  # noqa: E402


def call_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def by_key(got):
    order = torch.argsort(got[0])
    return [got[0][order]] + [c[order] for c in got[1]]


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000_000
    g = torch.Generator(device="cuda").manual_seed(7)
    vals = [torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device="cuda", generator=g) for _ in range(3)]
    specs = [("count", None, torch.int64), ("sum", vals[0], torch.int64), ("min", vals[1], torch.int64),
             ("max", vals[2], torch.int64)]
    for K in (16, 64, 256):
        key = torch.randint(0, K, (n,), dtype=torch.int64, device="cuda", generator=g)
        paths = {"matrix": lambda: MA.matrix_aggregate(key, specs), "hash": lambda: R.hash_aggregate(key, specs)}
        ms, out = {p: [] for p in paths}, {}
        for rep in range(4):                           # rep 0 warms both up
            for p, fn in paths.items():
                t, out[p] = call_ms(fn)
                if rep:
                    ms[p].append(t)
        assert out["matrix"] is not None and out["hash"] is not None
        same = all(torch.equal(a, b) for a, b in zip(by_key(out["matrix"]), by_key(out["hash"])))
        assert same, f"K = {K}: matrix_aggregate != hash_aggregate"
        m, h = ms["matrix"], ms["hash"]
        print(f"K = {K}: n = {n}: matrix_aggregate {min(m):.2f} .. {max(m):.2f} ms ({32 * n / min(m) / 1e6:.0f} GB/s); "
              f"hash_aggregate {min(h):.2f} .. {max(h):.2f} ms ({32 * n / min(h) / 1e6:.0f} GB/s); "
              f"hash / matrix {min(h) / min(m):.2f}x; outputs equal ({out['hash'][0].numel()} groups)", flush=True)
        del key, out


if __name__ == "__main__":
    main()
