"""OrderBy(...).Take(k) as a radix select against sort + slice (ops/topk.topk_entries,
csrc/kernels/topk.hip):

    python tools/micro/topk_bw.py [entries]

``entries`` (default 1e9) int64 keys in three distributions: uniform 64-bit, uniform in [0, 1000)
(heavy ties, shared high bits) and all equal.  Per distribution the stable sort of all entries
(S.sort_entries_hybrid, the path OrderBy + Take takes without the select) and the gather of all
rows that path also pays; per k in {10, 1e4, 1e6, n / 8} ``topk_entries`` and the k-row gather.
Min and max of 3 timed calls after a warm-up, host clock around work that ends in a device
synchronise; the entries are rebuilt (untimed) before every sort, which reorders them in place.
GB/s is entry bytes read by the select kernels (its ``stats``) over the call's time, and its
ratio to this device's ``copy_`` rate measured in the same process.  A last section times both
paths at small n for k = 10 (the TopKMinRows crossover)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

from dryad_amd.ops import relational as R  # noqa: E402
from dryad_amd.ops import sort as S  # noqa: E402
from dryad_amd.ops import topk as TK  # noqa: E402


def keys(dist, n, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if dist == "uniform64":
        top = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int64, device="cuda", generator=g)
        top <<= 32
        top |= torch.randint(0, 1 << 32, (n,), dtype=torch.int64, device="cuda", generator=g)
        return top
    if dist == "uniform1000":
        return torch.randint(0, 1000, (n,), dtype=torch.int64, device="cuda", generator=g)
    return torch.full((n,), 7, dtype=torch.int64, device="cuda")


def timed(fn, setup=None, reps=3):
    """(min, max) ms of ``reps`` calls after one warm-up call."""
    ts = []
    for i in range(reps + 1):
        arg = setup() if setup is not None else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn(arg) if setup is not None else fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        del r, arg
    return min(ts[1:]), max(ts[1:])


def perm_of(e):
    return (e[:, 0] & 0xFFFFFFFF).contiguous()


def copy_rate(n):
    a = torch.empty(n, dtype=torch.int64, device="cuda").fill_(7)
    b = torch.empty_like(a)
    lo, _ = timed(lambda: b.copy_(a), reps=5)
    return 2 * 8 * n / lo / 1e6          # GB/s, read + write


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000_000
    rate = copy_rate(n)
    print(f"copy_ of {n} int64 (read + write): {rate:.0f} GB/s", flush=True)
    for dist in ("uniform64", "uniform1000", "equal"):
        col = keys(dist, n)
        build = lambda: R.build_keys([col])[0]                        # noqa: E731
        e, b0, _ = R.build_keys([col])
        s_lo, s_hi = timed(lambda x: S.sort_entries_hybrid(x, b0), setup=build)
        srt = S.sort_entries_hybrid(build(), b0)
        perm = perm_of(srt)
        g_lo, g_hi = timed(lambda: col.index_select(0, perm))
        print(f"{dist}: n = {n}: sort_entries_hybrid {s_lo:.2f} .. {s_hi:.2f} ms; gather of all rows (8-byte) "
              f"{g_lo:.2f} .. {g_hi:.2f} ms", flush=True)
        for k in (10, 10_000, 1_000_000, n // 8):
            k = min(k, n)
            t_lo, t_hi = timed(lambda: TK.topk_entries(e, k, b0))
            st = dict(TK.stats)
            out = TK.topk_entries(e, k, b0)
            assert torch.equal(out, srt[:k]), "select != sort + slice"
            kp = perm_of(out)
            kg_lo, _ = timed(lambda: col.index_select(0, kp))
            gbs = st["bytes_read"] / t_lo / 1e6
            print(f"{dist}: k = {k}: topk_entries {t_lo:.2f} .. {t_hi:.2f} ms (+ k-row gather {kg_lo:.2f} ms) = "
                  f"{gbs:.0f} GB/s of {st['bytes_read'] / 1e9:.2f} GB entry bytes read, {gbs / rate:.2f} x copy_; "
                  f"levels {st['levels']}, histogram passes {st['hist_passes']}, candidates {st['candidates']}; "
                  f"sort + slice + k-row gather {s_lo + kg_lo:.2f} ms ({(s_lo + kg_lo) / (t_lo + kg_lo):.1f}x), "
                  f"with the gather of all rows {s_lo + g_lo:.2f} ms", flush=True)
            del out, kp
        del col, e, srt, perm
    for m in (1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20, 1 << 22, 1 << 24):
        col = keys("uniform64", m)
        e, b0, _ = R.build_keys([col])
        t_lo, _ = timed(lambda: TK.topk_entries(e, 10, b0), reps=5)
        f_lo, _ = timed(lambda: TK.topk_entries(e, m // 8, b0), reps=5)
        s_lo, _ = timed(lambda x: S.sort_entries_hybrid(x, b0)[:10], setup=lambda: R.build_keys([col])[0], reps=5)
        print(f"crossover: uniform64 n = {m}: topk_entries k = 10 {t_lo:.3f} ms, k = n / 8 {f_lo:.3f} ms; "
              f"sort + slice {s_lo:.3f} ms", flush=True)


if __name__ == "__main__":
    main()
