"""GroupBy over string and composite keys of one partition: the tag-and-verify hash aggregation
(ops/keyhash.key_aggregate; csrc/kernels/keyhash.hip) against the sort branch of
gpu/ops.op_group_partial (Rabin fingerprints of the string parts, _group_keys, seg_reduce_multi),
both followed by _key_outputs, with Count + Sum + Min + Max over int64:

    python tools/micro/keyhash_bw.py [string rows] [composite rows] [job rows]

Built in HBM from a seed, no files: ``gen://names``-shaped string keys ("u" + decimal, string rows
default 1e8) with 1e3, 1e5, 2e6 and 5e6 distinct names (the last past the capacity cap: the cost of
the sample that declines), and an (int64, int32) key (composite rows default 1e9) with 1e3 and
1e6 distinct pairs.  The two paths are called alternately in one process: min and max of 3 timed
calls each after a warm-up, host clock around a call that ends in a device synchronise.  The two
results are compared as dictionaries (every key stands for the id it was rendered from: sorted by
it, the aggregates must be equal).  Then the job step of FromStore("gen://names...").GroupBy(r =>
r.Name, ...) over job rows (default 1e8) with GroupByKeyHash on and off, two runs each,
alternating."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

import dryad_amd as D  # noqa: E402
from dryad_amd.gpu import ops as O  # noqa: E402
from dryad_amd.gpu import trace as TR  # noqa: E402
from dryad_amd.models import names as NM  # noqa: E402
from dryad_amd.ops import keyhash as KH  # noqa: E402
from dryad_amd.ops import relational as R  # noqa: E402

DEV = "cuda"
I64 = torch.int64


def call_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def sort_path(kcols, skeys, specs):
    kcols = TR.fingerprint_strings(kcols, skeys)
    srt, seg, nseg, rows_at_start, starts = O._group_keys(kcols, skeys)
    out, _ = O._key_outputs(kcols, skeys, rows_at_start, srt, starts)
    return rows_at_start, R.seg_reduce_multi(srt, seg, nseg, specs), out


def hash_path(kcols, skeys, specs, n):
    parts = [c if sk is None else (sk.heap, sk.off, sk.len) for c, sk in zip(kcols, skeys)]
    got = KH.key_aggregate(parts, specs, n)
    if got is None:
        return None
    return got[0], got[1], O._key_outputs(kcols, skeys, got[0])[0]


def as_dict(ids, res):
    """(the groups' ids ascending, their aggregates in that order)"""
    k, order = torch.sort(ids.index_select(0, res[0]))
    return [k] + [a.index_select(0, order) for a in res[1]]


def measure(name, ids, kcols, skeys):
    n = ids.shape[0]
    gen = torch.Generator(device=DEV).manual_seed(11)
    v = [torch.randint(-10**6, 10**6, (n,), device=DEV, generator=gen) for _ in range(3)]
    specs = [("count", None, I64), ("sum", v[0], I64), ("min", v[1], I64), ("max", v[2], I64)]
    ms, out = {"sort": [], "hash": []}, {}
    for rep in range(4):                              # rep 0 warms both up
        for k in ms:
            t, r = call_ms((lambda: sort_path(kcols, skeys, specs)) if k == "sort" else
                           (lambda: hash_path(kcols, skeys, specs, n)))
            if rep == 3:
                out[k] = None if r is None else as_dict(ids, r)
            if k == "hash":
                st = dict(KH.stats)
            del r
            if rep:
                ms[k].append(t)
    s, h = ms["sort"], ms["hash"]
    if out["hash"] is None:
        verdict = "hash path declined"
    else:
        assert all(torch.equal(a, b) for a, b in zip(out["sort"], out["hash"])), f"{name}: the two results differ"
        verdict = "results equal"
    print(f"{name}: n = {n}, {out['sort'][0].numel()} groups: sort {min(s):.2f} .. {max(s):.2f} ms; "
          f"hash {min(h):.2f} .. {max(h):.2f} ms (path {st['path']}, capacity {st['capacity']}, flushes "
          f"{st['flushes']}, overflow {st['overflow']}); sort / hash {min(s) / min(h):.2f}x; {verdict}", flush=True)


def job(rows, keys):
    src = f"gen://names?count={rows}&partitions=1&keys={keys}&seed=9"
    ctxs = {}
    for mode in ("off", "on"):
        ctxs[mode] = D.DryadLinqContext(platform="gpu")
        ctxs[mode].GroupByKeyHash = mode
    ms, got, path = {"off": [], "on": []}, {}, {}
    for rep in range(3):                              # rep 0 warms both up
        for mode, c in ctxs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got[mode] = sorted(c.FromStore(src).GroupBy(lambda r: r[0], lambda k, g: (
                k, g.Count(), g.Sum(lambda r: r[1]), g.Min(lambda r: r[2]), g.Max(lambda r: r[1]))))
            t = (time.perf_counter() - t0) * 1e3
            path[mode] = c._get_executor().last_result["group_path"]
            if rep:
                ms[mode].append(t)
    assert got["off"] == got["on"], "job: the two results differ"
    print(f"job gen://names {rows} rows, {keys} names: off ({path['off']}) {min(ms['off']):.1f} .. {max(ms['off']):.1f} ms; "
          f"on ({path['on']}) {min(ms['on']):.1f} .. {max(ms['on']):.1f} ms; results equal", flush=True)


def main():
    arg = [int(float(a)) for a in sys.argv[1:]] + [None] * 3
    ns, nc, nj = arg[0] or 100_000_000, arg[1] or 1_000_000_000, arg[2] or 100_000_000
    gen = torch.Generator(device=DEV).manual_seed(7)
    for d in (1_000, 100_000, 2_000_000, 5_000_000):
        ids = torch.randint(0, d, (ns,), device=DEV, generator=gen)
        sk = TR.StrCol(*NM.render(ids * 7919))
        measure(f"names {d}", ids, [None], [sk])
        del ids, sk
    for d in (1_000, 1_000_000):
        ids = torch.randint(0, d, (nc,), device=DEV, generator=gen)
        measure(f"(int64, int32) {d}", ids, [ids * 10**9 - 5 * 10**14, (ids % 1000).to(torch.int32)], [None, None])
        del ids
    job(nj, 1000)


if __name__ == "__main__":
    main()
