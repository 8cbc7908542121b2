"""GroupBy / Distinct over string and composite keys through LDS hash tables
(csrc/kernels/keyhash.hip): key_aggregate against a Python dictionary over the same rows (int64
and f64 values that are small integers, so every comparison is equality), and GroupBy / Distinct
queries through the public API against the LocalDebug oracle with GroupByKeyHash on."""
import random

import numpy as np
import pytest
import torch

import dryad_amd as D
from dryad_amd.ops.keyhash import STEP_ROWS, key_aggregate, lds_slots, stats

pytestmark = pytest.mark.gpu

I64, F64 = torch.int64, torch.float64
COUNT = [("count", None)]
ALL8 = [("count", None), ("sum", 0), ("min", 0), ("max", 1), ("sum", 2), ("min", 2), ("max", 3), ("sum", 1)]
FOLD = {"count": lambda a, v: a + 1, "sum": lambda a, v: a + v, "min": min, "max": max}


def _str_part(words):
    """(heap, off, len) on the device: each distinct word stored once, in shuffled order, the
    last one ending at the heap's last byte."""
    uniq = sorted(set(words))
    random.Random(len(uniq)).shuffle(uniq)
    off, heap = {}, b""
    for w in uniq:
        off[w] = len(heap)
        heap += w
    return (torch.tensor(list(heap), dtype=torch.uint8).cuda(), torch.tensor([off[w] for w in words]).cuda(),
            torch.tensor([len(w) for w in words]).cuda())


def _check(keys, dtypes, names, **kw):
    """key_aggregate over the rows ``keys`` (tuples; dtypes[c] None: a string part) and four seeded
    value columns against {key: [first row, aggregates]} built row by row."""
    n = len(keys)
    rng = np.random.default_rng(n)
    cols = [rng.integers(-1000, 1000, n) for _ in range(2)] + [rng.integers(-1000, 1000, n).astype(np.float64)
                                                               for _ in range(2)]
    expect = {}
    for i, k in enumerate(keys):
        acc = expect.setdefault(k, [i] + [0 if op in ("count", "sum") else cols[c][i].item() for op, c in names])
        acc[1:] = [FOLD[op](a, None if c is None else cols[c][i].item()) for a, (op, c) in zip(acc[1:], names)]
    parts = [_str_part([k[c] for k in keys]) if dt is None else torch.tensor([k[c] for k in keys], dtype=dt).cuda()
             for c, dt in enumerate(dtypes)]
    dev = [torch.from_numpy(c).cuda() for c in cols]
    specs = [(op, None if c is None else dev[c], I64 if c is None or c < 2 else F64) for op, c in names]
    first, outs = key_aggregate(parts, specs, n, **kw)
    assert first.tolist() == sorted(first.tolist())
    assert [o.dtype for o in outs] == [s[2] for s in specs]
    got = {keys[r]: [r, *vals] for r, *vals in zip(first.tolist(), *[o.tolist() for o in outs])}
    assert got == expect


@pytest.mark.parametrize("names", [COUNT, ALL8], ids=["count", "all8"])
@pytest.mark.parametrize("d", ["1", "slots-1", "slots+1", "4*slots"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, "grid+1", "keys+257"])
def test_key_aggregate_matches_dictionary(n, d, names):
    slots = lds_slots(len(names))
    d = {"1": 1, "slots-1": slots - 1, "slots+1": slots + 1, "4*slots": 4 * slots}[d]
    grid = {"grid+1": 2, "keys+257": 1}.get(n)         # one row past a full step of two workgroups; or
    n = {"grid+1": 2 * STEP_ROWS + 1, "keys+257": d + 257}.get(n, n)   # every key once in one workgroup, then again
    ids = list(range(d)) + np.random.default_rng(d).integers(0, d, 257).tolist()
    _check([(j * 10**12 - 5 * 10**13, j % 7) for j in ids[:n]], [I64, torch.int32], names, grid=grid)


LENGTHS = [0, 1, 7, 8, 9, 16, 17, 40]
SHAPES = {
    "lengths": ([(bytes([65 + j]) * LENGTHS[j % 8],) for j in range(40)], [None]),
    "prefix16": ([(b"0123456789abcdef" + bytes([j]),) for j in range(40)], [None]),
    "prefix-of": ([((b"abcdefghi" * 5)[:j],) for j in range(40)], [None]),
    "int64-int32": ([(j // 3 * 10**12, j % 3 - 1) for j in range(40)], [I64, torch.int32]),
    "int8-string": ([(j % 5 - 2, b"w%d" % (j // 5)) for j in range(40)], [torch.int8, None]),
    "string-string": ([(b"ab", b"c"), (b"a", b"bc"), (b"", b"abc"), (b"abc", b"")] +
                      [(b"s%d" % (j % 6), b"long suffix %d" % (j // 6)) for j in range(36)], [None, None]),
    "four": ([(j % 2 * -2**62, b"name%d" % (j % 5), j % 3 - 1, j % 4 == 0) for j in range(40)],
             [I64, None, torch.int16, torch.bool]),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_key_shapes(shape):
    pool, dtypes = SHAPES[shape]
    ids = list(range(len(pool))) + np.random.default_rng(3).integers(0, len(pool), 257 - len(pool)).tolist()
    random.Random(5).shuffle(ids)
    _check([pool[j] for j in ids], dtypes, ALL8)


def test_forced_paths():
    pool = [(j * 10**12, j % 3) for j in range(2000)]
    two = [I64, torch.int32]
    rows40 = [pool[j % 40] for j in range(257)]
    parts = [torch.tensor([k[c] for k in rows40], dtype=dt).cuda() for c, dt in enumerate(two)]
    count = [("count", None, I64)]
    assert key_aggregate(parts, count, 257, tag_bits=4) is None and stats["collision"]      # 40 keys, 16 tags
    p2000 = [torch.tensor([k[c] for k in pool], dtype=dt).cuda() for c, dt in enumerate(two)]
    assert key_aggregate(p2000, count, 2000, capacity=1024) is None and stats["overflow"]
    _check([pool[j % 40] for j in range(1025)], two, ALL8, flush_rows=64, grid=1)
    assert stats["flushes"] > 4
    assert key_aggregate([parts[0], parts[1].to(torch.float32)], count, 257) is None
    assert key_aggregate(parts, count * 9, 257) is None


SRC = "gen://names?count=200000&partitions=1&keys=1000&seed=9"
RESULT = lambda k, g: (k, g.Count(), g.Sum(lambda r: r[1]), g.Min(lambda r: r[2]), g.Max(lambda r: r[1]))  # noqa: E731
FLAT = lambda k, g: (k[0], k[1], g.Count(), g.Sum(lambda r: r[1]), g.Min(lambda r: r[2]))  # noqa: E731
QUERIES = {"string": lambda t: t.GroupBy(lambda r: r[0], RESULT),
           "composite": lambda t: t.GroupBy(lambda r: (r[0], r[1] % 7), RESULT),
           "composite-flat": lambda t: t.GroupBy(lambda r: (r[0], r[1] % 7), FLAT),
           "distinct": lambda t: t.Select(lambda r: (r[0], r[1] % 3)).Distinct()}


@pytest.mark.parametrize("kind", list(QUERIES))
def test_queries_run_the_keyhash_path(kind):
    """"composite" hands the tuple key back as one field of the result (records with a tuple-valued
    field: gpu/ops._nested_records); "composite-flat" hands its parts back as fields of their own."""
    gpu, local = D.DryadLinqContext(platform="gpu"), D.DryadLinqContext(1)
    gpu.GroupByKeyHash = "on"
    local.LocalDebug = True
    got, expect = (sorted(QUERIES[kind](c.FromStore(SRC))) for c in (gpu, local))
    assert got == expect
    res = gpu._get_executor().last_result
    assert res["fallbacks"] == []
    if kind != "distinct":
        assert res["group_path"] == "keyhash"
