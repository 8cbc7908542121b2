"""OrderBy(...).Take(k) as a radix select (csrc/kernels/topk.hip): topk_entries against plain
Python over the entries read back (exact, so compared with ==), and the query through the public
API against the LocalDebug oracle, where the select serves it and where it declines."""
import functools

import pytest
import torch

import dryad_amd as D
from dryad_amd.ops import relational as R
from dryad_amd.ops.topk import GRID, TILE, topk_entries

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
NS = [1, 2, 2049, TILE * GRID + 1]
SHAPES = ["uniform64", "small", "equal", "lo96", "uniform64-desc", "small-desc"]


@functools.lru_cache(maxsize=None)
def _case(shape, n):
    """(entries, begin_bit, the entries as unsigned (hi, lo) tuples in sorted order).  uniform64:
    random int64 (sign flip, two-pass flow).  small: [0, 7) (shared high bits, ties across the k
    boundary).  equal: one value (the descent runs in the row-index bits).  lo96: a constant int64
    then an int32 in [-1000, 1000) (deciding bits in ``lo``, every ``hi`` level degenerate)."""
    g = torch.Generator(device="cuda").manual_seed(n)
    kind, desc = shape.partition("-")[0], shape.endswith("-desc")
    if kind == "uniform64":
        top = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int64, device="cuda", generator=g)
        cols = [(top << 32) | torch.randint(0, 1 << 32, (n,), dtype=torch.int64, device="cuda", generator=g)]
    elif kind == "small":
        cols = [torch.randint(0, 7, (n,), dtype=torch.int64, device="cuda", generator=g)]
    elif kind == "equal":
        cols = [torch.full((n,), -42, dtype=torch.int64, device="cuda")]
    else:
        cols = [torch.full((n,), 1 << 40, dtype=torch.int64, device="cuda"),
                torch.randint(-1000, 1000, (n,), dtype=torch.int32, device="cuda", generator=g)]
    e, begin_bit, _ = R.build_keys(cols, [desc] * len(cols))
    return e, begin_bit, sorted((hi & M64, lo & M64) for lo, hi in e.tolist())


@pytest.mark.parametrize("k_of", [lambda n: 0, lambda n: 1, lambda n: n // 2, lambda n: n - 1, lambda n: n],
                         ids=["0", "1", "half", "n-1", "n"])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("shape", SHAPES)
def test_topk_entries_matches_python(shape, n, k_of):
    e, begin_bit, expect = _case(shape, n)
    k = min(max(k_of(n), 0), n)
    got = [(hi & M64, lo & M64) for lo, hi in topk_entries(e, k, begin_bit).tolist()]
    assert got == expect[:k]


RECS = [((i * 7919) % 50, ((i * 104729) % 97) / 4.0, "k%02d" % ((i * 31) % 23)) for i in range(5000)]


def _run(build, recs):
    local = D.DryadLinqContext(1)
    local.LocalDebug = True
    c = D.DryadLinqContext(platform="gpu")
    c.TopKMinRows = 0
    c.PartitionCount = 1
    got, expect = list(build(c.FromEnumerable(recs))), list(build(local.FromEnumerable(recs)))
    return got, expect, c._get_executor().last_result


@pytest.mark.parametrize("build", [lambda q: q.OrderBy(lambda r: r[0]).Take(17),
                                   lambda q: q.OrderByDescending(lambda r: r[1]).Take(17)], ids=["asc-int", "desc-float"])
def test_orderby_take_runs_the_select(build):
    got, expect, res = _run(build, [r[:2] for r in RECS])
    assert got == expect
    assert res["sort_path"] == "topk"
    assert res["fallbacks"] == []


@pytest.mark.parametrize("build,recs", [(lambda q: q.OrderBy(lambda r: r[2]).Take(5), RECS),
                                        (lambda q: q.OrderBy(lambda r: r[0]).Take(len(RECS) + 3), [r[:2] for r in RECS])],
                         ids=["string-key", "k>n"])
def test_declined_select_stays_correct(build, recs):
    got, expect, res = _run(build, recs)
    assert got == expect
    assert res["sort_path"] != "topk"
