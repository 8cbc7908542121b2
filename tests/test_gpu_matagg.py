"""Low-cardinality GroupBy on the matrix cores (csrc/kernels/matagg.hip): matrix_aggregate against
plain torch on int64 (bincount / index_add_ / scatter_reduce over torch.unique's inverse, on the
host), exact, compared after sorting by key; and the GroupBy query through the public API against
the LocalDebug oracle with GroupByMatrix on."""
import functools

import pytest
import torch

import dryad_amd as D
from dryad_amd.ops.matagg import grid_rows, matrix_aggregate

pytestmark = pytest.mark.gpu

I64 = torch.int64
LO, HI = -(1 << 63), (1 << 63) - 1
NS = [1, 63, 64, 65, 4097, "grid+1"]
SPECS = {"count": ["count"], "count+sum": ["count", "sum0"],
         "all": ["sum0", "sum1", "count", "sum2", "min0", "max1"]}


@functools.lru_cache(maxsize=None)
def _case(n, d, shape, absent=0):
    """(key, dictionary, three value columns) on the device.  Keys are sparse and signed, one of
    them INT64_MIN; the last ``absent`` keys of the data (about 1 % of the rows each) are left out
    of the dictionary.  small: 0..100.  full64: any int64, so sums wrap.  edge: the values around
    the limb bias and the sign limb."""
    g = torch.Generator().manual_seed(1000 * n + d)
    keys = torch.arange(d, dtype=I64) * 10**12 - 5 * 10**13
    keys[d // 2] = LO
    ids = torch.randint(0, d - absent, (n,), generator=g)
    if absent:
        rare = torch.randint(d - absent, d, (n,), generator=g)
        ids = torch.where(torch.rand(n, generator=g) < 0.01 * absent, rare, ids)
    if shape == "small":
        vals = [torch.randint(0, 101, (n,), generator=g) for _ in range(3)]
    elif shape == "full64":
        vals = [torch.randint(LO, HI, (n,), generator=g) for _ in range(3)]
    else:
        pool = torch.tensor([LO, HI, -1, 0, 255, 256], dtype=I64)
        vals = [pool[torch.randint(0, 6, (n,), generator=g)] for _ in range(3)]
    return keys[ids].cuda(), keys[:d - absent].cuda(), [v.cuda() for v in vals]


def _check(key, vals, names, run):
    specs = [(s.rstrip("012"), vals[int(s[-1])] if s != "count" else None, I64) for s in names]
    got = run(specs)
    uniq, inv = torch.unique(key.cpu(), return_inverse=True)
    order = torch.argsort(got[0])
    assert torch.equal(got[0][order].cpu(), uniq)
    for (op, v, _), res in zip(specs, got[1]):
        if op == "count":
            exp = torch.bincount(inv, minlength=uniq.numel())
        elif op == "sum":
            exp = torch.zeros(uniq.numel(), dtype=I64).index_add_(0, inv, v.cpu())
        else:
            exp = torch.full((uniq.numel(),), HI if op == "min" else LO, dtype=I64).scatter_reduce(
                0, inv, v.cpu(), "amin" if op == "min" else "amax")
        assert res.dtype == I64 and torch.equal(res[order].cpu(), exp), op


@pytest.mark.parametrize("names", list(SPECS.values()), ids=list(SPECS))
@pytest.mark.parametrize("shape", ["small", "full64", "edge"])
@pytest.mark.parametrize("d", [1, 15, 16, 17, 256])
@pytest.mark.parametrize("n", NS)
def test_matrix_aggregate_matches_torch(n, d, shape, names):
    grid = 2 if n == "grid+1" else None            # one row more than a full step of every wave
    key, dk, vals = _case(grid_rows(2) + 1 if grid else n, d, shape)
    _check(key, vals, names, lambda specs: matrix_aggregate(key, specs, dict_keys=dk, grid=grid))


@pytest.mark.parametrize("shape", ["edge", "small"])
def test_forced_flush_every_chunk(shape):
    key, dk, vals = _case(4097, 17, shape)
    _check(key, vals, SPECS["all"], lambda specs: matrix_aggregate(key, specs, dict_keys=dk, flush_rows=64, grid=1))


def test_accumulator_bound_at_default_flush():
    """One workgroup, one key, every value 0: each low limb is -128, so a wave's accumulators reach
    -2^31 exactly at the default flush_rows of 2^24."""
    n = 4 * ((1 << 24) + 64)
    key = torch.full((n,), 5, dtype=I64, device="cuda")
    keys, (cnt, tot) = matrix_aggregate(key, [("count", None, I64), ("sum", torch.zeros_like(key), I64)],
                                        dict_keys=key[:1], grid=1)
    assert keys.tolist() == [5] and cnt.tolist() == [n] and tot.tolist() == [0]


def test_rows_outside_the_dictionary():
    key, dk, vals = _case(20000, 20, "full64", absent=3)
    assert dk.numel() == 17 and torch.unique(key).numel() == 20
    _check(key, vals, SPECS["all"], lambda specs: matrix_aggregate(key, specs, dict_keys=dk))
    key, dk, vals = _case(4097, 8, "small")
    assert matrix_aggregate(key, [("count", None, I64)], dict_keys=dk[:1]) is None     # the miss list overflows


def test_declines():
    key, dk, vals = _case(4097, 17, "small")
    assert matrix_aggregate(key, [("sum", vals[0], torch.float64)], dict_keys=dk) is None
    assert matrix_aggregate(key, [("count", None, I64)], dict_keys=torch.arange(257, device="cuda")) is None


RESULTS = {"int": lambda k, g: (k, g.Count(), g.Sum(lambda r: r[1]), g.Min(lambda r: r[2]), g.Max(lambda r: r[3])),
           "with-average": lambda k, g: (k, g.Count(), g.Sum(lambda r: r[1]), g.Min(lambda r: r[2]),
                                         g.Max(lambda r: r[3]), g.Average(lambda r: r[1]))}


@pytest.mark.parametrize("kind", list(RESULTS))
def test_group_by_query_runs_the_matrix_path(kind):
    src = "gen://records64?count=200000&partitions=1&keys=64&seed=9"
    gpu, local = D.DryadLinqContext(platform="gpu"), D.DryadLinqContext(1)
    gpu.GroupByMatrix = "on"
    local.LocalDebug = True
    got, expect = (sorted(c.FromStore(src).GroupBy(lambda r: r[0], RESULTS[kind])) for c in (gpu, local))
    assert got == expect
    res = gpu._get_executor().last_result
    if kind == "int":
        assert res["group_path"] == "matrix" and res["fallbacks"] == []
    else:
        assert res["group_path"] != "matrix"
