"""Device OrderBy / RangePartition over string keys (csrc/kernels/strsort.hip): the permutation of
sort_strings and the destinations of range_dest_strings against plain Python (exact, stable, so
compared with ==), and string-key OrderBy through the public API against the LocalDebug oracle."""
import bisect
import functools
import random

import pytest
import torch

import dryad_amd as D
from dryad_amd.ops.strsort import FIN_CORE, FIN_EXT, W, W0, range_dest_strings, sort_strings

pytestmark = pytest.mark.gpu

NS = [1, 2, 257, FIN_CORE + FIN_EXT + 1, 3 * FIN_CORE + 5]
RUN = FIN_CORE + FIN_EXT + 300


@functools.lru_cache(maxsize=None)
def _strings(shape, n):
    """Byte strings of one input shape.  short: lengths 0..24 over {0x00, 0x61, 0xFF} (ties, prefix
    pairs, embedded NULs, empty strings, the byte a signed compare gets wrong).  prefix: a shared
    40-byte prefix, then 0..12 random bytes (depth > 0; the finisher's heap walk past its 16 staged
    bytes).  equal11 / equal18: one string n times, its length a window edge (W0, W0 + W).
    longrun: RUN strings sharing 30 bytes before distinct 4-byte tails (more than one finisher
    window: refinement passes) among n unrelated strings, every other one sorting before the run,
    so the run starts near position n / 2 and crosses a core boundary for both n it is used with."""
    rng = random.Random(f"{shape}/{n}")
    if shape == "short":
        return tuple(bytes(rng.choice((0x00, 0x61, 0xFF)) for _ in range(rng.randint(0, 24))) for _ in range(n))
    if shape == "prefix":
        pre = bytes(rng.randrange(256) for _ in range(40))
        return tuple(pre + bytes(rng.randrange(256) for _ in range(rng.randint(0, 12))) for _ in range(n))
    if shape in ("equal11", "equal18"):
        assert (W0, W0 + W) == (11, 18)
        return (bytes(range(65, 65 + int(shape[5:]))),) * n
    run = [b"m" * 30 + t.to_bytes(4, "big") for t in rng.sample(range(1 << 32), RUN)]
    other = [(b"A" if i % 2 else b"z") + bytes(rng.randrange(256) for _ in range(rng.randint(0, 20))) for i in range(n)]
    both = run + other
    rng.shuffle(both)
    return tuple(both)


def _device(strs):
    ln = torch.tensor([len(b) for b in strs], dtype=torch.int64)
    blob = b"".join(strs)
    heap = torch.frombuffer(bytearray(blob), dtype=torch.uint8) if blob else torch.zeros(0, dtype=torch.uint8)
    return heap.cuda(), (torch.cumsum(ln, 0) - ln).cuda(), ln.cuda()


CASES = [(s, n) for s in ("short", "prefix", "equal11", "equal18") for n in NS] + [("longrun", n) for n in NS[-2:]]


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("shape,n", CASES)
def test_sort_strings_matches_python(shape, n, descending):
    b = _strings(shape, n)
    expect = sorted(range(len(b)), key=lambda i: b[i], reverse=descending)
    assert sort_strings(*_device(b), descending=descending).tolist() == expect


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("nsep", [1, 2, 255])
def test_range_dest_strings_matches_bisect(nsep, descending):
    b = _strings("short", NS[-1])
    rng = random.Random(nsep)
    draw = [b""] + [rng.choice(b) for _ in range(nsep - 1)]
    if nsep > 1:
        draw[-1] = draw[-2]                    # a duplicated separator, whatever the draw held
    seps = sorted(draw, reverse=descending)
    # the host RangePartition: bisect_left under the (negated, when descending) comparison
    kf = functools.cmp_to_key((lambda x, y: (x < y) - (x > y)) if descending else (lambda x, y: (x > y) - (x < y)))
    ks = [kf(s) for s in seps]
    expect = [bisect.bisect_left(ks, kf(x)) for x in b]
    assert range_dest_strings(*_device(b), *_device(seps), descending=descending).tolist() == expect


KEYS = ["é", "日本", "z", "", "a", "a\0", "ab", "Zebra", "zebra", "naïve", "日本語", "éclair"]
RECS = [(i, KEYS[(i * 7919) % len(KEYS)] + ("" if i % 3 else str(i % 40))) for i in range(20_000)]
LINES = [r[1] + str(r[0] % 7) for r in RECS[:5_000]]


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("parts", [1, 3])
def test_string_key_orderby_on_device(parts, descending):
    def field(c):
        q = c.FromEnumerable(RECS)
        return q.OrderByDescending(lambda t: t[1]) if descending else q.OrderBy(lambda t: t[1])

    def whole(c):
        q = c.FromEnumerable(LINES)
        return q.OrderByDescending(lambda s: s) if descending else q.OrderBy(lambda s: s)

    local = D.DryadLinqContext(1)
    local.LocalDebug = True
    for build in (field, whole):
        c = D.DryadLinqContext(platform="gpu")
        c.PartitionCount = parts
        assert list(build(c)) == list(build(local))
        fb = c._get_executor().last_result["fallbacks"]
        assert not {"sort", "sample", "separators", "range_partition"} & {op for _, op, _ in fb}, fb
