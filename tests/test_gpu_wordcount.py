"""The fused tokenise-and-count kernels (ops/wordcount.py, csrc/kernels/wordcount.hip) against
collections.Counter over re.split, and the first index of each word."""
import re
from collections import Counter

import pytest
import torch

from dryad_amd.ops import text as TX
from dryad_amd.ops import tuning
from dryad_amd.ops import wordcount as WC
from dryad_amd.ops.wordcount import LDS_SLOTS, MIN_SPAN, TILE

pytestmark = pytest.mark.gpu


def _heap(s: bytes):
    return torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda() if s else torch.zeros(0, dtype=torch.uint8, device="cuda")


def _reference(text: bytes):
    first = {}
    for m in re.finditer(rb"[^ \t\r\n]+", text):
        first.setdefault(m.group(), m.start())
    return Counter(t for t in re.split(rb"[ \t\r\n]+", text) if t), first


def _words(k):
    return [b"%05x" % (i * 2654435761 % (1 << 20)) for i in range(k)]


def _corpus(tmp_path_factory, lines, vocab):
    from dryad_amd.models.wordcount import synthetic_corpus
    p = synthetic_corpus(str(tmp_path_factory.mktemp("wc") / "c.txt"), lines, vocab=vocab)
    return p, open(p, "rb").read()


LONG = bytes(range(33, 127)) * ((3 * TILE + 7) // 94 + 1)
FLUSH = (b" ".join(_words(3 * LDS_SLOTS)) + b" ") * 3          # one workgroup's span, flushed mid-span
assert len(FLUSH) < MIN_SPAN
CASES = {
    "empty": b"", "spaces": b" \t\r\n", "x": b"x", "x y": b"x y", "bytes": b"a\x0bb \x00 \xc3\xa9 a\x0bb",
    **{f"phase{s}": b" " * s + b"ab " * (2 * TILE // 3 + 5) for s in range(18)},
    **{f"cut{d:+d}": (b"ab " * TILE)[:TILE + d] for d in (-1, 0, 1)},
    "long": b"a bb " + LONG[:3 * TILE + 7] + b" c\n" + LONG[:3 * TILE + 7] + b" bb",
    "longer": LONG[:5] + b" " + (LONG * 3)[:(1 << 16) + 5] + b"\t" + (LONG * 3)[:(1 << 16) + 5],   # past the 16-bit length
    "one word": b"word " * 1_000_000,
    "flush": FLUSH,
}


@pytest.mark.parametrize("name", list(CASES) + ["corpus"])
def test_count_words_matches_counter(name, tmp_path_factory):
    text = CASES[name] if name in CASES else _corpus(tmp_path_factory, 20000, 3000)[1]
    exp, first = _reference(text)
    got = WC.count_words(_heap(text))
    assert got is not None and WC.stats["path"] == "hash"
    off, ln, cnt = (t.tolist() for t in got)
    words = [text[o:o + n] for o, n in zip(off, ln)]
    assert off == sorted(off) and len(words) == len(exp)
    assert dict(zip(words, cnt)) == exp
    assert off == [first[w] for w in words]
    if name == "flush":
        assert WC.stats["flushes"] >= 6           # 3 * LDS_SLOTS new words a round, half a table a flush


def test_overflow_falls_back_to_the_sort_path(monkeypatch):
    text = b"\n".join(_words(1000))
    buf = _heap(text)
    assert WC.count_words(buf, capacity=256) is None and WC.stats["overflow"]
    monkeypatch.setattr(WC, "DEFAULT_CAPACITY", 256)
    with tuning.scope(wordcount_kernel="hash"):
        t = TX.word_count_table(buf)
    assert TX.stats["path"] == "sort" and WC.stats["overflow"]
    assert dict(t.to_objects()) == {w.decode(): c for w, c in _reference(text)[0].items()}


def test_tag_collision_is_detected():
    assert WC.count_words(_heap(b" ".join(_words(100)) * 2), tag_bits=4) is None
    assert WC.stats["collision"] and not WC.stats["overflow"]


def test_wordcount_query_runs_the_hash_kernel(tmp_path_factory):
    import dryad_amd as D
    from dryad_amd.models.wordcount import word_count_query
    p, data = _corpus(tmp_path_factory, 5000, 800)
    g = D.DryadLinqContext(platform="gpu")
    g.PartitionCount = 2
    g.WordCountKernel = "hash"
    TX.stats.clear()
    got = dict(word_count_query(g, f"text://{p}?partitions=2"))
    assert got == dict(Counter(data.decode().split()))
    fb = {op for _, op, _ in g._get_executor().last_result["fallbacks"]}
    assert "read" not in fb and "apply" not in fb
    assert TX.stats["path"] == "hash"
