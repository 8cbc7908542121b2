"""WordCount as one fused tokenise-and-count pass (csrc/kernels/wordcount.hip): the distinct words
of a text heap with their counts, without marks, token offsets, hashes or sort entries in HBM.

``dr_wc_count`` reads the text once: every workgroup walks its span in tiles of ``TILE`` bytes
staged in LDS, hashes each token 8 bytes a step and counts it in an LDS open-addressing table of
``LDS_SLOTS`` slots, which it folds into a global table of ``capacity`` slots when it passes half
full, every MiB of its span and at the end.  ``dr_wc_verify`` reads the text a second time and
compares every token with the first occurrence of its group, bytes and length, so the result
does not rest on the 64-bit tags.  ``dr_wc_emit`` returns the occupied slots.

The global table takes 24 bytes a slot (tag, count, first occurrence << 16 | length).  The
default of 2^22 slots costs 96 MiB of HBM while a call runs and holds 2^21 distinct words (the
kernels refuse a load factor above 1/2), forty times the vocabulary of the benchmark corpus and
more than any natural-language corpus; clearing it costs what writing 96 MiB costs, well under a
tenth of one read of a 1 GB text.  A text with more distinct words overflows: ``count_words``
returns None and the caller sorts (ops/text.py).
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import c_i32, c_u64, ptr, stream_of, vp

_lib.register_signatures({
    "dr_wc_geometry": (c_i32, [vp, vp, vp]),
    "dr_wc_count": (c_i32, [vp, c_u64, vp, c_u64, vp, c_u64, vp]),
    "dr_wc_verify": (c_i32, [vp, c_u64, vp, c_u64, vp, c_u64, vp]),
    "dr_wc_emit": (c_i32, [vp, c_u64, vp, c_u64, vp, c_u64, vp, vp, vp, vp]),
})

# the kernels' geometry (kTile, kLdsSlots of wordcount.hip, and the least bytes one workgroup's
# span covers): checked against the library on first use
TILE = 8192
LDS_SLOTS = 4096
MIN_SPAN = 32 * TILE
DEFAULT_CAPACITY = 1 << 22
_USED, _OVERFLOW, _FLUSHES, _BAD, _EMITTED = range(5)
_checked = False

# the last call: path ("hash", or None when it gave up), groups, LDS flushes, overflow, collision
stats: dict = {}


def _check_geometry():
    global _checked
    if not _checked:
        g = [ctypes.c_uint32() for _ in range(3)]
        _lib.call("dr_wc_geometry", *[ctypes.byref(x) for x in g])
        assert [x.value for x in g] == [TILE, LDS_SLOTS, MIN_SPAN], "ops/wordcount.py and wordcount.hip disagree"
        _checked = True


def count_words(buf: torch.Tensor, capacity: int | None = None, tag_bits: int = 64):
    """-> (off, len, count), int64 [groups] each: the distinct whitespace-separated words of the
    uint8 text ``buf`` by their first occurrence ``buf[off: off + len]``, sorted by ``off``, with
    their number of occurrences; or None when the text has more than ``capacity`` / 2 distinct
    words (``capacity``: slots of the global table, a power of two) or two different words share
    a tag.  ``tag_bits`` < 64 keeps only that many bits of the tag, which makes such collisions
    likely: it exists for the tests of the exact check."""
    _lib.require_gpu_tensor(buf, "count_words")
    if buf.dtype != torch.uint8 or buf.dim() != 1:
        raise ValueError("count_words: a one-dimensional uint8 text")
    cap = DEFAULT_CAPACITY if capacity is None else int(capacity)
    if cap < 1 or cap & (cap - 1) or cap > 1 << 32:
        raise ValueError(f"count_words: capacity {capacity} is not a power of two up to 2^32")
    if not 1 <= tag_bits <= 64:
        raise ValueError("count_words: tag_bits outside [1, 64]")
    _check_geometry()
    n, dev, st = buf.shape[0], buf.device, stream_of(buf)
    if n >= 1 << 47:
        raise ValueError("count_words: 2^47 bytes or more")
    stats.clear()
    stats.update(path=None, groups=0, flushes=0, overflow=False, collision=False)
    if buf.data_ptr() % 16:                 # the tiles are loaded 16 bytes at a time
        buf = buf.clone()
    table = torch.empty((3, cap), dtype=torch.int64, device=dev)
    table[:2].zero_()
    table[2].fill_(-1)
    ctr = torch.zeros(8, dtype=torch.int32, device=dev)
    mask = c_u64((1 << tag_bits) - 1)
    _lib.call("dr_wc_count", ptr(buf), c_u64(n), ptr(table), c_u64(cap), ptr(ctr), mask, st)
    _lib.call("dr_wc_verify", ptr(buf), c_u64(n), ptr(table), c_u64(cap), ptr(ctr), mask, st)
    c = ctr.cpu().tolist()
    stats.update(flushes=c[_FLUSHES], overflow=bool(c[_OVERFLOW]), collision=bool(c[_BAD]))
    if c[_OVERFLOW] or c[_BAD]:
        return None
    g = c[_USED]
    off, ln, cnt = (torch.empty(g, dtype=torch.int64, device=dev) for _ in range(3))
    _lib.call("dr_wc_emit", ptr(buf), c_u64(n), ptr(table), c_u64(cap), ptr(ctr), c_u64(g), ptr(off), ptr(ln),
              ptr(cnt), st)
    off, order = torch.sort(off)
    stats.update(path="hash", groups=g)
    return off, ln.index_select(0, order), cnt.index_select(0, order)


__all__ = ["count_words", "stats", "TILE", "LDS_SLOTS", "MIN_SPAN", "DEFAULT_CAPACITY"]
