"""GroupBy / Distinct over string and composite keys in two streaming passes
(csrc/kernels/keyhash.hip): no fingerprint pass, no sort, no row permutation.

A key has 1..4 parts; a part is an integer / bool column, or a string column given as the tuple
``(heap, off, len)``.  ``dr_kh_aggregate`` hashes every row's key into a 64-bit tag and folds the
row into its workgroup's LDS open-addressing table (``lds_slots(nagg)`` slots: tag, first row,
accumulators), which it folds into a global table of ``capacity`` slots when it passes half full
and at the end of the workgroup's span.  ``dr_kh_verify`` reads the keys a second time and compares
every row, part for part, with the first row of its group, so the result does not rest on the
tags.  ``dr_kh_emit`` returns the occupied slots.

The global table takes 8 (2 + nagg) bytes a slot and refuses a load factor above 1/2.  Its default
capacity comes from the distinct tags of a strided sample of 2^16 rows (``estimate_distinct``); a
key with more than ``MAX_CAPACITY`` / 4 estimated distinct values is not served, and one whose
sample misled the estimate overflows: ``key_aggregate`` returns None either way and the caller
sorts (gpu/ops.py).
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import c_i32, c_u32, c_u64, ptr, stream_of, vp
from .radixagg import distinct_upper_estimate
from .relational import _MOPS

_lib.register_signatures({
    "dr_kh_geometry": (c_i32, [c_i32, vp, vp, vp]),
    "dr_kh_aggregate": (c_i32, [c_i32, vp, vp, vp, vp, vp, c_u64, c_i32, vp, vp, vp, c_u64, vp, c_u64, c_u64, c_u32, vp]),
    "dr_kh_verify": (c_i32, [c_i32, vp, vp, vp, vp, vp, c_u64, c_i32, vp, c_u64, vp, c_u64, vp]),
    "dr_kh_emit": (c_i32, [c_i32, vp, c_u64, vp, c_u64, vp, vp]),
    "dr_kh_tags": (c_i32, [c_i32, vp, vp, vp, vp, vp, c_u64, c_u64, c_u64, c_u64, vp, vp]),
})

MAX_PARTS = 4
MAX_AGGS = 8
STEP_ROWS = 256                    # rows a workgroup takes per step (kBlock of keyhash.hip)
SAMPLE = 1 << 16
MIN_CAPACITY = 1 << 10
MAX_CAPACITY = 1 << 22
_USED, _OVERFLOW, _FLUSHES, _BAD, _EMITTED = range(5)
_INT_PARTS = (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8, torch.bool, torch.uint16, torch.uint32,
              torch.uint64)

# the last call: path ("keyhash", or None when it gave up), groups, capacity, LDS flushes, overflow,
# collision (two keys under one tag, or a string outside its heap)
stats: dict = {}


def lds_slots(nagg: int) -> int:
    """Slots of a workgroup's LDS table for ``nagg`` aggregates (12 + 8 nagg bytes a slot, the
    largest power of two that keeps the workgroup at or under 64 KiB), as the library reports it."""
    slots, step, span = (ctypes.c_uint32() for _ in range(3))
    _lib.call("dr_kh_geometry", nagg, ctypes.byref(slots), ctypes.byref(step), ctypes.byref(span))
    assert step.value == STEP_ROWS, "ops/keyhash.py and keyhash.hip disagree"
    return slots.value


class _Key:
    """The key parts as the launchers take them (host arrays of pointers, heap sizes and widths)."""

    def __init__(self, parts, n):
        self.keep, rows = [], []           # rows: (base, off, len, heap bytes, width) of each part
        for p in parts:
            if isinstance(p, torch.Tensor):
                _lib.require_gpu_tensor(p, "key_aggregate")
                if p.dim() != 1 or p.shape[0] != n:
                    raise ValueError("key_aggregate: a key part is not a column of n values")
                c = p.view(torch.uint8) if p.dtype == torch.bool else p
                self.keep.append(c)
                rows.append((c.data_ptr(), 0, 0, 0, c.element_size()))
            else:
                heap, o, l = p
                _lib.require_gpu_tensor(heap, "key_aggregate")
                o, l = o.to(torch.int64).contiguous(), l.to(torch.int64).contiguous()
                if heap.dtype != torch.uint8 or heap.dim() != 1 or o.shape != (n,) or l.shape != (n,):
                    raise ValueError("key_aggregate: a string part is (uint8 heap, off [n], len [n])")
                self.keep += [heap, o, l]
                rows.append((heap.data_ptr(), o.data_ptr(), l.data_ptr(), heap.shape[0], 0))
        m = len(parts)
        base, off, ln, heap_n, width = zip(*rows)
        self.args = (m, (vp * m)(*base), (vp * m)(*off), (vp * m)(*ln), (c_u64 * m)(*heap_n), (c_i32 * m)(*width))


def _served(parts) -> bool:
    return 1 <= len(parts) <= MAX_PARTS and all(not isinstance(p, torch.Tensor) or
                                                (p.dtype in _INT_PARTS and p.dim() == 1) for p in parts)


def estimate_distinct(parts, n: int, tag_bits: int = 64):
    """Distinct keys of the n rows, estimated from the tags of an evenly strided sample of 2^16
    rows (radixagg.distinct_upper_estimate over their distinct count); None for keys key_aggregate
    does not serve."""
    if not _served(parts):
        return None
    if n == 0:
        return 0
    key = _Key(parts, n)
    stride = max(1, n // SAMPLE)
    m = min(SAMPLE, (n - 1) // stride + 1)
    dev = key.keep[0].device
    tags = torch.empty(m, dtype=torch.int64, device=dev)
    _lib.call("dr_kh_tags", *key.args, c_u64(n), c_u64(stride), c_u64(m), c_u64((1 << tag_bits) - 1), ptr(tags),
              stream_of(tags))
    return distinct_upper_estimate(int(torch.unique(tags).numel()), m, n)


def capacity_for(estimate: int):
    """Slots of the global table for an estimated number of distinct keys: a power of two at least
    4x the estimate, or None past MAX_CAPACITY."""
    cap = max(MIN_CAPACITY, 1 << (max(1, 4 * estimate) - 1).bit_length())
    return cap if cap <= MAX_CAPACITY else None


def key_aggregate(parts, specs, n, *, capacity=None, tag_bits=64, flush_rows=None, grid=None):
    """-> (first_rows, outs): the distinct keys of the n rows by the row of their first occurrence,
    int64 [groups] sorted ascending (LINQ's GroupBy / Distinct order), and one [groups] tensor per
    spec (``specs`` as for relational.seg_reduce_multi: (op, column or None, dtype), int64 or
    float64 results).  ``parts``: 1..4 key parts, each an integer / bool column [n] or a string
    column ``(heap uint8, off [n], len [n])``.

    None when a part is a floating-point column, there are more than 4 parts or 8 specs, the
    estimate asks for more than MAX_CAPACITY slots (no pass is run), the global table overflowed,
    or the verify pass found two different keys under one tag (or a string outside its heap).

    ``capacity`` (slots of the global table, a power of two; default: from estimate_distinct),
    ``tag_bits`` (< 64 keeps only that many bits of the tag), ``flush_rows`` (a workgroup folds its
    LDS table at least every so many rows) and ``grid`` (workgroups) exist so that tests reach the
    overflow, collision, flush and multi-workgroup paths with few rows."""
    stats.clear()
    stats.update(path=None, groups=0, capacity=0, flushes=0, overflow=False, collision=False)
    if not _served(parts) or len(specs) > MAX_AGGS:
        return None
    if not 1 <= tag_bits <= 64:
        raise ValueError("key_aggregate: tag_bits outside [1, 64]")
    if not 1 <= n < 1 << 47:
        raise ValueError("key_aggregate: no rows, or 2^47 or more")
    if capacity is None:
        capacity = capacity_for(estimate_distinct(parts, n, tag_bits))
        if capacity is None:
            return None
    cap = int(capacity)
    if cap < 1 or cap & (cap - 1) or cap > 1 << 32:
        raise ValueError(f"key_aggregate: capacity {capacity} is not a power of two up to 2^32")
    key = _Key(parts, n)
    dev, st = key.keep[0].device, stream_of(key.keep[0])
    nagg = len(specs)
    table = torch.empty((2 + nagg, cap), dtype=torch.int64, device=dev)
    table[0].zero_()
    table[1].fill_(-1)
    ops, vals, keep, isf = [], [], [], []
    for a, (op, v, dtype) in enumerate(specs):
        f = 0 if op == "count" or dtype in _INT_PARTS else 1
        tdt = torch.float64 if f else torch.int64
        acc = table[2 + a].view(tdt)
        acc.fill_({"sum": 0, "count": 0,
                   "min": float("inf") if f else torch.iinfo(torch.int64).max,
                   "max": float("-inf") if f else torch.iinfo(torch.int64).min}[op])
        vv = None if op == "count" else v.to(tdt).contiguous()
        if vv is not None and vv.shape != (n,):
            raise ValueError("key_aggregate: a value column is not a column of n values")
        keep.append(vv)
        ops.append(_MOPS[(op, f)])
        vals.append(0 if vv is None else vv.data_ptr())
        isf.append(f)
    ctr = torch.zeros(8, dtype=torch.int32, device=dev)
    mask = c_u64((1 << tag_bits) - 1)
    m = max(1, nagg)
    _lib.call("dr_kh_aggregate", *key.args, c_u64(n), nagg, (c_i32 * m)(*ops), (vp * m)(*vals), ptr(table), c_u64(cap),
              ptr(ctr), mask, c_u64(flush_rows or 0), c_u32(grid or 0), st)
    _lib.call("dr_kh_verify", *key.args, c_u64(n), nagg, ptr(table), c_u64(cap), ptr(ctr), mask, st)
    c = ctr.cpu().tolist()
    stats.update(capacity=cap, flushes=c[_FLUSHES], overflow=bool(c[_OVERFLOW]), collision=bool(c[_BAD]))
    if c[_OVERFLOW] or c[_BAD]:
        return None
    g = c[_USED]
    out = torch.empty((1 + nagg, g), dtype=torch.int64, device=dev)
    _lib.call("dr_kh_emit", nagg, ptr(table), c_u64(cap), ptr(ctr), c_u64(g), ptr(out), st)
    first, order = torch.sort(out[0])
    outs = [out[1 + a].index_select(0, order) for a in range(nagg)]
    stats.update(path="keyhash", groups=g)
    return first, [o.view(torch.float64) if f else o for o, f in zip(outs, isf)]


__all__ = ["key_aggregate", "estimate_distinct", "capacity_for", "lds_slots", "stats", "STEP_ROWS", "MAX_CAPACITY"]
