"""Exact, stable device ordering of string keys (csrc/kernels/strsort.hip).

``sort_strings`` orders (heap, off, len) byte strings in unsigned byte-wise lexicographic order
(a proper prefix first; Python's ``str`` order over the UTF-8 bytes), equal strings in input
order, ascending or descending.  Each pass keys every still-unordered string by a window of its
bytes (11 at depth 0, then 7 behind a 32-bit run id), sorts the E128 entries with the stable
sort of ops/sort.py, and lets the LDS finisher rank every run of tying strings that fits one
workgroup by the strings' remaining bytes.  Runs too long for that are compacted and keyed again
one window deeper; the run id leads their keys, so they never leave their positions.

``range_dest_strings`` is the RangePartition destination of each string among <= 255 separators.
"""
from __future__ import annotations

import torch

from . import _lib
from . import sort as S
from ._lib import c_i32, c_u32, c_u64, ptr, stream_of, vp

_lib.register_signatures({
    "dr_str_window_keys": (c_i32, [vp, c_u64, vp, vp, vp, vp, c_u64, c_i32, c_u64, vp, vp]),
    "dr_str_boundaries": (c_i32, [vp, c_u64, c_u32, c_i32, vp, vp, vp]),
    "dr_str_finish": (c_i32, [vp, c_u64, vp, vp, vp, vp, vp, c_u64, c_i32, c_u64, vp]),
    "dr_str_range_dest": (c_i32, [vp, c_u64, vp, vp, c_u64, vp, c_u64, vp, vp, c_u32, c_i32, c_u32, vp, vp]),
})

# the finisher's geometry (kFinCore / kFinExt of strsort.hip) and the window widths in bytes
FIN_CORE = 1024
FIN_EXT = 256
W0 = 11
W = 7
MAX_SEPARATORS = 255


def _triple(heap, off, ln):
    _lib.require_gpu_tensor(off, "strsort")
    return heap.contiguous(), off.to(torch.int64).contiguous(), ln.to(torch.int64).contiguous()


def sort_strings(heap: torch.Tensor, off: torch.Tensor, ln: torch.Tensor, descending: bool = False) -> torch.Tensor:
    """int64 perm[n]: string perm[j] is the j-th in order (stable).  n < 2^32."""
    n = off.shape[0]
    if n >= (1 << 32):
        raise ValueError("sort_strings: 2^32 strings or more (32-bit row index in the sort entries)")
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=off.device)
    heap, off, ln = _triple(heap, off, ln)
    dev, st, desc = off.device, stream_of(off), int(bool(descending))
    hn = c_u64(heap.numel())
    max_passes = int(ln.max()) // W + 2
    perm = active = rows = rid = None
    depth, width, m = 0, W0, n
    for _ in range(max_passes):
        ent = S.empty_entries(m, dev)
        _lib.call("dr_str_window_keys", ptr(heap), hn, ptr(off), ptr(ln), ptr(rows), ptr(rid), c_u64(depth), desc,
                  c_u64(m), ptr(ent), st)
        srt = S.sort_entries_hybrid(ent, 32)
        cur = torch.empty(m, dtype=torch.int64, device=dev)
        flags = torch.empty(m, dtype=torch.uint8, device=dev)
        _lib.call("dr_str_boundaries", ptr(srt), c_u64(m), c_u32(width), desc, ptr(cur), ptr(flags), st)
        long_start = torch.zeros(m, dtype=torch.uint8, device=dev)
        _lib.call("dr_str_finish", ptr(heap), hn, ptr(off), ptr(ln), ptr(cur), ptr(flags), ptr(long_start),
                  c_u64(depth + width), desc, c_u64(m), st)
        if perm is None:
            perm = cur
        else:
            perm[active] = cur                 # the j-th sorted slot is the j-th active position
        if not bool(long_start.any()):
            return perm
        # positions of the long runs, compacted; their run number is the next pass's leading key
        start = flags & 1
        run = torch.cumsum(start, 0, dtype=torch.int64) - 1
        is_long = long_start[torch.nonzero(start).flatten()]
        sel = torch.nonzero(is_long[run]).flatten()
        active = sel if active is None else active[sel]
        rows, rid = cur[sel].contiguous(), run[sel].contiguous()
        depth, width, m = depth + width, W, sel.shape[0]
    raise AssertionError(f"sort_strings: strings still unordered after {max_passes} passes")


def range_dest_strings(heap: torch.Tensor, off: torch.Tensor, ln: torch.Tensor, sep_heap: torch.Tensor,
                       sep_off: torch.Tensor, sep_ln: torch.Tensor, descending: bool = False,
                       count: int | None = None) -> torch.Tensor:
    """int32 dest[n]: the number of separators strictly before each string in the (ascending or
    descending) order the separators are sorted in, at most ``count - 1`` (count: the number of
    partitions, one more than the separators unless given) -- ``bisect_left`` of the host
    RangePartition."""
    n, nsep = off.shape[0], sep_off.shape[0]
    if nsep > MAX_SEPARATORS:
        raise ValueError("range_dest_strings: more than 255 separators")
    dest = torch.empty(n, dtype=torch.int32, device=off.device)
    if n == 0:
        return dest
    heap, off, ln = _triple(heap, off, ln)
    sep_heap, sep_off, sep_ln = _triple(sep_heap, sep_off, sep_ln)
    top = (nsep if count is None else max(count, 1) - 1)
    _lib.call("dr_str_range_dest", ptr(heap), c_u64(heap.numel()), ptr(off), ptr(ln), c_u64(n), ptr(sep_heap),
              c_u64(sep_heap.numel()), ptr(sep_off), ptr(sep_ln), c_u32(nsep), int(bool(descending)), c_u32(top),
              ptr(dest), stream_of(off))
    return dest


__all__ = ["sort_strings", "range_dest_strings", "FIN_CORE", "FIN_EXT", "W0", "W", "MAX_SEPARATORS"]
