"""Low-cardinality GroupBy on the matrix cores (csrc/kernels/matagg.hip): exact integer Count /
Sum / Min / Max of a key column whose values come from a dictionary of at most 256 keys.

Count and sums are a one-hot int8 matrix (group x row) times the rows' byte limbs on
``v_mfma_i32_16x16x64_i8``, so the per-row path of the sums has no atomic; min and max touch an
LDS atomic only when a row improves its group.  The dictionary is the caller's, or the sorted
distinct keys of the strided sample ``estimate_distinct`` draws; rows whose key is not in it come
back as a list of row indices and go through ``hash_aggregate``, so a sample that missed a rare
key costs a gather of those rows, never a wrong result.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from . import relational as R
from ._lib import c_i32, c_u32, c_u64, ptr, stream_of, vp

_lib.register_signatures({
    "dr_matrix_aggregate": (c_i32, [vp, c_u64, vp, c_i32, c_i32, vp, c_i32, vp, vp, vp, vp, c_u32, vp, c_u32, c_u32,
                                    vp]),
    "dr_matagg_step_rows": (c_i32, []),
    "dr_matagg_waves": (c_i32, []),
})

MAX_GROUPS = 256
MAX_SUMS, MAX_MINMAX = 3, 4
MAX_FLUSH_ROWS = 1 << 24
_INTS = (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8, torch.bool)


def grid_rows(grid: int) -> int:
    """Rows that give every wave of ``grid`` workgroups exactly one full step."""
    return grid * int(_lib.lib().dr_matagg_waves()) * int(_lib.lib().dr_matagg_step_rows())


def matrix_aggregate(key: torch.Tensor, specs: list, dict_keys: torch.Tensor | None = None,
                     flush_rows: int = MAX_FLUSH_ROWS, grid: int | None = None):
    """``key``: integer column; ``specs`` as for hash_aggregate.  Returns (keys, outs) for the
    distinct keys (unordered) like hash_aggregate, or None where this path does not serve: a float
    key or aggregate, more than 3 sums or 4 min / max columns, 2^32 rows or more, more than 256
    dictionary keys, or more rows outside the dictionary than the miss list holds.

    ``flush_rows`` (64..2^24): rows a wave accumulates in i32 before it adds them to the 64-bit
    partials; ``grid``: workgroups (None: sized to the device)."""
    n = key.shape[0]
    dev = key.device
    if key.is_floating_point() or n >= (1 << 32):
        return None
    sums, mms, where = [], [], []
    for op, v, dtype in specs:
        if op == "count":
            where.append(0)
            continue
        if dtype not in _INTS or op not in ("sum", "min", "max"):
            return None
        (sums if op == "sum" else mms).append((op, v))
        where.append(len(sums) if op == "sum" else -len(mms))
    if len(sums) > MAX_SUMS or len(mms) > MAX_MINMAX:
        return None
    k64 = key.to(torch.int64).contiguous()
    if n == 0:
        return key[:0], [torch.empty(0, dtype=torch.int64, device=dev) for _ in specs]
    dk = R.sample_distinct_values(k64) if dict_keys is None else torch.unique(dict_keys.to(device=dev, dtype=torch.int64))
    d = int(dk.numel())
    if d > MAX_GROUPS or d == 0:
        return None
    ns, nm = len(sums), len(mms)
    svals = [v.to(torch.int64).contiguous() for _, v in sums]
    mvals = [v.to(torch.int64).contiguous() for _, v in mms]
    out = torch.zeros((1 + ns + nm, d), dtype=torch.int64, device=dev)
    for j, (op, _) in enumerate(mms):
        out[1 + ns + j].fill_(torch.iinfo(torch.int64).max if op == "min" else torch.iinfo(torch.int64).min)
    cap = n // 16 + 1024
    miss_rows = torch.empty(cap, dtype=torch.int32, device=dev)
    miss_count = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("dr_matrix_aggregate", ptr(k64), c_u64(n), ptr(dk), d, ns,
              (ctypes.c_void_p * max(ns, 1))(*[v.data_ptr() for v in svals]), nm,
              (ctypes.c_void_p * max(nm, 1))(*[v.data_ptr() for v in mvals]),
              (ctypes.c_int * max(nm, 1))(*[int(op == "max") for op, _ in mms]), ptr(out), ptr(miss_rows),
              c_u32(cap), ptr(miss_count), c_u32(flush_rows), c_u32(grid or 0), stream_of(k64))
    missed = int(miss_count.item()) & 0xFFFFFFFF
    if missed > cap:
        return None
    used = torch.nonzero(out[0] > 0, as_tuple=False).flatten()
    keys_out = dk.index_select(0, used)
    rows = [0 if w == 0 else w if w > 0 else ns - w for w in where]
    res = [out[r].index_select(0, used) for r in rows]
    if missed:
        # keys the dictionary lacks (disjoint from its groups): the hash path over those rows only
        idx = miss_rows[:missed].to(torch.int64) & 0xFFFFFFFF
        got = R.hash_aggregate(k64.index_select(0, idx),
                               [(op, None if v is None else v.index_select(0, idx), dt) for op, v, dt in specs])
        if got is None:
            return None
        keys_out = torch.cat([keys_out, got[0]])
        res = [torch.cat([a, b]) for a, b in zip(res, got[1])]
    return keys_out.to(key.dtype), res


__all__ = ["matrix_aggregate", "grid_rows", "MAX_GROUPS"]
