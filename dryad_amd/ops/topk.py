"""The k smallest sort entries by radix select (csrc/kernels/topk.hip): what
``OrderBy(key).Take(k)`` needs instead of a full sort.

The E128 entries of one table (ops/sort.py: ``[n, 2]`` int64, ``lo`` / ``hi``; key bits from
``begin_bit`` up, the row index in bits [0, 32)) are distinct as unsigned 128-bit numbers and
their numeric order is the stable OrderBy order, so the first k rows of the sort are the k
smallest entries.  ``topk_entries`` finds the k-th smallest value digit by digit:

* pass 0 (``dr_topk_hist``) reads the entries once: histogram of the top digit and the bitwise
  AND / OR of all entries.  AND ^ OR names the first bit that varies; a degenerate top digit
  (small integers in an int64 column) costs one more histogram pass at that bit.
* the host reads the counters (one small copy per level), picks the bucket ``b`` holding rank k;
* ``dr_topk_filter`` reads the candidates once: digit < b are winners, digit == b the next
  level's candidates, whose next digit it histograms in the same pass.

After the key bits the descent goes on in the row-index bits, which resolves ties at the k
boundary in input order.  The k winners come out unordered and are sorted here (k entries only).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import sort as S
from ._lib import c_i32, c_u32, c_u64, ptr, stream_of, vp

_lib.register_signatures({
    "dr_topk_workspace": (c_u64, []),
    "dr_topk_hist": (c_i32, [vp, c_u64, c_i32, c_i32, vp, c_i32, c_i32, vp]),
    "dr_topk_filter": (c_i32, [vp, c_u64, c_i32, c_i32, c_u32, c_u32, vp, c_u64, vp, c_u64, c_i32, c_i32, vp, c_i32,
                               c_i32, vp]),
})

# the kernels' geometry (kTkDigitBits, kTkTile, kTkGrid of topk.hip): a persistent grid of at most
# GRID workgroups walks tiles of TILE entries
DIGIT_BITS = 11
TILE = 512
GRID = 1024
_BINS = 1 << DIGIT_BITS
_HDR, _ST_WORDS = 4, _BINS + 16            # workspace layout in uint32 words (see topk.hip)
_NO_BUCKET = 0xFFFFFFFF

# keys varying over at least this many bits: the winners are sorted by the hybrid sort from bit 0
WIDE_KEY_BITS = 40
_WS_CACHE: dict = {}

# the last selection, for logs and the microbenchmark: levels (filter passes), extra histogram
# passes, the candidates entering each level, entry bytes read
stats: dict = {}


def _workspace(device) -> torch.Tensor:
    ws = _WS_CACHE.get(device)
    if ws is None:
        nbytes = int(_lib.lib().dr_topk_workspace())
        assert nbytes == (_HDR + 2 * _ST_WORDS) * 4, "ops/topk.py and topk.hip disagree on the workspace layout"
        ws = _WS_CACHE[device] = torch.empty(nbytes // 4, dtype=torch.int32, device=device)
    return ws


def _digit(top: int, begin_bit: int) -> tuple[int, int]:
    """(shift, bits) of the digit right below composite bit ``top``: key bits down to
    ``begin_bit``, then the row-index bits [0, 32); never the unused bits in between."""
    if top <= begin_bit:
        top = min(top, 32)
        shift = max(0, top - DIGIT_BITS)
    else:
        shift = max(begin_bit, top - DIGIT_BITS)
    return shift, top - shift


def _read_state(ws: torch.Tensor, slot: int, begin_bit: int):
    """-> (histogram as int64, number of the highest varying bit + 1, candidates written)."""
    a = _HDR + slot * _ST_WORDS
    w = ws[a:a + _ST_WORDS].cpu().numpy().view(np.uint32)
    q = w[_BINS:_BINS + 8].view(np.uint64)
    x = ((int(q[1]) ^ int(q[3])) << 64) | (int(q[0]) ^ int(q[2]))
    x &= ~((1 << begin_bit) - 1) | 0xFFFFFFFF          # key bits and row index only
    return w[:_BINS].astype(np.int64), x.bit_length(), int(w[_BINS + 8])


def select_entries(entries: torch.Tensor, k: int, begin_bit: int, equal_keys: bool = True):
    """-> (the k smallest entries in no particular order, number of the highest key bit that
    varies + 1 or None when no histogram pass ran), 0 < k <= n.  ``equal_keys`` False: (None, 32)
    after pass 0 when every key is the same (the stable sort is then the input order, which costs
    the caller nothing, while the select would descend through the row-index bits)."""
    n = entries.shape[0]
    dev, st = entries.device, stream_of(entries)
    ws = _workspace(dev)
    out = S.empty_entries(k, dev)
    info = dict(n=n, k=k, levels=0, hist_passes=0, candidates=[], bytes_read=0)
    cur, m, need, slot, first = entries, n, k, 0, 1
    shift, bits = _digit(128, begin_bit)
    hist = key_top = None
    while True:
        if need == m:                                  # every candidate left is a winner
            info["levels"] += 1
            info["candidates"].append(m)
            info["bytes_read"] += 16 * m
            _lib.call("dr_topk_filter", ptr(cur), c_u64(m), shift, bits, c_u32(_BINS), c_u32(_NO_BUCKET), ptr(out),
                      c_u64(k), None, c_u64(0), 0, 0, ptr(ws), slot ^ 1, first, st)
            break
        if hist is None:                               # pass 0
            _lib.call("dr_topk_hist", ptr(cur), c_u64(m), shift, bits, ptr(ws), slot, first, st)
            first = 0
            info["hist_passes"] += 1
            info["bytes_read"] += 16 * m
            hist, top, _ = _read_state(ws, slot, begin_bit)
            key_top = max(top, 32)
            if key_top == 32 and not equal_keys:
                return None, key_top
        if top <= shift:                               # degenerate digit: histogram the first varying bits
            if top == 0:
                raise RuntimeError("topk: entries that are not distinct (row-index field)")
            shift, bits = _digit(top, begin_bit)
            _lib.call("dr_topk_hist", ptr(cur), c_u64(m), shift, bits, ptr(ws), slot, 0, st)
            info["hist_passes"] += 1
            info["bytes_read"] += 16 * m
            hist, top, _ = _read_state(ws, slot, begin_bit)
        csum = np.cumsum(hist[: 1 << bits])
        if int(csum[-1]) != m:
            raise RuntimeError(f"topk: histogram counts {int(csum[-1])} of {m} entries")
        b = int(np.searchsorted(csum, need, side="left"))
        cnt = int(hist[b])
        rest = need - (int(csum[b]) - cnt)             # rank inside bucket b, 1 <= rest <= cnt
        info["levels"] += 1
        info["candidates"].append(m)
        info["bytes_read"] += 16 * m
        if rest == cnt:                                # the whole bucket wins: done
            _lib.call("dr_topk_filter", ptr(cur), c_u64(m), shift, bits, c_u32(b + 1), c_u32(_NO_BUCKET), ptr(out),
                      c_u64(k), None, c_u64(0), 0, 0, ptr(ws), slot ^ 1, first, st)
            break
        cand = S.empty_entries(cnt, dev)
        nshift, nbits = _digit(shift, begin_bit)
        if nbits == 0:
            raise RuntimeError("topk: entries that are not distinct (row-index field)")
        _lib.call("dr_topk_filter", ptr(cur), c_u64(m), shift, bits, c_u32(b), c_u32(b), ptr(out), c_u64(k),
                  ptr(cand), c_u64(cnt), nshift, nbits, ptr(ws), slot ^ 1, first, st)
        slot ^= 1
        hist, top, wrote = _read_state(ws, slot, begin_bit)
        if wrote != cnt:
            raise RuntimeError(f"topk: {wrote} candidates written, {cnt} counted")
        cur, m, need, shift, bits = cand, cnt, rest, nshift, nbits
    wrote = int(ws[0].item()) & 0xFFFFFFFF
    if wrote != k:
        raise RuntimeError(f"topk: {wrote} winners written, {k} expected")
    stats.clear()
    stats.update(info)
    return out, key_top


def topk_entries(entries: torch.Tensor, k: int, begin_bit: int, equal_keys: bool = True) -> torch.Tensor | None:
    """The k numerically smallest E128 entries in ascending order: the first k entries of the
    stable sort on bits [begin_bit, 128) of entries built in row order.  n < 2^32, 0 <= k <= n.
    Always the select kernels, at any n; with ``equal_keys`` False, None when all keys are equal
    (see select_entries)."""
    _lib.require_gpu_tensor(entries, "topk_entries")
    n = entries.shape[0]
    if entries.dim() != 2 or entries.shape[1] != 2 or entries.dtype != torch.int64:
        raise ValueError("topk_entries: [n, 2] int64 sort entries")
    if n >= (1 << 32):
        raise ValueError("topk_entries: 2^32 entries or more (32-bit row index in the sort entries)")
    if not 0 <= k <= n:
        raise ValueError(f"topk_entries: k = {k} outside [0, {n}]")
    if not 32 <= begin_bit <= 128:
        raise ValueError("topk_entries: begin_bit outside [32, 128]")
    if k == 0:
        return entries[:0]
    out, key_top = select_entries(entries, k, begin_bit, equal_keys)
    if out is None or k == 1:
        return out
    # the winners are in no order, so the row index is part of the sort key.  Keys varying over
    # WIDE_KEY_BITS or more: the hybrid sort from bit 0 (its top window, then whole entries
    # compared in LDS).  Narrow keys would make that a byte-wise LSD sort of all 128 - begin_bit
    # + 32 bits: the index bits first instead, then the stable sort of the few key bits.
    if key_top is not None and key_top - begin_bit >= WIDE_KEY_BITS:
        return S.sort_entries_hybrid(out, 0)
    return S.sort_entries_hybrid(S.sort_entries(out, 0, 32), begin_bit)


__all__ = ["topk_entries", "select_entries", "stats", "DIGIT_BITS", "TILE", "GRID"]
