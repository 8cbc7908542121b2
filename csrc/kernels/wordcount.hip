// WordCount: fused tokenise-and-count with LDS hash tables (K15 + K6).
//
// The text of a partition is one byte heap in HBM.  Whitespace is ' ', '\t', '\r', '\n' (text.hip);
// every other byte, 0x00, 0x0b, 0x0c and >= 0x80 included, is a word byte.  Nothing per token ever
// reaches HBM: no marks, offsets, hashes or sort entries.
//
//   dr_wc_count  : each workgroup owns a contiguous span and walks it in tiles of kTile bytes.  A
//                  tile is staged in LDS (16-byte loads, prefetched into registers while the
//                  previous tile is scanned) with the 16 bytes before it and kExt bytes after it.
//                  A lane scans its own 32-byte chunk for token starts with SWAR byte tests, walks
//                  each token that starts there to its end (LDS while staged, global memory beyond,
//                  never past n) hashing 8 bytes per step, and inserts the 64-bit tag into the
//                  workgroup's open-addressing LDS table: ds CAS on the tag, ds add on the count,
//                  ds min on (window-relative offset << 12 | length).  The table is flushed into
//                  the global table (same shape; 64-bit count, offset << 16 | length) when it is
//                  more than half full, at the end of a 1 MiB window (so the 20-bit relative offset
//                  and the 32-bit count cannot wrap) and at the end of the span.  A token that finds
//                  no LDS slot within kLdsProbes steps goes straight to the global table.
//   dr_wc_verify : the same walk again; every token is looked up in the now read-only global
//                  table and compared, bytes and length, with its group's representative (the first
//                  occurrence).  A difference means two words share a tag.
//   dr_wc_emit   : the occupied global slots as (offset, length, count), in no order.
//
// Every loop is bounded by n or by a slot count; nothing waits for another lane's store (the
// accumulators start at their identities, so an inserter's CAS is all that orders a slot).
// (ops/wordcount.py exports the geometry as TILE / LDS_SLOTS / MIN_SPAN: keep the two in step)
#include "common.h"

namespace {

constexpr uint32_t kTile = 8192;                 // bytes per tile: 256 lanes x 32-byte chunks
constexpr uint32_t kExt = 64;                    // bytes staged past the tile for tokens that leave it
constexpr uint32_t kStaged = kTile + kExt;       // tile-relative bytes a walk may read from LDS
constexpr uint32_t kPieces = (16 + kStaged + 16) / 16;   // 16-byte pieces: 16 before, 16 of padding after
constexpr int kPieceIters = (kPieces + kBlock - 1) / kBlock;
constexpr uint32_t kLdsSlots = 4096;             // 16 bytes a slot: 64 KiB + the stage, two workgroups a CU
constexpr uint32_t kLdsLog = 12;
constexpr int kLdsProbes = 128;
constexpr uint32_t kWindow = 1u << 20;           // bytes of a span between forced flushes
constexpr uint32_t kLenBits = 12, kLongLen = (1u << kLenBits) - 1;      // LDS: offset << 12 | length
constexpr uint32_t kGLenBits = 16;                                      // global: offset << 16 | length
constexpr uint64_t kGLongLen = (1ull << kGLenBits) - 1;
constexpr uint64_t kOnes = 0x0101010101010101ull;
enum Ctr : int { USED = 0, OVERFLOW = 1, FLUSHES = 2, BAD = 3, EMITTED = 4 };

// 0x80 in every byte of w that equals c (exact: no carries between bytes)
__device__ __forceinline__ uint64_t eq_bytes(uint64_t w, uint8_t c) {
  const uint64_t x = w ^ (kOnes * c);
  const uint64_t t = (x & (kOnes * 0x7f)) + kOnes * 0x7f;
  return ~(t | x | (kOnes * 0x7f));
}

__device__ __forceinline__ uint64_t space_bytes(uint64_t w) {
  return eq_bytes(w, ' ') | eq_bytes(w, '\t') | eq_bytes(w, '\n') | eq_bytes(w, '\r');
}

// the text as a walk sees it: the staged tile (tile byte i at stage[16 + i]) and the heap behind it
struct Text {
  const uint8_t* stage;
  const uint8_t* buf;
  uint64_t tile0, n;
};

// 8 bytes of the heap at g, bytes at and past n reading as ' '
__device__ __forceinline__ uint64_t global_word(const uint8_t* __restrict__ buf, uint64_t g, uint64_t n) {
  uint64_t w;
  if (g + 8 <= n) {
    __builtin_memcpy(&w, buf + g, 8);
    return w;
  }
  w = 0;
  for (int b = 0; b < 8; ++b) w |= (uint64_t)(g + b < n ? buf[g + b] : (uint8_t)' ') << (8 * b);
  return w;
}

// 8 bytes at tile-relative q: two aligned LDS words while staged, the heap beyond
__device__ __forceinline__ uint64_t text_word(const Text& tx, uint64_t q) {
  if (q + 8 > kStaged) return global_word(tx.buf, tx.tile0 + q, tx.n);
  const uint32_t a = 16u + (uint32_t)q;
  const uint64_t* p = reinterpret_cast<const uint64_t*>(tx.stage + (a & ~7u));
  const uint32_t sh = (a & 7u) * 8u;
  const uint64_t lo = p[0], hi = p[1];
  return sh ? (lo >> sh) | (hi << (64u - sh)) : lo;
}

__device__ __forceinline__ uint64_t mix_word(uint64_t h, uint64_t w) {
  h = (h ^ w) * 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 29);
}

// hash and length of the token that starts at tile-relative p (the bytes past its end masked off)
__device__ __forceinline__ void walk_token(const Text& tx, uint32_t p, uint64_t& hash, uint64_t& len) {
  uint64_t h = 0x243F6A8885A308D3ull, L = 0;
  for (uint64_t q = p; tx.tile0 + q < tx.n; q += 8) {
    uint64_t w = text_word(tx, q);
    const uint64_t sp = space_bytes(w);
    if (sp) {
      const uint32_t j = (uint32_t)__builtin_ctzll(sp) >> 3;
      if (j) h = mix_word(h, w & ((1ull << (8 * j)) - 1));
      L += j;
      break;
    }
    h = mix_word(h, w);
    L += 8;
  }
  hash = mix64(h ^ L);
  len = L;
}

__device__ __forceinline__ uint64_t tag_of(uint64_t hash, uint64_t tagmask) {
  const uint64_t t = hash & tagmask;
  return t ? t : 1ull;                            // 0 marks a free slot
}

// home slot from the tag alone, so that equal tags probe alike whatever tagmask kept of the hash
__device__ __forceinline__ uint32_t slot_hash(uint64_t tag) { return ((uint32_t)tag ^ (uint32_t)(tag >> 32)) * 0x9E3779B1u; }

// length of the token at heap offset off, by bytes (flushes and emits of very long tokens only)
__device__ uint64_t token_length(const uint8_t* __restrict__ buf, uint64_t off, uint64_t n) {
  uint64_t L = 0;
  for (uint64_t g = off; g < n; g += 8) {
    const uint64_t sp = space_bytes(global_word(buf, g, n));
    if (sp) return L + ((uint32_t)__builtin_ctzll(sp) >> 3);
    L += 8;
  }
  return n - off;
}

struct GTable {
  unsigned long long* tag;    // [cap], 0 = free
  unsigned long long* cnt;    // [cap], 0
  unsigned long long* pack;   // [cap], ~0: first occurrence << 16 | min(length, 0xFFFF)
  uint64_t cap;
  uint32_t caplog;
  uint32_t* ctr;
};

// slot of tag in the global table, inserting it; cap when the table is full (overflow raised)
__device__ __forceinline__ uint64_t global_insert(const GTable& g, uint64_t tag) {
  uint64_t h = g.caplog ? slot_hash(tag) >> (32u - g.caplog) : 0;
  for (uint64_t probe = 0; probe < g.cap; ++probe) {
    const unsigned long long cur = g.tag[h];
    if (cur == tag) return h;
    if (cur == 0) {
      const unsigned long long prev = atomicCAS(&g.tag[h], 0ull, (unsigned long long)tag);
      if (prev == 0) {
        if ((uint64_t)atomicAdd(&g.ctr[USED], 1u) + 1 > g.cap / 2) atomicOr(&g.ctr[OVERFLOW], 1u);
        return h;
      }
      if (prev == tag) return h;
    }
    h = (h + 1) & (g.cap - 1);
  }
  atomicOr(&g.ctr[OVERFLOW], 1u);
  return g.cap;
}

__device__ __forceinline__ void global_add(const GTable& g, uint64_t tag, uint64_t count, uint64_t off, uint64_t len) {
  const uint64_t s = global_insert(g, tag);
  if (s >= g.cap) return;
  atomicAdd(&g.cnt[s], (unsigned long long)count);
  atomicMin(&g.pack[s], (unsigned long long)((off << kGLenBits) | (len < kGLongLen ? len : kGLongLen)));
}

// read-only lookup: slot of tag, or cap
__device__ __forceinline__ uint64_t global_find(const GTable& g, uint64_t tag) {
  uint64_t h = g.caplog ? slot_hash(tag) >> (32u - g.caplog) : 0;
  for (uint64_t probe = 0; probe < g.cap; ++probe) {
    const unsigned long long cur = g.tag[h];
    if (cur == tag) return h;
    if (cur == 0) return g.cap;
    h = (h + 1) & (g.cap - 1);
  }
  return g.cap;
}

// ---- tile staging --------------------------------------------------------------------------------
struct Pieces {
  uint4 r[kPieceIters];
};

// piece pc holds tile-relative bytes [16 (pc - 1), 16 pc): the heap, '\n' before byte 0, ' ' from n on
__device__ __forceinline__ void load_pieces(Pieces& ps, const uint8_t* __restrict__ buf, uint64_t tile0, uint64_t n) {
#pragma unroll
  for (int i = 0; i < kPieceIters; ++i) {
    const uint32_t pc = threadIdx.x + i * kBlock;
    if (pc >= kPieces) break;
    if (pc == 0 && tile0 == 0) {
      ps.r[i] = make_uint4(0x0a0a0a0au, 0x0a0a0a0au, 0x0a0a0a0au, 0x0a0a0a0au);
      continue;
    }
    const uint64_t g = tile0 + 16ull * pc - 16;
    if (g + 16 <= n) {
      ps.r[i] = *reinterpret_cast<const uint4*>(buf + g);
    } else {
      uint32_t w[4] = {0x20202020u, 0x20202020u, 0x20202020u, 0x20202020u};
      for (uint32_t b = 0; b < 16 && g + b < n; ++b)
        w[b >> 2] = (w[b >> 2] & ~(0xffu << (8 * (b & 3)))) | ((uint32_t)buf[g + b] << (8 * (b & 3)));
      ps.r[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
}

__device__ __forceinline__ void store_pieces(const Pieces& ps, uint8_t* stage) {
#pragma unroll
  for (int i = 0; i < kPieceIters; ++i) {
    const uint32_t pc = threadIdx.x + i * kBlock;
    if (pc < kPieces) reinterpret_cast<uint4*>(stage)[pc] = ps.r[i];
  }
}

// f(p, hash, len) for every token that starts in this lane's chunk of the tile, below tile_len
template <typename F>
__device__ __forceinline__ void scan_chunk(const Text& tx, uint32_t tile_len, F f) {
  const uint32_t c = threadIdx.x * (kTile / kBlock);
  if (c >= tile_len) return;
  const uint8_t pb = tx.stage[16 + c - 1];
  uint64_t prev = (pb == ' ' || pb == '\t' || pb == '\n' || pb == '\r') ? 0x80ull : 0ull;
  const uint64_t* words = reinterpret_cast<const uint64_t*>(tx.stage + 16 + c);
#pragma unroll
  for (uint32_t i = 0; i < kTile / kBlock / 8; ++i) {
    const uint64_t sp = space_bytes(words[i]);
    uint64_t starts = ~sp & (kOnes * 0x80) & ((sp << 8) | prev);
    prev = sp >> 56;
    while (starts) {
      const uint32_t p = c + 8 * i + ((uint32_t)__builtin_ctzll(starts) >> 3);
      starts &= starts - 1;
      if (p >= tile_len) break;
      uint64_t hash, len;
      walk_token(tx, p, hash, len);
      f(p, hash, len);
    }
  }
}

struct LTable {
  unsigned long long tag[kLdsSlots];
  uint32_t cnt[kLdsSlots];
  uint32_t pack[kLdsSlots];   // window-relative first occurrence << 12 | min(length, 0xFFF)
};

__device__ __forceinline__ void lds_clear(LTable& lt) {
  for (uint32_t s = threadIdx.x; s < kLdsSlots; s += kBlock) {
    lt.tag[s] = 0;
    lt.cnt[s] = 0;
    lt.pack[s] = 0xFFFFFFFFu;
  }
}

// the LDS table folded into the global one and cleared; both ends are barriers
__device__ void lds_flush(LTable& lt, uint32_t& used, const GTable& g, const uint8_t* __restrict__ buf, uint64_t winbase,
                          uint64_t n) {
  __syncthreads();
  for (uint32_t s = threadIdx.x; s < kLdsSlots; s += kBlock) {
    const uint64_t tag = lt.tag[s];
    if (tag == 0) continue;
    const uint32_t pk = lt.pack[s];
    const uint64_t off = winbase + (pk >> kLenBits);
    uint64_t len = pk & kLongLen;
    if (len == kLongLen) len = token_length(buf, off, n);
    global_add(g, tag, lt.cnt[s], off, len);
    lt.tag[s] = 0;
    lt.cnt[s] = 0;
    lt.pack[s] = 0xFFFFFFFFu;
  }
  if (threadIdx.x == 0) {
    used = 0;
    atomicAdd(&g.ctr[FLUSHES], 1u);
  }
  __syncthreads();
}

__global__ __launch_bounds__(kBlock) void wc_count_kernel(const uint8_t* __restrict__ buf, uint64_t n, uint64_t span,
                                                          uint64_t tagmask, GTable g) {
  __shared__ LTable lt;
  __shared__ __attribute__((aligned(16))) uint8_t stage[kPieces * 16];
  __shared__ uint32_t used, stop, fill;         // fill: `used` as of the last barrier, the same for every lane
  const uint64_t beg = (uint64_t)blockIdx.x * span;
  if (beg >= n) return;
  const uint64_t end = beg + span < n ? beg + span : n;
  lds_clear(lt);
  if (threadIdx.x == 0) used = 0;
  Pieces ps;
  load_pieces(ps, buf, beg, n);
  uint64_t winbase = beg;
  for (uint64_t tile0 = beg; tile0 < end; tile0 += kTile) {
    store_pieces(ps, stage);
    if (threadIdx.x == 0) {
      stop = __hip_atomic_load(&g.ctr[OVERFLOW], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      fill = used;
    }
    __syncthreads();
    if (stop) break;
    if (tile0 + kTile < end) load_pieces(ps, buf, tile0 + kTile, n);   // in flight while this tile is scanned
    if (fill * 2 > kLdsSlots || tile0 + kTile - winbase > kWindow) {
      lds_flush(lt, used, g, buf, winbase, n);
      winbase = tile0;
    }
    const Text tx{stage, buf, tile0, n};
    const uint32_t tile_len = end - tile0 < kTile ? (uint32_t)(end - tile0) : kTile;
    const uint32_t rel = (uint32_t)(tile0 - winbase);
    scan_chunk(tx, tile_len, [&](uint32_t p, uint64_t hash, uint64_t len) {
      const uint64_t tag = tag_of(hash, tagmask);
      uint32_t h = slot_hash(tag) >> (32u - kLdsLog);
      int slot = -1;
      for (int probe = 0; probe < kLdsProbes; ++probe) {
        const unsigned long long cur = lt.tag[h];
        if (cur == tag) { slot = (int)h; break; }
        if (cur == 0) {
          const unsigned long long prev = atomicCAS(&lt.tag[h], 0ull, (unsigned long long)tag);
          if (prev == 0) atomicAdd(&used, 1u);
          if (prev == 0 || prev == tag) { slot = (int)h; break; }
        }
        h = (h + 1) & (kLdsSlots - 1);
      }
      if (slot >= 0) {
        atomicAdd(&lt.cnt[slot], 1u);
        atomicMin(&lt.pack[slot], ((rel + p) << kLenBits) | (len < kLongLen ? (uint32_t)len : kLongLen));
      } else {
        global_add(g, tag, 1, tile0 + p, len);
      }
    });
    __syncthreads();
  }
  lds_flush(lt, used, g, buf, winbase, n);
}

__global__ __launch_bounds__(kBlock) void wc_verify_kernel(const uint8_t* __restrict__ buf, uint64_t n, uint64_t span,
                                                           uint64_t tagmask, GTable g) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kPieces * 16];
  const uint64_t beg = (uint64_t)blockIdx.x * span;
  if (beg >= n || g.ctr[OVERFLOW]) return;      // set, if at all, before this kernel started
  const uint64_t end = beg + span < n ? beg + span : n;
  Pieces ps;
  load_pieces(ps, buf, beg, n);
  for (uint64_t tile0 = beg; tile0 < end; tile0 += kTile) {
    store_pieces(ps, stage);
    __syncthreads();
    if (tile0 + kTile < end) load_pieces(ps, buf, tile0 + kTile, n);
    const Text tx{stage, buf, tile0, n};
    const uint32_t tile_len = end - tile0 < kTile ? (uint32_t)(end - tile0) : kTile;
    scan_chunk(tx, tile_len, [&](uint32_t p, uint64_t hash, uint64_t len) {
      const uint64_t s = global_find(g, tag_of(hash, tagmask));
      bool bad = s >= g.cap;
      if (!bad) {
        const uint64_t pk = g.pack[s];
        const uint64_t roff = pk >> kGLenBits, rlen = pk & kGLongLen;
        if (roff == tile0 + p) return;
        // the representative starts after whitespace as every token does, so it equals this token
        // when len bytes agree and it ends there too (its stored length, or whitespace / n past it)
        bad = rlen < kGLongLen ? rlen != len : len < kGLongLen;
        for (uint64_t k = 0; !bad && k < len; k += 8) {
          const uint64_t m = len - k < 8 ? (1ull << (8 * (len - k))) - 1 : ~0ull;
          bad = ((text_word(tx, p + k) ^ global_word(buf, roff + k, n)) & m) != 0;
        }
        if (!bad && rlen == kGLongLen && roff + len < n) bad = (space_bytes(buf[roff + len]) & 0x80) == 0;
      }
      if (bad) atomicOr(&g.ctr[BAD], 1u);
    });
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBlock) void wc_emit_kernel(const uint8_t* __restrict__ buf, uint64_t n, GTable g,
                                                         uint64_t room, int64_t* __restrict__ off,
                                                         int64_t* __restrict__ len, int64_t* __restrict__ cnt) {
  for (uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x; s < g.cap; s += (uint64_t)gridDim.x * kBlock) {
    if (g.tag[s] == 0) continue;
    const uint64_t i = atomicAdd(&g.ctr[EMITTED], 1u);
    if (i >= room) continue;
    const uint64_t pk = g.pack[s];
    const uint64_t o = pk >> kGLenBits, L = pk & kGLongLen;
    off[i] = (int64_t)o;
    len[i] = (int64_t)(L == kGLongLen ? token_length(buf, o, n) : L);
    cnt[i] = (int64_t)g.cnt[s];
  }
}

inline bool table_args(GTable& g, unsigned long long* table, uint64_t cap, uint32_t* ctr) {
  if (cap == 0 || (cap & (cap - 1)) || cap > (1ull << 32) || table == nullptr || ctr == nullptr) return false;
  uint32_t lg = 0;
  while ((1ull << lg) < cap) ++lg;
  g = GTable{table, table + cap, table + 2 * cap, cap, lg, ctr};
  return true;
}

inline uint64_t span_for(uint64_t n, uint32_t min_span, unsigned& blocks) {
  int dev = 0, cus = 256;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  uint64_t span = (n + 2ull * cus - 1) / (2ull * cus);          // two resident workgroups a CU
  if (span < min_span) span = min_span;
  span = (span + kTile - 1) / kTile * kTile;
  blocks = (unsigned)((n + span - 1) / span);
  return span;
}

}  // namespace

// kTile, kLdsSlots and the least bytes of a workgroup's span, for ops/wordcount.py and the tests
DR_API int dr_wc_geometry(uint32_t* tile, uint32_t* lds_slots, uint32_t* min_span) {
  *tile = kTile;
  *lds_slots = kLdsSlots;
  *min_span = 32 * kTile;
  return 0;
}

// buf: 16-byte aligned text [n], n < 2^47.  table: uint64 [3][cap] = tags (0), counts (0), packs
// (~0); cap a power of two.  ctr: uint32 [8] zeroed (Ctr above).  tagmask: the tag bits kept.
DR_API int dr_wc_count(const uint8_t* buf, uint64_t n, unsigned long long* table, uint64_t cap, uint32_t* ctr,
                       uint64_t tagmask, hipStream_t s) {
  GTable g;
  if (!table_args(g, table, cap, ctr) || ((uintptr_t)buf & 15) || n >= (1ull << 47)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  unsigned blocks;
  const uint64_t span = span_for(n, 32 * kTile, blocks);
  wc_count_kernel<<<blocks, kBlock, 0, s>>>(buf, n, span, tagmask, g);
  DR_LAUNCH_CHECK();
  return 0;
}

DR_API int dr_wc_verify(const uint8_t* buf, uint64_t n, unsigned long long* table, uint64_t cap, uint32_t* ctr,
                        uint64_t tagmask, hipStream_t s) {
  GTable g;
  if (!table_args(g, table, cap, ctr) || ((uintptr_t)buf & 15) || n >= (1ull << 47)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  unsigned blocks;
  const uint64_t span = span_for(n, 4 * kTile, blocks);          // no table to amortise: short spans
  wc_verify_kernel<<<blocks, kBlock, 0, s>>>(buf, n, span, tagmask, g);
  DR_LAUNCH_CHECK();
  return 0;
}

// off / len / cnt: int64 [room]; ctr[EMITTED] counts the occupied slots
DR_API int dr_wc_emit(const uint8_t* buf, uint64_t n, unsigned long long* table, uint64_t cap, uint32_t* ctr,
                      uint64_t room, int64_t* off, int64_t* len, int64_t* cnt, hipStream_t s) {
  GTable g;
  if (!table_args(g, table, cap, ctr)) return (int)hipErrorInvalidValue;
  if (room == 0) return 0;
  wc_emit_kernel<<<grid_for(cap, kBlock, 4096), kBlock, 0, s>>>(buf, n, g, room, off, len, cnt);
  DR_LAUNCH_CHECK();
  return 0;
}
