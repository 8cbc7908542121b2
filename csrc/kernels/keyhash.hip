// GroupBy / Distinct over any equality key: tag-and-verify hash aggregation (K6).
//
// A key has 1..4 parts, each a column of 1-, 2-, 4- or 8-byte integers or a string column
// (heap, off, len).  A row's 64-bit hash mixes, part by part, the zero-extended value, or the
// string's bytes 8 at a time (the last word masked to the string) followed by its length: with
// both in the hash, ("ab", "c") and ("a", "bc") differ.  The row's tag is the hash under tagmask,
// 0 (a free slot) remapped to 1.  No string read leaves its heap: a word that would pass the
// heap's end is assembled byte by byte, and a row whose (off, len) does not lie inside the heap
// hashes as the empty string and is reported by the verify pass.
//
//   dr_kh_aggregate : each workgroup owns a contiguous span of rows and takes one row per lane per
//                     step.  The value columns are loaded coalesced, then the row's tag goes into
//                     the workgroup's open-addressing LDS table: ds CAS on the tag, ds min on the
//                     span-relative row (u32), ds atomics on the 64-bit accumulators (SoA, so lanes
//                     that hit neighbouring slots hit neighbouring banks).  The table holds the
//                     largest power of two of slots that keeps the workgroup at or under 64 KiB
//                     for the call's aggregates (a template parameter): two workgroups a CU.  It is
//                     folded into the global table (tags, first row by atomicMin, one accumulator
//                     array per aggregate) when it is more than half full, every flush_rows rows
//                     and at the end of the span.  A row that finds no LDS slot within kLdsProbes
//                     steps goes straight to the global table.
//   dr_kh_verify    : every row is looked up in the now read-only global table and compared, part
//                     by part (values; lengths and bytes), with its group's first row.  A
//                     difference means two keys share a tag.  Nothing is written per row.
//   dr_kh_emit      : the occupied global slots as (first row, accumulators), in no order.
//   dr_kh_tags      : the tags of every stride-th row, for the caller's distinct estimate.
//
// Every loop is bounded by n, a slot count or a string length; nothing waits for another lane's
// store (the accumulators start at their identities, so an inserter's CAS is all that orders a slot).
#include "aggops.h"

namespace {

constexpr int kMaxParts = 4;
constexpr int kLdsProbes = 64;
constexpr uint32_t kLdsBudget = 64 * 1024;       // tag + row + accumulators of every slot, and the control words
constexpr int kMinLog = 9, kMaxLog = 12;
constexpr uint32_t kMinSpan = 16 * kBlock;       // rows: below this a workgroup's flush costs more than its rows
enum Ctr : int { USED = 0, OVERFLOW = 1, FLUSHES = 2, BAD = 3, EMITTED = 4 };

struct Part {
  const uint8_t* base;      // the column of `width`-byte values, or the string heap
  const int64_t* off;       // strings: each row's offset and length in the heap
  const int64_t* len;
  uint64_t heap_n;
  uint32_t width;           // 1, 2, 4, 8; 0: a string
};

struct Key {
  Part part[kMaxParts];
  int nparts;
};

struct Aggs {
  int nagg;
  int op[kMaxAggs];
  const uint64_t* vals[kMaxAggs];   // 64-bit value columns (unused for COUNT)
};

struct GTable {
  unsigned long long* tag;     // [cap], 0 = free
  unsigned long long* first;   // [cap], ~0: the least row of the tag
  uint64_t* acc[kMaxAggs];     // [cap] each, preset to the op's identity
  uint64_t cap;
  uint32_t caplog;
  uint32_t* ctr;
};

// log2 of the LDS slots for nagg aggregates: 12 + 8 nagg bytes a slot
__host__ __device__ constexpr int lds_log(int nagg) {
  int lg = kMaxLog;
  while (lg > kMinLog && (uint32_t)(12 + 8 * nagg) << lg > kLdsBudget - 64) --lg;
  return lg;
}

__device__ __forceinline__ uint64_t mix_word(uint64_t h, uint64_t w) {
  h = (h ^ w) * 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 29);
}

__device__ __forceinline__ uint64_t part_value(const Part& p, uint64_t i) {
  switch (p.width) {
    case 1: return p.base[i];
    case 2: return reinterpret_cast<const uint16_t*>(p.base)[i];
    case 4: return reinterpret_cast<const uint32_t*>(p.base)[i];
    default: return reinterpret_cast<const uint64_t*>(p.base)[i];
  }
}

// row i's string: false (and the empty string) when (off, len) does not lie inside the heap
__device__ __forceinline__ bool part_string(const Part& p, uint64_t i, uint64_t& off, uint64_t& len) {
  const int64_t o = p.off[i], l = p.len[i];
  const bool ok = o >= 0 && l >= 0 && (uint64_t)o <= p.heap_n && (uint64_t)l <= p.heap_n - (uint64_t)o;
  off = ok ? (uint64_t)o : 0;
  len = ok ? (uint64_t)l : 0;
  return ok;
}

// 8 bytes of the heap at g, bytes at and past n reading as 0
__device__ __forceinline__ uint64_t heap_word(const uint8_t* __restrict__ heap, uint64_t g, uint64_t n) {
  uint64_t w;
  if (g + 8 <= n) {
    __builtin_memcpy(&w, heap + g, 8);
    return w;
  }
  w = 0;
  for (int b = 0; b < 8; ++b) w |= (uint64_t)(g + b < n ? heap[g + b] : (uint8_t)0) << (8 * b);
  return w;
}

__device__ __forceinline__ uint64_t tail_mask(uint64_t left) { return left < 8 ? (1ull << (8 * left)) - 1 : ~0ull; }

// hash of row i's key; ok cleared when a string part lies outside its heap
__device__ __forceinline__ uint64_t row_hash(const Key& key, uint64_t i, bool& ok) {
  uint64_t h = 0x243F6A8885A308D3ull;
#pragma unroll
  for (int k = 0; k < kMaxParts; ++k) {
    if (k >= key.nparts) break;
    const Part& p = key.part[k];
    if (p.width) {
      h = mix_word(h, part_value(p, i));
      continue;
    }
    uint64_t off, len;
    ok &= part_string(p, i, off, len);
    for (uint64_t q = 0; q < len; q += 8) h = mix_word(h, heap_word(p.base, off + q, p.heap_n) & tail_mask(len - q));
    h = mix_word(h, len);
  }
  return mix64(h);
}

// rows i and r hold the same key, part for part
__device__ __forceinline__ bool rows_equal(const Key& key, uint64_t i, uint64_t r) {
  bool same = true;
#pragma unroll
  for (int k = 0; k < kMaxParts; ++k) {
    if (k >= key.nparts) break;
    const Part& p = key.part[k];
    if (p.width) {
      same &= part_value(p, i) == part_value(p, r);
      continue;
    }
    uint64_t oi, li, orr, lr;
    same &= part_string(p, i, oi, li) & part_string(p, r, orr, lr);
    same &= li == lr;
    for (uint64_t q = 0; same && q < li; q += 8)
      same = ((heap_word(p.base, oi + q, p.heap_n) ^ heap_word(p.base, orr + q, p.heap_n)) & tail_mask(li - q)) == 0;
  }
  return same;
}

__device__ __forceinline__ uint64_t tag_of(uint64_t hash, uint64_t tagmask) {
  const uint64_t t = hash & tagmask;
  return t ? t : 1ull;                            // 0 marks a free slot
}

// home slot from the tag alone, so that equal tags probe alike whatever tagmask kept of the hash
__device__ __forceinline__ uint32_t slot_hash(uint64_t tag) { return ((uint32_t)tag ^ (uint32_t)(tag >> 32)) * 0x9E3779B1u; }

// slot of tag in the global table, inserting it; cap when the table is full (overflow raised)
__device__ __forceinline__ uint64_t global_insert(const GTable& g, uint64_t tag) {
  uint64_t h = g.caplog ? slot_hash(tag) >> (32u - g.caplog) : 0;
  for (uint64_t probe = 0; probe < g.cap; ++probe) {
    const unsigned long long cur = g.tag[h];
    if (cur == tag) return h;
    if (cur == 0) {
      const unsigned long long prev = atomicCAS(&g.tag[h], 0ull, (unsigned long long)tag);
      if (prev == 0) {
        // past half full the probe sequences grow long: give up while they are short
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

// the workgroup's table, carved from dynamic LDS: tag [slots], acc [nagg][slots], row [slots]
template <int kLog>
struct LTable {
  static constexpr uint32_t kSlots = 1u << kLog;
  unsigned long long* tag;
  uint64_t* acc;
  uint32_t* row;            // first row of the tag, relative to the span's first row
  __device__ LTable(unsigned long long* smem, int nagg)
      : tag(smem), acc(reinterpret_cast<uint64_t*>(smem + kSlots)),
        row(reinterpret_cast<uint32_t*>(smem + (size_t)kSlots * (1 + nagg))) {}
};

template <int kLog>
__device__ __forceinline__ void lds_clear(const LTable<kLog>& lt, const Aggs& ag) {
  for (uint32_t s = threadIdx.x; s < lt.kSlots; s += kBlock) {
    lt.tag[s] = 0;
    lt.row[s] = 0xFFFFFFFFu;
#pragma unroll
    for (int a = 0; a < kMaxAggs; ++a)
      if (a < ag.nagg) lt.acc[a * lt.kSlots + s] = identity(ag.op[a]);
  }
}

// the LDS table folded into the global one and cleared; both ends are barriers
template <int kLog>
__device__ void lds_flush(const LTable<kLog>& lt, uint32_t& used, const Aggs& ag, const GTable& g, uint64_t beg) {
  __syncthreads();
  for (uint32_t s = threadIdx.x; s < lt.kSlots; s += kBlock) {
    const uint64_t tag = lt.tag[s];
    if (tag == 0) continue;
    const uint64_t gs = global_insert(g, tag);
    if (gs < g.cap) {
      atomicMin(&g.first[gs], (unsigned long long)(beg + lt.row[s]));
#pragma unroll
      for (int a = 0; a < kMaxAggs; ++a)
        if (a < ag.nagg) combine_atomic(g.acc[a] + gs, lt.acc[a * lt.kSlots + s], ag.op[a]);
    }
    lt.tag[s] = 0;
    lt.row[s] = 0xFFFFFFFFu;
#pragma unroll
    for (int a = 0; a < kMaxAggs; ++a)
      if (a < ag.nagg) lt.acc[a * lt.kSlots + s] = identity(ag.op[a]);
  }
  if (threadIdx.x == 0) {
    used = 0;
    atomicAdd(&g.ctr[FLUSHES], 1u);
  }
  __syncthreads();
}

template <int kLog>
__global__ __launch_bounds__(kBlock) void kh_aggregate_kernel(Key key, uint64_t n, uint64_t span, uint64_t tagmask,
                                                              uint64_t flush_rows, Aggs ag, GTable g) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long kh_smem[];
  __shared__ uint32_t used;
  __shared__ uint32_t ctl[2][2];                // {overflow, used} as of a step's barrier, by step parity
  const LTable<kLog> lt(kh_smem, ag.nagg);
  const uint64_t beg = (uint64_t)blockIdx.x * span;
  if (beg >= n) return;
  const uint64_t end = beg + span < n ? beg + span : n;
  lds_clear(lt, ag);
  if (threadIdx.x == 0) used = 0;
  uint64_t since = 0;                           // rows since the last flush
  uint32_t par = 0;
  for (uint64_t row0 = beg; row0 < end; row0 += kBlock, par ^= 1u) {
    // a step's control words are written two barriers after they were last read (this step's and
    // the one before): one barrier a step is enough
    if (threadIdx.x == 0) {
      ctl[par][0] = __hip_atomic_load(&g.ctr[OVERFLOW], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ctl[par][1] = used;
    }
    __syncthreads();
    if (ctl[par][0]) return;                    // the caller drops the table: nothing left to fold
    if (ctl[par][1] * 2 > lt.kSlots || since >= flush_rows) {
      lds_flush(lt, used, ag, g, beg);
      since = 0;
    }
    since += kBlock;
    const uint64_t i = row0 + threadIdx.x;
    if (i >= end) continue;
    uint64_t val[kMaxAggs];
#pragma unroll
    for (int a = 0; a < kMaxAggs; ++a) val[a] = a < ag.nagg && ag.op[a] != COUNT ? ag.vals[a][i] : 1ull;
    bool ok = true;
    const uint64_t tag = tag_of(row_hash(key, i, ok), tagmask);
    uint32_t h = slot_hash(tag) >> (32u - kLog);
    int slot = -1;
    for (int probe = 0; probe < kLdsProbes; ++probe) {
      const unsigned long long cur = lt.tag[h];
      if (cur == tag) { slot = (int)h; break; }
      if (cur == 0) {
        const unsigned long long prev = atomicCAS(&lt.tag[h], 0ull, (unsigned long long)tag);
        if (prev == 0) atomicAdd(&used, 1u);
        if (prev == 0 || prev == tag) { slot = (int)h; break; }
      }
      h = (h + 1) & (lt.kSlots - 1);
    }
    if (slot >= 0) {
      atomicMin(&lt.row[slot], (uint32_t)(i - beg));
#pragma unroll
      for (int a = 0; a < kMaxAggs; ++a)
        if (a < ag.nagg) combine_atomic(&lt.acc[a * lt.kSlots + slot], val[a], ag.op[a]);
    } else {
      const uint64_t gs = global_insert(g, tag);
      if (gs < g.cap) {
        atomicMin(&g.first[gs], (unsigned long long)i);
#pragma unroll
        for (int a = 0; a < kMaxAggs; ++a)
          if (a < ag.nagg) combine_atomic(g.acc[a] + gs, val[a], ag.op[a]);
      }
    }
  }
  lds_flush(lt, used, ag, g, beg);
}

__global__ __launch_bounds__(kBlock) void kh_verify_kernel(Key key, uint64_t n, uint64_t tagmask, GTable g) {
  if (g.ctr[OVERFLOW]) return;                  // set, if at all, before this kernel started
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    bool ok = true;
    const uint64_t s = global_find(g, tag_of(row_hash(key, i, ok), tagmask));
    if (ok && s < g.cap) {
      const uint64_t r = g.first[s];
      ok = r == i || (r < n && rows_equal(key, i, r));
    } else {
      ok = false;
    }
    if (!ok) atomicOr(&g.ctr[BAD], 1u);
  }
}

// out: int64 [1 + nagg][room]
__global__ __launch_bounds__(kBlock) void kh_emit_kernel(GTable g, int nagg, uint64_t room, int64_t* __restrict__ out) {
  for (uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x; s < g.cap; s += (uint64_t)gridDim.x * kBlock) {
    if (g.tag[s] == 0) continue;
    const uint64_t i = atomicAdd(&g.ctr[EMITTED], 1u);
    if (i >= room) continue;
    out[i] = (int64_t)g.first[s];
#pragma unroll
    for (int a = 0; a < kMaxAggs; ++a)
      if (a < nagg) out[(uint64_t)(1 + a) * room + i] = (int64_t)g.acc[a][s];
  }
}

__global__ __launch_bounds__(kBlock) void kh_tags_kernel(Key key, uint64_t n, uint64_t stride, uint64_t m,
                                                         uint64_t tagmask, int64_t* __restrict__ out) {
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < m; j += (uint64_t)gridDim.x * kBlock) {
    const uint64_t i = j * stride;
    bool ok = true;
    out[j] = i < n ? (int64_t)tag_of(row_hash(key, i, ok), tagmask) : 0;
  }
}

inline bool key_args(Key& key, int nparts, const void* const* base, const void* const* off, const void* const* len,
                     const uint64_t* heap_n, const int* width) {
  if (nparts < 1 || nparts > kMaxParts) return false;
  key.nparts = nparts;
  for (int k = 0; k < kMaxParts; ++k) {
    if (k >= nparts) {
      key.part[k] = Part{nullptr, nullptr, nullptr, 0, 8};
      continue;
    }
    const int w = width[k];
    if (w != 0 && w != 1 && w != 2 && w != 4 && w != 8) return false;
    if (w == 0 ? (off[k] == nullptr || len[k] == nullptr || (base[k] == nullptr && heap_n[k])) : base[k] == nullptr)
      return false;
    key.part[k] = Part{static_cast<const uint8_t*>(base[k]), w ? nullptr : static_cast<const int64_t*>(off[k]),
                       w ? nullptr : static_cast<const int64_t*>(len[k]), w ? 0 : heap_n[k], (uint32_t)w};
  }
  return true;
}

// table: uint64 [2 + nagg][cap] = tags (0), first rows (~0), one accumulator array per aggregate
inline bool table_args(GTable& g, unsigned long long* table, uint64_t cap, int nagg, uint32_t* ctr) {
  if (cap == 0 || (cap & (cap - 1)) || cap > (1ull << 32) || table == nullptr || ctr == nullptr || nagg < 0 ||
      nagg > kMaxAggs)
    return false;
  uint32_t lg = 0;
  while ((1ull << lg) < cap) ++lg;
  g.tag = table;
  g.first = table + cap;
  for (int a = 0; a < kMaxAggs; ++a) g.acc[a] = a < nagg ? reinterpret_cast<uint64_t*>(table + (2 + a) * cap) : nullptr;
  g.cap = cap;
  g.caplog = lg;
  g.ctr = ctr;
  return true;
}

template <int kLog>
int launch_aggregate(const Key& key, uint64_t n, uint64_t span, unsigned blocks, uint64_t tagmask, uint64_t flush_rows,
                     const Aggs& ag, const GTable& g, hipStream_t s) {
  const size_t smem = ((size_t)12 + 8 * ag.nagg) << kLog;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kh_aggregate_kernel<kLog>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  kh_aggregate_kernel<kLog><<<blocks, kBlock, smem, s>>>(key, n, span, tagmask, flush_rows, ag, g);
  DR_LAUNCH_CHECK();
  return 0;
}

}  // namespace

// slots of a workgroup's LDS table for nagg aggregates, rows a workgroup takes per step and the
// least rows of a workgroup's span, for ops/keyhash.py and the tests
DR_API int dr_kh_geometry(int nagg, uint32_t* lds_slots, uint32_t* step_rows, uint32_t* min_span) {
  if (nagg < 0 || nagg > kMaxAggs) return (int)hipErrorInvalidValue;
  *lds_slots = 1u << lds_log(nagg);
  *step_rows = kBlock;
  *min_span = kMinSpan;
  return 0;
}

// The key of row i is part 0 .. nparts - 1: width[k] in {1, 2, 4, 8}: base[k] a column of n such
// values; width[k] == 0: a string, bytes [off[k][i], off[k][i] + len[k][i]) of the heap base[k] of
// heap_n[k] bytes (off, len: int64 [n]).  ops[a] as in hashagg.hip, vals[a] 64-bit columns [n]
// (ignored for COUNT).  table: uint64 [2 + nagg][cap] = tags (0), first rows (~0), accumulators
// (each op's identity); cap a power of two.  ctr: uint32 [8] zeroed (Ctr above).  tagmask: the
// tag bits kept.  flush_rows: rows of a span between forced flushes (0: none).  grid: workgroups
// (0: two a CU, spans of at least kMinSpan rows).
DR_API int dr_kh_aggregate(int nparts, const void* const* base, const void* const* off, const void* const* len,
                           const uint64_t* heap_n, const int* width, uint64_t n, int nagg, const int* ops,
                           const void* const* vals, unsigned long long* table, uint64_t cap, uint32_t* ctr,
                           uint64_t tagmask, uint64_t flush_rows, uint32_t grid, hipStream_t s) {
  Key key;
  GTable g;
  if (!key_args(key, nparts, base, off, len, heap_n, width) || !table_args(g, table, cap, nagg, ctr) ||
      n >= (1ull << 47))
    return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  Aggs ag;
  ag.nagg = nagg;
  for (int a = 0; a < kMaxAggs; ++a) {
    ag.op[a] = a < nagg ? ops[a] : (int)COUNT;
    ag.vals[a] = a < nagg ? static_cast<const uint64_t*>(vals[a]) : nullptr;
    if (a < nagg && (ag.op[a] < SUM_I || ag.op[a] > MAX_F || (ag.op[a] != COUNT && ag.vals[a] == nullptr)))
      return (int)hipErrorInvalidValue;
  }
  uint64_t want = grid;
  if (want == 0) {
    int dev = 0, cus = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    want = 2ull * cus;
  }
  uint64_t span = (n + want - 1) / want;
  if (grid == 0 && span < kMinSpan) span = kMinSpan;
  span = (span + kBlock - 1) / kBlock * kBlock;
  if (span > (1ull << 31)) span = 1ull << 31;          // the LDS table keeps span-relative rows in 32 bits
  const unsigned blocks = (unsigned)((n + span - 1) / span);
  if (flush_rows == 0) flush_rows = ~0ull;
  switch (lds_log(nagg)) {
    case 9: return launch_aggregate<9>(key, n, span, blocks, tagmask, flush_rows, ag, g, s);
    case 10: return launch_aggregate<10>(key, n, span, blocks, tagmask, flush_rows, ag, g, s);
    case 11: return launch_aggregate<11>(key, n, span, blocks, tagmask, flush_rows, ag, g, s);
    default: return launch_aggregate<12>(key, n, span, blocks, tagmask, flush_rows, ag, g, s);
  }
}

DR_API int dr_kh_verify(int nparts, const void* const* base, const void* const* off, const void* const* len,
                        const uint64_t* heap_n, const int* width, uint64_t n, int nagg, unsigned long long* table,
                        uint64_t cap, uint32_t* ctr, uint64_t tagmask, hipStream_t s) {
  Key key;
  GTable g;
  if (!key_args(key, nparts, base, off, len, heap_n, width) || !table_args(g, table, cap, nagg, ctr))
    return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  kh_verify_kernel<<<grid_for(n, kBlock, 4096), kBlock, 0, s>>>(key, n, tagmask, g);
  DR_LAUNCH_CHECK();
  return 0;
}

// out: int64 [1 + nagg][room] = first rows, accumulators; ctr[EMITTED] counts the occupied slots
DR_API int dr_kh_emit(int nagg, unsigned long long* table, uint64_t cap, uint32_t* ctr, uint64_t room, int64_t* out,
                      hipStream_t s) {
  GTable g;
  if (!table_args(g, table, cap, nagg, ctr) || (room && out == nullptr)) return (int)hipErrorInvalidValue;
  if (room == 0) return 0;
  kh_emit_kernel<<<grid_for(cap, kBlock, 4096), kBlock, 0, s>>>(g, nagg, room, out);
  DR_LAUNCH_CHECK();
  return 0;
}

// out[j] = the tag of row j * stride, j < m; (m - 1) * stride < n
DR_API int dr_kh_tags(int nparts, const void* const* base, const void* const* off, const void* const* len,
                      const uint64_t* heap_n, const int* width, uint64_t n, uint64_t stride, uint64_t m,
                      uint64_t tagmask, int64_t* out, hipStream_t s) {
  Key key;
  if (!key_args(key, nparts, base, off, len, heap_n, width) || out == nullptr || stride == 0 ||
      (m && (m - 1) > (n - 1) / stride) || (m && n == 0))
    return (int)hipErrorInvalidValue;
  if (m == 0) return 0;
  kh_tags_kernel<<<grid_for(m, kBlock, 4096), kBlock, 0, s>>>(key, n, stride, m, tagmask, out);
  DR_LAUNCH_CHECK();
  return 0;
}
