// Radix select over E128 sort entries: the kernels behind OrderBy(...).Take(k)
// on the device (dryad_amd/ops/topk.py).
//
// The entries of one table are distinct as unsigned 128-bit numbers (the row index sits in the
// low 32 bits), and their numeric order is the stable OrderBy order.  "The first k rows of the
// sort" is therefore "the k numerically smallest entries": find the k-th smallest value T digit
// by digit from the top, keep every entry below T's bucket at each level, descend into the
// bucket.  The k winners are written unordered; the caller sorts those k entries only.
//
//   dr_topk_hist   : one streaming read.  Histogram of one digit (<= 11 bits at any bit offset of
//                    the 128-bit value) and the bitwise AND and OR of all entries, so the host can
//                    start at the first bit that varies at all.
//   dr_topk_filter : one streaming read of the current candidates.  digit < b_win: a winner, to
//                    out[]; digit == b_cand: a candidate of the next level, to cand[]; and in the
//                    same pass the histogram of the candidates' NEXT digit plus their AND / OR,
//                    so each further level costs one read of its (small) candidate set.
//
// How the work is split: a persistent grid of at most kTkGrid workgroups walks tiles of kTkTile
// entries, kTkPer 16-byte loads per thread issued back to back.  Every wave owns a private copy
// of the 2048-bin histogram in LDS (4 x 8 KB per workgroup, four workgroups per CU); the copies
// are summed once per workgroup into the level's global counters with vector atomics.
//
// Skew: lanes whose digit equals the first active lane's are counted with one ballot and added by
// one lane when they are at least kTkAggMin of the wave.  An all-equal or dominant-value column
// (and the row-index digits of consecutive rows) then costs one LDS atomic per wave instead of 64
// serialised ones; uniform digits pay one ballot and go through the plain per-lane atomics.
//
// Compaction: per tile one packed block scan (winners in the low, candidates in the high 16 bits)
// and one global atomic per workgroup and kind for the write positions, so a 1e9-entry pass does
// ~2e6 atomics on each counter, not one per wave.  Every store is guarded by the buffer's size:
// a histogram that does not count the entries can lose entries (the host checks the counters),
// never write past a buffer.
//
// Level state in global memory (uint32 words): [0, 2048) histogram, [2048, 2052) AND (lo, hi as
// two 64-bit words), [2052, 2056) OR, [2056] candidates written.  The workspace holds a header
// (word 0: winners written) and two such states, so a filter pass can fill the next level's
// while the host still holds the current one.
#include "common.h"

namespace {

// (ops/topk.py exports the geometry as DIGIT_BITS / TILE / GRID: keep the two in step)
constexpr int kTkDigitBits = 11, kTkBins = 1 << kTkDigitBits;
constexpr int kTkPer = 2, kTkTile = kBlock * kTkPer, kTkGrid = 1024;
constexpr int kTkWaves = kBlock / kWave;
constexpr uint32_t kTkAggMin = 16;
constexpr int kStAnd = kTkBins, kStOr = kTkBins + 4, kStCand = kTkBins + 8, kStWords = kTkBins + 16;
constexpr int kHdrWords = 4;
static_assert(kTkTile < (1 << 16), "the packed block scan keeps two 16-bit counts");

// Bits [shift, shift + popcount(mask)) of the 128-bit value; mask has at most 11 low bits set.
__device__ __forceinline__ uint32_t digit_of(const E128& e, int shift, uint32_t mask) {
  uint64_t v;
  if (shift >= 64) v = e.hi >> (shift - 64);
  else if (shift == 0) v = e.lo;
  else v = (e.lo >> shift) | (e.hi << (64 - shift));
  return (uint32_t)v & mask;
}

// Count digit `d` of the lanes with `valid` into the wave's histogram.  Wave-uniform call.
__device__ __forceinline__ void hist_add(uint32_t* __restrict__ h, uint32_t d, bool valid) {
  const uint64_t act = ballot64(valid);
  if (act == 0) return;
  const int first = __ffsll((unsigned long long)act) - 1;
  const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)d, first);
  const uint64_t same = ballot64(valid && d == d0);
  const uint32_t cnt = (uint32_t)__popcll(same);
  if (cnt >= kTkAggMin) {
    if (lane_id() == first) atomicAdd(&h[d0], cnt);
    if (valid && d != d0) atomicAdd(&h[d], 1u);
  } else if (valid) {
    atomicAdd(&h[d], 1u);
  }
}

struct AndOr {
  uint64_t a_lo = ~0ull, a_hi = ~0ull, o_lo = 0, o_hi = 0;
  __device__ __forceinline__ void add(const E128& e) {
    a_lo &= e.lo; a_hi &= e.hi; o_lo |= e.lo; o_hi |= e.hi;
  }
};

__device__ __forceinline__ uint64_t wave_and64(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v &= __shfl_xor(v, d, 64);
  return v;
}

__device__ __forceinline__ uint64_t wave_or64(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v |= __shfl_xor(v, d, 64);
  return v;
}

// The workgroup's wave histograms and AND / OR words into the level state.  All threads call it.
__device__ __forceinline__ void flush_level(uint32_t (*s_hist)[kTkBins], AndOr ao, uint32_t* __restrict__ st) {
  __syncthreads();
  for (int b = threadIdx.x; b < kTkBins; b += kBlock) {
    uint32_t sum = 0;
#pragma unroll
    for (int w = 0; w < kTkWaves; ++w) sum += s_hist[w][b];
    if (sum) atomicAdd(&st[b], sum);
  }
  const uint64_t a_lo = wave_and64(ao.a_lo), a_hi = wave_and64(ao.a_hi);
  const uint64_t o_lo = wave_or64(ao.o_lo), o_hi = wave_or64(ao.o_hi);
  if (lane_id() == 0 && (o_lo | o_hi | ~a_lo | ~a_hi) != 0) {
    unsigned long long* a = reinterpret_cast<unsigned long long*>(st + kStAnd);
    unsigned long long* o = reinterpret_cast<unsigned long long*>(st + kStOr);
    atomicAnd(a, (unsigned long long)a_lo);
    atomicAnd(a + 1, (unsigned long long)a_hi);
    atomicOr(o, (unsigned long long)o_lo);
    atomicOr(o + 1, (unsigned long long)o_hi);
  }
}

__device__ __forceinline__ void clear_hist(uint32_t (*s_hist)[kTkBins]) {
  uint32_t* p = &s_hist[0][0];
  for (int i = threadIdx.x; i < kTkWaves * kTkBins; i += kBlock) p[i] = 0;
  __syncthreads();
}

// Empty level state (AND words all ones); `hdr` non-null: also no winners written yet.
__global__ __launch_bounds__(kBlock) void tk_init_kernel(uint32_t* __restrict__ st, uint32_t* __restrict__ hdr) {
  for (int i = threadIdx.x; i < kStWords; i += kBlock) st[i] = (i >= kStAnd && i < kStOr) ? 0xFFFFFFFFu : 0u;
  if (hdr != nullptr && threadIdx.x < kHdrWords) hdr[threadIdx.x] = 0;
}

__global__ __launch_bounds__(kBlock) void tk_hist_kernel(const E128* __restrict__ src, uint64_t m, int shift,
                                                         uint32_t mask, uint32_t* __restrict__ st) {
  __shared__ uint32_t s_hist[kTkWaves][kTkBins];
  clear_hist(s_hist);
  uint32_t* h = s_hist[wave_id()];
  AndOr ao;
  for (uint64_t base = (uint64_t)blockIdx.x * kTkTile; base < m; base += (uint64_t)gridDim.x * kTkTile) {
    E128 e[kTkPer];
    bool ok[kTkPer];
#pragma unroll
    for (int k = 0; k < kTkPer; ++k) {
      const uint64_t i = base + (uint64_t)k * kBlock + threadIdx.x;
      ok[k] = i < m;
      e[k] = ok[k] ? src[i] : E128{0, 0};
    }
#pragma unroll
    for (int k = 0; k < kTkPer; ++k) {
      if (ok[k]) ao.add(e[k]);
      hist_add(h, digit_of(e[k], shift, mask), ok[k]);
    }
  }
  flush_level(s_hist, ao, st);
}

__global__ __launch_bounds__(kBlock) void tk_filter_kernel(const E128* __restrict__ src, uint64_t m, int shift,
                                                           uint32_t mask, uint32_t b_win, uint32_t b_cand,
                                                           E128* __restrict__ out, uint32_t out_cap,
                                                           uint32_t* __restrict__ out_count, E128* __restrict__ cand,
                                                           uint32_t cand_cap, int nshift, uint32_t nmask,
                                                           uint32_t* __restrict__ nst) {
  __shared__ uint32_t s_hist[kTkWaves][kTkBins];
  __shared__ uint32_t s_scan[4];
  __shared__ uint32_t s_base[2];
  clear_hist(s_hist);
  uint32_t* h = s_hist[wave_id()];
  AndOr ao;
  for (uint64_t base = (uint64_t)blockIdx.x * kTkTile; base < m; base += (uint64_t)gridDim.x * kTkTile) {
    E128 e[kTkPer];
    bool win[kTkPer], cnd[kTkPer];
    uint32_t packed = 0;                       // winners | candidates << 16 of this thread
#pragma unroll
    for (int k = 0; k < kTkPer; ++k) {
      const uint64_t i = base + (uint64_t)k * kBlock + threadIdx.x;
      const bool ok = i < m;
      e[k] = ok ? src[i] : E128{0, 0};
      const uint32_t d = digit_of(e[k], shift, mask);
      win[k] = ok && d < b_win;
      cnd[k] = ok && d == b_cand;
      packed += (win[k] ? 1u : 0u) + (cnd[k] ? 0x10000u : 0u);
    }
    uint32_t total;
    const uint32_t ex = block_exclusive_scan256(packed, s_scan, total);
    if (total != 0) {                          // (the same in every thread)
      if (threadIdx.x == 0) {
        s_base[0] = (total & 0xFFFFu) ? atomicAdd(out_count, total & 0xFFFFu) : 0u;
        s_base[1] = (total >> 16) ? atomicAdd(nst + kStCand, total >> 16) : 0u;
      }
      __syncthreads();
      uint64_t wpos = (uint64_t)s_base[0] + (ex & 0xFFFFu), cpos = (uint64_t)s_base[1] + (ex >> 16);
#pragma unroll
      for (int k = 0; k < kTkPer; ++k) {
        if (win[k]) {
          if (wpos < out_cap) out[wpos] = e[k];
          ++wpos;
        }
        if (cnd[k]) {
          if (cpos < cand_cap) cand[cpos] = e[k];
          ++cpos;
          ao.add(e[k]);
        }
      }
#pragma unroll
      for (int k = 0; k < kTkPer; ++k) hist_add(h, digit_of(e[k], nshift, nmask), cnd[k]);
    }
  }
  flush_level(s_hist, ao, nst);
}

inline bool digit_ok(int shift, int bits) { return shift >= 0 && bits >= 1 && bits <= kTkDigitBits && shift + bits <= 128; }

inline uint32_t* state_of(void* ws, int slot) { return static_cast<uint32_t*>(ws) + kHdrWords + slot * kStWords; }

}  // namespace

// Bytes of the workspace: the header and two level states.
DR_API uint64_t dr_topk_workspace(void) { return (uint64_t)(kHdrWords + 2 * kStWords) * sizeof(uint32_t); }

// Level state `slot` := histogram of digit [shift, shift + bits) and AND / OR of src[0, m).
// `first`: a new selection starts (no winners written yet).
DR_API int dr_topk_hist(const E128* src, uint64_t m, int shift, int bits, void* ws, int slot, int first,
                        hipStream_t s) {
  if (m == 0 || m >= (1ull << 32) || !digit_ok(shift, bits) || (slot & ~1) || ws == nullptr)
    return (int)hipErrorInvalidValue;
  uint32_t* st = state_of(ws, slot);
  tk_init_kernel<<<1, kBlock, 0, s>>>(st, first ? static_cast<uint32_t*>(ws) : nullptr);
  DR_LAUNCH_CHECK();
  tk_hist_kernel<<<grid_for(m, kTkTile, kTkGrid), kBlock, 0, s>>>(src, m, shift, (1u << bits) - 1u, st);
  DR_LAUNCH_CHECK();
  return 0;
}

// One level: entries of src[0, m) with digit [shift, shift + bits) < b_win are appended to
// out[0, out_cap) (position from the header's counter), those with digit == b_cand to
// cand[0, cand_cap) (b_cand >= 2048: none, cand may be null); level state `nslot` := histogram of
// the candidates' digit [nshift, nshift + nbits), their AND / OR and their count.
// `first`: a new selection starts.
DR_API int dr_topk_filter(const E128* src, uint64_t m, int shift, int bits, uint32_t b_win, uint32_t b_cand,
                          E128* out, uint64_t out_cap, E128* cand, uint64_t cand_cap, int nshift, int nbits,
                          void* ws, int nslot, int first, hipStream_t s) {
  if (m == 0 || m >= (1ull << 32) || !digit_ok(shift, bits) || (nslot & ~1) || ws == nullptr ||
      out_cap >= (1ull << 32) || cand_cap >= (1ull << 32))
    return (int)hipErrorInvalidValue;
  const bool cands = b_cand < (uint32_t)kTkBins;
  if (cands && (cand == nullptr || !digit_ok(nshift, nbits))) return (int)hipErrorInvalidValue;
  if (out == nullptr && out_cap != 0) return (int)hipErrorInvalidValue;
  uint32_t* st = state_of(ws, nslot);
  tk_init_kernel<<<1, kBlock, 0, s>>>(st, first ? static_cast<uint32_t*>(ws) : nullptr);
  DR_LAUNCH_CHECK();
  tk_filter_kernel<<<grid_for(m, kTkTile, kTkGrid), kBlock, 0, s>>>(
      src, m, shift, (1u << bits) - 1u, b_win, cands ? b_cand : 0xFFFFFFFFu, out, (uint32_t)out_cap,
      static_cast<uint32_t*>(ws), cands ? cand : nullptr, cands ? (uint32_t)cand_cap : 0u, cands ? nshift : 0,
      cands ? (1u << nbits) - 1u : 0u, st);
  DR_LAUNCH_CHECK();
  return 0;
}
