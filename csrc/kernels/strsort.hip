// Exact, stable ordering of variable-length byte strings on the device: the
// kernels behind OrderBy / RangePartition over string keys (dryad_amd/ops/strsort.py).
//
// Order: unsigned byte-wise lexicographic over the UTF-8 bytes, a proper prefix first (Python's
// str order, which the LocalDebug oracle uses); equal strings keep their input order, ascending
// and descending alike.
//
//   dr_str_window_keys : one E128 sort entry per string, its 96 key bits
//                          depth 0 : [11 window bytes, big-endian, zero padded | valid byte count]
//                          later   : [32-bit run id | 7 window bytes | valid byte count]
//                        and the row index in the low 32 bits.  (padded bytes, count) orders
//                        "a" < "a\0" without a terminator symbol; descending complements window
//                        and count, never the run id.  The entries then go through the stable
//                        E128 sort of sort.hip over bits [32, 128).
//   dr_str_boundaries  : per sorted entry, bit 0 = its key bits differ from its predecessor's
//                        (run start), bit 1 = the window held fewer valid bytes than its width
//                        (every string of the run is consumed: the run is equal strings, already
//                        in stable order); also unpacks the row indices.
//   dr_str_finish      : LDS finisher.  Runs of strings that tie on every byte seen so far are
//                        ranked inside one workgroup by the strings' remaining bytes; a run too
//                        long for its owner's window is flagged for another window-key pass.
//   dr_str_range_dest  : destination partition of each string among <= 255 separator strings.
//
// Finisher design (ownership scheme of seg_sort_kernel in sort.hip): a workgroup of 256 threads
// owns the runs that START in its core of 1024 positions and reads 256 positions more, so a run
// spilling past the core is finished by its owner.  For every member of an owned, unfinished run
// it stages in LDS the address and length of the string's remainder past the known common depth
// and the next 16 bytes as two big-endian words.  Rank of x in its run = #(y < x) + #(y == x, y
// before x); lanes of a wave walk the same run in lockstep, so the LDS reads are mostly
// broadcasts.  Two words decide almost every comparison; only a tie on all 16 staged bytes of two
// strings that both go on walks the heap.  Positions are rewritten in place inside the run, which
// no other workgroup reads.
//
// Heap reads never leave [off, off + len), clipped to the heap size as well: 8-byte loads where
// the address is aligned and 8 valid bytes remain, single bytes otherwise.
#include "common.h"

namespace {

// (ops/strsort.py exports the geometry as FIN_CORE / FIN_EXT: keep the two in step)
constexpr int kFinCore = 1024, kFinExt = 256, kFinWin = kFinCore + kFinExt, kFinPer = kFinWin / 256;  // 5
constexpr uint32_t kStaged = 16;

// Valid bytes of string (off, len) from `depth` on, clipped to the heap; p = heap index of the first.
__device__ __forceinline__ uint64_t remainder_of(int64_t off, int64_t len, uint64_t depth, uint64_t heap_n,
                                                 uint64_t& p) {
  p = 0;
  if (off < 0 || len <= 0 || (uint64_t)len <= depth) return 0;
  const uint64_t q = (uint64_t)off + depth;
  if (q >= heap_n) return 0;
  p = q;
  const uint64_t r = (uint64_t)len - depth;
  return r < heap_n - q ? r : heap_n - q;
}

// Bytes a[0, cnt), cnt <= 8, big-endian from the top byte down, zero padded.
__device__ __forceinline__ uint64_t load_be(const uint8_t* __restrict__ a, uint32_t cnt) {
  if (cnt >= 8 && (((uintptr_t)a) & 7) == 0) return __builtin_bswap64(*reinterpret_cast<const uint64_t*>(a));
  uint64_t v = 0;
#pragma unroll
  for (uint32_t k = 0; k < 8; ++k)
    if (k < cnt) v |= (uint64_t)a[k] << (56 - 8 * k);
  return v;
}

// The next 16 bytes of a remainder as two big-endian words.
__device__ __forceinline__ void load_staged(const uint8_t* __restrict__ a, uint64_t rem, uint64_t& w0, uint64_t& w1) {
  const uint32_t c = rem < kStaged ? (uint32_t)rem : kStaged;
  w0 = c ? load_be(a, c < 8 ? c : 8) : 0ull;
  w1 = c > 8 ? load_be(a + 8, c - 8) : 0ull;
}

// Order of remainders a[0, ra) and b[0, rb) that agree on their first 16 bytes (ra, rb > 16).
__device__ __forceinline__ int compare_tails(const uint8_t* __restrict__ a, uint64_t ra, const uint8_t* __restrict__ b,
                                             uint64_t rb) {
  const uint64_t m = ra < rb ? ra : rb;
  uint64_t k = kStaged;
  if (((((uintptr_t)(a + k)) | ((uintptr_t)(b + k))) & 7) == 0) {
    for (; k + 8 <= m; k += 8) {
      const uint64_t x = __builtin_bswap64(*reinterpret_cast<const uint64_t*>(a + k));
      const uint64_t y = __builtin_bswap64(*reinterpret_cast<const uint64_t*>(b + k));
      if (x != y) return x < y ? -1 : 1;
    }
  }
  for (; k < m; ++k) {
    const uint8_t x = a[k], y = b[k];
    if (x != y) return x < y ? -1 : 1;
  }
  return ra < rb ? -1 : (ra > rb ? 1 : 0);
}

// Order of two remainders from their staged words; equal padded words with a remainder that ends
// inside them mean one is a prefix of the other: the shorter is first.
__device__ __forceinline__ int compare_staged(uint64_t a0, uint64_t a1, const uint8_t* __restrict__ a, uint64_t ra,
                                              uint64_t b0, uint64_t b1, const uint8_t* __restrict__ b, uint64_t rb) {
  if (a0 != b0) return a0 < b0 ? -1 : 1;
  if (a1 != b1) return a1 < b1 ? -1 : 1;
  if (ra > kStaged && rb > kStaged) return compare_tails(a, ra, b, rb);
  return ra < rb ? -1 : (ra > rb ? 1 : 0);
}

__global__ __launch_bounds__(256) void window_keys_kernel(const uint8_t* __restrict__ heap, uint64_t heap_n,
                                                          const int64_t* __restrict__ off,
                                                          const int64_t* __restrict__ len,
                                                          const int64_t* __restrict__ rows,
                                                          const int64_t* __restrict__ rid, uint64_t depth, int desc,
                                                          uint64_t m, E128* __restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t row = rows ? (uint64_t)rows[i] : i;
    uint64_t p;
    const uint64_t rem = remainder_of(off[row], len[row], depth, heap_n, p);
    E128 e;
    if (rid == nullptr) {                      // 11 window bytes + count
      const uint32_t c = rem < 11 ? (uint32_t)rem : 11u;
      const uint64_t w0 = c ? load_be(heap + p, c < 8 ? c : 8) : 0ull;
      const uint64_t w1 = c > 8 ? load_be(heap + p + 8, c - 8) : 0ull;
      e.hi = w0;
      e.lo = (w1 & 0xFFFFFF0000000000ull) | ((uint64_t)c << 32);
      if (desc) {
        e.hi = ~e.hi;
        e.lo ^= 0xFFFFFFFF00000000ull;
      }
    } else {                                   // run id + 7 window bytes + count
      const uint32_t c = rem < 7 ? (uint32_t)rem : 7u;
      const uint64_t w = c ? load_be(heap + p, c) : 0ull;
      e.hi = ((uint64_t)rid[i] << 32) | (w >> 32);
      e.lo = ((w << 32) & 0xFFFFFF0000000000ull) | ((uint64_t)c << 32);
      if (desc) {
        e.hi ^= 0xFFFFFFFFull;
        e.lo ^= 0xFFFFFFFF00000000ull;
      }
    }
    e.lo |= row & 0xFFFFFFFFull;
    out[i] = e;
  }
}

__global__ __launch_bounds__(256) void boundaries_kernel(const E128* __restrict__ srt, uint64_t m, uint32_t width,
                                                         int desc, int64_t* __restrict__ rows,
                                                         uint8_t* __restrict__ flags) {
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (uint64_t)gridDim.x * blockDim.x) {
    const E128 e = srt[j];
    bool start = j == 0;
    if (!start) {
      const E128 q = srt[j - 1];
      start = q.hi != e.hi || (q.lo >> 32) != (e.lo >> 32);
    }
    uint32_t c = (uint32_t)(e.lo >> 32) & 0xFFu;
    if (desc) c ^= 0xFFu;
    flags[j] = (uint8_t)((start ? 1u : 0u) | (c < width ? 2u : 0u));
    rows[j] = (int64_t)(e.lo & 0xFFFFFFFFull);
  }
}

__global__ __launch_bounds__(256) void finish_kernel(const uint8_t* __restrict__ heap, uint64_t heap_n,
                                                     const int64_t* __restrict__ off, const int64_t* __restrict__ len,
                                                     int64_t* __restrict__ rows, const uint8_t* __restrict__ flags,
                                                     uint8_t* __restrict__ long_start, uint64_t depth, int desc,
                                                     uint64_t m) {
  __shared__ uint64_t s_w0[kFinWin], s_w1[kFinWin];   // the 16 staged bytes
  __shared__ uint64_t s_ptr[kFinWin], s_rem[kFinWin]; // heap index and length of the remainder
  __shared__ uint32_t s_row[kFinWin];
  __shared__ uint16_t rid_of[kFinWin];
  __shared__ uint16_t rstart[kFinWin + 1];
  __shared__ uint8_t s_flag[kFinWin];
  __shared__ uint32_t sc[4];
  const int t = threadIdx.x;
  const uint64_t c0 = (uint64_t)blockIdx.x * kFinCore;
  if (c0 >= m) return;
  const uint32_t core = (uint32_t)((m - c0) < (uint64_t)kFinCore ? (m - c0) : kFinCore);
  const uint64_t wend = (c0 + kFinWin) < m ? c0 + kFinWin : m;
  const uint32_t L = (uint32_t)(wend - c0);
#pragma unroll
  for (int k = 0; k < kFinPer; ++k) {
    const uint32_t i = t + k * 256;
    if (i < L) s_flag[i] = flags[c0 + i];
  }
  // the window's last run goes on past it unless the next position starts a run
  const bool open_end = wend < m && (flags[wend] & 1u) == 0;
  __syncthreads();
  uint32_t f = 0;
#pragma unroll
  for (int k = 0; k < kFinPer; ++k) {
    const uint32_t p = t * kFinPer + k;
    if (p < L && (s_flag[p] & 1u)) f |= 1u << k;
  }
  uint32_t nruns;
  const uint32_t base = block_exclusive_scan256((uint32_t)__popc(f), sc, nruns);
  uint32_t id = base;
#pragma unroll
  for (int k = 0; k < kFinPer; ++k) {
    const uint32_t p = t * kFinPer + k;
    if (p < L) {
      if (f & (1u << k)) { rstart[id] = (uint16_t)p; ++id; }
      rid_of[p] = (uint16_t)(id - 1);   // 0xFFFF: run started before this window
    }
  }
  if (t == 0) rstart[nruns] = (uint16_t)L;
  __syncthreads();
  // stage the members of owned runs that still need an order: not a single string, not consumed,
  // ending inside the window
  uint32_t todo = 0;
#pragma unroll
  for (int k = 0; k < kFinPer; ++k) {
    const uint32_t p = t + k * 256;
    if (p >= L) continue;
    const uint32_t r = rid_of[p];
    if (r == 0xFFFFu) continue;
    const uint32_t rs = rstart[r];
    if (rs >= core) continue;                       // owned by the next workgroup
    if (s_flag[rs] & 2u) continue;                  // equal, fully consumed strings
    if (open_end && r + 1 == nruns) {               // long run: another window-key pass
      if (p == rs) long_start[c0 + rs] = 1;
      continue;
    }
    if (rstart[r + 1] - rs == 1) continue;
    const uint64_t row = (uint64_t)rows[c0 + p];
    uint64_t q;
    const uint64_t rem = remainder_of(off[row], len[row], depth, heap_n, q);
    uint64_t w0, w1;
    load_staged(heap + q, rem, w0, w1);
    s_row[p] = (uint32_t)row;
    s_ptr[p] = q;
    s_rem[p] = rem;
    s_w0[p] = w0;
    s_w1[p] = w1;
    todo |= 1u << k;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kFinPer; ++k) {
    if (!(todo & (1u << k))) continue;
    const uint32_t p = t + k * 256;
    const uint32_t r = rid_of[p];
    const uint32_t rs = rstart[r], re = rstart[r + 1];
    const uint64_t x0 = s_w0[p], x1 = s_w1[p], rx = s_rem[p];
    const uint8_t* px = heap + s_ptr[p];
    // rank = #{y in run : (y, j) < (x, p)} in the requested direction
    uint32_t cnt = 0;
    for (uint32_t j = rs; j < re; ++j) {
      int c = compare_staged(s_w0[j], s_w1[j], heap + s_ptr[j], s_rem[j], x0, x1, px, rx);
      if (desc) c = -c;
      cnt += (c < 0 || (c == 0 && j < p)) ? 1u : 0u;
    }
    rows[c0 + rs + cnt] = (int64_t)s_row[p];
  }
}

__global__ __launch_bounds__(256) void range_dest_kernel(const uint8_t* __restrict__ heap, uint64_t heap_n,
                                                         const int64_t* __restrict__ off,
                                                         const int64_t* __restrict__ len, uint64_t n,
                                                         const uint8_t* __restrict__ sheap, uint64_t sheap_n,
                                                         const int64_t* __restrict__ soff,
                                                         const int64_t* __restrict__ slen, uint32_t nsep, int desc,
                                                         uint32_t max_dest, int32_t* __restrict__ dest) {
  __shared__ uint64_t s_w0[256], s_w1[256], s_ptr[256], s_rem[256];
  for (uint32_t k = threadIdx.x; k < nsep; k += blockDim.x) {
    uint64_t q, w0, w1;
    const uint64_t rem = remainder_of(soff[k], slen[k], 0, sheap_n, q);
    load_staged(sheap + q, rem, w0, w1);
    s_ptr[k] = q;
    s_rem[k] = rem;
    s_w0[k] = w0;
    s_w1[k] = w1;
  }
  __syncthreads();
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t q, x0, x1;
    const uint64_t rx = remainder_of(off[i], len[i], 0, heap_n, q);
    const uint8_t* px = heap + q;
    load_staged(px, rx, x0, x1);
    // count of separators "before" the key: below it (ascending) or above it (descending)
    uint32_t lo = 0, hi = nsep;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      const int c = compare_staged(s_w0[mid], s_w1[mid], sheap + s_ptr[mid], s_rem[mid], x0, x1, px, rx);
      const bool before = desc ? c > 0 : c < 0;
      lo = before ? mid + 1 : lo;
      hi = before ? hi : mid;
    }
    dest[i] = (int32_t)(lo < max_dest ? lo : max_dest);
  }
}

}  // namespace

DR_API int dr_str_window_keys(const uint8_t* heap, uint64_t heap_n, const int64_t* off, const int64_t* len,
                              const int64_t* rows, const int64_t* rid, uint64_t depth, int descending, uint64_t m,
                              E128* out, hipStream_t s) {
  if (m == 0) return 0;
  if (m >= (1ull << 32)) return (int)hipErrorInvalidValue;
  window_keys_kernel<<<grid_for(m, 256, 16384), 256, 0, s>>>(heap, heap_n, off, len, rows, rid, depth, descending, m,
                                                             out);
  DR_LAUNCH_CHECK();
  return 0;
}

DR_API int dr_str_boundaries(const E128* sorted, uint64_t m, uint32_t width, int descending, int64_t* rows,
                             uint8_t* flags, hipStream_t s) {
  if (m == 0) return 0;
  boundaries_kernel<<<grid_for(m, 256, 16384), 256, 0, s>>>(sorted, m, width, descending, rows, flags);
  DR_LAUNCH_CHECK();
  return 0;
}

// `long_start` (zeroed by the caller) gets a 1 at the first position of every run left untouched.
DR_API int dr_str_finish(const uint8_t* heap, uint64_t heap_n, const int64_t* off, const int64_t* len, int64_t* rows,
                         const uint8_t* flags, uint8_t* long_start, uint64_t depth, int descending, uint64_t m,
                         hipStream_t s) {
  if (m == 0) return 0;
  const uint64_t g = (m + kFinCore - 1) / kFinCore;
  finish_kernel<<<(unsigned)g, 256, 0, s>>>(heap, heap_n, off, len, rows, flags, long_start, depth, descending, m);
  DR_LAUNCH_CHECK();
  return 0;
}

DR_API int dr_str_range_dest(const uint8_t* heap, uint64_t heap_n, const int64_t* off, const int64_t* len, uint64_t n,
                             const uint8_t* sep_heap, uint64_t sep_heap_n, const int64_t* sep_off,
                             const int64_t* sep_len, uint32_t nsep, int descending, uint32_t max_dest, int32_t* dest,
                             hipStream_t s) {
  if (nsep > 255) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  range_dest_kernel<<<grid_for(n, 256, 16384), 256, 0, s>>>(heap, heap_n, off, len, n, sep_heap, sep_heap_n, sep_off,
                                                            sep_len, nsep, descending, max_dest, dest);
  DR_LAUNCH_CHECK();
  return 0;
}
