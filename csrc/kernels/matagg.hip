// Low-cardinality GroupBy on the matrix cores (K6 / K11): exact integer Count / Sum / Min / Max
// for a key column whose values come from a dictionary of D <= 256 keys, with no atomic on the
// per-row path of the sums (dryad_amd/ops/matagg.py; the hash path is hashagg.hip).
//
// Count and sums are one matrix product per 64 rows on v_mfma_i32_16x16x64_i8:
//
//     acc[group][column] += onehot[group][row] * limb[row][column]            (i8 x i8 -> i32)
//
// onehot[g][r] = 1 when row r's key is dictionary entry g.  The columns are the 8 bytes ("limbs")
// of each sum column side by side, then one column that is 1 for every row found in the
// dictionary (the count): 8 * nsum + 1 <= 25 columns in 1 or 2 column tiles of 16.  MFMA i8 is
// signed, so limbs 0..6 are stored as byte ^ 0x80 (= byte - 128) and limb 7, the sign limb, as it
// is; the epilogue adds 128 * count back per biased limb.  Sum = sum_j limbsum_j << 8j in wrapping
// int64, which is what torch and the hash path compute.
//
// How the work is split.  A workgroup is 4 waves; every wave owns one contiguous slice of rows
// and walks it in steps of kChunks chunks of 64 rows (lane = row), all of a step's loads issued
// before the first use.  Per row: the key is looked up in a read-only open-addressing table in
// LDS that the workgroup built once from the dictionary (empty slots are marked in the id field,
// so every int64, INT64_MIN too, is a legal key); a key that is not there is a miss: its one-hot
// is all zero and its row index goes to the miss list, one global atomic per wave and step.  Min
// and max read the group's current value from an LDS table and issue the LDS atomic only when
// the row improves it.
//
// Transposition: through LDS, not v_perm_b32.  A lane holds one row's int64 (row-major); the
// MFMA wants, per lane, one limb column of 16 rows.  Each lane stores its 8 limbs as 8 byte
// stores into a per-wave strip laid out [column][row], so a limb column of 16 rows is one
// 16-byte LDS read; the ids and the found-bytes are two more columns of the same strip.  A
// v_perm_b32 network would still have to move bytes between 16 lanes (DPP or ds_bpermute per
// word), which is the same LDS crossbar with more instructions.
//
// Operand invariant (all this file relies on; no k-ordering of the instruction is assumed): the
// contraction runs over rows, and lane (q = lane / 16, i = lane % 16) feeds A row i and B column
// i with 16 bytes each for the instruction's k-slots of lane group q.  Here byte p of BOTH
// operands of lane group q names row 16 q + p of the chunk: A is built from strip[ids][16q + p],
// B is strip[column][16q + p].  Any pairing of (q, p) with k is then the same sum.  Only the
// result layout is used: register r of lane (q, i) is D[row 4q + r][column i].
//
// Overflow: |limb| <= 128 and a one-hot entry is <= 1, so a wave adds its i32 accumulators into
// the workgroup's int64 LDS table after at most flush_rows <= 2^24 rows (128 * 2^24 = 2^31 is
// reached only by -128, which fits).  The accumulators, up to 16 group tiles x 2 column tiles x
// 4 registers, stay in registers: kernels are specialised on the tile counts (group tiles
// rounded up to a power of two, tiles past ceil(D / 16) skipped by a wave-uniform test in the
// unrolled loop).  The workgroup table goes to the global result with one atomic per
// (workgroup, group, column), limbs already recombined and the bias added.
#include "common.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaMaxGroups = 256, kMaMaxSums = 3, kMaMaxMm = 4;
constexpr int kChunks = 4;                        // 64-row chunks per wave step
constexpr int kMaWaves = kBlock / kWave;
constexpr int kDictSlots = 512;                   // load factor <= 1/2
constexpr uint32_t kNoId = 0xFFFFFFFFu;           // empty slot, marked in the id field
constexpr uint64_t kLimbBias = 0x0080808080808080ull;   // limbs 0..6 are stored ^ 0x80
constexpr uint32_t kMaxFlushRows = 1u << 24;

struct MaArgs {
  const int64_t* keys;
  const int64_t* dict;            // [D] distinct keys
  const int64_t* sums[kMaMaxSums];
  const int64_t* mm[kMaMaxMm];
  int mm_is_max[kMaMaxMm];
  unsigned long long* out;        // [1 + nsum + nmm][D]: count, sums (zeroed), min / max (identity)
  uint32_t* miss_rows;            // [miss_cap]
  uint32_t* miss_count;           // rows missed (may pass miss_cap: then the list is incomplete)
  uint64_t n, per_wave;           // per_wave is a multiple of 64
  uint32_t miss_cap, flush_rows;
  int D, nsum, nmm;
};

__device__ __forceinline__ uint32_t dict_hash(uint64_t k) {
  return (((uint32_t)k ^ (uint32_t)(k >> 32)) * 0x9E3779B1u) >> 23;       // 9 bits
}

// 0x01 in every byte of x that is zero, 0x00 elsewhere (exact: no carry crosses a byte).
__device__ __forceinline__ uint32_t zero_bytes(uint32_t x) {
  const uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
  return (~(t | x | 0x7F7F7F7Fu)) >> 7;
}

// LDS layout (bytes), every part 16-byte aligned.
__host__ __device__ constexpr size_t ma_strip_cols(int nsum) { return 8 * (size_t)nsum + 2; }
__host__ __device__ constexpr size_t ma_lds_bytes(int gtiles, int nsum, int nmm) {
  return (size_t)kDictSlots * 12 + (size_t)gtiles * 16 * (nsum + 1 + nmm) * 8 +
         (size_t)kMaWaves * kChunks * ma_strip_cols(nsum) * 64;
}

template <int GTM, int CT>
__global__ __launch_bounds__(kBlock, (GTM * CT >= 16 ? 1 : 2)) void matagg_kernel(const MaArgs a) {
  constexpr int NSM = CT == 1 ? 1 : kMaMaxSums;   // sums that fit CT column tiles
  extern __shared__ __attribute__((aligned(16))) unsigned char ma_smem[];
  const int D = a.D, nsum = a.nsum, nmm = a.nmm;
  const int gt = (D + 15) >> 4, G = gt * 16, tabw = nsum + 1;
  unsigned long long* dkey = reinterpret_cast<unsigned long long*>(ma_smem);        // [kDictSlots]
  unsigned long long* tab = dkey + kDictSlots;                                      // [G][nsum + 1]
  long long* mmt = reinterpret_cast<long long*>(tab + G * tabw);                    // [nmm][G]
  uint32_t* did = reinterpret_cast<uint32_t*>(mmt + nmm * G);                       // [kDictSlots]
  unsigned char* strips = reinterpret_cast<unsigned char*>(did + kDictSlots);
  const int tid = threadIdx.x, l = lane_id(), w = wave_id(), q = l >> 4, i = l & 15;
  const int ncol = 8 * nsum, idcol = ncol + 1;    // strip columns: limbs, found (= count), ids
  const int chunk_bytes = (ncol + 2) * 64;
  unsigned char* strip = strips + (size_t)w * kChunks * chunk_bytes;

  for (int s = tid; s < kDictSlots; s += kBlock) did[s] = kNoId;
  for (int s = tid; s < G * tabw; s += kBlock) tab[s] = 0ull;
  for (int s = tid; s < nmm * G; s += kBlock)
    mmt[s] = a.mm_is_max[s / G] ? (long long)0x8000000000000000ull : 0x7FFFFFFFFFFFFFFFll;
  __syncthreads();
  if (tid < D) {                                  // the dictionary's keys are distinct
    const unsigned long long k = (unsigned long long)a.dict[tid];
    uint32_t h = dict_hash(k);
    while (atomicCAS(&did[h], kNoId, (uint32_t)tid) != kNoId) h = (h + 1) & (kDictSlots - 1);
    dkey[h] = k;
  }
  __syncthreads();

  i32x4 acc[GTM][CT];
#pragma unroll
  for (int t = 0; t < GTM; ++t)
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[t][c] = i32x4{0, 0, 0, 0};

  // wave partials -> the workgroup's int64 table: register r of lane (q, i) of tile (t, c) is
  // group 16 t + 4 q + r, column 16 c + i
  auto flush = [&]() {
#pragma unroll
    for (int t = 0; t < GTM; ++t) {
      if (t < gt) {
#pragma unroll
        for (int c = 0; c < CT; ++c) {
          const int col = 16 * c + i;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int v = acc[t][c][r];
            if (v != 0 && col <= ncol) {
              const int g = 16 * t + 4 * q + r;
              const unsigned long long add = (unsigned long long)(long long)v;
              if (col == ncol) atomicAdd(&tab[g * tabw + nsum], add);
              else atomicAdd(&tab[g * tabw + (col >> 3)], add << (8 * (col & 7)));
            }
          }
          acc[t][c] = i32x4{0, 0, 0, 0};
        }
      }
    }
  };

  const uint64_t wv = (uint64_t)blockIdx.x * kMaWaves + w;
  const uint64_t beg = wv * a.per_wave < a.n ? wv * a.per_wave : a.n;
  const uint64_t end = beg + a.per_wave < a.n ? beg + a.per_wave : a.n;
  uint32_t held = 0;                              // rows in the accumulators since the last flush

  for (uint64_t base = beg; base < end; base += 64 * kChunks) {
    const int nch = end - base >= 64 * kChunks ? kChunks : (int)((end - base + 63) >> 6);
    unsigned long long key[kChunks], sv[kChunks][NSM];
    long long mv[kChunks][kMaMaxMm];
    bool live[kChunks], miss[kChunks];
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {           // every load of the step first
      const uint64_t row = base + 64 * c + l;
      live[c] = row < end;
      key[c] = live[c] ? (unsigned long long)__builtin_nontemporal_load(a.keys + row) : 0ull;
#pragma unroll
      for (int s = 0; s < NSM; ++s)
        sv[c][s] = (s < nsum && live[c]) ? (unsigned long long)__builtin_nontemporal_load(a.sums[s] + row) : 0ull;
#pragma unroll
      for (int m = 0; m < kMaMaxMm; ++m)
        mv[c][m] = (m < nmm && live[c]) ? __builtin_nontemporal_load(a.mm[m] + row) : 0ll;
    }
    uint32_t nmiss = 0, before[kChunks];
    uint64_t mbal[kChunks];
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
      uint32_t id = kNoId;
      if (live[c]) {
        uint32_t h = dict_hash(key[c]);
        for (;;) {                                // plain LDS reads; ends at an empty slot
          const uint32_t e = did[h];
          if (e == kNoId) break;
          if (dkey[h] == key[c]) { id = e; break; }
          h = (h + 1) & (kDictSlots - 1);
        }
      }
      const bool found = id != kNoId;
      miss[c] = live[c] && !found;
      mbal[c] = ballot64(miss[c]);
      before[c] = nmiss;
      nmiss += (uint32_t)__popcll(mbal[c]);
      if (c < nch) {
        unsigned char* sc = strip + c * chunk_bytes;
        sc[idcol * 64 + l] = (unsigned char)id;
        sc[ncol * 64 + l] = found ? 1 : 0;        // masks the one-hot and is the count column
#pragma unroll
        for (int s = 0; s < NSM; ++s) {
          if (s < nsum) {
            const unsigned long long x = sv[c][s] ^ kLimbBias;
#pragma unroll
            for (int j = 0; j < 8; ++j) sc[(8 * s + j) * 64 + l] = (unsigned char)(x >> (8 * j));
          }
        }
      }
#pragma unroll
      for (int m = 0; m < kMaMaxMm; ++m) {
        if (m < nmm && found) {
          long long* p = &mmt[m * G + (int)id];
          const long long cur = *p, x = mv[c][m];
          if (a.mm_is_max[m]) { if (x > cur) atomicMax(p, x); }
          else if (x < cur) atomicMin(p, x);
        }
      }
    }
    if (nmiss) {                                  // one global atomic per wave step
      uint32_t at = 0;
      if (l == 0) at = atomicAdd(a.miss_count, nmiss);
      at = (uint32_t)__builtin_amdgcn_readfirstlane((int)at);
#pragma unroll
      for (int c = 0; c < kChunks; ++c) {
        const uint64_t pos = (uint64_t)at + before[c] + popc_below(mbal[c]);
        if (miss[c] && pos < a.miss_cap) a.miss_rows[pos] = (uint32_t)(base + 64 * c + l);
      }
    }
    // the strip is private to the wave: its stores above are read by other lanes below
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    for (int c = 0; c < nch; ++c) {
      if (held + 64 > a.flush_rows) { flush(); held = 0; }
      held += 64;
      const unsigned char* sc = strip + c * chunk_bytes;
      const uint4 idw = *reinterpret_cast<const uint4*>(sc + idcol * 64 + 16 * q);
      const uint4 fw = *reinterpret_cast<const uint4*>(sc + ncol * 64 + 16 * q);
      i32x4 b[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const int col = 16 * ct + i;              // past the count column: a zero column
        const uint4 x = *reinterpret_cast<const uint4*>(sc + (col <= ncol ? col : ncol) * 64 + 16 * q);
        const uint32_t keep = col <= ncol ? 0xFFFFFFFFu : 0u;
        b[ct] = i32x4{(int)(x.x & keep), (int)(x.y & keep), (int)(x.z & keep), (int)(x.w & keep)};
      }
#pragma unroll
      for (int t = 0; t < GTM; ++t) {
        if (t < gt) {
          const uint32_t tgt = (uint32_t)(16 * t + i) * 0x01010101u;
          const i32x4 oh = i32x4{(int)(zero_bytes(idw.x ^ tgt) & fw.x), (int)(zero_bytes(idw.y ^ tgt) & fw.y),
                                 (int)(zero_bytes(idw.z ^ tgt) & fw.z), (int)(zero_bytes(idw.w ^ tgt) & fw.w)};
#pragma unroll
          for (int ct = 0; ct < CT; ++ct)
            acc[t][ct] = __builtin_amdgcn_mfma_i32_16x16x64_i8(oh, b[ct], acc[t][ct], 0, 0, 0);
        }
      }
    }
    // the next step's stores must not pass this step's reads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  flush();
  __syncthreads();

  for (int g = tid; g < D; g += kBlock) {         // one atomic per (workgroup, group, column)
    const unsigned long long cnt = tab[g * tabw + nsum];
    if (cnt == 0) continue;
    atomicAdd(&a.out[g], cnt);
    for (int s = 0; s < nsum; ++s) atomicAdd(&a.out[(size_t)(1 + s) * D + g], tab[g * tabw + s] + cnt * kLimbBias);
    for (int m = 0; m < nmm; ++m) {
      long long* o = reinterpret_cast<long long*>(a.out) + (size_t)(1 + nsum + m) * D + g;
      if (a.mm_is_max[m]) atomicMax(o, mmt[m * G + g]);
      else atomicMin(o, mmt[m * G + g]);
    }
  }
}

template <int GTM, int CT>
int ma_launch(const MaArgs& a, unsigned grid, size_t smem, hipStream_t s) {
  hipFuncSetAttribute(reinterpret_cast<const void*>(matagg_kernel<GTM, CT>),
                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  matagg_kernel<GTM, CT><<<grid, kBlock, smem, s>>>(a);
  DR_LAUNCH_CHECK();
  return 0;
}

template <int CT>
int ma_dispatch(int gt, const MaArgs& a, unsigned grid, size_t smem, hipStream_t s) {
  if (gt <= 1) return ma_launch<1, CT>(a, grid, smem, s);
  if (gt <= 2) return ma_launch<2, CT>(a, grid, smem, s);
  if (gt <= 4) return ma_launch<4, CT>(a, grid, smem, s);
  if (gt <= 8) return ma_launch<8, CT>(a, grid, smem, s);
  return ma_launch<16, CT>(a, grid, smem, s);
}

}  // namespace

// Rows per wave step and waves per workgroup (ops/matagg.py sizes its test grids from them).
DR_API int dr_matagg_step_rows() { return 64 * kChunks; }
DR_API int dr_matagg_waves() { return kMaWaves; }

// keys [n] int64; dict [D] distinct int64, 1 <= D <= 256; sums[s] / mm[m] int64 columns [n];
// mm_is_max[m] != 0 for a max.  out [1 + nsum + nmm][D] int64: row 0 counts and rows 1..nsum sums,
// zeroed by the caller, then the min / max rows preset to their identity.  miss_rows [miss_cap]
// uint32 and *miss_count (zeroed): the rows whose key is not in dict; more than miss_cap misses
// leave the list incomplete and the count right.  64 <= flush_rows <= 2^24; grid 0 = pick one.
DR_API int dr_matrix_aggregate(const int64_t* keys, uint64_t n, const int64_t* dict, int D, int nsum,
                               const void* const* sums, int nmm, const void* const* mm, const int* mm_is_max,
                               void* out, uint32_t* miss_rows, uint32_t miss_cap, uint32_t* miss_count,
                               uint32_t flush_rows, uint32_t grid, hipStream_t s) {
  if (D < 1 || D > kMaMaxGroups || nsum < 0 || nsum > kMaMaxSums || nmm < 0 || nmm > kMaMaxMm ||
      flush_rows < 64 || flush_rows > kMaxFlushRows || n >= (1ull << 32))
    return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  MaArgs a{};
  a.keys = keys;
  a.dict = dict;
  for (int i = 0; i < nsum; ++i) a.sums[i] = reinterpret_cast<const int64_t*>(sums[i]);
  for (int i = 0; i < nmm; ++i) {
    a.mm[i] = reinterpret_cast<const int64_t*>(mm[i]);
    a.mm_is_max[i] = mm_is_max[i] != 0;
  }
  a.out = reinterpret_cast<unsigned long long*>(out);
  a.miss_rows = miss_rows;
  a.miss_cap = miss_cap;
  a.miss_count = miss_count;
  a.n = n;
  a.flush_rows = flush_rows;
  a.D = D;
  a.nsum = nsum;
  a.nmm = nmm;
  if (grid == 0) {                                // a few workgroups per CU, a full step per wave at least
    int dev = 0, cus = 256;
    hipGetDevice(&dev);
    hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    grid = grid_for(n, 64 * kChunks * kMaWaves, (unsigned)cus * 4);
  }
  const uint64_t waves = (uint64_t)grid * kMaWaves;
  a.per_wave = ((n + waves - 1) / waves + 63) & ~63ull;
  const int gt = (D + 15) / 16;
  const size_t smem = ma_lds_bytes(gt, nsum, nmm);
  return nsum <= 1 ? ma_dispatch<1>(gt, a, grid, smem, s) : ma_dispatch<2>(gt, a, grid, smem, s);
}
