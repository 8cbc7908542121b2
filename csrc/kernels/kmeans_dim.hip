// k-means step on the bf16 plane for any point dimension 1 <= D <= 512 and 1 <= K <= 1024 (gfx950).
//
// kmeans.hip is compiled for D = 128.  This file generalises its K-tiled plane path
// (kmeans_assign_tiled_kernel: points stationary in registers, split centroids streamed through
// LDS) along the D axis; D = 128 itself keeps running kmeans.hip.
//
//   plane       xh = bf16(x) as [n, DP] with DP = 32 NS >= D, zero in the pad, and |x| per point,
//               written once per point table (kmd_plane_kernel).  NS, the number of k-steps of
//               v_mfma_f32_16x16x32_bf16, is one of 1, 2, 3, 4, 6, 8, 12, 16: a D between two widths
//               takes the next one (the extra dims are zeros and cost plane bytes only).  The plane
//               pitch is a multiple of 64 bytes, so the 16-byte fragment loads are aligned for any D.
//   f32 rows    stay at their natural pitch D, which is not 16-byte aligned when D % 4 != 0: every
//               kernel here that reads them reads dwords with lanes across dims (coalesced).
//   assignment  kmd_assign_kernel<NS>: one 16-point tile per wave, NS bf16x8 per lane, 16 centroids
//               per LDS chunk, d ~ |c|^2 - 2 xh.(ch + cm); near ties flagged in bit 31 of assign.
//   re-rank     kmd_rerank_kernel: exact f32 fma distances of the flagged points to all K centroids.
//   sums        kmd_movers_kernel<SW>: f64 [K][SW] LDS slab per dimension slice; the f32 rows of
//               the points whose cluster changed move between the kept f64 sums.
//
// Lane map of the 16x16x32 bf16 MFMA (lane l, r = l & 15, g = l >> 4): A[row r][k = 8 g + j],
// B[k = 8 g + j][col r], C col = r, row = 4 g + reg.  A = centroids, B = points: lane (r, g) ends up
// with the distances of point r to centroids 4 g .. 4 g + 3 of the 16-centroid sub-tile.
#include "common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxD = 512;
constexpr int kMaxK = 1024;
constexpr int kAsWaves = 8;   // waves per assignment workgroup

// Geometry of the assignment kernel for NS k-steps.
//
// LDS row pitch.  A centroid row is DP bf16 plus 16 bf16 of padding: 16 NS + 8 dwords, i.e.
// 8 (mod 16) dwords for every NS.  A ds_read_b128 is served per group of 16 lanes, 8 consecutive
// rows r at two adjacent 16-byte columns g (the grouping DR_KM_CROW in kmeans.hip was measured
// with: its 136-bf16 pitch, 4 (mod 64) dwords, showed 2-way conflicts, 144 none).  Lane (r, g) of
// a group reads dwords P r + 16 s + 4 g .. + 3.  With P = 8 m, m odd, P r mod 64 runs over the 8
// distinct multiples of 8 for r = 0 .. 7 (m is invertible mod 8), and 4 g adds 0 or 4 (mod 8) for
// the two columns: 16 distinct 4-bank sets covering all 64 banks, for every NS and every s.
//
// T = 1 tile per wave and CB = 16 centroids (one sub-tile) per chunk for every NS: at most 64
// VGPRs of point data for the block in work and the same again for the prefetch, and two chunk
// buffers of at most 33856 bytes each.  The template carries T and CB through, but only this
// geometry is built: with T = 2 or 4 tiles per wave (CB = 32 or 64), at every NS tried, a step on
// an MI355X returned now and then (4 to 40 of 40 steps, by shape) a 16-point tile with the
// distance to one centroid, always number 13 or 29 of its 32, far too small; with T = 1 none of
// 560 steps over 14 shapes did.  The cause is not found, so a lane's fragments serve one tile.
template <int NS>
struct Geo {
  static constexpr int DP = 32 * NS;
  static constexpr int ROW = DP + 16;                         // bf16 per LDS centroid row
  static constexpr int CB = 16;
  static constexpr int NSUB = CB / 16;                        // 16-centroid sub-tiles per chunk
  static constexpr int BYTES = 2 * CB * ROW * 2 + CB * 4;     // [ch CB x ROW][cm CB x ROW][|c|^2 CB]
  static constexpr int UNITS = BYTES / 16;
  static constexpr int SUBU = UNITS / NSUB;                   // staged under one sub-tile's MFMAs
  static constexpr int T = 1;
  static_assert(BYTES % 16 == 0 && UNITS % NSUB == 0 && (ROW * 2) % 16 == 0, "chunk image must be b128-copyable");
  static_assert(T * NS <= 16 && 2 * BYTES <= 2 * 37120, "register / LDS budget");
};

// Instantiated plane width for D (0: out of range).
__host__ __device__ constexpr int ns_for(int d) {
  if (d < 1 || d > kMaxD) return 0;
  const int ns = (d + 31) / 32;
  return ns <= 4 ? ns : ns <= 6 ? 6 : ns <= 8 ? 8 : ns <= 12 ? 12 : 16;
}

struct GeoRt {
  int ns, dp, row, cb, bytes;
};

GeoRt geo_rt(int d) {
  const int ns = ns_for(d);
  switch (ns) {
#define DR_GEO(N) case N: return GeoRt{N, Geo<N>::DP, Geo<N>::ROW, Geo<N>::CB, Geo<N>::BYTES}
    DR_GEO(1); DR_GEO(2); DR_GEO(3); DR_GEO(4); DR_GEO(6); DR_GEO(8); DR_GEO(12); DR_GEO(16);
#undef DR_GEO
  }
  return GeoRt{0, 0, 0, 0, 0};
}

// Near-tie bound.  The estimate of x.c is fl(sum xh_i ch_i + xh_i cm_i) over DP dims.  Against the
// exact x.c, relative to sum |x_i c_i| <= |x| |c|:
//   xh rounding    |x_i - xh_i| <= 2^-9 |x_i| (bf16 keeps 8 significand bits)             2^-9
//   cm residual    |c_i - ch_i - cm_i| <= 2^-9 2^-9 |c_i|, plus the cross terms of the
//                  two roundings and the f32 rounding of |x|: all below                     2^-16
//   accumulation   the bf16 products are exact in f32; 2 DP of them are added with at most
//                  one ulp (2^-23, covering a truncating adder) each                        2 DP 2^-23
// d = |c|^2 - 2 x.c doubles it:  |d_est - d| <= kmd_tol(DP) |x| max|c| + 2^-20 max|c|^2, where the
// second term covers what does not scale with |x|: the f32 rounding of |c|^2 (one rounding of an
// f64 sum here, 2^-24 |c|^2) and of the final fma (2^-24 (|c|^2 + 2 |x| |c|)).  Two estimates can
// swap order only when they are closer than twice that, so such points are flagged and re-ranked.
// At DP = 128 kmd_tol is 3.998e-3, the kKmTolH of kmeans.hip.
__host__ __device__ constexpr float kmd_tol(int dp) {
  return 2.f * (0x1p-9f + 0x1p-16f + (float)dp * 0x1p-22f);
}
constexpr float kKmdTolC = 0x1p-20f;

// |c|^2 per centroid, accumulated in f64 and rounded once.
__global__ __launch_bounds__(64) void kmd_norms_kernel(const float* __restrict__ C, int K, int D,
                                                       float* __restrict__ out) {
  const int j = blockIdx.x;
  double s = 0.0;
  for (int d = threadIdx.x; d < D; d += 64) {
    const double v = (double)C[(uint64_t)j * D + d];
    s += v * v;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  if (threadIdx.x == 0) out[j] = (float)s;
}

// The plane: LP = 32 or 64 lanes per point (64 / LP points per wave instruction), lane dl walks
// dims dl, dl + LP, ... of the padded row; the f32 row is read as dwords at pitch D.
__global__ __launch_bounds__(256) void kmd_plane_kernel(const float* __restrict__ X, uint64_t n, int D, int DP,
                                                        __bf16* __restrict__ XH, float* __restrict__ xnorm) {
  const int LP = DP < 64 ? 32 : 64;
  const int PPW = 64 / LP;
  const int l = threadIdx.x & 63, dl = l & (LP - 1), sub = l / LP;
  const uint64_t nw = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const uint64_t groups = (n + PPW - 1) / PPW;
  for (uint64_t q = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; q < groups; q += nw) {
    const uint64_t p = q * PPW + sub;
    const bool ok = p < n;
    float ss = 0.f;
    for (int d = dl; d < DP; d += LP) {
      const float v = (ok && d < D) ? X[p * D + d] : 0.f;
      ss = fmaf(v, v, ss);
      if (ok) XH[p * DP + d] = (__bf16)v;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const float o = __shfl_xor(ss, m, 64);
      if (m < LP) ss += o;
    }
    if (ok && dl == 0) xnorm[p] = sqrtf(ss);
  }
}

// Split centroids c = ch + cm in the byte image of an LDS chunk (see Geo), one workgroup per chunk;
// rows past K and dims past D are zero, |c|^2 past K is +inf.  cmax = sqrt(max |c|^2) follows the
// last chunk.  Staging a chunk is then a straight 16-byte-per-lane copy.
__global__ __launch_bounds__(256) void kmd_cprep_kernel(const float* __restrict__ C, const float* __restrict__ cnorm,
                                                        int K, int D, int ROW, int CB, int BYTES,
                                                        unsigned char* __restrict__ cws) {
  __shared__ float wmax[4];
  const int j = blockIdx.x, t = threadIdx.x;
  __bf16* chi = reinterpret_cast<__bf16*>(cws + (size_t)j * BYTES);
  __bf16* cmd = chi + CB * ROW;
  float* cn = reinterpret_cast<float*>(cmd + CB * ROW);
  for (int i = t; i < CB * ROW; i += 256) {
    const int c = CB * j + i / ROW, d = i % ROW;
    const float v = (c < K && d < D) ? C[(uint64_t)c * D + d] : 0.f;
    const __bf16 vh = (__bf16)v;
    chi[i] = vh;
    cmd[i] = (__bf16)(v - (float)vh);
  }
  if (t < CB) cn[t] = CB * j + t < K ? cnorm[CB * j + t] : __builtin_inff();
  if (j == 0) {
    float m = 0.f;
    for (int c = t; c < K; c += 256) m = fmaxf(m, cnorm[c]);
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) m = fmaxf(m, __shfl_xor(m, x, 64));
    if ((t & 63) == 0) wmax[t >> 6] = m;
    __syncthreads();
    if (t == 0)
      *reinterpret_cast<float*>(cws + (size_t)gridDim.x * BYTES) =
          sqrtf(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3])));
  }
}

// Assignment.  A workgroup of 8 waves owns a block of 16 T 8 points: every wave keeps T 16-point
// tiles of the plane in registers (lane (r, g): dims 32 s + 8 g .. + 7 of point r, s < NS) and the
// workgroup walks the ceil(K / CB) centroid chunks.  Per 16-centroid sub-tile and 32-dim slice the
// ah / am fragments are read from LDS once and feed 2 T MFMAs.  Chunks are double-buffered: a
// sub-tile's share of chunk j + 1 is fetched into registers before the sub-tile's MFMAs and stored
// to the other buffer after them, one barrier per chunk; the chunk sequence runs on across point
// blocks, so the pipeline never drains.  When all K centroids fit one chunk (MULTI = false) it is
// staged once and the loop neither copies nor synchronises.  Best, runner-up and index are carried
// per lane over all chunks and merged over the 4 lanes of a point once per block.  The next block's
// tiles are requested at the top of a block and land under its MFMAs.
template <int NS, bool MULTI>
__global__ __launch_bounds__(64 * kAsWaves) void kmd_assign_kernel(const __bf16* __restrict__ XH,
                                                                   const float* __restrict__ xnorm, uint64_t n,
                                                                   const uint4* __restrict__ cws,
                                                                   const float* __restrict__ cmax_p, int K,
                                                                   int32_t* __restrict__ assign) {
  using G = Geo<NS>;
  constexpr int T = G::T, W = kAsWaves, NT = 64 * W, DP = G::DP, ROW = G::ROW, CB = G::CB;
  constexpr int NQ = (G::SUBU + NT - 1) / NT;
  constexpr uint64_t PB = 16 * T * W;
  constexpr float kTol2 = 2.f * kmd_tol(DP), kTolC2 = 2.f * kKmdTolC;
  __shared__ uint4 cbuf[2 * G::UNITS];
  const int t = threadIdx.x, w = t >> 6, l = t & 63, r = l & 15, g = l >> 4;
  const int nch = (K + CB - 1) / CB;
  for (int i = t; i < G::UNITS; i += NT) cbuf[i] = cws[i];
  const float cmax = *cmax_p;
  __syncthreads();
  struct Pts {
    bf16x8 x[NS];
    float xn;
  };
  const uint64_t blocks = (n + PB - 1) / PB;
  // clamped rows: a point past n re-reads point n - 1 and stores nothing
  auto load = [&](uint64_t blk, Pts* d) {
#pragma unroll
    for (int tt = 0; tt < T; ++tt) {
      const uint64_t p = min(blk * PB + (uint64_t)((w * T + tt) * 16 + r), n - 1);
#pragma unroll
      for (int s_ = 0; s_ < NS; ++s_) d[tt].x[s_] = *reinterpret_cast<const bf16x8*>(XH + p * DP + 32 * s_ + 8 * g);
      d[tt].xn = xnorm[p];
    }
  };
  Pts cur[T], nxt[T];
  if ((uint64_t)blockIdx.x < blocks) load(blockIdx.x, cur);
  int par = 0;
  for (uint64_t blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
    // compiler barrier: keeps the single chunk's fragment reads inside the loop (hoisted, they
    // would take the registers of the prefetch)
    asm volatile("" ::: "memory");
    const uint64_t nb = blk + gridDim.x;
    load(nb < blocks ? nb : blk, nxt);
    float bd[T], sd[T];
    int bj[T];
#pragma unroll
    for (int tt = 0; tt < T; ++tt) {
      bd[tt] = __builtin_inff();
      sd[tt] = __builtin_inff();
      bj[tt] = 0;
    }
#pragma unroll 1
    for (int j = 0; j < nch; ++j) {
      const int jn = j + 1 < nch ? j + 1 : 0;
      const uint4* src = cws + (size_t)jn * G::UNITS;
      uint4* dst = cbuf + (par ^ 1) * G::UNITS;
      const __bf16* chi = reinterpret_cast<const __bf16*>(cbuf + par * G::UNITS);
      const __bf16* cmd = chi + CB * ROW;
      const float* cn = reinterpret_cast<const float*>(cmd + CB * ROW);
#pragma unroll 1
      for (int ct = 0; ct < G::NSUB; ++ct) {
        uint4 st[NQ];
        if constexpr (MULTI) {
#pragma unroll
          for (int q = 0; q < NQ; ++q) st[q] = src[ct * G::SUBU + min(t + NT * q, G::SUBU - 1)];
        }
        f32x4 Dt[T];
#pragma unroll
        for (int tt = 0; tt < T; ++tt) Dt[tt] = f32x4{};
#pragma unroll
        for (int s_ = 0; s_ < NS; ++s_) {
          const bf16x8 ah = *reinterpret_cast<const bf16x8*>(chi + (ct * 16 + r) * ROW + 32 * s_ + 8 * g);
          const bf16x8 am = *reinterpret_cast<const bf16x8*>(cmd + (ct * 16 + r) * ROW + 32 * s_ + 8 * g);
#pragma unroll
          for (int tt = 0; tt < T; ++tt) {
            Dt[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, cur[tt].x[s_], Dt[tt], 0, 0, 0);
            Dt[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, cur[tt].x[s_], Dt[tt], 0, 0, 0);
          }
          // the fragments stay live past the k-step's last MFMA, so no accumulator is allocated on
          // the registers an MFMA still in flight reads as its A operand
          asm volatile("" ::"v"(ah), "v"(am));
          // T = 1: nothing else separates the k-steps, and the scheduler would issue all 2 NS
          // fragment reads first (128 more registers at NS = 16); let it look 4 k-steps ahead
          if constexpr (NS > 8)
            if (s_ % 4 == 3) __builtin_amdgcn_sched_barrier(0);
        }
        const float4 cv = *reinterpret_cast<const float4*>(cn + ct * 16 + 4 * g);
        const float cc[4] = {cv.x, cv.y, cv.z, cv.w};
#pragma unroll
        for (int tt = 0; tt < T; ++tt)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int c = CB * j + ct * 16 + 4 * g + q;
            const float d = fmaf(-2.f, Dt[tt][q], cc[q]);
            sd[tt] = fminf(sd[tt], fmaxf(bd[tt], d));
            bj[tt] = d < bd[tt] ? c : bj[tt];
            bd[tt] = fminf(bd[tt], d);
          }
        if constexpr (MULTI) {
#pragma unroll
          for (int q = 0; q < NQ; ++q) {
            const int i = t + NT * q;
            if (i < G::SUBU) dst[ct * G::SUBU + i] = st[q];
          }
        }
      }
      if constexpr (MULTI) {
        __syncthreads();
        par ^= 1;
      }
    }
#pragma unroll
    for (int tt = 0; tt < T; ++tt) {
      float b = bd[tt], s2 = sd[tt];
      int bi = bj[tt];
#pragma unroll
      for (int m = 16; m <= 32; m <<= 1) {
        const float obd = __shfl_xor(b, m, 64), osd = __shfl_xor(s2, m, 64);
        const int obj = __shfl_xor(bi, m, 64);
        if (obd < b || (obd == b && obj < bi)) {
          s2 = fminf(b, osd);
          b = obd;
          bi = obj;
        } else {
          s2 = fminf(s2, obd);
        }
      }
      const uint64_t p = blk * PB + (uint64_t)((w * T + tt) * 16 + r);
      const bool near = K > 1 && (s2 - b) <= fmaf(kTol2 * cur[tt].xn, cmax, kTolC2 * cmax * cmax);
      if (g == 0 && p < n) assign[p] = near ? (int32_t)((uint32_t)bi | 0x80000000u) : bi;
    }
#pragma unroll
    for (int tt = 0; tt < T; ++tt) cur[tt] = nxt[tt];
  }
}

// Zeroes the near-tie count + pad (4 words) before a step (a kernel, so that a captured step
// resets it on every replay like an eager run does).
__global__ void kmd_near_reset(uint32_t* __restrict__ near_cnt) {
  if (threadIdx.x < 4) near_cnt[threadIdx.x] = 0u;
}

// Lists the points flagged near-tie (bit 31 of assign) as (point, estimate) pairs and clears the
// flag; capacity n entries, writes past it are dropped.
__global__ __launch_bounds__(256) void kmd_near_list(int32_t* __restrict__ assign, uint64_t n,
                                                     uint32_t* __restrict__ near_cnt, uint32_t* __restrict__ near_list) {
  for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x; b < n; b += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t p = b + threadIdx.x;
    const int32_t a = p < n ? assign[p] : 0;
    const bool near = a < 0;
    const uint64_t m = __ballot(near);
    if (m) {
      const int l = threadIdx.x & 63;
      const int first = __builtin_ctzll(m);
      uint32_t base = 0;
      if (l == first) base = atomicAdd(near_cnt, (uint32_t)__popcll(m));
      base = __shfl(base, first, 64);
      if (near) {
        const uint32_t o = base + popc_below(m);
        const uint32_t est = (uint32_t)a & 0x7FFFFFFFu;
        if (o < n) {
          near_list[2 * (uint64_t)o] = (uint32_t)p;
          near_list[2 * (uint64_t)o + 1] = est;
        }
        assign[p] = (int32_t)est;
      }
    }
  }
}

__global__ __launch_bounds__(256) void kmd_copy_assign(const int32_t* __restrict__ assign, uint64_t n,
                                                       int32_t* __restrict__ prev) {
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (uint64_t)gridDim.x * blockDim.x)
    prev[p] = assign[p];
}

// Exact f32 re-rank of the listed points for any D and K: one wave per P listed points.  Their f32
// rows are staged in LDS with lanes across dims (dword reads at pitch D); lane l then scans
// centroids l, l + 64, ... with two fma accumulators (even / odd dims), the point values broadcast
// from LDS, and keeps its best (lowest index on ties); a 6-step butterfly merges the lanes.  A
// centroid value fetched by a lane serves P points.  Corrects assign only.
template <int P>
__global__ __launch_bounds__(64) void kmd_rerank_kernel(const float* __restrict__ X, const float* __restrict__ C,
                                                        const float* __restrict__ cnorm, int K, int D,
                                                        const uint32_t* __restrict__ near_cnt,
                                                        const uint32_t* __restrict__ near_list,
                                                        int32_t* __restrict__ assign, uint64_t n) {
  __shared__ float xs[P][kMaxD];
  const uint32_t total = (uint64_t)*near_cnt < n ? *near_cnt : (uint32_t)n;
  const int l = threadIdx.x;
  for (uint64_t i0 = (uint64_t)blockIdx.x * P; i0 < total; i0 += (uint64_t)gridDim.x * P) {
    uint64_t p[P];
    int est[P], bj[P];
    float d[P];
    __syncthreads();   // the previous group's readers are done with xs
#pragma unroll
    for (int u = 0; u < P; ++u) {
      // a short last group repeats its last entry (the same value is stored twice)
      const uint64_t i = i0 + u < total ? i0 + u : total - 1;
      p[u] = near_list[2 * i];
      est[u] = (int)near_list[2 * i + 1];
      d[u] = __builtin_inff();
      bj[u] = l;
      for (int k = l; k < D; k += 64) xs[u][k] = X[p[u] * D + k];
    }
    __syncthreads();
    for (int c = l; c < K; c += 64) {
      const float* cr = C + (uint64_t)c * D;
      float a0[P], a1[P];
#pragma unroll
      for (int u = 0; u < P; ++u) a0[u] = a1[u] = 0.f;
      int k = 0;
      for (; k + 1 < D; k += 2) {
        const float c0 = cr[k], c1 = cr[k + 1];
#pragma unroll
        for (int u = 0; u < P; ++u) {
          a0[u] = fmaf(xs[u][k], c0, a0[u]);
          a1[u] = fmaf(xs[u][k + 1], c1, a1[u]);
        }
      }
      if (k < D) {
        const float c0 = cr[k];
#pragma unroll
        for (int u = 0; u < P; ++u) a0[u] = fmaf(xs[u][k], c0, a0[u]);
      }
      const float cnc = cnorm[c];
#pragma unroll
      for (int u = 0; u < P; ++u) {
        const float dc = cnc - 2.f * (a0[u] + a1[u]);
        if (dc < d[u]) { d[u] = dc; bj[u] = c; }
      }
    }
#pragma unroll
    for (int u = 0; u < P; ++u) {
      float du = d[u];
      int bu = bj[u];
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        const float od = __shfl_xor(du, m, 64);
        const int oj = __shfl_xor(bu, m, 64);
        if (od < du || (od == du && oj < bu)) { du = od; bu = oj; }
      }
      if (l == 0 && bu != est[u]) assign[p[u]] = bu;
    }
  }
}

// Movers for any D and K: grid (blocks, ceil(D / SW)), a workgroup keeps the f64 [K][SW] slab of
// dimension slice blockIdx.y (the last slice may be ragged: dims >= D are neither read nor
// flushed).  A slab row belongs to one wave (row & 3) and, when a row is narrower than a wave, to
// one of its 64 / SW lane groups ((row >> 2) % G), so every update is a plain f64
// read-modify-write by the lanes that own those words: G rows per wave instruction, a lane per
// dimension (dword reads of the f32 rows).  Each lane group walks its own ballot of the 64-point
// sub-batch.  prev is only read here (the slices of a batch run concurrently); kmd_copy_assign
// brings it up to date afterwards.  Slice 0 keeps the counts.
template <int SW>
__global__ __launch_bounds__(256) void kmd_movers_kernel(const float* __restrict__ X, uint64_t n, int D,
                                                         const int32_t* __restrict__ assign,
                                                         const int32_t* __restrict__ prev, int K,
                                                         double* __restrict__ S, long long* __restrict__ cnt) {
  extern __shared__ __attribute__((aligned(16))) double kmd_slab[];   // [K][SW]
  int* dcnt = reinterpret_cast<int*>(kmd_slab + (size_t)K * SW);      // [K]
  int* cur_s = dcnt + K;                                              // [256]
  int* old_s = cur_s + 256;                                           // [256]
  constexpr int LW = SW < 64 ? SW : 64;   // lanes per row
  constexpr int G = 64 / LW;              // rows per wave instruction
  constexpr int NV = SW / LW;             // dims per lane
  constexpr int U = 8;                    // rows in flight per lane group
  const int t = threadIdx.x, w = t >> 6, l = t & 63, gi = l / LW, dl = l % LW;
  const int d0 = blockIdx.y * SW;
  bool dok[NV];
#pragma unroll
  for (int e = 0; e < NV; ++e) dok[e] = d0 + dl + 64 * e < D;
  for (int i = t; i < K * SW; i += 256) kmd_slab[i] = 0.0;
  for (int i = t; i < K; i += 256) dcnt[i] = 0;
  for (uint64_t b = (uint64_t)blockIdx.x * 256; b < n; b += (uint64_t)gridDim.x * 256) {
    const uint64_t p = b + t;
    int a = -1, o = -1;
    if (p < n) {
      a = assign[p];
      o = prev[p];
    }
    __syncthreads();   // the previous batch's readers are done with cur_s / old_s (and the zeroing)
    cur_s[t] = a;
    old_s[t] = o;
    __syncthreads();
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {
      const int ca = cur_s[64 * c + l], co = old_s[64 * c + l];
      const bool mv = ca != co;
      uint64_t madd = 0, msub = 0;
#pragma unroll 1
      for (int own = 0; own < G; ++own) {
        const uint64_t ma = ballot64(mv && ca >= 0 && (ca & 3) == w && ((ca >> 2) % G) == own);
        const uint64_t ms = ballot64(mv && co >= 0 && (co & 3) == w && ((co >> 2) % G) == own);
        if (gi == own) {
          madd = ma;
          msub = ms;
        }
      }
      while (__any((madd | msub) != 0)) {
        int idx[U], row[U];
        double sgn[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          idx[u] = 0;
          row[u] = -1;
          sgn[u] = 0.0;
          if (madd) {
            idx[u] = __builtin_ctzll(madd);
            madd &= madd - 1;
            row[u] = cur_s[64 * c + idx[u]];
            sgn[u] = 1.0;
          } else if (msub) {
            idx[u] = __builtin_ctzll(msub);
            msub &= msub - 1;
            row[u] = old_s[64 * c + idx[u]];
            sgn[u] = -1.0;
          }
        }
        float v[U][NV];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          // a listed idx is a point of this sub-batch (< n); unlisted entries read nothing
          const float* xr = X + (b + 64 * c + idx[u]) * D + d0 + dl;
#pragma unroll
          for (int e = 0; e < NV; ++e) v[u][e] = (row[u] >= 0 && dok[e]) ? xr[64 * e] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (row[u] >= 0) {
            double* dst = kmd_slab + (size_t)row[u] * SW + dl;
#pragma unroll
            for (int e = 0; e < NV; ++e) dst[64 * e] += sgn[u] * (double)v[u][e];
            if (blockIdx.y == 0 && dl == 0) dcnt[row[u]] += sgn[u] > 0 ? 1 : -1;
          }
        }
      }
    }
  }
  __syncthreads();
  for (int i = t; i < K * SW; i += 256) {
    const double v = kmd_slab[i];
    const int d = d0 + i % SW;
    if (v != 0.0 && d < D) atomicAdd(S + (uint64_t)(i / SW) * D + d, v);
  }
  if (blockIdx.y == 0)
    for (int i = t; i < K; i += 256)
      if (dcnt[i]) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + i), (unsigned long long)(long long)dcnt[i]);
}

// The blob generator of kmeans.hip for any d (it depends on d only through e / d, e % d).  Every
// multiply and add is rounded on its own, as numpy rounds them: contraction is switched off for
// the kernel body (the __fmul_rn / __fadd_rn wrappers are plain operators that the compiler may
// still fuse into an fma, one rounding instead of two), so models/kmeans_cpu.gen_points
// reproduces it bit for bit.
__device__ __forceinline__ float kmd_u01(uint64_t z) { return (float)(mix64(z) >> 40) * (1.0f / 16777216.0f); }

__global__ __launch_bounds__(256) void kmd_gen_kernel(float* __restrict__ X, uint64_t n, uint64_t dim, uint64_t first,
                                                      int blobs, uint64_t seed) {
#pragma clang fp contract(off)
  for (uint64_t e =(uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n * dim; e += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = e / dim + first;
    const uint64_t d = e % dim;
    const uint64_t b = (i * 2654435761ull) % (uint64_t)blobs;
    const float centre = 10.f * kmd_u01(seed ^ (b * 0x9E3779B97F4A7C15ull) ^ (d * 0x632BE59BD9B4E019ull)) - 5.f;
    const float noise = kmd_u01(seed * 31 + i * 0xD1B54A32D192ED03ull + d) - 0.5f;
    X[e] = centre + 0.2f * noise;
  }
}

int g_cus = 0;

int cus() {
  if (g_cus == 0) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&g_cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (g_cus <= 0) g_cus = 256;
  }
  return g_cus;
}

template <int NS, bool MULTI>
void launch_assign(const __bf16* XH, const float* xnorm, uint64_t n, const unsigned char* cwb, int K, int32_t* assign,
                   hipStream_t s) {
  using G = Geo<NS>;
  static int per_cu = 0;   // resident workgroups per CU (registers and the two chunk buffers)
  if (per_cu == 0) {
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kmd_assign_kernel<NS, MULTI>, 64 * kAsWaves, 0);
    if (per_cu < 1) per_cu = 1;
  }
  const int nch = (K + G::CB - 1) / G::CB;
  const uint64_t pb = 16 * G::T * kAsWaves;
  const uint64_t blocks = (n + pb - 1) / pb;
  const uint64_t cap = (uint64_t)per_cu * cus();
  kmd_assign_kernel<NS, MULTI><<<(unsigned)(blocks < cap ? blocks : cap), 64 * kAsWaves, 0, s>>>(
      XH, xnorm, n, reinterpret_cast<const uint4*>(cwb), reinterpret_cast<const float*>(cwb + (size_t)nch * G::BYTES),
      K, assign);
}

template <int SW>
void launch_movers(const float* X, uint64_t n, int D, const int32_t* assign, const int32_t* prev, int K, double* S,
                   long long* cnt, hipStream_t s) {
  const uint32_t sm = (uint32_t)K * SW * 8 + (uint32_t)K * 4 + 2 * 256 * 4;
  const unsigned slices = (unsigned)((D + SW - 1) / SW);
  // workgroups per CU that the slab leaves room for (of 160 KB), four at the most, over all slices
  const uint64_t fit = (160u * 1024u) / sm < 4 ? (160u * 1024u) / sm : 4;
  const uint64_t mb = (n + 255) / 256;
  uint64_t mcap = fit * (uint64_t)cus() / slices;
  if (mcap < 1) mcap = 1;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kmd_movers_kernel<SW>), hipFuncAttributeMaxDynamicSharedMemorySize,
                      (int)sm);
  kmd_movers_kernel<SW><<<dim3((unsigned)(mb < mcap ? mb : mcap), slices), 256, sm, s>>>(X, n, D, assign, prev, K, S, cnt);
}

}  // namespace

// Width of the plane rows for dimension d (a multiple of 32; 0 when d is outside 1 .. 512).
DR_API int dr_kmeans_dim_padded(int d) { return 32 * ns_for(d); }

// bf16 plane of n points of dimension d: XH = n * dp bf16 with dp = dr_kmeans_dim_padded(d), zero
// in the pad; xnorm = n f32 (|x|).
DR_API int dr_kmeans_dim_plane(const float* X, uint64_t n, int d, int dp, __bf16* XH, float* xnorm, hipStream_t s) {
  if (ns_for(d) == 0 || dp != 32 * ns_for(d) || (n >> 32) != 0) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const uint64_t waves = (n + (dp < 64 ? 2 : 1) - 1) / (dp < 64 ? 2 : 1);
  kmd_plane_kernel<<<grid_for(waves * 64, 256, 16384), 256, 0, s>>>(X, n, d, dp, XH, xnorm);
  DR_LAUNCH_CHECK();
  return 0;
}

// Bytes of the split-centroid workspace of dr_kmeans_dim_step for K clusters of dimension d (0
// when either is out of range).
DR_API uint64_t dr_kmeans_dim_centroid_workspace(int K, int d) {
  const GeoRt g = geo_rt(d);
  if (g.ns == 0 || K < 1 || K > kMaxK) return 0;
  return (uint64_t)((K + g.cb - 1) / g.cb) * g.bytes + 16;
}

// One k-means step on the plane of dr_kmeans_dim_plane, 1 <= d <= 512, 1 <= K <= 1024, n < 2^32.
// X holds the f32 rows at pitch d.  assign (n) receives the final assignment; prev (n, -1 = none),
// S (K * d f64) and cnt (K i64) are the table's running per-cluster state: zero S / cnt and fill
// prev with -1 whenever K or the points change.  cnorm_ws: K f32; near_ws: 8 n + 16 bytes; cws:
// dr_kmeans_dim_centroid_workspace(K, d) bytes.  After the call S / cnt hold the sums / counts of
// this step's assignment.
DR_API int dr_kmeans_dim_step(const __bf16* XH, const float* xnorm, const float* X, uint64_t n, int d, const float* C,
                              int K, float* cnorm_ws, int32_t* assign, int32_t* prev, double* S, long long* cnt,
                              void* near_ws, void* cws, hipStream_t s) {
  const GeoRt g = geo_rt(d);
  if (g.ns == 0 || K < 1 || K > kMaxK || (n >> 32) != 0) return (int)hipErrorInvalidValue;
  if (!assign || !prev || !S || !cnt || !near_ws || !cws || !cnorm_ws) return (int)hipErrorInvalidValue;
  kmd_norms_kernel<<<K, 64, 0, s>>>(C, K, d, cnorm_ws);
  if (n == 0) {
    DR_LAUNCH_CHECK();
    return 0;
  }
  const int nch = (K + g.cb - 1) / g.cb;
  unsigned char* cwb = reinterpret_cast<unsigned char*>(cws);
  kmd_cprep_kernel<<<nch, 256, 0, s>>>(C, cnorm_ws, K, d, g.row, g.cb, g.bytes, cwb);
  uint32_t* near_cnt = reinterpret_cast<uint32_t*>(near_ws);
  uint32_t* near_list = near_cnt + 4;
  kmd_near_reset<<<1, 64, 0, s>>>(near_cnt);
  switch (g.ns) {
#define DR_KMD(N)                                                            \
  case N:                                                                    \
    if (nch > 1) launch_assign<N, true>(XH, xnorm, n, cwb, K, assign, s);    \
    else launch_assign<N, false>(XH, xnorm, n, cwb, K, assign, s);           \
    break
    DR_KMD(1); DR_KMD(2); DR_KMD(3); DR_KMD(4); DR_KMD(6); DR_KMD(8); DR_KMD(12); DR_KMD(16);
#undef DR_KMD
    default: return (int)hipErrorInvalidValue;
  }
  kmd_near_list<<<grid_for(n, 256, 4096), 256, 0, s>>>(assign, n, near_cnt, near_list);
  kmd_rerank_kernel<4><<<8192, 64, 0, s>>>(X, C, cnorm_ws, K, d, near_cnt, near_list, assign, n);
  // slice width: the widest f64 [K][SW] slab within 128 KB, no wider than the points need
  int sw = K <= 128 ? 128 : K <= 256 ? 64 : K <= 512 ? 32 : 16;
  while (sw > 16 && sw / 2 >= d) sw /= 2;
  if (d <= 4) sw = 4;
  switch (sw) {
#define DR_KMM(V) case V: launch_movers<V>(X, n, d, assign, prev, K, S, cnt, s); break
    DR_KMM(128); DR_KMM(64); DR_KMM(32); DR_KMM(16); DR_KMM(4);
#undef DR_KMM
  }
  kmd_copy_assign<<<grid_for(n, 256, 4096), 256, 0, s>>>(assign, n, prev);
  DR_LAUNCH_CHECK();
  return 0;
}

// gen://points for any dimension 1 <= d <= 512 (dr_kmeans_gen of kmeans.hip serves d = 128).
DR_API int dr_kmeans_dim_gen(float* X, uint64_t n, int d, uint64_t first, int blobs, uint64_t seed, hipStream_t s) {
  if (d < 1 || d > kMaxD || blobs < 1) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  kmd_gen_kernel<<<grid_for(n * (uint64_t)d, 256, 16384), 256, 0, s>>>(X, n, (uint64_t)d, first, blobs, seed);
  DR_LAUNCH_CHECK();
  return 0;
}
