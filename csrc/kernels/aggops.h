// Aggregate operators of the hash aggregations (hashagg.hip, keyhash.hip): op codes, identities and
// the atomic combine of one 64-bit accumulator, in LDS or HBM (generic address space).
#pragma once
#include "common.h"

namespace {
constexpr int kMaxAggs = 8;
enum Op : int { SUM_I = 0, MIN_I = 1, MAX_I = 2, COUNT = 3, SUM_F = 4, MIN_F = 5, MAX_F = 6 };

__device__ __forceinline__ uint64_t identity(int op) {
  switch (op) {
    case MIN_I: return 0x7FFFFFFFFFFFFFFFull;
    case MAX_I: return 0x8000000000000000ull;
    case MIN_F: return (uint64_t)__double_as_longlong(__builtin_inf());
    case MAX_F: return (uint64_t)__double_as_longlong(-__builtin_inf());
    default: return 0ull;
  }
}

__device__ __forceinline__ void fmin_max_atomic(unsigned long long* p, double v, bool is_min) {
  unsigned long long old = *p, assumed;
  do {
    assumed = old;
    const double cur = __longlong_as_double((long long)assumed);
    const double nv = is_min ? (v < cur ? v : cur) : (v > cur ? v : cur);
    if (nv == cur) break;
    old = atomicCAS(p, assumed, (unsigned long long)__double_as_longlong(nv));
  } while (assumed != old);
}

// works for LDS and global pointers (generic address space)
__device__ __forceinline__ void combine_atomic(uint64_t* p, uint64_t v, int op) {
  unsigned long long* q = reinterpret_cast<unsigned long long*>(p);
  switch (op) {
    case SUM_I: case COUNT: atomicAdd(q, (unsigned long long)v); break;
    case MIN_I: atomicMin(reinterpret_cast<long long*>(p), (long long)v); break;
    case MAX_I: atomicMax(reinterpret_cast<long long*>(p), (long long)v); break;
    case SUM_F: atomicAdd(reinterpret_cast<double*>(p), __longlong_as_double((long long)v)); break;
    case MIN_F: fmin_max_atomic(q, __longlong_as_double((long long)v), true); break;
    default: fmin_max_atomic(q, __longlong_as_double((long long)v), false); break;
  }
}
}  // namespace
