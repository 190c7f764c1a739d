// A cloud held in the registers of one workgroup (corrupt.hip, mix.hip): lane t holds the 8 consecutive rows
// 8 t .. 8 t + 7, so the index order of the rows is the order (lane, slot).  One text for both kernels: the workgroup
// count and prefix sum, the counting select of the m smallest keys, the Philox block of augment's counter layout at
// chain position 0 under the caller's key, and the draw of one row out of `a`.  Device only; the translation unit is
// built with -ffp-contract=off.
#pragma once
#include "common.h"
#include "philox_draws.h"
#include "pointset.h"

namespace simamba {

constexpr int kCorMaxPoints = 8192;
constexpr int kCorPerLane = 8;
constexpr int kCorMaxThreads = kCorMaxPoints / kCorPerLane;
constexpr int kCorMaxWaves = kCorMaxThreads / 64;
constexpr int kCorIndexBits = 13;                          // 2^13 = kCorMaxPoints rows under the 32-bit rank
constexpr int kCorKeyBits = 32 + kCorIndexBits;
constexpr unsigned long long kCorDead = ~0ull;             // above every real key

struct CorRng {
  uint32_t k0, k1, cloud, step_lo, step_hi;
};

// block `index` of the per-cloud or the per-point stream of (cloud, step): augment's layout at chain position 0
__device__ __forceinline__ Philox4 cor_block(const CorRng& r, bool per_point, uint32_t index) {
  const uint32_t c3 = (r.step_hi & 0x0FFFFFFFu) | (per_point ? 0x80000000u : 0u);
  return philox4x32_10(r.k0, r.k1, index, r.cloud, r.step_lo, c3);
}

// the sum of v over the workgroup, in every lane
__device__ __forceinline__ int cor_block_count(int v, int* s, int lane, int wave, int waves) {
  v = wave_xor_sum(v);
  __syncthreads();                                         // the row may still be read from the call before
  if (lane == 0) s[wave] = v;
  __syncthreads();
  int t = 0;
  for (int w = 0; w < waves; ++w) t += s[w];
  return t;
}

// the sum of v over the lanes in front of this one, and the workgroup's total
__device__ __forceinline__ int cor_block_scan(int v, int* s, int lane, int wave, int waves, int& total) {
  int inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(inc, off);
    if (lane >= off) inc += t;
  }
  __syncthreads();
  if (lane == 63) s[wave] = inc;
  __syncthreads();
  int base = 0, tot = 0;
  for (int w = 0; w < waves; ++w) {
    if (w < wave) base += s[w];
    tot += s[w];
  }
  total = tot;
  return base + inc - v;
}

// Remove the m >= 1 alive rows with the smallest keys; keys are distinct and below 2^45, dead rows hold kCorDead.
// t ends as the m-th smallest key: the largest value with fewer than m keys below it.  Uniform over the workgroup.
__device__ __forceinline__ void cor_remove_smallest(const unsigned long long (&key)[kCorPerLane], int m, unsigned& alive,
                                                    int* s, int lane, int wave, int waves) {
  unsigned long long t = 0;
  for (int bit = kCorKeyBits - 1; bit >= 0; --bit) {
    const unsigned long long c = t | 1ull << bit;
    int below = 0;
#pragma unroll
    for (int j = 0; j < kCorPerLane; ++j) below += key[j] < c ? 1 : 0;
    if (cor_block_count(below, s, lane, wave, waves) < m) t = c;
  }
#pragma unroll
  for (int j = 0; j < kCorPerLane; ++j)
    if (key[j] <= t) alive &= ~(1u << j);
}

// min((int)(u * float(a)), a - 1), a >= 1
__device__ __forceinline__ int cor_pick(uint32_t w, int a) {
  const int r = static_cast<int>(__fmul_rn(aug_uniform(w), static_cast<float>(a)));
  return r < a - 1 ? r : a - 1;
}

// the lanes a cloud of K rows takes: whole waves
static inline int cor_threads(int K) {
  const int t = ((K + kCorPerLane - 1) / kCorPerLane + 63) / 64 * 64;
  return t > kCorMaxThreads ? kCorMaxThreads : t;
}

// do [a, a + na) and [b, b + nb) share a byte
static inline bool cor_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + nb && pb < pa + na;
}

}  // namespace simamba
