// Device helpers the point-set kernels share: per-cloud lengths, the (x, y, z, payload) LDS tile of the tiled pair
// walks (chamfer_large.hip, sinkhorn.hip) and their fixed-order fp64 workgroup sum.
#pragma once
#include "common.h"

namespace simamba {

// The length of cloud (or pair) `i`: lengths[i] clamped to [1, padded], or `padded` without lengths.  T: int, long long.
template <typename T>
__device__ __forceinline__ int clamped_length(const T* __restrict__ lengths, long long i, int padded) {
  return lengths ? static_cast<int>(min(max(lengths[i], static_cast<T>(1)), static_cast<T>(padded))) : padded;
}

// Stage points [t0, t0 + cnt) of `set` as the xyz of tile[0 .. cnt); .w is left alone.  Coalesced: consecutive lanes,
// consecutive floats.  Every thread of the kThreads-wide workgroup calls it.
template <int kThreads>
__device__ __forceinline__ void stage_points(float4* tile, const float* __restrict__ set, int t0, int cnt) {
  float* s = reinterpret_cast<float*>(tile);
  const float* g = set + static_cast<long long>(t0) * 3;
  for (int e = threadIdx.x; e < cnt * 3; e += kThreads) {
    const int t = e / 3;
    s[4 * t + (e - 3 * t)] = g[e];
  }
}

// tile[t].w = the bits of w[t0 + t], a 4-byte payload that rides with the point; without w, .w is left alone
template <int kThreads, typename W>
__device__ __forceinline__ void stage_w(float4* tile, const W* __restrict__ w, int t0, int cnt) {
  if (w)
    for (int t = threadIdx.x; t < cnt; t += kThreads) tile[t].w = __builtin_bit_cast(float, w[t0 + t]);
}

// K sums over the workgroup at once, in a fixed order: thread t left its partial in s[k][t]; a tree over the kThreads
// entries leaves the totals in s[k][0].  Every thread calls it (barriers).
template <int kThreads, int K>
__device__ __forceinline__ void block_tree_sum(double (&s)[K][kThreads]) {
  __syncthreads();
  for (int w = kThreads / 2; w >= 1; w >>= 1) {
    if (threadIdx.x < w) {
#pragma unroll
      for (int k = 0; k < K; ++k) s[k][threadIdx.x] += s[k][threadIdx.x + w];
    }
    __syncthreads();
  }
}

}  // namespace simamba
