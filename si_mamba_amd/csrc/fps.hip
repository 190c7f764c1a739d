// Farthest-point sampling for gfx950 -- first step of the tokeniser that feeds the hot path
// ("next" row 1).
//
// Replaces pytorch3d.ops.sample_farthest_points as called at the reference's models/point_mamba.py:93
// (K = num_group centres per cloud, start at point 0).  One workgroup per cloud: the cloud and the running
// minimum distances live in registers (4 points per lane for N = 1024; a 1024-lane variant with 8 points per lane
// takes 4096 < N <= 8192), each of the K rounds is
//   broadcast the last pick through LDS -> update min-distance -> (value, index) arg-max by DPP wave
//   reduction -> 4-entry LDS combine,
// i.e. two workgroup barriers per round and no global traffic besides the initial 12 N bytes.
// Distances are accumulated exactly like the torch formulation ((dx^2 + dy^2) + dz^2, no FMA contraction;
// this file is built with -ffp-contract=off) and ties go to the lower index, so the picks are bit-identical
// to the oracle's.
//
// Ragged batches (kRagged): clouds padded to a common N with lengths[b] real points each.  A workgroup reads its length
// once; points >= len are never loaded (their lanes carry md = -1 like the lanes beyond N, so whatever the padding
// holds -- NaN, Inf -- enters no arithmetic), the first pick is start[b] instead of point 0 when given, min(K, len)
// picks are made and the remaining idx / centers slots are written as -1 / 0, pytorch3d's padding.  The picks are
// those of the unpadded cloud run alone.  The kRagged = false instantiations are the fixed-length kernels unchanged.
#include "pointset.h"

namespace simamba {

constexpr int kFpsThreads = 256;
constexpr int kFpsMaxPer = 16;     // points per lane: N <= 4096
// 4096 < N <= 8192: the same rounds on a 1024-lane workgroup, 8 points per lane (16 waves per CU; the combine reads
// 16 wave results instead of 4)
constexpr int kFpsWideThreads = 1024;
constexpr int kFpsWidePer = 8;     // points per lane: N <= 8192

__device__ __forceinline__ void argmax_combine(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

template <bool kRagged>
__global__ __launch_bounds__(kFpsThreads) void fps_kernel(const float* __restrict__ pts, long long* __restrict__ idx,
                                                          float* __restrict__ centers, int N, int K,
                                                          const long long* __restrict__ lengths,
                                                          const long long* __restrict__ start) {
  __shared__ float sCur[3];
  __shared__ float sVal[kFpsThreads / 64];
  __shared__ int sIdx[kFpsThreads / 64];
  const float* P = pts + static_cast<size_t>(blockIdx.x) * N * 3;
  const int tid = threadIdx.x;
  int len = N, cur = 0;
  if constexpr (kRagged) {
    len = clamped_length(lengths, blockIdx.x, N);
    if (start) cur = static_cast<int>(min(max(start[blockIdx.x], 0LL), static_cast<long long>(len - 1)));
  }
  const int picks = kRagged ? min(K, len) : K;
  float px[kFpsMaxPer], py[kFpsMaxPer], pz[kFpsMaxPer], md[kFpsMaxPer];
#pragma unroll
  for (int k = 0; k < kFpsMaxPer; ++k) {
    const int i = tid + k * kFpsThreads;
    const bool ok = i < len;
    px[k] = ok ? P[3 * i] : 0.f;
    py[k] = ok ? P[3 * i + 1] : 0.f;
    pz[k] = ok ? P[3 * i + 2] : 0.f;
    md[k] = ok ? __builtin_inff() : -1.f;    // padding never wins the arg-max
  }
  for (int r = 0; r < picks; ++r) {
    if (tid == 0) {
      idx[static_cast<size_t>(blockIdx.x) * K + r] = cur;
      const float cx = P[3 * cur], cy = P[3 * cur + 1], cz = P[3 * cur + 2];
      sCur[0] = cx; sCur[1] = cy; sCur[2] = cz;
      if (centers) {
        float* c = centers + (static_cast<size_t>(blockIdx.x) * K + r) * 3;
        c[0] = cx; c[1] = cy; c[2] = cz;
      }
    }
    __syncthreads();
    const float cx = sCur[0], cy = sCur[1], cz = sCur[2];
    float bv = -2.f;
    int bi = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < kFpsMaxPer; ++k) {
      if (k * kFpsThreads < len) {
        const float dx = px[k] - cx, dy = py[k] - cy, dz = pz[k] - cz;
        const float d = (dx * dx + dy * dy) + dz * dz;
        md[k] = fminf(md[k], d);
        argmax_combine(bv, bi, md[k], tid + k * kFpsThreads);
      }
    }
    // wave arg-max (butterfly over 64 lanes)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off);
      const int oi = __shfl_xor(bi, off);
      argmax_combine(bv, bi, ov, oi);
    }
    if ((tid & 63) == 0) { sVal[tid >> 6] = bv; sIdx[tid >> 6] = bi; }
    __syncthreads();
    bv = sVal[0]; bi = sIdx[0];
#pragma unroll
    for (int w = 1; w < kFpsThreads / 64; ++w) argmax_combine(bv, bi, sVal[w], sIdx[w]);
    cur = bi;
  }
  if constexpr (kRagged) {                       // fewer points than picks: pytorch3d's padding
    for (int r = picks + tid; r < K; r += kFpsThreads) {
      idx[static_cast<size_t>(blockIdx.x) * K + r] = -1;
      if (centers) {
        float* c = centers + (static_cast<size_t>(blockIdx.x) * K + r) * 3;
        c[0] = 0.f; c[1] = 0.f; c[2] = 0.f;
      }
    }
  }
}

// The same rounds as fps_kernel, 1024 lanes x 8 points.  A copy rather than a template shared with fps_kernel: the
// shared form changes fps_kernel's register allocation, and the N <= 4096 path is kept exactly as it was.
template <bool kRagged>
__global__ __launch_bounds__(kFpsWideThreads) void fps_wide_kernel(const float* __restrict__ pts,
                                                                   long long* __restrict__ idx,
                                                                   float* __restrict__ centers, int N, int K,
                                                                   const long long* __restrict__ lengths,
                                                                   const long long* __restrict__ start) {
  __shared__ float sCur[3];
  __shared__ float sVal[kFpsWideThreads / 64];
  __shared__ int sIdx[kFpsWideThreads / 64];
  const float* P = pts + static_cast<size_t>(blockIdx.x) * N * 3;
  const int tid = threadIdx.x;
  int len = N, cur = 0;
  if constexpr (kRagged) {
    len = clamped_length(lengths, blockIdx.x, N);
    if (start) cur = static_cast<int>(min(max(start[blockIdx.x], 0LL), static_cast<long long>(len - 1)));
  }
  const int picks = kRagged ? min(K, len) : K;
  float px[kFpsWidePer], py[kFpsWidePer], pz[kFpsWidePer], md[kFpsWidePer];
#pragma unroll
  for (int k = 0; k < kFpsWidePer; ++k) {
    const int i = tid + k * kFpsWideThreads;
    const bool ok = i < len;
    px[k] = ok ? P[3 * i] : 0.f;
    py[k] = ok ? P[3 * i + 1] : 0.f;
    pz[k] = ok ? P[3 * i + 2] : 0.f;
    md[k] = ok ? __builtin_inff() : -1.f;    // padding never wins the arg-max
  }
  for (int r = 0; r < picks; ++r) {
    if (tid == 0) {
      idx[static_cast<size_t>(blockIdx.x) * K + r] = cur;
      const float cx = P[3 * cur], cy = P[3 * cur + 1], cz = P[3 * cur + 2];
      sCur[0] = cx; sCur[1] = cy; sCur[2] = cz;
      if (centers) {
        float* c = centers + (static_cast<size_t>(blockIdx.x) * K + r) * 3;
        c[0] = cx; c[1] = cy; c[2] = cz;
      }
    }
    __syncthreads();
    const float cx = sCur[0], cy = sCur[1], cz = sCur[2];
    float bv = -2.f;
    int bi = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < kFpsWidePer; ++k) {
      if (k * kFpsWideThreads < len) {
        const float dx = px[k] - cx, dy = py[k] - cy, dz = pz[k] - cz;
        const float d = (dx * dx + dy * dy) + dz * dz;
        md[k] = fminf(md[k], d);
        argmax_combine(bv, bi, md[k], tid + k * kFpsWideThreads);
      }
    }
    // wave arg-max (butterfly over 64 lanes)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off);
      const int oi = __shfl_xor(bi, off);
      argmax_combine(bv, bi, ov, oi);
    }
    if ((tid & 63) == 0) { sVal[tid >> 6] = bv; sIdx[tid >> 6] = bi; }
    __syncthreads();
    bv = sVal[0]; bi = sIdx[0];
#pragma unroll
    for (int w = 1; w < kFpsWideThreads / 64; ++w) argmax_combine(bv, bi, sVal[w], sIdx[w]);
    cur = bi;
  }
  if constexpr (kRagged) {                       // fewer points than picks: pytorch3d's padding
    for (int r = picks + tid; r < K; r += kFpsWideThreads) {
      idx[static_cast<size_t>(blockIdx.x) * K + r] = -1;
      if (centers) {
        float* c = centers + (static_cast<size_t>(blockIdx.x) * K + r) * 3;
        c[0] = 0.f; c[1] = 0.f; c[2] = 0.f;
      }
    }
  }
}

}  // namespace simamba

using namespace simamba;

namespace {

template <bool kRagged>
void launch_fps(const float* points, const long long* lengths, const long long* start, long long* idx, float* centers,
                int B, int N, int K, hipStream_t s) {
  if (N <= kFpsThreads * kFpsMaxPer)
    hipLaunchKernelGGL(fps_kernel<kRagged>, dim3(B), dim3(kFpsThreads), 0, s, points, idx, centers, N, K, lengths, start);
  else
    hipLaunchKernelGGL(fps_wide_kernel<kRagged>, dim3(B), dim3(kFpsWideThreads), 0, s, points, idx, centers, N, K, lengths,
                       start);
}

}  // namespace

extern "C" int simamba_farthest_point_sample_ex(const float* points, const long long* lengths, const long long* start,
                                                long long* idx, float* centers, int B, int N, int K, void* stream) {
  if (B < 0 || N <= 0 || K < 0 || K > N || N > kFpsWideThreads * kFpsWidePer) return SIMAMBA_E_SHAPE;
  if (B == 0 || K == 0) return SIMAMBA_OK;
  if (!points || !idx) return SIMAMBA_E_NULLPTR;
  if (lengths || start) launch_fps<true>(points, lengths, start, idx, centers, B, N, K, static_cast<hipStream_t>(stream));
  else launch_fps<false>(points, nullptr, nullptr, idx, centers, B, N, K, static_cast<hipStream_t>(stream));
  return static_cast<int>(hipGetLastError());
}

extern "C" int simamba_farthest_point_sample(const float* points, long long* idx, float* centers, int B, int N, int K,
                                             void* stream) {
  return simamba_farthest_point_sample_ex(points, nullptr, nullptr, idx, centers, B, N, K, stream);
}
