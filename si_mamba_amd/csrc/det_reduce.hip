// Fixed-order partial sums for the deterministic backwards, for gfx950.
//
// One launch serves every destination of a backward (scan: dB, dC, dA, dD, ddelta_bias; conv: dw, dbias).  A thread
// owns 4 consecutive outputs of one job and walks k = 0, 1, ..., K-1 with 16-byte loads (4 loads in flight, added in
// ascending k), so every output is the same fp32 sum in the same order on every run and every launch shape.
// Bytes: K * n * 4 read + n * 4 written per job.
#include "det_reduce.h"

namespace simamba {

constexpr int kDetSumThreads = 256;
constexpr int kDetSumPerBlock = 4 * kDetSumThreads;

struct DetSumArgs {
  DetSumJob job[kDetSumMaxJobs];
  int vec[kDetSumMaxJobs];
  int blk0[kDetSumMaxJobs + 1];   // first block of every job; blk0[njobs] = grid size
  int njobs;
};

__global__ __launch_bounds__(kDetSumThreads) void det_sum_kernel(DetSumArgs a) {
  const int blk = blockIdx.x;
  int j = 0;
#pragma unroll
  for (int q = 1; q < kDetSumMaxJobs; ++q) j = (q < a.njobs && blk >= a.blk0[q]) ? q : j;
  const float* __restrict__ part = a.job[j].part;
  float* __restrict__ out = a.job[j].out;
  const long long ks = a.job[j].kstride, n = a.job[j].n;
  const int K = a.job[j].K;
  const long long i0 = (static_cast<long long>(blk - a.blk0[j]) * kDetSumThreads + threadIdx.x) * 4;
  if (i0 >= n) return;
  if (a.vec[j] && i0 + 4 <= n) {
    const float* p = part + i0;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int k = 0;
    for (; k + 4 <= K; k += 4) {
      float4 v[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) v[m] = *reinterpret_cast<const float4*>(p + (k + m) * ks);
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        acc.x += v[m].x; acc.y += v[m].y; acc.z += v[m].z; acc.w += v[m].w;
      }
    }
    for (; k < K; ++k) {
      const float4 v = *reinterpret_cast<const float4*>(p + k * ks);
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    *reinterpret_cast<float4*>(out + i0) = acc;
    return;
  }
  for (long long i = i0; i < n && i < i0 + 4; ++i) {
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc += part[k * ks + i];
    out[i] = acc;
  }
}

int det_sum_launch(const DetSumJob* jobs, int njobs, hipStream_t s) {
  DetSumArgs a{};
  int blocks = 0, m = 0;
  for (int i = 0; i < njobs && m < kDetSumMaxJobs; ++i) {
    if (jobs[i].n <= 0) continue;
    a.job[m] = jobs[i];
    a.vec[m] = (reinterpret_cast<uintptr_t>(jobs[i].part) & 15u) == 0 && (reinterpret_cast<uintptr_t>(jobs[i].out) & 15u) == 0 &&
               jobs[i].kstride % 4 == 0;
    a.blk0[m] = blocks;
    blocks += static_cast<int>((jobs[i].n + kDetSumPerBlock - 1) / kDetSumPerBlock);
    ++m;
  }
  if (!m) return static_cast<int>(hipSuccess);
  a.njobs = m;
  for (int q = m; q <= kDetSumMaxJobs; ++q) a.blk0[q] = blocks;
  hipLaunchKernelGGL(det_sum_kernel, dim3(blocks), dim3(kDetSumThreads), 0, s, a);
  return static_cast<int>(hipGetLastError());
}

}  // namespace simamba
