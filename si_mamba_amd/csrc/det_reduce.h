// Fixed-order sum of per-workgroup partials: the second half of every deterministic backward
// (SIMAMBA_BWD_DETERMINISTIC; scan_bwd.hip, scan_bwd_seq.hip, conv1d.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace simamba {

// out[i] = sum_{k = 0 .. K-1} part[k * kstride + i] for i < n, k ascending, fp32; out is written whole (K == 0: zeros)
struct DetSumJob {
  const float* part;
  float* out;
  long long kstride;
  long long n;
  int K;
};

constexpr int kDetSumMaxJobs = 5;

// up to kDetSumMaxJobs jobs in one launch on `s`; returns a hipError_t
int det_sum_launch(const DetSumJob* jobs, int njobs, hipStream_t s);

}  // namespace simamba
