// pc_norm of a cloud held in the registers of one workgroup (dataset.hip, corrupt.hip, mix.hip): subtract the mean of
// the valid rows, divide by their largest norm.  One text for both kernels; the arithmetic and its order are stated in
// include/simamba.h under simamba_dataset_fetch.  The translation unit is built with -ffp-contract=off and every
// operation is spelled __fadd_rn / __fmul_rn / __fdiv_rn / __fsqrt_rn: one correctly rounded fp32 operation each.
#pragma once
#include "common.h"

namespace simamba {

// the sum of v over the workgroup in a fixed order (lanes by butterfly, then the waves in ascending order), in every lane
__device__ __forceinline__ float ds_block_sum(float v, float* s, int lane, int wave, int waves) {
  v = wave_xor_sum(v);
  __syncthreads();                                         // the row may still be read from the call before
  if (lane == 0) s[wave] = v;
  __syncthreads();
  float t = s[0];
  for (int w = 1; w < waves; ++w) t = __fadd_rn(t, s[w]);
  return t;
}

__device__ __forceinline__ float ds_block_max(float v, float* s, int lane, int wave, int waves) {
  v = wave_xor_max(v);
  __syncthreads();
  if (lane == 0) s[wave] = v;
  __syncthreads();
  float t = s[0];
  for (int w = 1; w < waves; ++w) t = fmaxf(t, s[w]);
  return t;
}

// Every lane holds P rows; bit j of `valid` says that its row j belongs to the cloud, `len` >= 1 is how many such rows
// the workgroup holds, (fx, fy, fz) is one of them (the same in every lane), s has one float per wave.
// Relative to that row first: coinciding rows become exact zeros, and the mean loses no bits to an offset.  Rows
// that are not valid take no part and come back meaningless: the caller does not store them.  All rows coincide
// (m == 0): zeros, no 0 / 0.  Every lane calls it.
template <int P>
__device__ __forceinline__ void unit_sphere_rows(float (&x)[P], float (&y)[P], float (&z)[P], unsigned valid, int len,
                                                 float fx, float fy, float fz, float* s, int lane, int wave,
                                                 int waves) {
  float sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    if (valid >> j & 1u) {
      x[j] = __fsub_rn(x[j], fx);
      y[j] = __fsub_rn(y[j], fy);
      z[j] = __fsub_rn(z[j], fz);
      sx = __fadd_rn(sx, x[j]);
      sy = __fadd_rn(sy, y[j]);
      sz = __fadd_rn(sz, z[j]);
    }
  }
  const float flen = static_cast<float>(len);                        // exact: len <= 8192
  const float mx = __fdiv_rn(ds_block_sum(sx, s, lane, wave, waves), flen);
  const float my = __fdiv_rn(ds_block_sum(sy, s, lane, wave, waves), flen);
  const float mz = __fdiv_rn(ds_block_sum(sz, s, lane, wave, waves), flen);
  float big = 0.f;                                                   // the largest squared norm; a NaN is passed over
#pragma unroll
  for (int j = 0; j < P; ++j) {
    if (valid >> j & 1u) {
      x[j] = __fsub_rn(x[j], mx);
      y[j] = __fsub_rn(y[j], my);
      z[j] = __fsub_rn(z[j], mz);
      big = fmaxf(big, __fadd_rn(__fadd_rn(__fmul_rn(x[j], x[j]), __fmul_rn(y[j], y[j])), __fmul_rn(z[j], z[j])));
    }
  }
  const float m = __fsqrt_rn(ds_block_max(big, s, lane, wave, waves));
#pragma unroll
  for (int j = 0; j < P; ++j) {
    x[j] = m > 0.f ? __fdiv_rn(x[j], m) : 0.f;
    y[j] = m > 0.f ? __fdiv_rn(y[j], m) : 0.f;
    z[j] = m > 0.f ? __fdiv_rn(z[j], m) : 0.f;
  }
}

}  // namespace simamba
