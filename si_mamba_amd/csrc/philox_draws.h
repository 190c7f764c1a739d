// The maps from Philox words to the values the point kernels draw (augment.hip, corrupt.hip, mix.hip): one text for
// all, so the uniform and the Box-Muller normals of one are those of the others bit for bit.  Device only; the
// translation unit is built with -ffp-contract=off, every product here is one correctly rounded fp32 operation.
#pragma once
#include "philox.h"

namespace simamba {

__device__ __forceinline__ float aug_uniform(uint32_t w) {           // [0, 1), a multiple of 2^-24: exact
  return static_cast<float>(w >> 8) * 0x1p-24f;
}

// Box-Muller: two standard normals from two words; the logarithm's argument is in (0, 1], the angle 2 pi u as 2 u half turns
__device__ __forceinline__ void aug_normal_pair(uint32_t wa, uint32_t wb, float& n0, float& n1) {
  const float a = static_cast<float>((wa >> 8) + 1u) * 0x1p-24f;
  const float r = sqrtf(__fmul_rn(-2.f, logf(a)));
  float s, c;
  sincospif(__fmul_rn(2.f, aug_uniform(wb)), &s, &c);
  n0 = __fmul_rn(r, c);
  n1 = __fmul_rn(r, s);
}

// the three normals of one per-point block: (w0, w1) -> x, y; (w2, w3) -> z
__device__ __forceinline__ void aug_block_normals(const Philox4& q, float& n0, float& n1, float& n2) {
  float unused;
  aug_normal_pair(q.w[0], q.w[1], n0, n1);
  aug_normal_pair(q.w[2], q.w[3], n2, unused);
}

}  // namespace simamba
