// The arithmetic of the causal depthwise conv1d (+SiLU), stated once: conv1d.hip (forward, and both backward kernels'
// recompute) and the conv fused into the staging of xdt_proj.hip / xdt_proj_bf16.hip call these, so that the forward,
// its fused forms and the backward's pre-activation cannot round apart (tests/test_gpu_xdt_proj.py pins the fused
// forms torch.equal to the stand-alone kernel).
#pragma once
#include "common.h"

namespace simamba {

// Pre-activation of one output step: the bias, then the four taps in tap-index order as one fmaf chain.
// w4: the taps right-aligned in 4 (narrower convs lead with zeros); win: the step's input and the 3 in front of it,
// oldest first (win[3] is the step itself).
__device__ __forceinline__ float conv_pre(const float (&w4)[4], const float* win, float bias) {
  float acc = bias;
#pragma unroll
  for (int j = 0; j < 4; ++j) acc = fmaf(w4[j], win[j], acc);
  return acc;
}

// Backward of P consecutive output steps t0 .. t0 + P - 1 of one row.
//   xw = x[t0 - 3 .. t0 + P + 2], gv = dout[t0 .. t0 + P + 2] (zeros outside the row);
//   dx[i] = sum_j w4[j] * dpre[i + 3 - j], with dpre = dout * silu'(pre) (or dout), recomputed through conv_pre;
//   gw / gb accumulate the pack's share of the tap / bias gradients.
// kGuard: `valid` = steps of the row from t0 on; positions past it are zeroed by select (a ragged last pack, or loads
// that do not zero them).  Without it the caller guarantees gv = 0 there.
// (gb is __restrict__: a register of the caller's that none of the arrays alias -- with that said, the bf16 pipelined
// kernel compiles to the instructions it had with this body written out in place)
template <int P, bool kGuard>
__device__ __forceinline__ void conv_bwd_pack(const float (&w4)[4], float bias, bool silu, const float (&xw)[P + 6],
                                              const float (&gv)[P + 3], int valid, float (&dx)[P], float (&gw)[4],
                                              float& __restrict__ gb) {
  float dpre[P + 3];
#pragma unroll
  for (int i = 0; i < P + 3; ++i) {
    float g = gv[i];
    if (silu) {
      const float pre = conv_pre(w4, xw + i, bias);
      const float sg = sigmoid_f(pre);
      g = g * sg * (1.f + pre * (1.f - sg));
    }
    dpre[i] = (!kGuard || i < valid) ? g : 0.f;
  }
#pragma unroll
  for (int i = 0; i < P; ++i) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = fmaf(w4[j], dpre[i + 3 - j], acc);
    dx[i] = acc;
    gb += dpre[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) gw[j] = fmaf(dpre[i], xw[i + j], gw[j]);
  }
}

}  // namespace simamba
