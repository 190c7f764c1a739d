// Gather-sum-scatter over the rows of a (batch, L, C) sequence: the per-layer cross-merge of the orderings
// (reference models/point_mamba.py:350-370 cross_merg, :394-409 the re-expansion) in one pass, and its adjoint.
//
// With add_after_layer the reference sums, after every block, the M = 2 k copies of each of the G patch tokens that
// the SAST sequence holds (L = M G) and lays the sum out again in the same M orderings: about twenty torch ops and
// some eight passes over the hidden tensor.  Here, for every (b, g):
//     s = ((x[b, gi_0] + x[b, gi_H]) + (x[b, gi_1] + x[b, gi_{H+1}])) + ... + (x[b, gi_{H-1}] + x[b, gi_{M-1}])
//     y[b, si_m] = s   for m = 0 .. M-1                                (H = M / 2, gi_m = gather_idx[b, m, g], ...)
// in fp32 in exactly that order (the reference's: pairs of a forward and a reversed copy first, then the pairs in
// turn), rounded once to the I/O type.  L rows read, L rows written.  The backward is the same call with the two
// index maps swapped, so there is one kernel: no atomics, a fixed order of additions, the same bits every time.
//
// One wave per token (four tokens per workgroup): the token is wave-uniform, so its 2 M indices are read once per
// wave, ahead of the channel loop, and every row access is one contiguous run of 16 (bf16: 8) bytes per lane.  The M
// row reads of a lane are independent and issued together.  No LDS, a few dozen VGPRs: HBM-bound.
// The kernel takes whatever maps it is given and does not validate their values.
#include "host_common.h"

namespace simamba {

constexpr int kCmThreads = 256;
constexpr int kCmWaves = kCmThreads / 64;
constexpr int kCmMaxM = 16;

template <typename T, int H>
__global__ __launch_bounds__(kCmThreads) void gather_sum_scatter_kernel(const T* __restrict__ x,
                                                                        const int* __restrict__ gather_idx,
                                                                        const int* __restrict__ scatter_idx,
                                                                        T* __restrict__ y, int L, int G, int C) {
  constexpr int M = 2 * H;
  const int b = blockIdx.y;
  const int g = blockIdx.x * kCmWaves + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  if (g >= G) return;                                 // wave-uniform
  const int lane = threadIdx.x & 63;
  const int* gi = gather_idx + (static_cast<size_t>(b) * M) * G + g;
  const int* si = scatter_idx + (static_cast<size_t>(b) * M) * G + g;
  int src[M], dst[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    src[m] = gi[static_cast<size_t>(m) * G];
    dst[m] = si[static_cast<size_t>(m) * G];
  }
  const T* xb = x + static_cast<size_t>(b) * L * C;
  T* yb = y + static_cast<size_t>(b) * L * C;
  for (int c = 4 * lane; c < C; c += 4 * 64) {
    Pack<T, 4> row[M];
#pragma unroll
    for (int m = 0; m < M; ++m) row[m] = *reinterpret_cast<const Pack<T, 4>*>(xb + static_cast<size_t>(src[m]) * C + c);
    Pack<T, 4> out;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float s = to_f32<T>(row[0].v[i]) + to_f32<T>(row[H].v[i]);
#pragma unroll
      for (int h = 1; h < H; ++h) s += to_f32<T>(row[h].v[i]) + to_f32<T>(row[H + h].v[i]);
      out.v[i] = from_f32<T>(s);
    }
#pragma unroll
    for (int m = 0; m < M; ++m) *reinterpret_cast<Pack<T, 4>*>(yb + static_cast<size_t>(dst[m]) * C + c) = out;
  }
}

template <typename T>
static void launch_gather_sum_scatter(int H, dim3 grid, hipStream_t s, const void* x, const int* gi, const int* si,
                                      void* y, int L, int G, int C) {
  const T* xt = static_cast<const T*>(x);
  T* yt = static_cast<T*>(y);
#define SIMAMBA_CM_CASE(h) \
  case h: hipLaunchKernelGGL((gather_sum_scatter_kernel<T, h>), grid, dim3(kCmThreads), 0, s, xt, gi, si, yt, L, G, C); \
    break;
  switch (H) {
    SIMAMBA_CM_CASE(1) SIMAMBA_CM_CASE(2) SIMAMBA_CM_CASE(3) SIMAMBA_CM_CASE(4)
    SIMAMBA_CM_CASE(5) SIMAMBA_CM_CASE(6) SIMAMBA_CM_CASE(7) SIMAMBA_CM_CASE(8)
  }
#undef SIMAMBA_CM_CASE
}

}  // namespace simamba

using namespace simamba;

extern "C" int simamba_gather_sum_scatter(const void* x, const int* gather_idx, const int* scatter_idx, void* y,
                                          int batch, int L, int G, int M, int C, int io_dtype, void* stream) {
  if (const int rc = check_io_dtype(io_dtype)) return rc;
  if (batch == 0) return SIMAMBA_OK;
  if (batch < 0 || batch > 65535 || G <= 0 || L <= 0 || C <= 0 || (C % 4) != 0) return SIMAMBA_E_SHAPE;
  if (M < 2 || M > kCmMaxM || (M % 2) != 0 || static_cast<long long>(M) * G != L) return SIMAMBA_E_SHAPE;
  if (!x || !gather_idx || !scatter_idx || !y) return SIMAMBA_E_NULLPTR;
  const size_t row_align = 4 * io_esz(io_dtype) - 1;          // one lane's pack
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & row_align) return SIMAMBA_E_ALIGN;
  const dim3 grid((G + kCmWaves - 1) / kCmWaves, batch);
  with_io_type(io_dtype, [&](auto tag) {
    using T = decltype(tag);
    launch_gather_sum_scatter<T>(M / 2, grid, static_cast<hipStream_t>(stream), x, gather_idx, scatter_idx, y, L, G, C);
  });
  return static_cast<int>(hipGetLastError());
}
