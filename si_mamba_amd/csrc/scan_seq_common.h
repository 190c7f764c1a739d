// Device helpers shared by the two sequential ("lanes per channel") scan kernels, scan_fwd_seq.hip and
// scan_bwd_seq.hip.  The backward recomputes what the forward computed (softplus(delta), the tile layout), so both must
// run the very same code: it lives here once.
#pragma once
#include "scan_common.h"

namespace simamba {

constexpr int kSeqTC = 32;                 // timesteps per chunk: one 128-byte line of an fp32 row

using f32x4_t = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

// One aligned 4-element pack per lane (16 B fp32 / 8 B bf16).  The dispatcher only takes this kernel when
// rows are pack-aligned (L % 4 == 0 for fp32, L % 8 == 0 for bf16), so a pack is either entirely inside the
// sequence or entirely outside.  A pack beyond the end of the sequence (last chunk of a ragged L) re-reads the
// FIRST pack of its own row -- valid memory, finite whenever the row is -- and is neutralised once per pack, not
// per element: its delta gets a bias of -1e30, which softplus maps to exactly 0 (a_t = 1, x_t = 0: the state
// passes through), and its outputs are not stored.  No per-element guards, no divergent branches.
// Addressing is "uniform base pointer + 32-bit BYTE offset" throughout (the dispatcher guarantees every tensor
// spans < 4 GiB): global_load/store then take the base in SGPRs and one VGPR of offset, instead of a 64-bit
// VGPR address per access that the compiler hoists out of the chunk loop and spills.
template <typename T>
__device__ __forceinline__ void load4(const T* __restrict__ base, unsigned boff, float (&v)[4]) {
  const Pack<T, 4> pk = *reinterpret_cast<const Pack<T, 4>*>(reinterpret_cast<const char*>(base) + boff);
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = to_f32<T>(pk.v[i]);
}
template <typename T>
__device__ __forceinline__ void store4(T* __restrict__ base, unsigned boff, const float (&v)[4]) {
  Pack<T, 4> pk;
#pragma unroll
  for (int i = 0; i < 4; ++i) pk.v[i] = from_f32<T>(v[i]);
  *reinterpret_cast<Pack<T, 4>*>(reinterpret_cast<char*>(base) + boff) = pk;
}

// softplus(x) with x handed over as x2 = x * log2(e) (the caller folds the scale into one fma with the bias):
// 2 transcendentals + 7 plain ops, branch-free.  Above torch's threshold (x > 20) the result is x itself (and the
// exp2 overflow beyond x ~ 88 never shows); below -15 the series log(1 + e) = e keeps the relative accuracy that
// 1 + e loses.  x2 = -inf-like (-1e30 from a padded pack) gives e = 0 and exactly 0.
__device__ __forceinline__ float softplus_log2(float x2) {
  const float e = fast_exp2(x2);
  float sp = log1p_exp(e);
  sp = (x2 < -15.f * kLog2e) ? e : sp;
  return (x2 > 20.f * kLog2e) ? x2 * kLn2 : sp;
}

// float offset of 16-byte column group g (0..7) of a tile row
__device__ __forceinline__ int tile_off(int row, int g) { return row * kSeqTC + 4 * (g ^ ((row >> 1) & 7)); }

}  // namespace simamba
