// Device helpers shared by the matrix-core projection kernels (xdt_proj*.hip, in_proj_*.hip, out_norm_bf16.hip):
// register vector types, buffer-descriptor accesses, asm LDS reads with counted waits, bf16 pairs in a dword.
// conv1d.hip, no MFMA kernel, includes it for the bf16 pair helpers alone (its unpack16).
#pragma once
#include <type_traits>

#include "common.h"

namespace simamba {

// ---- register vectors ------------------------------------------------------------------------------------------------
// MFMA operands / accumulators, and 16-byte register values as NATIVE vectors: HIP's uint4 / float4 are structs whose
// copies hipcc lowers to memcpy between address spaces, and an array of them that lives across loop iterations then
// stays in scratch memory instead of registers.
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ---- buffer-descriptor accesses: out-of-range lanes load zeros / store nothing ------------------------------------------
using rsrc_t = __amdgpu_buffer_rsrc_t;
constexpr unsigned kOob = 0xfffff000u;   // a byte offset past every descriptor's range

__device__ __forceinline__ rsrc_t make_rsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, static_cast<int>(bytes), 0x00020000);
}
// The 128-bit builtins' own vector type, reached by bit_cast only: initialising an ext_vector_type(4) from the
// builtin's result compiles (hipcc, ROCm 7.2) to a ONE-dword load splatted over the four lanes.
using bvec4_t = decltype(__builtin_amdgcn_raw_buffer_load_b128(make_rsrc(nullptr, 0u), 0u, 0u, 0));
template <typename V>                    // V: float4 or uint4
__device__ __forceinline__ V bload16(rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
template <typename V>
__device__ __forceinline__ void bstore16(V v, rsrc_t r, unsigned voff, unsigned soff) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(bvec4_t, v), r, voff, soff, 0);
}
__device__ __forceinline__ void bstore4(float f, rsrc_t r, unsigned voff, unsigned soff) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, f), r, voff, soff, 0);
}
__device__ __forceinline__ void bstore2(unsigned short v, rsrc_t r, unsigned voff, unsigned soff) {
  __builtin_amdgcn_raw_buffer_store_b16(v, r, voff, soff, 0);
}

// ---- LDS reads issued ahead -------------------------------------------------------------------------------------------
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}
// A 16-byte LDS read (V: u32x4 or f32x4) the compiler can neither sink next to its use nor count: issued here, waited
// for by lds_wait.  (Left to itself hipcc moved every A-fragment read directly in front of its MFMAs and waited
// lgkmcnt(0) each time -- one LDS latency per k step, 2.5 us per channel block at one wave per SIMD.)
// Contract: the destination may only be READ through lds_wait (which hands the compiler a new value): to hipcc the
// register is defined the moment this statement issues.  A copy of it made before the wait -- a live-range split or a
// spill into an AGPR under register pressure -- would copy stale contents, so a read is not held across many steps
// either: issue it shortly before its wait.  The current builds make no such copy (checked in the .s: every
// ds_read_b128 destination is next touched by the s_waitcnt statement or the MFMA behind it), and
// tests/test_gpu_in_proj.py compares every output element on every build.
template <int OFF, typename V>
__device__ __forceinline__ void lds_read16(V& dst, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
}
// LDS operations of a wave return in order: at most N of them still outstanding means every read older than the N youngest
// has landed.  `v` ties the wait to the value about to be used.
template <int N, typename V>
__device__ __forceinline__ void lds_wait(V& v) {
  asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(v) : "n"(N) : "memory");
}

// ---- two bf16 in a dword (the element at the lower address in the low half) ----------------------------------------------
__device__ __forceinline__ unsigned bf16_pack2(float lo, float hi) {
  return static_cast<unsigned>(f32_to_bf16(lo)) | (static_cast<unsigned>(f32_to_bf16(hi)) << 16);
}
__device__ __forceinline__ float bf16_lo(unsigned w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float bf16_hi(unsigned w) { return __builtin_bit_cast(float, w & 0xffff0000u); }

}  // namespace simamba
