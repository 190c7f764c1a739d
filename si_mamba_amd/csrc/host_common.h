// Shared host helpers of the entry points: what they all make of `io_dtype`, and of a pointer's alignment.
#pragma once
#include "common.h"

namespace simamba {

inline int check_io_dtype(int io_dtype) {
  return (io_dtype != SIMAMBA_F32 && io_dtype != SIMAMBA_BF16) ? SIMAMBA_E_DTYPE : SIMAMBA_OK;
}
inline size_t io_esz(int io_dtype) { return io_dtype == SIMAMBA_F32 ? 4 : 2; }      // bytes per activation element
inline int io_pack(int io_dtype) { return io_dtype == SIMAMBA_F32 ? 4 : 8; }        // elements per 16 bytes
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// f(T{}) with T the element type of a checked io_dtype:
//   with_io_type(io_dtype, [&](auto tag) { using T = decltype(tag); hipLaunchKernelGGL(kernel<T>, ...); });
template <typename F>
inline decltype(auto) with_io_type(int io_dtype, F&& f) {
  if (io_dtype == SIMAMBA_F32) return f(float{});
  return f(bf16_t{});
}

}  // namespace simamba
