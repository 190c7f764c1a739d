// Shared host helpers of the entry points: what they all make of `io_dtype`, and of a pointer's alignment.
#pragma once
#include <atomic>

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

// Raise kKernel's dynamic-LDS cap to `bytes`, once per kernel and device (the attribute belongs to the device's copy of
// the code object; `bytes` is a constant of the kernel, so this is not observable state).  Returns the hipError_t of the
// attribute call; a failure is not remembered, so the next call tries again.
template <auto kKernel>
inline hipError_t ensure_lds_cap(int bytes) {
  static std::atomic<unsigned long long> done{0};          // bit d: device d has the cap
  int dev = 0;
  if (const hipError_t e = hipGetDevice(&dev)) return e;
  const unsigned long long bit = (dev >= 0 && dev < 64) ? 1ull << dev : 0;
  if (bit && (done.load(std::memory_order_acquire) & bit)) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kKernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done.fetch_or(bit, std::memory_order_release);
  return e;
}

}  // namespace simamba
