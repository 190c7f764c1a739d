// y[i] = expf(x[i]) with the device library's expf as csrc/mix.hip calls it (the same compiler flags: -O3
// -ffp-contract=off, no fast-math), for tools/bench_mix.py to hold against float64.  Built as a shared library:
//   hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -shared tools/expf_probe.hip -o tools/expf_probe.so
#include <hip/hip_runtime.h>

__global__ void expf_probe_kernel(const float* __restrict__ x, float* __restrict__ y, long long n) {
  const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) y[i] = expf(x[i]);
}

extern "C" int expf_probe(const float* x, float* y, long long n, void* stream) {
  if (!x || !y || n < 1 || n > (1ll << 31)) return -1;
  const unsigned blocks = static_cast<unsigned>((n + 255) / 256);
  hipLaunchKernelGGL(expf_probe_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), x, y, n);
  return static_cast<int>(hipGetLastError());
}
