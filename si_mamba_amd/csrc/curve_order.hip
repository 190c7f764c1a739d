// Space-filling-curve token orders: centres (B, G, 3) -> order (B, k, G), one launch, one workgroup per (cloud, curve).
//
// Per workgroup: the box (the cloud's own isotropic cube, or one fixed cube), every centre's cell on a 2^bits lattice in
// float64, the Morton or Hilbert code of the cell on the workgroup's curve and an ascending sort by (code, patch index).
// The cell is a subtraction, a division and a multiplication by a power of two in float64 -- each one correctly
// rounded operation with nothing to contract -- so a numpy restatement (tests/curve_ref.py) gives the same integers.
// code << 13 | index is one 64-bit key (48 + 13 bits), which makes the tie-break part of the compare; the keys are
// sorted by a bitonic network in LDS over the next power of two, padded with all-ones keys (64 KB at G = 8192).
// The k curves of a cloud are k workgroups, each with the box and the cells to itself: the sort is a chain of barriers
// (28 stages at G = 128, 91 at 8192) on B of 256 CUs, so the curves side by side cost what one costs, and three floats
// per centre read k times cost nothing next to it.  Plain vector stores only, no atomics, nothing
// read on the host: the same bits on every call.
#include <math.h>

#include "common.h"
#include "host_common.h"

namespace simamba {
namespace {

constexpr int kCurveMaxG = 8192;
constexpr int kCurveMaxK = 8;
constexpr int kCurveMaxBits = 16;
constexpr int kCurveIndexBits = 13;                    // 2^13 = kCurveMaxG patch indices under the code
constexpr int kCurveMaxThreads = 1024;
constexpr unsigned long long kCurvePad = ~0ull;        // above every real key (61 bits)

struct CurveArgs {
  const float* centers;
  long long* order;
  long long* codes;
  int G, n, k, bits, box;
  float lo, hi;
  int curve[kCurveMaxK];
};

__device__ __forceinline__ bool finite_bits(float x) {
  return (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) != 0x7f800000u;
}

// bit i of the low 16 bits of v -> bit 3 i
__device__ __forceinline__ unsigned long long spread3(uint32_t v) {
  unsigned long long x = v & 0xffffu;
  x = (x | x << 16) & 0x0000ff0000ffull;
  x = (x | x << 8) & 0x00f00f00f00full;
  x = (x | x << 4) & 0x0c30c30c30c3ull;
  x = (x | x << 2) & 0x249249249249ull;
  return x;
}

// bit i of X[0], X[1], X[2] -> bits 3 i + 2, 3 i + 1, 3 i
__device__ __forceinline__ unsigned long long interleave3(const uint32_t (&X)[3]) {
  return spread3(X[0]) << 2 | spread3(X[1]) << 1 | spread3(X[2]);
}

// Skilling, "Programming the Hilbert curve" (2004), AxestoTranspose for three axes of `bits` bits: X becomes the
// Hilbert index in transposed form, which interleave3 reads out.
__device__ __forceinline__ void hilbert_transpose(uint32_t (&X)[3], int bits) {
  const uint32_t M = 1u << (bits - 1);
  for (uint32_t Q = M; Q > 1; Q >>= 1) {
    const uint32_t P = Q - 1;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if (X[i] & Q) {
        X[0] ^= P;
      } else {
        const uint32_t t = (X[0] ^ X[i]) & P;
        X[0] ^= t;
        X[i] ^= t;
      }
    }
  }
  X[1] ^= X[0];
  X[2] ^= X[1];
  uint32_t t = 0;
  for (uint32_t Q = M; Q > 1; Q >>= 1)
    if (X[2] & Q) t ^= Q - 1;
  X[0] ^= t;
  X[1] ^= t;
  X[2] ^= t;
}

// Ascending bitonic sort of keys[0 .. n), n a power of two, by the whole workgroup; ends in a barrier.
__device__ __forceinline__ void bitonic_sort_lds(unsigned long long* keys, int n) {
  const int T = blockDim.x;
  for (int span = 2; span <= n; span <<= 1) {
    for (int j = span >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (n >> 1); t += T) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int l = i | j;
        const unsigned long long lo = keys[i], hi = keys[l];
        if ((lo > hi) == ((i & span) == 0)) {
          keys[i] = hi;
          keys[l] = lo;
        }
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(kCurveMaxThreads) void curve_order_kernel(const CurveArgs a) {
  extern __shared__ unsigned long long keys[];
  const int tid = threadIdx.x, T = blockDim.x, G = a.G;
  const long long cloud = blockIdx.x;
  const float* __restrict__ c = a.centers + cloud * G * 3;

  // ---- box: per-axis minimum and the largest extent of the finite coordinates, or the fixed cube
  float lo[3], ext;
  if (a.box == SIMAMBA_CURVE_BOX_FIXED) {
    lo[0] = lo[1] = lo[2] = a.lo;
    ext = a.hi - a.lo;
  } else {
    float hi[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      lo[d] = INFINITY;
      hi[d] = -INFINITY;
    }
    for (int i = tid; i < G; i += T) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const float x = c[3 * i + d];
        if (finite_bits(x)) {
          lo[d] = fminf(lo[d], x);
          hi[d] = fmaxf(hi[d], x);
        }
      }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      lo[d] = -wave_xor_max(-lo[d]);
      hi[d] = wave_xor_max(hi[d]);
    }
    const int waves = T >> 6;
    if (waves > 1) {                                   // 6 floats per wave, in the key buffer before it holds keys
      float* red = reinterpret_cast<float*>(keys);
      if ((tid & 63) == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          red[(tid >> 6) * 6 + d] = lo[d];
          red[(tid >> 6) * 6 + 3 + d] = hi[d];
        }
      }
      __syncthreads();
      for (int w = 0; w < waves; ++w) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          lo[d] = fminf(lo[d], red[w * 6 + d]);
          hi[d] = fmaxf(hi[d], red[w * 6 + 3 + d]);
        }
      }
      __syncthreads();
    }
    ext = 0.f;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (hi[d] >= lo[d]) ext = fmaxf(ext, hi[d] - lo[d]);
      else lo[d] = 0.f;                                // no finite coordinate on this axis: every cell is the last
    }
  }

  // ---- cells, float64: q = floor((x - lo) / ext * 2^bits) clamped to [0, 2^bits - 1]
  const uint32_t top = (1u << a.bits) - 1u;
  const double scale = static_cast<double>(1u << a.bits);
  const int id = a.curve[blockIdx.y];
  const long long row = (cloud * a.k + blockIdx.y) * G;
  for (int i = tid; i < G; i += T) {
    uint32_t X[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float x = c[3 * i + d];
      if (!finite_bits(x)) {
        X[d] = top;
      } else if (ext == 0.f) {
        X[d] = 0;
      } else {
        const double v = (static_cast<double>(x) - static_cast<double>(lo[d])) / static_cast<double>(ext) * scale;
        X[d] = !(v >= 0.0) ? 0u : (v >= scale ? top : static_cast<uint32_t>(v));
      }
    }
    // ---- the code on this workgroup's curve, and the key
    if (id & SIMAMBA_CURVE_TRANS) {
      const uint32_t t = X[0];
      X[0] = X[1];
      X[1] = t;
    }
    if (id & SIMAMBA_CURVE_HILBERT) hilbert_transpose(X, a.bits);
    const unsigned long long code = interleave3(X);
    if (a.codes) a.codes[row + i] = static_cast<long long>(code);
    keys[i] = code << kCurveIndexBits | static_cast<unsigned long long>(i);
  }
  for (int i = G + tid; i < a.n; i += T) keys[i] = kCurvePad;
  __syncthreads();
  bitonic_sort_lds(keys, a.n);
  for (int r = tid; r < G; r += T) a.order[row + r] = static_cast<long long>(keys[r] & (kCurveMaxG - 1));
}

}  // namespace
}  // namespace simamba

using namespace simamba;

extern "C" int simamba_curve_order(const float* centers, const int* curves, long long* order, long long* codes,
                                   int B, int G, int k, int bits, int box, float box_lo, float box_hi, void* stream) {
  if (B < 0 || G < 2 || G > kCurveMaxG || k < 1 || k > kCurveMaxK || bits < 1 || bits > kCurveMaxBits)
    return SIMAMBA_E_SHAPE;
  if (!centers || !curves || !order) return SIMAMBA_E_NULLPTR;
  if (box != SIMAMBA_CURVE_BOX_CLOUD && box != SIMAMBA_CURVE_BOX_FIXED) return SIMAMBA_E_VARIANT;
  CurveArgs a{};
  for (int i = 0; i < k; ++i) {
    if (curves[i] < 0 || curves[i] > (SIMAMBA_CURVE_HILBERT | SIMAMBA_CURVE_TRANS)) return SIMAMBA_E_VARIANT;
    a.curve[i] = curves[i];
  }
  if (box == SIMAMBA_CURVE_BOX_FIXED && !(std::isfinite(box_lo) && std::isfinite(box_hi) && box_lo < box_hi))
    return SIMAMBA_E_SHAPE;
  if (B == 0) return SIMAMBA_OK;
  int n = 2;
  while (n < G) n <<= 1;
  const int threads = n / 2 < 64 ? 64 : (n / 2 > kCurveMaxThreads ? kCurveMaxThreads : n / 2);
  const int lds = static_cast<int>(sizeof(unsigned long long)) * n;
  a.centers = centers;
  a.order = order;
  a.codes = codes;
  a.G = G;
  a.n = n;
  a.k = k;
  a.bits = bits;
  a.box = box;
  a.lo = box_lo;
  a.hi = box_hi;
  if (lds >= 64 * 1024)
    if (const hipError_t e = ensure_lds_cap<curve_order_kernel>(lds)) return static_cast<int>(e);
  hipLaunchKernelGGL(curve_order_kernel, dim3(B, k), dim3(threads), lds, static_cast<hipStream_t>(stream), a);
  return static_cast<int>(hipGetLastError());
}
