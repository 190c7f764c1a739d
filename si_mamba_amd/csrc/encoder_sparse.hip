// Backward of "linear, then max over the n points of a patch" (the patch encoder's last layer: reference
// models/point_mamba.py:57 + :68) without the dense gradient between the two.
//
// The max routes dout[g][c] to ONE of the patch's n rows, idx[g][c].  The dense route writes that as a (G n, C_out)
// matrix with n-1 of every n entries zero and runs two full GEMMs on it.  Here the zeros are never formed:
//
//   dX[g n + r][:] = sum over {c : idx[g][c] == r} of dout[g][c] * W[c][:]          (simamba_max_linear_bwd_dx)
//   dW[c][:]       = sum over g of dout[g][c] * X[g n + idx[g][c]][:]               (simamba_max_linear_bwd_dw)
//
// 1/n of the dense products, fp32 arithmetic, no atomics, a fixed order of every sum (ascending c, ascending g).
//
// Both kernels: a workgroup of 16 waves owns 64 columns (lane = column) and a slab of patches, so the row of W / X a
// product needs is wave-uniform and comes out of LDS as one conflict-free ds_read_b32 per wave.
//
//   dx : the 64-column block of W sits in LDS for the whole kernel (C_out x 64 fp32, 96 KB at C_out = 384: one workgroup
//        per CU).  A wave takes a patch: lane l holds idx / dout of channels l, 64 + l, ... in registers; for row r the
//        ballot of (idx == r) over each 64-channel chunk is the list of channels of that row, walked in ascending order
//        with scalar bit operations.  No LDS bucketing, no barrier after the staging of W.  Every row of dX is written
//        once, rows nobody chose as zeros.  An idx >= n matches no row.
//   dw : a wave owns C_out / 16 (<= 24) channels with one fp32 accumulator per channel and lane.  X tiles of 8 patches
//        (8 n x 64 fp32, plus a zero row that padding and bad indices read) are double-buffered in LDS, the next tile's global loads in flight during the products; X is
//        read once overall.  Per-slab partials (slabs, C_out, C_in) are summed in slab order by det_reduce.hip.
#include "det_reduce.h"
#include "host_common.h"

namespace simamba {

constexpr int kSpCols = 64;                         // columns per workgroup = lanes of a wave
constexpr int kSpWaves = 16;
constexpr int kSpThreads = kSpWaves * 64;
constexpr int kSpMaxN = 32;                         // points per patch
constexpr int kSpMaxCout = 384;                     // rows of the W block in LDS (96 KB)
constexpr int kSpChunks = kSpMaxCout / 64;
constexpr int kSpCpw = kSpMaxCout / kSpWaves;       // dw: channels per wave
constexpr int kSpTilePatches = 8;                   // dw: patches per LDS tile
constexpr int kSpTileRegs = kSpCpw / 8;             // dw: (idx, dout) registers per lane and tile
constexpr int kSpTileQuads = kSpTilePatches * kSpMaxN * (kSpCols / 4) / kSpThreads;   // 16-byte loads per thread
constexpr int kSpTargetWorkgroups = 256;            // one per CU
constexpr long long kSpMaxGroups = 1ll << 30;      // slab and grid arithmetic stay in 32 bits
constexpr int kSpDxMinSlab = kSpWaves;              // dx: patches per workgroup at least (the W block is staged per workgroup)
static_assert(kSpTilePatches * 8 == 64 && kSpCpw % 8 == 0, "a register holds 8 channels of each of a tile's 8 patches");

template <typename T>
__device__ __forceinline__ float4 load_quad(const T* p) {
  const Pack<T, 4> pk = *reinterpret_cast<const Pack<T, 4>*>(p);
  return make_float4(to_f32<T>(pk.v[0]), to_f32<T>(pk.v[1]), to_f32<T>(pk.v[2]), to_f32<T>(pk.v[3]));
}

__device__ __forceinline__ float read_lane(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// ---- input gradient -----------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kSpThreads) void max_linear_bwd_dx_kernel(
    const T* __restrict__ dout, const unsigned char* __restrict__ idx, const T* __restrict__ W, T* __restrict__ dx,
    long long groups, int n, int cin, int cout, int slab) {
  extern __shared__ __attribute__((aligned(16))) float sW[];          // [cout][64]
  const int col0 = blockIdx.x * kSpCols;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int e = threadIdx.x; e < cout * (kSpCols / 4); e += kSpThreads) {
    const int c = e / (kSpCols / 4), q = e % (kSpCols / 4);
    *reinterpret_cast<float4*>(sW + c * kSpCols + 4 * q) = load_quad<T>(W + static_cast<long long>(c) * cin + col0 + 4 * q);
  }
  __syncthreads();
  const float* wl = sW + lane;
  const long long g0 = static_cast<long long>(blockIdx.y) * slab;
  const long long g1 = min(g0 + slab, groups);
  for (long long g = g0 + wave; g < g1; g += kSpWaves) {
    int id[kSpChunks];
    float d[kSpChunks];
#pragma unroll
    for (int k = 0; k < kSpChunks; ++k) {
      const int c = 64 * k + lane;
      const bool ok = c < cout;
      id[k] = ok ? static_cast<int>(idx[g * cout + c]) : 255;            // 255: no row (n <= 32)
      d[k] = ok ? to_f32<T>(dout[g * cout + c]) : 0.f;
    }
    T* out = dx + g * n * cin + col0 + lane;
    for (int r = 0; r < n; ++r) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < kSpChunks; ++k) {
        unsigned long long m = __ballot(id[k] == r);
        while (m) {                                                      // wave-uniform: ascending channel
          const int j = __builtin_ctzll(m);
          m &= m - 1;
          acc = fmaf(read_lane(d[k], j), wl[(64 * k + j) * kSpCols], acc);
        }
      }
      out[static_cast<long long>(r) * cin] = from_f32<T>(acc);
    }
  }
}

// ---- weight gradient ----------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kSpThreads) void max_linear_bwd_dw_kernel(
    const T* __restrict__ dout, const unsigned char* __restrict__ idx, const T* __restrict__ X,
    float* __restrict__ partial, long long groups, int n, int cin, int cout, int slab) {
  extern __shared__ __attribute__((aligned(16))) float sX[];          // [2][kSpTilePatches * n + 1][64]
  const int col0 = blockIdx.x * kSpCols;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int cpw = (cout + kSpWaves - 1) / kSpWaves;                    // channels per wave, <= kSpCpw
  const int c0 = wave * cpw;
  const int cnt = max(0, min(cpw, cout - c0));
  const int tile_rows = kSpTilePatches * n;
  const long long g0 = static_cast<long long>(blockIdx.y) * slab;
  const long long g1 = min(g0 + slab, groups);

  float acc[kSpCpw];
#pragma unroll
  for (int j = 0; j < kSpCpw; ++j) acc[j] = 0.f;

  float4 xq[kSpTileQuads];
  int id[kSpTileRegs];
  float d[kSpTileRegs];
  // this thread's share of the tile that starts at patch g: X quads, and the (idx, dout) of patch p = lane / 8, channel
  // j = 8 q + lane % 8 of this wave; what lies past the slab or the wave's channels is (zero row, 0)
  auto fetch = [&](long long g) {
    const long long rows = min(static_cast<long long>(kSpTilePatches), g1 - g) * n;
#pragma unroll
    for (int q = 0; q < kSpTileQuads; ++q) {
      const int e = q * kSpThreads + threadIdx.x;
      const int row = e / (kSpCols / 4), quad = e % (kSpCols / 4);
      xq[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < rows) xq[q] = load_quad<T>(X + (g * n + row) * cin + col0 + 4 * quad);
    }
#pragma unroll
    for (int q = 0; q < kSpTileRegs; ++q) {
      const int p = lane / 8, j = q * 8 + lane % 8;
      const bool ok = j < cnt && g + p < g1;
      const long long at = (g + p) * cout + c0 + j;
      const int r = ok ? static_cast<int>(idx[at]) : n;
      id[q] = r < n ? p * n + r : tile_rows;                            // row of the tile; padding and an idx >= n read
      d[q] = r < n ? to_f32<T>(dout[at]) : 0.f;                         // the tile's zero row: 0 * 0, whatever X holds
    }
  };

  if (threadIdx.x < 2 * kSpCols)                                        // each buffer's zero row, behind its tile
    sX[(threadIdx.x / kSpCols) * (tile_rows + 1) * kSpCols + tile_rows * kSpCols + threadIdx.x % kSpCols] = 0.f;
  int buf = 0;
  if (g0 < g1) fetch(g0);
  for (long long g = g0; g < g1; g += kSpTilePatches) {
    float* tile = sX + buf * (tile_rows + 1) * kSpCols;
#pragma unroll
    for (int q = 0; q < kSpTileQuads; ++q) {
      const int e = q * kSpThreads + threadIdx.x;
      if (e < tile_rows * (kSpCols / 4)) *reinterpret_cast<float4*>(tile + 4 * e) = xq[q];
    }
    int idc[kSpTileRegs];
    float dc[kSpTileRegs];
#pragma unroll
    for (int q = 0; q < kSpTileRegs; ++q) { idc[q] = id[q]; dc[q] = d[q]; }
    __syncthreads();
    if (g + kSpTilePatches < g1) fetch(g + kSpTilePatches);             // in flight during the products
    const float* xl = tile + lane;
#pragma unroll 1
    for (int p = 0; p < kSpTilePatches; ++p) {                          // rolled: 24 reads in flight are enough
#pragma unroll
      for (int j = 0; j < kSpCpw; ++j) {
        const int row = __builtin_amdgcn_readlane(idc[j / 8], p * 8 + j % 8);
        acc[j] = fmaf(read_lane(dc[j / 8], p * 8 + j % 8), xl[row * kSpCols], acc[j]);
      }
    }
    buf ^= 1;
  }
  float* out = partial + (static_cast<long long>(blockIdx.y) * cout + c0) * cin + col0 + lane;
#pragma unroll
  for (int j = 0; j < kSpCpw; ++j)
    if (j < cnt) out[static_cast<long long>(j) * cin] = acc[j];
}

constexpr int kSpDxLds = kSpMaxCout * kSpCols * 4;
constexpr int kSpDwLds = 2 * (kSpTilePatches * kSpMaxN + 1) * kSpCols * 4;

// dtype, empty, shape, pointers, alignment
static int max_linear_check(int io_dtype, long long groups, int n, int cin, int cout, bool pointers, bool aligned) {
  if (const int rc = check_io_dtype(io_dtype)) return rc;
  if (groups == 0) return 1;
  if (groups < 0 || groups > kSpMaxGroups || n < 1 || n > kSpMaxN || cin < kSpCols || (cin % kSpCols) != 0 ||
      cin > 65536 || cout < 4 || (cout % 4) != 0 || cout > kSpMaxCout)
    return SIMAMBA_E_SHAPE;
  if (!pointers) return SIMAMBA_E_NULLPTR;
  if (!aligned) return SIMAMBA_E_ALIGN;
  return SIMAMBA_OK;
}

// patches per workgroup for about one workgroup per CU, at least `floor`
static int slab_of(long long groups, int cin, int floor) {
  const long long slabs = max(1ll, static_cast<long long>(kSpTargetWorkgroups / (cin / kSpCols)));
  return static_cast<int>(max(static_cast<long long>(floor), (groups + slabs - 1) / slabs));
}

}  // namespace simamba

using namespace simamba;

extern "C" int simamba_max_linear_bwd_slabs(long long groups, int c_in) {
  if (groups <= 0 || c_in < kSpCols || (c_in % kSpCols) != 0) return 0;
  const int slab = slab_of(groups, c_in, kSpTilePatches);
  return static_cast<int>((groups + slab - 1) / slab);
}

extern "C" int simamba_max_linear_bwd_dx(const void* dout, const unsigned char* idx, const void* weight, void* dx,
                                         long long groups, int n, int c_in, int c_out, int io_dtype, void* stream) {
  if (const int rc = max_linear_check(io_dtype, groups, n, c_in, c_out, dout && idx && weight && dx,
                                      aligned16(dout) && aligned16(weight) && aligned16(dx)))
    return rc > 0 ? SIMAMBA_OK : rc;
  const int slab = slab_of(groups, c_in, kSpDxMinSlab);
  const dim3 grid(c_in / kSpCols, static_cast<unsigned>((groups + slab - 1) / slab));
  const size_t lds = sizeof(float) * c_out * kSpCols;
  return with_io_type(io_dtype, [&](auto tag) {
    using T = decltype(tag);
    if (const hipError_t e = ensure_lds_cap<max_linear_bwd_dx_kernel<T>>(kSpDxLds)) return static_cast<int>(e);
    hipLaunchKernelGGL(max_linear_bwd_dx_kernel<T>, grid, dim3(kSpThreads), lds, static_cast<hipStream_t>(stream),
                       static_cast<const T*>(dout), idx, static_cast<const T*>(weight), static_cast<T*>(dx), groups, n,
                       c_in, c_out, slab);
    return static_cast<int>(hipGetLastError());
  });
}

extern "C" int simamba_max_linear_bwd_dw(const void* dout, const unsigned char* idx, const void* x, float* dw,
                                         float* partial, long long groups, int n, int c_in, int c_out, int io_dtype,
                                         void* stream) {
  if (const int rc = max_linear_check(io_dtype, groups, n, c_in, c_out, dout && idx && x && dw && partial,
                                      aligned16(dout) && aligned16(x) && aligned16(dw) && aligned16(partial)))
    return rc > 0 ? SIMAMBA_OK : rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int slab = slab_of(groups, c_in, kSpTilePatches);
  const int slabs = static_cast<int>((groups + slab - 1) / slab);
  const dim3 grid(c_in / kSpCols, slabs);
  const size_t lds = sizeof(float) * 2 * (kSpTilePatches * n + 1) * kSpCols;
  const int rc = with_io_type(io_dtype, [&](auto tag) {
    using T = decltype(tag);
    if (const hipError_t e = ensure_lds_cap<max_linear_bwd_dw_kernel<T>>(kSpDwLds)) return static_cast<int>(e);
    hipLaunchKernelGGL(max_linear_bwd_dw_kernel<T>, grid, dim3(kSpThreads), lds, s, static_cast<const T*>(dout), idx,
                       static_cast<const T*>(x), partial, groups, n, c_in, c_out, slab);
    return static_cast<int>(hipGetLastError());
  });
  if (rc) return rc;
  const long long elems = static_cast<long long>(c_out) * c_in;
  const DetSumJob job{partial, dw, elems, elems, slabs};
  return det_sum_launch(&job, 1, s);
}
