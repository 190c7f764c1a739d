// Chamfer distance between whole clouds (1 <= n, m <= 8192 points per set), with gradients for both sets: the tiled
// family beside the one-wave kernels of chamfer.hip (n, m <= 64, the MAE patch loss).  pytorch3d semantics: squared
// L2 to the nearest neighbour, mean over each set's points, both directions summed; one value per pair of sets.
//
//   * chamfer_large_nn_kernel: both directions in one launch.  A workgroup owns 256 * Q query points of one set of
//     one pair (Q = 1, 2 or 4 per thread, in registers) and walks the other set in LDS tiles of kChTile points,
//     staged coalesced and padded to (x, y, z, -) so that one LDS read serves a target (ds_read_b96 here, where the
//     fourth dword is unused; ds_read_b128 in the backward, where it carries an index); every lane reads the same
//     address (a broadcast), and Q queries share each read.  Distance from direct differences, dx*dx + dy*dy + dz*dz
//     as in chamfer.hip; strict `<` in ascending target index, so the lowest index wins a tie.  Writes the nearest
//     distance (fp32) and index (int32) of every query.
//   * chamfer_large_reduce_kernel: dist[p] = mean_i d1[p, i] + mean_j d2[p, j], one workgroup per pair, fp64 partial
//     sums in a fixed order (thread t takes elements t, t + 256, ...; then a tree over the 256 threads).  No atomics.
//   * chamfer_large_bwd_kernel: for either or both sets,
//       dX_i = g ( 2/n (x_i - y[a(i)]) + 2/m sum_{j : b(j) = i} (x_i - y_j) ),
//     the reverse matches found by the same tiled sweep: the tile holds (y_j, b(j)) in one float4, a thread compares
//     b(j) against its own i and adds in ascending j.  n * m compares like the forward, no float atomics: the same
//     bits on every call.
// The result of a query does not depend on Q, the tile size or the grid mapping.
//
// Ragged batches and pytorch3d's other arguments (simamba_chamfer_ragged_*) run the same three kernels:
//   * per-pair lengths xlen[p], ylen[p] (NULL = the padded n, m), clamped to [1, n] and [1, m] here and read once per
//     workgroup (a uniform load).  The grid is sized by the padded n, m; a workgroup whose first query lies at or behind
//     its pair's length writes that part of the padding (distance 0, index 0, gradient 0) and leaves before the first
//     barrier, the others loop to the pair's own target length: no address at or behind a length is loaded, and every
//     pair's result is what the pair returns alone.
//   * NORM, a template parameter: 2 = squared L2 as above, 1 = |dx| + |dy| + |dz| (abs is an operand modifier of the
//     adds), gradient sign(a - b) per coordinate with sign(0) = 0.
//   * the reduce kernel divides by the length (mean) or not at all (sum) and is not launched for no reduction; the
//     backward's coefficients are ddist / length, ddist, or (POINTWISE) per-point upstream gradients that ride with
//     the tile in a second LDS array; one-way (x against y only) has no y blocks in the forward, and in the backward x
//     keeps its own-nearest term and y the reverse matches.
// NaN and inf do not propagate as they do in pytorch3d: the search starts from 3.0e38 with a strict `<`, as in
// chamfer.hip, so a query with a NaN coordinate, or one whose targets are all NaN, reports distance 3.0e38 and index 0,
// and a diverged cloud shows as a huge finite (or inf) loss, not as NaN.
#include <type_traits>

#include "host_common.h"
#include "pointset.h"

namespace simamba {

constexpr int kChThreads = 256;
constexpr int kChTile = 1024;        // targets per LDS tile: 16 KB
constexpr int kChMaxPoints = 8192;

// rho(a, b) of one coordinate triple, from the differences
template <int NORM>
__device__ __forceinline__ float rho(float dx, float dy, float dz) {
  if constexpr (NORM == 2) return dx * dx + dy * dy + dz * dz;
  else return fabsf(dx) + fabsf(dy) + fabsf(dz);
}

// d rho / d (difference) up to the factor the caller folds into its coefficient (2 for L2): d, or sign(d)
template <int NORM>
__device__ __forceinline__ float drho(float d) {
  if constexpr (NORM == 2) return d;
  else return static_cast<float>(d > 0.f) - static_cast<float>(d < 0.f);
}

// Work item `r` of a pair: blocks [0, bx) serve set X against Y, blocks [bx, bx + by) set Y against X (by = 0: one-way).
template <int Q, int NORM>
__global__ __launch_bounds__(kChThreads) void chamfer_large_nn_kernel(const float* __restrict__ x,
                                                                      const float* __restrict__ y,
                                                                      const int* __restrict__ xlen,
                                                                      const int* __restrict__ ylen,
                                                                      int* __restrict__ idx1, int* __restrict__ idx2,
                                                                      float* __restrict__ d1, float* __restrict__ d2,
                                                                      int n, int m, int bx, int by) {
  __shared__ float4 sT[kChTile];
  const long long pr = blockIdx.x / (bx + by);
  const int r = static_cast<int>(blockIdx.x - pr * (bx + by));
  const bool fwd = r < bx;                                       // workgroup-uniform
  const int nqp = fwd ? n : m, ntp = fwd ? m : n;                // padded sizes: the strides
  const int nq = clamped_length(fwd ? xlen : ylen, pr, nqp), nt = clamped_length(fwd ? ylen : xlen, pr, ntp);
  const float* qs = (fwd ? x : y) + pr * nqp * 3;
  const float* ts = (fwd ? y : x) + pr * ntp * 3;
  int* oi = (fwd ? idx1 : idx2) + pr * nqp;
  float* od = (fwd ? d1 : d2) + pr * nqp;
  const int q0 = (fwd ? r : r - bx) * (kChThreads * Q) + threadIdx.x;
  if (q0 - static_cast<int>(threadIdx.x) >= nq) {                // all padding: zeros, and out before any barrier
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int i = q0 + q * kChThreads;
      if (i < nqp) { od[i] = 0.f; oi[i] = 0; }
    }
    return;
  }

  float qx[Q], qy[Q], qz[Q], best[Q];
  int bi[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int i = min(q0 + q * kChThreads, nq - 1);              // lanes past the end repeat the last query
    qx[q] = qs[3 * i]; qy[q] = qs[3 * i + 1]; qz[q] = qs[3 * i + 2];
    best[q] = 3.0e38f; bi[q] = 0;
  }
  const bool wave_live = q0 - (threadIdx.x & 63) < nq;           // a wave with no query only helps staging
  for (int t0 = 0; t0 < nt; t0 += kChTile) {
    const int cnt = min(kChTile, nt - t0);
    __syncthreads();
    stage_points<kChThreads>(sT, ts, t0, cnt);
    __syncthreads();
    if (!wave_live) continue;
#pragma unroll 4
    for (int j = 0; j < cnt; ++j) {
      const float4 t = sT[j];
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const float dx = qx[q] - t.x, dy = qy[q] - t.y, dz = qz[q] - t.z;
        const float d = rho<NORM>(dx, dy, dz);
        if (d < best[q]) { best[q] = d; bi[q] = t0 + j; }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int i = q0 + q * kChThreads;
    if (i < nq) { od[i] = best[q]; oi[i] = bi[q]; }
    else if (i < nqp) { od[i] = 0.f; oi[i] = 0; }
  }
}

__global__ __launch_bounds__(kChThreads) void chamfer_large_reduce_kernel(const float* __restrict__ d1,
                                                                          const float* __restrict__ d2,
                                                                          const int* __restrict__ xlen,
                                                                          const int* __restrict__ ylen,
                                                                          float* __restrict__ dist, int n, int m,
                                                                          int mean) {
  __shared__ double sS[2][kChThreads];
  const long long pr = blockIdx.x;
  const int nx = clamped_length(xlen, pr, n), ny = clamped_length(ylen, pr, m);
  const float* a = d1 + pr * n;
  const float* b = d2 ? d2 + pr * m : nullptr;                   // one-way: no second term
  double t1 = 0.0, t2 = 0.0;
  for (int i = threadIdx.x; i < nx; i += kChThreads) t1 += static_cast<double>(a[i]);
  if (b)
    for (int j = threadIdx.x; j < ny; j += kChThreads) t2 += static_cast<double>(b[j]);
  sS[0][threadIdx.x] = t1; sS[1][threadIdx.x] = t2;
  block_tree_sum(sS);
  if (threadIdx.x == 0) {
    const double a1 = mean ? sS[0][0] / nx : sS[0][0], a2 = mean ? sS[1][0] / ny : sS[1][0];
    dist[pr] = static_cast<float>(b ? a1 + a2 : a1);
  }
}

// Blocks [0, bx) of a pair write dx, blocks [bx, bx + by) dy; bx or by is 0 when that gradient is not wanted.
// `mean`: the coefficients are ddist / length, else ddist (sum).  POINTWISE: they are dd1[p][i], dd2[p][j] instead
// (no reduction), and those of the other set ride with the tile in sC.  `oneway`: x has no reverse matches and y has
// no nearest of its own.
template <int Q, int NORM, bool POINTWISE>
__global__ __launch_bounds__(kChThreads) void chamfer_large_bwd_kernel(const float* __restrict__ x,
                                                                       const float* __restrict__ y,
                                                                       const int* __restrict__ xlen,
                                                                       const int* __restrict__ ylen,
                                                                       const float* __restrict__ ddist,
                                                                       const float* __restrict__ dd1,
                                                                       const float* __restrict__ dd2,
                                                                       const int* __restrict__ idx1,
                                                                       const int* __restrict__ idx2,
                                                                       float* __restrict__ dx, float* __restrict__ dy,
                                                                       int n, int m, int bx, int by, int mean,
                                                                       int oneway) {
  __shared__ float4 sT[kChTile];
  __shared__ float sC[POINTWISE ? kChTile : 1];
  constexpr float kScale = NORM == 2 ? 2.f : 1.f;
  const long long pr = blockIdx.x / (bx + by);
  const int r = static_cast<int>(blockIdx.x - pr * (bx + by));
  const bool forx = r < bx;
  const int nsp = forx ? n : m, nop = forx ? m : n;              // own set, other set: padded sizes (the strides)
  const int ns = clamped_length(forx ? xlen : ylen, pr, nsp), no = clamped_length(forx ? ylen : xlen, pr, nop);
  const float* self = (forx ? x : y) + pr * nsp * 3;
  const float* other = (forx ? y : x) + pr * nop * 3;
  const int* near_other = (forx ? idx1 : idx2) + pr * nsp;       // nearest of the other set, per own point
  const int* near_self = (forx ? idx2 : idx1) + pr * nop;        // nearest own point, per point of the other set
  float* out = (forx ? dx : dy) + pr * nsp * 3;
  const int q0 = (forx ? r : r - bx) * (kChThreads * Q) + threadIdx.x;
  if (q0 - static_cast<int>(threadIdx.x) >= ns) {                // all padding: zeros, and out before any barrier
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int i = q0 + q * kChThreads;
      if (i < nsp) { out[3 * i] = 0.f; out[3 * i + 1] = 0.f; out[3 * i + 2] = 0.f; }
    }
    return;
  }
  const bool nearest = forx || !oneway, reverse = !forx || !oneway;      // the two terms; workgroup-uniform
  const float* c_self = POINTWISE ? (forx ? dd1 : dd2) + pr * nsp : nullptr;
  const float* c_other = POINTWISE ? (forx ? dd2 : dd1) + pr * nop : nullptr;
  float k1 = 0.f, k2 = 0.f;
  if constexpr (!POINTWISE) {
    const float g = ddist[pr];
    k1 = mean ? kScale * g / static_cast<float>(ns) : kScale * g;
    k2 = mean ? kScale * g / static_cast<float>(no) : kScale * g;
  }

  float px[Q], py[Q], pz[Q], gx[Q], gy[Q], gz[Q];
  int own[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int i = q0 + q * kChThreads;
    const int ic = min(i, ns - 1);
    own[q] = i < ns ? i : -1;                                    // -1 matches no index
    px[q] = self[3 * ic]; py[q] = self[3 * ic + 1]; pz[q] = self[3 * ic + 2];
    gx[q] = 0.f; gy[q] = 0.f; gz[q] = 0.f;
    if (nearest) {
      if constexpr (POINTWISE) k1 = kScale * c_self[ic];
      const int a = min(max(near_other[ic], 0), no - 1);         // an index from outside the forward stays in range
      gx[q] = k1 * drho<NORM>(px[q] - other[3 * a]); gy[q] = k1 * drho<NORM>(py[q] - other[3 * a + 1]);
      gz[q] = k1 * drho<NORM>(pz[q] - other[3 * a + 2]);
    }
  }
  const bool wave_live = q0 - (threadIdx.x & 63) < ns;
  for (int t0 = 0; reverse && t0 < no; t0 += kChTile) {
    const int cnt = min(kChTile, no - t0);
    __syncthreads();
    stage_points<kChThreads>(sT, other, t0, cnt);
    stage_w<kChThreads>(sT, near_self, t0, cnt);    // (y_j, b(j)) in one float4
    if constexpr (POINTWISE)
      for (int t = threadIdx.x; t < cnt; t += kChThreads) sC[t] = kScale * c_other[t0 + t];
    __syncthreads();
    if (!wave_live) continue;
#pragma unroll 4
    for (int j = 0; j < cnt; ++j) {
      const float4 t = sT[j];
      const int b = __builtin_bit_cast(int, t.w);
      if constexpr (POINTWISE) k2 = sC[j];
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        if (b == own[q]) {
          gx[q] += k2 * drho<NORM>(px[q] - t.x); gy[q] += k2 * drho<NORM>(py[q] - t.y);
          gz[q] += k2 * drho<NORM>(pz[q] - t.z);
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int i = q0 + q * kChThreads;
    if (i < ns) { out[3 * i] = gx[q]; out[3 * i + 1] = gy[q]; out[3 * i + 2] = gz[q]; }
    else if (i < nsp) { out[3 * i] = 0.f; out[3 * i + 1] = 0.f; out[3 * i + 2] = 0.f; }
  }
}

// Queries per thread: as many as still leave two workgroups per CU, and no more than the smaller set fills.
inline int chamfer_large_q(long long pairs, int n, int m) {
  for (int q = 4; q > 1; q >>= 1) {
    const int per = kChThreads * q;
    if (n >= per && m >= per && pairs * ((n + per - 1) / per + (m + per - 1) / per) >= 512) return q;
  }
  return 1;
}

// f(std::integral_constant<int, Q>{}) for the chosen Q
template <typename F>
inline void with_queries_per_thread(int q, F&& f) {
  if (q == 4) f(std::integral_constant<int, 4>{});
  else if (q == 2) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 1>{});
}

// f(std::integral_constant<int, NORM>{}) for norm 1 or 2
template <typename F>
inline void with_norm(int norm, F&& f) {
  if (norm == 1) f(std::integral_constant<int, 1>{});
  else f(std::integral_constant<int, 2>{});
}

constexpr int kChMean = 0, kChSum = 1, kChNone = 2;              // `reduction`
constexpr int kChOneWay = 1;                                     // `flags`

// `queries`: 0 = chamfer_large_q's choice; 1, 2 or 4 force that kernel (parity tests)
inline int chamfer_large_check(long long pairs, int n, int m, int queries, int norm = 2, int reduction = kChMean,
                               int flags = 0) {
  if (queries != 0 && queries != 1 && queries != 2 && queries != 4) return SIMAMBA_E_VARIANT;
  if ((norm != 1 && norm != 2) || (reduction != kChMean && reduction != kChSum && reduction != kChNone) ||
      (flags & ~kChOneWay))
    return SIMAMBA_E_VARIANT;
  if (pairs < 0 || n < 1 || m < 1 || n > kChMaxPoints || m > kChMaxPoints) return SIMAMBA_E_SHAPE;
  return SIMAMBA_OK;
}

}  // namespace simamba

using namespace simamba;

extern "C" int simamba_chamfer_ragged_fwd(const float* x, const float* y, const int* xlen, const int* ylen,
                                          float* dist, int* idx1, int* idx2, float* d1, float* d2, long long pairs,
                                          int n, int m, int norm, int reduction, int flags, int queries,
                                          void* stream) {
  if (const int rc = chamfer_large_check(pairs, n, m, queries, norm, reduction, flags)) return rc;
  if (pairs == 0) return SIMAMBA_OK;
  const bool oneway = flags & kChOneWay;
  if (!x || !y || !idx1 || !d1 || (reduction != kChNone && !dist) || (!oneway && (!idx2 || !d2)))
    return SIMAMBA_E_NULLPTR;
  const int q = queries ? queries : chamfer_large_q(pairs, n, m), per = kChThreads * q;
  const int bx = (n + per - 1) / per, by = oneway ? 0 : (m + per - 1) / per;
  const long long grid = pairs * (bx + by);
  if (grid > 0x7fffffffll) return SIMAMBA_E_SHAPE;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 g(static_cast<unsigned>(grid)), b(kChThreads);
  with_queries_per_thread(q, [&](auto tq) {
    with_norm(norm, [&](auto tn) {
      hipLaunchKernelGGL((chamfer_large_nn_kernel<decltype(tq)::value, decltype(tn)::value>), g, b, 0, st, x, y, xlen,
                         ylen, idx1, idx2, d1, d2, n, m, bx, by);
    });
  });
  if (const hipError_t e = hipGetLastError()) return static_cast<int>(e);
  if (reduction == kChNone) return SIMAMBA_OK;
  hipLaunchKernelGGL(chamfer_large_reduce_kernel, dim3(static_cast<unsigned>(pairs)), b, 0, st, d1,
                     oneway ? nullptr : d2, xlen, ylen, dist, n, m, reduction == kChMean);
  return static_cast<int>(hipGetLastError());
}

extern "C" int simamba_chamfer_large_fwd_ex(const float* x, const float* y, float* dist, int* idx1, int* idx2,
                                            float* d1, float* d2, long long pairs, int n, int m, int queries,
                                            void* stream) {
  return simamba_chamfer_ragged_fwd(x, y, nullptr, nullptr, dist, idx1, idx2, d1, d2, pairs, n, m, 2, kChMean, 0,
                                    queries, stream);
}

extern "C" int simamba_chamfer_large_fwd(const float* x, const float* y, float* dist, int* idx1, int* idx2, float* d1,
                                         float* d2, long long pairs, int n, int m, void* stream) {
  return simamba_chamfer_large_fwd_ex(x, y, dist, idx1, idx2, d1, d2, pairs, n, m, 0, stream);
}

extern "C" int simamba_chamfer_ragged_bwd(const float* x, const float* y, const int* xlen, const int* ylen,
                                          const float* ddist, const float* dd1, const float* dd2, const int* idx1,
                                          const int* idx2, float* dx, float* dy, long long pairs, int n, int m,
                                          int norm, int reduction, int flags, int queries, void* stream) {
  if (const int rc = chamfer_large_check(pairs, n, m, queries, norm, reduction, flags)) return rc;
  if (pairs == 0) return SIMAMBA_OK;
  const bool oneway = flags & kChOneWay, pointwise = reduction == kChNone;
  if (!x || !y || !idx1 || (!oneway && !idx2)) return SIMAMBA_E_NULLPTR;
  if (pointwise ? (!dd1 || (!oneway && !dd2)) : !ddist) return SIMAMBA_E_NULLPTR;
  if (!dx && !dy) return SIMAMBA_OK;
  const int q = queries ? queries : chamfer_large_q(pairs, n, m), per = kChThreads * q;
  const int bx = dx ? (n + per - 1) / per : 0, by = dy ? (m + per - 1) / per : 0;
  const long long grid = pairs * (bx + by);
  if (grid > 0x7fffffffll) return SIMAMBA_E_SHAPE;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 g(static_cast<unsigned>(grid)), b(kChThreads);
  const int mean = reduction == kChMean, ow = oneway;
  with_queries_per_thread(q, [&](auto tq) {
    with_norm(norm, [&](auto tn) {
      constexpr int Q = decltype(tq)::value, NORM = decltype(tn)::value;
      if (pointwise)
        hipLaunchKernelGGL((chamfer_large_bwd_kernel<Q, NORM, true>), g, b, 0, st, x, y, xlen, ylen, ddist, dd1, dd2,
                           idx1, idx2, dx, dy, n, m, bx, by, mean, ow);
      else
        hipLaunchKernelGGL((chamfer_large_bwd_kernel<Q, NORM, false>), g, b, 0, st, x, y, xlen, ylen, ddist, dd1, dd2,
                           idx1, idx2, dx, dy, n, m, bx, by, mean, ow);
    });
  });
  return static_cast<int>(hipGetLastError());
}

extern "C" int simamba_chamfer_large_bwd_ex(const float* x, const float* y, const float* ddist, const int* idx1,
                                            const int* idx2, float* dx, float* dy, long long pairs, int n, int m,
                                            int queries, void* stream) {
  return simamba_chamfer_ragged_bwd(x, y, nullptr, nullptr, ddist, nullptr, nullptr, idx1, idx2, dx, dy, pairs, n, m, 2,
                                    kChMean, 0, queries, stream);
}

extern "C" int simamba_chamfer_large_bwd(const float* x, const float* y, const float* ddist, const int* idx1,
                                         const int* idx2, float* dx, float* dy, long long pairs, int n, int m,
                                         void* stream) {
  return simamba_chamfer_large_bwd_ex(x, y, ddist, idx1, idx2, dx, dy, pairs, n, m, 0, stream);
}
