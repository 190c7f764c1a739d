// k-NN graph and top-k Laplacian eigenpairs for 128 < G <= 512 patches ("large G").
//
// The G <= 128 kernels (spectral.hip, spectral_tridiag.hip) keep the whole G x G problem in LDS; at G = 512 the
// matrix alone is 1 MiB.  Here it lives in global memory instead, owned by one workgroup per sample, so the only
// ordering ever needed is the workgroup barrier (with its fence): no atomics, no traffic between workgroups.
//
//   knn_rows_kernel<false>  zero-fills rows of adj and writes the first index_put phase of the reference,
//                           A[i, nn] = w (every node writes its own row);
//   knn_rows_kernel<true>   the second phase, A[nn, i] = w (node i writes column i only), SYMMETRIC only.
//     The launch boundary orders the two phases.  128 nodes per workgroup, 8 lanes per node; the selection is
//     the lexicographic (distance, index) sweep of knn_graph_kernel with the distances recomputed from the
//     LDS-resident points in every pass (a node's 512 distances do not fit its registers), and the second
//     phase recomputes the lists rather than storing them.  Same arithmetic as knn_graph_kernel: identical edges,
//     identical weights.
//
//   laplacian_large_kernel  the algorithm of laplacian_tridiag_kernel with the matrix in the caller's workspace:
//     1. S = mirrored lower triangle of I - D^-1 A (or the MATRIX_SYM form), built exactly as there;
//     2. Householder tridiagonalisation.  The rank-2 update of reflector k is fused with the matvec of
//        reflector k+1: row k+1 is updated first (it is all the next reflector needs), then ONE pass over the
//        trailing block applies update k and forms S22 v_{k+1}.  That is one read and one write of the block per
//        reflector instead of two reads and a write.  The reflector is stored in the (dead) row k, contiguous,
//        for the back-transformation;
//     3. fp64 Sturm multisection, one wave per eigenvalue;
//     4. fp64 inverse iteration (pivoted tridiagonal LU; the factors of at most four vectors share LDS at a time),
//        modified Gram-Schmidt, back-transformation with the next reflector's load in flight;
//     5. sign convention, MATRIX_SYM skip, smallest / largest selection, rank-sort argsort into `order`.
// Compiled with -ffp-contract=off like spectral.hip: distances and Laplacian entries round like the reference's
// unfused torch ops, and every S update is the same expression in every element (S stays exactly symmetric).
#include "spectral_common.h"

namespace simamba {

// Workgroup barrier for data that goes through global memory.  __syncthreads() is a workgroup-scope fence, for which
// the compiler waits on LDS traffic only (a workgroup shares one CU's vector L1); the explicit vmcnt(0) wait also
// drains this wave's global stores before any other wave of the workgroup can pass the barrier.
__device__ __forceinline__ void global_barrier() {
  __builtin_amdgcn_s_waitcnt(0x0F70);              // vmcnt(0); expcnt, lgkmcnt left at their maximum
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------
constexpr int kKnnRows = 128;                      // nodes per workgroup
constexpr int kKnnRowLanes = 8;                    // lanes per node
constexpr int kKnnRowThreads = kKnnRows * kKnnRowLanes;

template <bool kMirror>
__global__ __launch_bounds__(kKnnRowThreads) void knn_rows_kernel(const float* __restrict__ pts,
                                                                  float* __restrict__ adj,
                                                                  const double* __restrict__ dist_sum, int B, int G,
                                                                  int F, int knn, float alpha, unsigned flags) {
  extern __shared__ float sP[];                    // [G][F]: every point of the sample
  const int tid = threadIdx.x;
  const float* P = pts + static_cast<size_t>(blockIdx.x) * G * F;
  float* A = adj + static_cast<size_t>(blockIdx.x) * G * G;
  const int r0 = blockIdx.y * kKnnRows;
  const int nrows = min(kKnnRows, G - r0);
  for (int e = tid; e < G * F; e += kKnnRowThreads) sP[e] = P[e];
  if (!kMirror)
    for (int e = tid; e < nrows * G; e += kKnnRowThreads) A[static_cast<size_t>(r0) * G + e] = 0.f;
  global_barrier();
  const bool self_loop = flags & SIMAMBA_SPEC_SELF_LOOP;
  const bool binary = flags & SIMAMBA_SPEC_BINARY;
  float inv2s2 = 0.f;
  if (flags & SIMAMBA_SPEC_SIGMA_MEAN) {
    const float sigma = static_cast<float>(*dist_sum / (static_cast<double>(B) * G * G));
    inv2s2 = 2.f * (sigma * sigma);
  }
  const int i = r0 + tid / kKnnRowLanes, part = tid % kKnnRowLanes;
  if (i >= G) return;                              // whole 8-lane groups leave together; no barrier follows
  float pv = -1.f;                                 // previous pick, ascending lexicographic (value, index) order
  int pi = -1;
  for (int m = 0; m <= knn; ++m) {
    float bv = 3.0e38f;
    int bi = 0x7fffffff;
    for (int j = part; j < G; j += kKnnRowLanes) {   // ascending j inside the lane: first hit is the lowest
      float d2 = 0.f;
      for (int f = 0; f < F; ++f) {
        const float df = sP[i * F + f] - sP[j * F + f];
        d2 = d2 + df * df;
      }
      const float v = sqrtf(d2);
      const bool after_prev = (v > pv) || (v == pv && j > pi);
      if (after_prev && (v < bv)) { bv = v; bi = j; }
    }
#pragma unroll
    for (int off = 1; off < kKnnRowLanes; off <<= 1) {
      const float ov = __shfl_xor(bv, off);
      const int oi = __shfl_xor(bi, off);
      const bool take = (ov < bv) || (ov == bv && static_cast<unsigned>(oi) < static_cast<unsigned>(bi));
      bv = take ? ov : bv;
      bi = take ? oi : bi;
    }
    pv = bv; pi = bi;
    if (bi == 0x7fffffff) break;                   // NaN distances: nothing left to pick (group-uniform)
    if (m == 0 && !self_loop) continue;            // drop the nearest (the point itself)
    float w = 1.f;
    if (!binary) {
      const float dd = bv * bv;
      w = (flags & SIMAMBA_SPEC_SIGMA_MEAN) ? expf(-dd / inv2s2) : expf(-1.f * alpha * dd);
    }
    if (part == 0) {
      if (kMirror) A[static_cast<size_t>(bi) * G + i] = w;
      else A[static_cast<size_t>(i) * G + bi] = w;
    }
  }
}

int launch_knn_graph_large(const float* pts, float* adj, const double* dist_sum, int B, int G, int F, int knn,
                           float alpha, unsigned flags, hipStream_t s) {
  static const bool once = [] {
    const int cap = static_cast<int>(sizeof(float)) * kSpecMaxGLarge * 64;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(knn_rows_kernel<false>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, cap);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(knn_rows_kernel<true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, cap);
    return true;
  }();
  (void)once;
  const dim3 grid(B, (G + kKnnRows - 1) / kKnnRows);
  const size_t smem = sizeof(float) * static_cast<size_t>(G) * F;
  hipLaunchKernelGGL(knn_rows_kernel<false>, grid, dim3(kKnnRowThreads), smem, s, pts, adj, dist_sum, B, G, F, knn,
                     alpha, flags);
  if (flags & SIMAMBA_SPEC_SYMMETRIC)
    hipLaunchKernelGGL(knn_rows_kernel<true>, grid, dim3(kKnnRowThreads), smem, s, pts, adj, dist_sum, B, G, F, knn,
                       alpha, flags);
  return static_cast<int>(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------
constexpr int kLgThreads = 1024;
constexpr int kLgWaves = kLgThreads / 64;
constexpr int kLgGroups = kLgThreads / 16;         // 16-lane DPP rows: one matrix row each
constexpr int kLgVecBatch = 4;                     // inverse-iteration vectors whose LU factors share LDS at once
constexpr int kLgBtPer = kSpecMaxGLarge / 64;      // reflector entries per lane in the back-transformation
// dynamic LDS: sZ [kTdMaxSel][512] + 4 LU arrays [kLgVecBatch][512] (fp64) + pivots [kLgVecBatch][512]
constexpr size_t kLgDynLds = sizeof(double) * (kTdMaxSel + 4 * kLgVecBatch) * kSpecMaxGLarge +
                             kLgVecBatch * kSpecMaxGLarge;

__device__ __forceinline__ double lg_wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__device__ __forceinline__ float lg_wave_sum_f32(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// 1/x to ~1 ulp (see spectral_tridiag.hip)
__device__ __forceinline__ double lg_rcp_f64(double x) {
  double r = __builtin_amdgcn_rcp(x);
  return fma(fma(-x, r, 1.0), r, r);
}

__device__ __forceinline__ int lg_sturm_count(const double* d, const double* e2, int n, double sigma,
                                              double pivmin) {
  double q = d[0] - sigma;
  if (fabs(q) < pivmin) q = -pivmin;
  int cnt = q < 0.0;
  for (int i = 1; i < n; ++i) {
    q = d[i] - sigma - e2[i - 1] * lg_rcp_f64(q);
    if (fabs(q) < pivmin) q = -pivmin;
    cnt += q < 0.0;
  }
  return cnt;
}

__global__ __launch_bounds__(kLgThreads) void laplacian_large_kernel(EigArgs p, float* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) double dsm[];
  constexpr int NG = kSpecMaxGLarge;
  double* sZ = dsm;                                          // [kTdMaxSel][NG]
  double* sLa = sZ + kTdMaxSel * NG;                         // [kLgVecBatch][NG] each
  double* sLb = sLa + kLgVecBatch * NG;
  double* sLc = sLb + kLgVecBatch * NG;
  double* sLl = sLc + kLgVecBatch * NG;
  unsigned char* sPiv = reinterpret_cast<unsigned char*>(sLl + kLgVecBatch * NG);
  __shared__ float sDeg[NG];
  __shared__ float sV[2][NG];                                // reflectors k (cur) and k-1 (pending update)
  __shared__ float sW[2][NG];                                // p = tau S22 v of the same two steps
  __shared__ float sTau[NG];
  __shared__ double sD[NG], sE[NG], sE2[NG];
  __shared__ __attribute__((aligned(16))) float sPart[kLgWaves], sPd[kLgGroups];
  __shared__ float sX0;
  __shared__ double sRed[3][kLgWaves];
  __shared__ double sLam[kTdMaxSel];
  __shared__ float sSign[kTdMaxSel];

  const int G = p.G;
  const int tid = threadIdx.x;
  const int lane16 = tid & 15, grp = tid >> 4;
  const int wave = tid >> 6, lane = tid & 63;
  const float* A = p.adj + static_cast<size_t>(blockIdx.x) * G * G;
  float* S = ws + static_cast<size_t>(blockIdx.x) * G * G;  // row-major, pitch G
  const bool msym = p.flags & SIMAMBA_SPEC_MATRIX_SYM;
  const bool smallest = p.flags & SIMAMBA_SPEC_SMALLEST;
  const int skip = msym ? 1 : 0;
  const int nsel = p.k;
  const int ntot = nsel + skip;

  // ---- 1. Laplacian (the same expressions as laplacian_tridiag_kernel) -----------------------------------------
  if (tid < G) {
    float s = 0.f;
    for (int j = 0; j < G; ++j) s = s + (A[tid * G + j] + A[j * G + tid]) / 2.f;
    sDeg[tid] = s;
  }
  __syncthreads();
  for (int e = tid; e < G * G; e += kLgThreads) {
    const int i = e / G, j = e - i * G;
    if (i >= j) {   // eigh(UPLO='L'): only the lower triangle of the (unsymmetric) L is read
      const float aij = (A[i * G + j] + A[j * G + i]) / 2.f;
      float l;
      if (msym) {
        const float di = powf(sDeg[i], -0.5f), dj = powf(sDeg[j], -0.5f);
        l = (i == j ? 1.f : 0.f) - (di * aij) * dj;
      } else {
        const float dinv = 1.0f / (sDeg[i] + 1e-6f);
        l = (i == j ? 1.f : 0.f) - dinv * aij;
      }
      S[i * G + j] = l;
      S[j * G + i] = l;
    }
  }
  global_barrier();

  // ---- 2. Householder tridiagonalisation, update k fused with matvec k+1 ------------------------------------------
  // Invariant at the top of step k: rows / columns >= k of S still lack the rank-2 update of reflector k-1
  // (vp = sV[cur^1], w = alphap * vp + sW[cur^1], indexed from row k), unless taup == 0.
  float taup = 0.f, alphap = 0.f;
  int cur = 0;
  for (int k = 0; k + 2 < G; ++k) {
    const int m = G - k - 1;                       // order of the trailing block
    const float* vp = sV[cur ^ 1];
    const float* pp = sW[cur ^ 1];
    float* vc = sV[cur];
    float* pc = sW[cur];
    // (a) row k (= column k) with the pending update: one entry per lane; its squares beyond the diagonal
    const int t = tid;                             // column k + t, t <= m <= 511
    float s = 0.f, sq = 0.f;
    if (t <= m) {
      s = S[k * G + k + t];
      if (taup != 0.f) {
        const float vi = vp[0], wi = fmaf(alphap, vi, pp[0]);
        const float vj = vp[t], wj = fmaf(alphap, vj, pp[t]);
        s = s - (vi * wj + wi * vj);
      }
      if (t >= 1) sq = s * s;
    }
    sq = lg_wave_sum_f32(sq);
    if (lane == 0) sPart[wave] = sq;
    if (tid == 0) sD[k] = s;
    if (tid == 1) sX0 = s;
    __syncthreads();                                                               // (1) norm partials, x0
    float nrm2 = 0.f;
#pragma unroll
    for (int q = 0; q < kLgWaves / 4; ++q) {
      const float4 v = *reinterpret_cast<const float4*>(sPart + 4 * q);
      nrm2 += (v.x + v.y) + (v.z + v.w);
    }
    const float x0 = sX0;
    const float rest = nrm2 - x0 * x0;
    float tau = 0.f, scale = 0.f, beta = x0;
    if (rest > 1e-30f && rest > 1e-12f * nrm2) {   // identical in every lane
      beta = -copysignf(sqrtf(nrm2), x0);
      tau = (beta - x0) / beta;
      scale = 1.0f / (x0 - beta);
    }
    if (tid == 0) { sTau[k] = tau; sE[k] = beta; }
    if (t >= 1 && t <= m) {
      const float v = (t == 1) ? 1.f : s * scale;
      vc[t - 1] = v;
      if (t >= 2) S[k * G + k + t] = v;           // row k is dead: it keeps the reflector (leading 1 implicit)
    }
    global_barrier();                                                              // (2) v
    // (b) rows k+1.. : pending update, then p = tau S22 v on the updated values (one read + one write per entry)
    if (tau != 0.f || taup != 0.f) {
      float pdot = 0.f;
      for (int r = grp; r < m; r += kLgGroups) {
        float* row = S + static_cast<size_t>(k + 1 + r) * G + (k + 1);
        float vi = 0.f, wi = 0.f;
        if (taup != 0.f) { vi = vp[r + 1]; wi = fmaf(alphap, vi, pp[r + 1]); }
        float acc = 0.f;
        for (int c = lane16; c < m; c += 16) {
          float x = row[c];
          if (taup != 0.f) {
            const float vj = vp[c + 1], wj = fmaf(alphap, vj, pp[c + 1]);
            x = x - (vi * wj + wi * vj);
            row[c] = x;
          }
          acc = fmaf(x, vc[c], acc);
        }
        if (tau != 0.f) {
          acc = row_allreduce_sum(acc);
          const float pi = tau * acc;
          if (lane16 == 0) { pc[r] = pi; pdot = fmaf(pi, vc[r], pdot); }
        }
      }
      if (lane16 == 0) sPd[grp] = pdot;
    }
    global_barrier();                                                              // (3) S22 updated, p, p.v
    if (tau != 0.f) {
      float pd = 0.f;
#pragma unroll
      for (int q = 0; q < kLgGroups / 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(sPd + 4 * q);
        pd += (v.x + v.y) + (v.z + v.w);
      }
      alphap = -0.5f * tau * pd;
    }
    taup = tau;
    cur ^= 1;
  }
  // the last 2 x 2 block with the pending update of reflector G-3
  if (tid == 0) {
    float d0 = S[(G - 2) * G + (G - 2)], e0 = S[(G - 1) * G + (G - 2)], d1 = S[(G - 1) * G + (G - 1)];
    if (taup != 0.f) {
      const float* vp = sV[cur ^ 1];
      const float* pp = sW[cur ^ 1];
      const float v0 = vp[0], w0 = fmaf(alphap, v0, pp[0]);
      const float v1 = vp[1], w1 = fmaf(alphap, v1, pp[1]);
      d0 = d0 - (v0 * w0 + w0 * v0);
      e0 = e0 - (v1 * w0 + w1 * v0);
      d1 = d1 - (v1 * w1 + w1 * v1);
    }
    sD[G - 2] = d0; sE[G - 2] = e0;
    sD[G - 1] = d1; sE[G - 1] = 0.0;
  }
  __syncthreads();
  if (tid < G) sE2[tid] = sE[tid] * sE[tid];
  // Gershgorin range and pivmin
  double glo = 1e300, ghi = -1e300, emax = 0.0;
  if (tid < G) {
    const double el = tid > 0 ? fabs(sE[tid - 1]) : 0.0, er = tid + 1 < G ? fabs(sE[tid]) : 0.0;
    glo = sD[tid] - el - er;
    ghi = sD[tid] + el + er;
    emax = er * er;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    glo = fmin(glo, __shfl_xor(glo, off));
    ghi = fmax(ghi, __shfl_xor(ghi, off));
    emax = fmax(emax, __shfl_xor(emax, off));
  }
  if (lane == 0) { sRed[0][wave] = glo; sRed[1][wave] = ghi; sRed[2][wave] = emax; }
  __syncthreads();
  glo = sRed[0][0]; ghi = sRed[1][0]; emax = sRed[2][0];
#pragma unroll
  for (int w = 1; w < kLgWaves; ++w) {
    glo = fmin(glo, sRed[0][w]); ghi = fmax(ghi, sRed[1][w]); emax = fmax(emax, sRed[2][w]);
  }
  const double tnorm = fmax(fabs(glo), fabs(ghi));
  const double pivmin = fmax(emax, 1.0) * 2.2250738585072014e-308 * 4.0 + 1e-290;
  glo -= 1e-12 * tnorm + 1e-300;
  ghi += 1e-12 * tnorm + 1e-300;

  // ---- 3. wanted eigenvalues: multisection, one wave = 64 shifts per eigenvalue and round -------------------------
  {
    const int want = smallest ? wave : (G - 1 - wave);   // ascending index of the eigenvalue this wave finds
    double lo = glo, hi = ghi;
    if (wave < ntot) {
      for (int round = 0; round < 5; ++round) {   // 65^-5 ~ 1e-9 of the Gershgorin range
        const double step = (hi - lo) * (1.0 / 65.0);
        const double sigma = lo + step * (lane + 1);
        const int cnt = lg_sturm_count(sD, sE2, G, sigma, pivmin);
        const unsigned long long above = __ballot(cnt > want);
        const int tt = above ? __builtin_ctzll(above) : 64;
        const double nlo = lo + step * tt;
        hi = (tt == 64) ? hi : lo + step * (tt + 1);
        lo = nlo;
      }
      if (lane == 0) sLam[wave] = 0.5 * (lo + hi);
    }
  }
  __syncthreads();

  // ---- 4a. inverse iteration, one lane (of its own wave) per vector, kLgVecBatch vectors per LDS batch -------------
  for (int b0 = 0; b0 < ntot; b0 += kLgVecBatch) {
    if (lane == 0 && wave >= b0 && wave < b0 + kLgVecBatch && wave < ntot) {
      const int sv = wave, slot = wave - b0, n = G;
      double* ra = sLa + slot * NG; double* ub = sLb + slot * NG; double* uc = sLc + slot * NG;
      double* l = sLl + slot * NG; double* z = sZ + sv * NG;
      unsigned char* piv = sPiv + slot * NG;
      const double lam = sLam[sv];
      const double tiny = fmax(tnorm, 1.0) * 1.1e-16;
      double ai = sD[0] - lam;
      double bi = (n > 1) ? sE[0] : 0.0;
      for (int i = 0; i + 1 < n; ++i) {
        const double sub = sE[i];
        const double a1 = sD[i + 1] - lam;
        const double b1 = (i + 2 < n) ? sE[i + 1] : 0.0;
        if (fabs(ai) >= fabs(sub)) {
          if (fabs(ai) < tiny) ai = tiny;
          const double r = lg_rcp_f64(ai);
          const double mult = sub * r;
          ra[i] = r; ub[i] = bi; uc[i] = 0.0; l[i] = mult; piv[i] = 0;
          ai = a1 - mult * bi;
          bi = b1;
        } else {
          const double r = lg_rcp_f64(sub);
          const double mult = ai * r;
          ra[i] = r; ub[i] = a1; uc[i] = b1; l[i] = mult; piv[i] = 1;
          ai = bi - mult * a1;
          bi = -mult * b1;
        }
      }
      if (fabs(ai) < tiny) ai = tiny;
      ra[n - 1] = lg_rcp_f64(ai); ub[n - 1] = 0.0; uc[n - 1] = 0.0;
      unsigned rng = 12345u + 977u * sv;
      for (int i = 0; i < n; ++i) {               // deterministic start vector in (-1, 1)
        rng = rng * 1664525u + 1013904223u;
        z[i] = (static_cast<double>(rng >> 8) / 8388608.0) - 1.0;
      }
      for (int it = 0; it < 3; ++it) {
        double zi = z[0];
        for (int i = 0; i + 1 < n; ++i) {
          double zn = z[i + 1];
          if (piv[i]) { const double tmp = zi; zi = zn; zn = tmp; }
          z[i] = zi;
          zi = zn - l[i] * zi;
        }
        double z1 = zi * ra[n - 1], z2 = 0.0, nr = z1 * z1;
        z[n - 1] = z1;
        for (int i = n - 2; i >= 0; --i) {
          const double zc = (z[i] - ub[i] * z1 - uc[i] * z2) * ra[i];
          z[i] = zc;
          nr = fma(zc, zc, nr);
          z2 = z1; z1 = zc;
        }
        nr = 1.0 / sqrt(nr);
        for (int i = 0; i < n; ++i) z[i] *= nr;
      }
    }
    __syncthreads();
  }
  // ---- 4b. modified Gram-Schmidt (wave 0) -------------------------------------------------------------------------
  if (tid < 64) {
    for (int sv = 1; sv < ntot; ++sv) {
      double* zs = sZ + sv * NG;
      for (int t2 = 0; t2 < sv; ++t2) {
        const double* zt = sZ + t2 * NG;
        double dot = 0.0;
        for (int i = tid; i < G; i += 64) dot += zs[i] * zt[i];
        dot = lg_wave_sum_f64(dot);
        for (int i = tid; i < G; i += 64) zs[i] -= dot * zt[i];
      }
      double nr = 0.0;
      for (int i = tid; i < G; i += 64) nr += zs[i] * zs[i];
      nr = 1.0 / sqrt(lg_wave_sum_f64(nr));
      for (int i = tid; i < G; i += 64) zs[i] *= nr;
    }
  }
  __syncthreads();
  // ---- 4c. back-transformation v = H_0 ... H_{G-3} z, one wave per vector; reflector k sits in row k of S ---------
  for (int sv = wave; sv < ntot; sv += kLgWaves) {
    double* z = sZ + sv * NG;
    float vn[kLgBtPer];
    auto load_refl = [&](int k, float (&v)[kLgBtPer]) {
      const int m = G - k - 1;
#pragma unroll
      for (int q = 0; q < kLgBtPer; ++q) {
        const int i = lane + 64 * q;
        v[q] = (i == 0) ? 1.f : (i < m ? S[k * G + k + 1 + i] : 0.f);
      }
    };
    if (G >= 3) load_refl(G - 3, vn);
    for (int k = G - 3; k >= 0; --k) {
      float vk[kLgBtPer];
#pragma unroll
      for (int q = 0; q < kLgBtPer; ++q) vk[q] = vn[q];
      if (k > 0) load_refl(k - 1, vn);           // next reflector in flight while this one is applied
      const double tau = sTau[k];
      if (tau == 0.0) continue;                    // uniform
      const int m = G - k - 1;
      double dot = 0.0;
#pragma unroll
      for (int q = 0; q < kLgBtPer; ++q) {
        const int i = lane + 64 * q;
        if (i < m) dot += static_cast<double>(vk[q]) * z[k + 1 + i];
      }
      dot = lg_wave_sum_f64(dot) * tau;
#pragma unroll
      for (int q = 0; q < kLgBtPer; ++q) {
        const int i = lane + 64 * q;
        if (i < m) z[k + 1 + i] -= dot * static_cast<double>(vk[q]);
      }
    }
    // sign convention: component of largest magnitude positive (first such index on ties)
    double best = -1.0; int bi = 0x7fffffff;
    for (int i = lane; i < G; i += 64) {
      const double v = fabs(static_cast<double>(static_cast<float>(z[i])));
      if (v > best) { best = v; bi = i; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ob = __shfl_xor(best, off);
      const int oi = __shfl_xor(bi, off);
      if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) sSign[sv] = z[bi] < 0.0 ? -1.f : 1.f;
  }
  __syncthreads();

  // ---- 5. outputs (the first `skip` extracted pairs are dropped: MATRIX_SYM) -----------------------------------------
  if (p.evals && tid < nsel)
    p.evals[static_cast<size_t>(blockIdx.x) * nsel + tid] = static_cast<float>(sLam[tid + skip]);
  if (p.evecs) {
    float* out = p.evecs + static_cast<size_t>(blockIdx.x) * G * nsel;
    for (int e = tid; e < G * nsel; e += kLgThreads) {
      const int i = e / nsel, mm = e - i * nsel;
      out[e] = static_cast<float>(sZ[(mm + skip) * NG + i]) * sSign[mm + skip];
    }
  }
  if (p.order) {
    long long* out = p.order + static_cast<size_t>(blockIdx.x) * nsel * G;
    for (int e = tid; e < G * nsel; e += kLgThreads) {
      const int mm = e / G, i = e - mm * G;
      const double* z = sZ + (mm + skip) * NG;
      const float sg = sSign[mm + skip];
      const float vi = static_cast<float>(z[i]) * sg;
      int rk = 0;
      for (int j = 0; j < G; ++j) {
        const float vj = static_cast<float>(z[j]) * sg;
        rk += (vj < vi) || (vj == vi && j < i);
      }
      out[mm * G + rk] = i;
    }
  }
}

int launch_laplacian_large_topk(const EigArgs& a, float* ws, hipStream_t s) {
  static const bool once = [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(laplacian_large_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kLgDynLds));
    return true;
  }();
  (void)once;
  hipLaunchKernelGGL(laplacian_large_kernel, dim3(a.B), dim3(kLgThreads), kLgDynLds, s, a, ws);
  return static_cast<int>(hipGetLastError());
}

}  // namespace simamba
