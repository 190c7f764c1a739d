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
//     phase recomputes the lists rather than storing them.  Distances, order predicates and weights are the
//     functions of spectral_device.h that knn_graph_kernel calls: identical edges, identical weights.
//
//   laplacian_large_kernel  the top-k solver of laplacian_tridiag_kernel with the matrix in the caller's workspace
//     (1024 lanes, vectors of pitch 512).  Written here:
//     2. Householder tridiagonalisation.  The rank-2 update of reflector k is fused with the matvec of
//        reflector k+1: row k+1 is updated first (it is all the next reflector needs), then ONE pass over the
//        trailing block applies update k and forms S22 v_{k+1}.  That is one read and one write of the block per
//        reflector instead of two reads and a write.  The reflector is stored in the (dead) row k, contiguous,
//        for the back-transformation;
//     4a. the batching of the inverse iteration: the LU factors of at most four vectors share LDS at a time;
//     4c. the back-transformation with the next reflector's load in flight.
//     Everything else (Laplacian entry, reflector parameters, Gershgorin range, Sturm multisection, the inverse
//     iteration itself, Gram-Schmidt, sign convention, outputs) is spectral_device.h.
// Compiled with -ffp-contract=off like spectral.hip: distances and Laplacian entries round like the reference's
// unfused torch ops, and every S update is the same expression in every element (S stays exactly symmetric).
#include "spectral_device.h"


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
  const float inv2s2 = knn_inv2s2(flags, dist_sum, B, G);
  const int i = r0 + tid / kKnnRowLanes, part = tid % kKnnRowLanes;
  if (i >= G) return;                              // whole 8-lane groups leave together; no barrier follows
  float pv = -1.f;                                 // previous pick, ascending lexicographic (value, index) order
  int pi = -1;
  for (int m = 0; m <= knn; ++m) {
    float bv = 3.0e38f;
    int bi = 0x7fffffff;
    for (int j = part; j < G; j += kKnnRowLanes) {   // ascending j inside the lane: first hit is the lowest
      const float v = point_dist(sP, i, j, F);
      const bool after_prev = (v > pv) || (v == pv && j > pi);
      if (after_prev && (v < bv)) { bv = v; bi = j; }
    }
#pragma unroll
    for (int off = 1; off < kKnnRowLanes; off <<= 1) {
      const float ov = __shfl_xor(bv, off);
      const int oi = __shfl_xor(bi, off);
      const bool take = knn_take(ov, oi, bv, bi);
      bv = take ? ov : bv;
      bi = take ? oi : bi;
    }
    pv = bv; pi = bi;
    if (bi == 0x7fffffff) break;                   // NaN distances: nothing left to pick (group-uniform)
    if (m == 0 && !self_loop) continue;            // drop the nearest (the point itself)
    const float w = knn_edge_weight(flags, bv, alpha, inv2s2);
    if (part == 0) {
      if (kMirror) A[static_cast<size_t>(bi) * G + i] = w;
      else A[static_cast<size_t>(i) * G + bi] = w;
    }
  }
}

int launch_knn_graph_large(const float* pts, float* adj, const double* dist_sum, int B, int G, int F, int knn,
                           float alpha, unsigned flags, hipStream_t s) {
  const int cap = static_cast<int>(sizeof(float)) * kSpecMaxGLarge * 64;
  (void)ensure_lds_cap<knn_rows_kernel<false>>(cap);
  (void)ensure_lds_cap<knn_rows_kernel<true>>(cap);
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

  // ---- 1. Laplacian ---------------------------------------------------------------------------------------------
  if (tid < G) sDeg[tid] = degree_sum(A, G, tid);
  __syncthreads();
  for (int e = tid; e < G * G; e += kLgThreads) {
    const int i = e / G, j = e - i * G;
    if (i >= j) {
      const float l = laplacian_entry(sym_adj(A, G, i, j), sDeg[i], sDeg[j], i == j, msym);
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
    sq = wave_xor_sum(sq);
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
    float beta, tau, scale;
    householder_params(nrm2, x0, &beta, &tau, &scale);      // identical in every lane
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
  // ---- 3. Gershgorin range, then one wave per wanted eigenvalue ---------------------------------------------------
  double glo, ghi, emax, tnorm, pivmin;
  gershgorin_wave(sD, sE, G, tid, &glo, &ghi, &emax);
  gershgorin_block<kLgThreads>(sRed[0], sRed[1], sRed[2], tid, &glo, &ghi, emax, &tnorm, &pivmin);
  if (wave < ntot) {
    const int want = smallest ? wave : (G - 1 - wave);   // ascending index of the eigenvalue this wave finds
    const double lam = multisect_eigenvalue(sD, sE2, G, want, glo, ghi, pivmin, lane);
    if (lane == 0) sLam[wave] = lam;
  }
  __syncthreads();

  // ---- 4a. inverse iteration, one lane (of its own wave) per vector, kLgVecBatch vectors per LDS batch -------------
  for (int b0 = 0; b0 < ntot; b0 += kLgVecBatch) {
    if (lane == 0 && wave >= b0 && wave < b0 + kLgVecBatch && wave < ntot) {
      const int slot = wave - b0;
      tridiag_inverse_iteration(G, sLam[wave], tnorm, inverse_iteration_seed(wave), sD, sE, sLa + slot * NG,
                                sLb + slot * NG, sLc + slot * NG, sLl + slot * NG, sPiv + slot * NG, sZ + wave * NG);
    }
    __syncthreads();
  }
  // ---- 4b. modified Gram-Schmidt (wave 0) -------------------------------------------------------------------------
  if (tid < 64) gram_schmidt_wave0<NG>(sZ, ntot, G, tid);
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
      dot = wave_xor_sum(dot) * tau;
#pragma unroll
      for (int q = 0; q < kLgBtPer; ++q) {
        const int i = lane + 64 * q;
        if (i < m) z[k + 1 + i] -= dot * static_cast<double>(vk[q]);
      }
    }
    sign_of_largest(z, G, lane, &sSign[sv]);
  }
  __syncthreads();

  // ---- 5. outputs (the first `skip` extracted pairs are dropped: MATRIX_SYM) -----------------------------------------
  write_topk_outputs<kLgThreads, NG>(p, sZ, sLam, sSign, skip);
}

int launch_laplacian_large_topk(const EigArgs& a, float* ws, hipStream_t s) {
  (void)ensure_lds_cap<laplacian_large_kernel>(static_cast<int>(kLgDynLds));
  hipLaunchKernelGGL(laplacian_large_kernel, dim3(a.B), dim3(kLgThreads), kLgDynLds, s, a, ws);
  return static_cast<int>(hipGetLastError());
}

}  // namespace simamba
