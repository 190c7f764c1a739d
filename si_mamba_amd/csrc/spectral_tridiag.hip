// Top-k eigenpairs of the graph Laplacian for G <= 128: Householder tridiagonalisation + bisection + inverse iteration.
//
// Same contract as laplacian_eig_kernel (spectral.hip) for the outputs the reference's forward consumes
// (models/point_mamba.py:884 uses only the k selected pairs): evals (B,k), evecs (B,G,k), order (B,k,G).
// The Jacobi kernel diagonalises the whole matrix (8-9 sweeps x 127 barrier-separated steps, 3.6 ms per
// workgroup); only k <= 7 pairs are needed, so this kernel does what LAPACK's ?syevx does, one workgroup
// (512 lanes) per sample, everything in LDS:
//   1. S = mirrored lower triangle of the Laplacian (laplacian_entry), fp32, 66 KiB;
//   2. Householder reduction to tridiagonal T, written here: G-2 reflectors; per reflector one matvec and one
//      rank-2 update of the trailing block, 16-lane DPP rows own matrix rows, reflectors stay in the zeroed
//      columns; 3 barriers per reflector;
//   3.-5. the solver stages of spectral_device.h on T: Gershgorin range, fp64 Sturm multisection (one wave per
//      eigenvalue), fp64 inverse iteration (one lane per vector), modified Gram-Schmidt; then, written here, the
//      back-transformation through the reflectors (one wave per vector); sign convention and outputs shared again.
// Compiled with -ffp-contract=off (the Laplacian entries must round like the reference's torch ops).
#include "spectral_device.h"


namespace simamba {

constexpr int kTdThreads = 512;
constexpr int kTdGroups = kTdThreads / 16;   // 16-lane DPP rows
constexpr int kTdLD = kSpecMaxG + 1;      // odd pitch: row- and column-wise walks are both conflict-free

// per-group partial sums of the squares of column `col` below the diagonal (rows col+1 .. G-1) -> sPart[grp]
__device__ __forceinline__ void colnorm_partials(const float* S, int LD, int G, int col, float* sPart) {
  const int lane16 = threadIdx.x & 15, grp = threadIdx.x >> 4;
  if (lane16 == 0) {
    float acc = 0.f;
    for (int r = col + 1 + grp; r < G; r += kTdGroups) {
      const float x = S[r * LD + col];
      acc = fmaf(x, x, acc);
    }
    sPart[grp] = acc;
  }
}

// sum of the kTdGroups (= 32) group partials, read as 8 broadcast float4
__device__ __forceinline__ float sum_partials(const float* sPart) {
  float acc = 0.f;
#pragma unroll
  for (int q = 0; q < kTdGroups / 4; ++q) {
    const float4 v = *reinterpret_cast<const float4*>(sPart + 4 * q);
    acc += (v.x + v.y) + (v.z + v.w);
  }
  return acc;
}

__global__ __launch_bounds__(kTdThreads) void laplacian_tridiag_kernel(EigArgs p) {
  extern __shared__ __attribute__((aligned(16))) float S[];     // [G][kTdLD]
  __shared__ float sDeg[kSpecMaxG];
  __shared__ float sV[kSpecMaxG];           // current reflector
  __shared__ float sW[kSpecMaxG];           // p = tau S22 v
  __shared__ float sTau[kSpecMaxG];
  __shared__ double sD[kSpecMaxG], sE[kSpecMaxG], sE2[kSpecMaxG];
  __shared__ __attribute__((aligned(16))) float sPart[kTdGroups], sPd[kTdGroups];
  __shared__ double sLam[kTdMaxSel];
  __shared__ double sZ[kTdMaxSel][kSpecMaxG];
  __shared__ double sLa[kTdMaxSel][kSpecMaxG], sLb[kTdMaxSel][kSpecMaxG], sLc[kTdMaxSel][kSpecMaxG],
      sLl[kTdMaxSel][kSpecMaxG];
  __shared__ unsigned char sPiv[kTdMaxSel][kSpecMaxG];
  __shared__ float sSign[kTdMaxSel];

  const int G = p.G;
  constexpr int LD = kTdLD;
  const int tid = threadIdx.x;
  const int lane16 = tid & 15, grp = tid >> 4;      // 16 groups of 16 lanes
  const float* A = p.adj + static_cast<size_t>(blockIdx.x) * G * G;
  const bool msym = p.flags & SIMAMBA_SPEC_MATRIX_SYM;
  const bool smallest = p.flags & SIMAMBA_SPEC_SMALLEST;
  const int skip = msym ? 1 : 0;
  const int nsel = p.k;
  const int ntot = nsel + skip;                     // eigenpairs actually extracted (<= kTdMaxSel)

  // ---- 1. Laplacian ------------------------------------------------------------------------------------
  if (tid < G) sDeg[tid] = degree_sum(A, G, tid);
  __syncthreads();
  for (int e = tid; e < G * G; e += kTdThreads) {
    const int i = e / G, j = e - i * G;
    if (i >= j) {
      const float l = laplacian_entry(sym_adj(A, G, i, j), sDeg[i], sDeg[j], i == j, msym);
      S[i * LD + j] = l;
      S[j * LD + i] = l;
    }
  }
  __syncthreads();

  // ---- 2. Householder tridiagonalisation ------------------------------------------------------------------
  // Three barriers per reflector: every lane derives (beta, tau, scale) itself from the group partials of the
  // column norm, the p.v product rides on the matvec, and the NEXT column's norm partials ride on the update.
  colnorm_partials(S, LD, G, 0, sPart);
  __syncthreads();
  for (int k = 0; k + 2 < G; ++k) {
    const int m = G - k - 1;                        // order of the trailing block
    const float nrm2 = sum_partials(sPart);
    const float x0 = S[(k + 1) * LD + k];
    float beta, tau, scale;
    householder_params(nrm2, x0, &beta, &tau, &scale);      // identical in every lane
    if (tid == 0) { sTau[k] = tau; sE[k] = beta; sD[k] = S[k * LD + k]; }
    if (tid < m) {
      const float xi = S[(k + 1 + tid) * LD + k];
      const float v = (tid == 0) ? 1.f : xi * scale;
      sV[tid] = v;
      // keep the reflector for the back-transformation; its leading 1 stays implicit (the slot still holds
      // x0, which the other lanes are reading right now)
      if (tid > 0) S[(k + 1 + tid) * LD + k] = v;
    }
    __syncthreads();                                                              // (1) v, params
    if (tau != 0.f) {
      // p = tau * S22 v : rows owned by 16-lane groups; partial p.v per group
      float pdot = 0.f;
      for (int i = grp; i < m; i += kTdGroups) {
        const float* row = S + (k + 1 + i) * LD + (k + 1);
        float acc = 0.f;
        for (int j = lane16; j < m; j += 16) acc = fmaf(row[j], sV[j], acc);
        acc = row_allreduce_sum(acc);
        const float pi = tau * acc;
        if (lane16 == 0) { sW[i] = pi; pdot = fmaf(pi, sV[i], pdot); }
      }
      if (lane16 == 0) sPd[grp] = pdot;
      __syncthreads();                                                            // (2) p, partial dots
      // w = p - (tau/2)(p.v) v is formed where it is used (same fmaf everywhere, so every lane sees the same w):
      // no write-back of w and no barrier for it
      const float alpha = -0.5f * tau * sum_partials(sPd);
      // S22 -= v w^T + w v^T ; lane 0 of a group also sees the new column k+1 -> next reflector's norm
      float sq = 0.f;
      for (int i = grp; i < m; i += kTdGroups) {
        float* row = S + (k + 1 + i) * LD + (k + 1);
        const float vi = sV[i], wi = fmaf(alpha, vi, sW[i]);
        for (int j = lane16; j < m; j += 16) {
          const float vj = sV[j], wj = fmaf(alpha, vj, sW[j]);
          const float nv = row[j] - (vi * wj + wi * vj);
          row[j] = nv;
          if (j == 0 && i >= 1) sq = fmaf(nv, nv, sq);
        }
      }
      if (lane16 == 0) sPart[grp] = sq;
    } else {
      colnorm_partials(S, LD, G, k + 1, sPart);
    }
    __syncthreads();                                                              // (3) trailing block, norms
  }
  if (tid == 0) {
    if (G >= 2) {
      sD[G - 2] = S[(G - 2) * LD + (G - 2)];
      sE[G - 2] = S[(G - 1) * LD + (G - 2)];
    }
    sD[G - 1] = S[(G - 1) * LD + (G - 1)];
    sE[G - 1] = 0.0;
  }
  __syncthreads();
  if (tid < G) sE2[tid] = sE[tid] * sE[tid];
  // ---- 3. Gershgorin range (partials in the still unused LU rows), then one wave per wanted eigenvalue ----------
  double glo, ghi, emax, tnorm, pivmin;
  gershgorin_wave(sD, sE, G, tid, &glo, &ghi, &emax);
  __syncthreads();
  gershgorin_block<kTdThreads>(sLa[0], sLb[0], sLc[0], tid, &glo, &ghi, emax, &tnorm, &pivmin);
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;         // 8 waves
  if (wave < ntot) {
    const int want = smallest ? wave : (G - 1 - wave);  // ascending index of the eigenvalue this wave finds
    const double lam = multisect_eigenvalue(sD, sE2, G, want, glo, ghi, pivmin, lane);
    if (lane == 0) sLam[wave] = lam;
  }
  __syncthreads();
  // ---- 4a. eigenvectors of T: lane 0 of wave s iterates vector s, so the chains run side by side ------------
  if (lane == 0 && wave < ntot)
    tridiag_inverse_iteration(G, sLam[wave], tnorm, inverse_iteration_seed(wave), sD, sE, sLa[wave], sLb[wave],
                              sLc[wave], sLl[wave], sPiv[wave], sZ[wave]);
  __syncthreads();
  // ---- 4b. modified Gram-Schmidt among the vectors -------------------------------------------------------------
  if (tid < 64) gram_schmidt_wave0<kSpecMaxG>(&sZ[0][0], ntot, G, tid);
  __syncthreads();
  // ---- 4c. back-transformation v = H_0 H_1 ... H_{G-3} z : one wave per vector -------------------------------
  for (int s = wave; s < ntot; s += kTdThreads / 64) {
    double* z = sZ[s];
    for (int k = G - 3; k >= 0; --k) {
      const double tau = sTau[k];
      if (tau == 0.0) continue;                      // uniform
      const int m = G - k - 1;
      double dot = 0.0;
      for (int i = lane; i < m; i += 64) {
        const double vi = (i == 0) ? 1.0 : static_cast<double>(S[(k + 1 + i) * LD + k]);
        dot += vi * z[k + 1 + i];
      }
      dot = wave_xor_sum(dot) * tau;
      for (int i = lane; i < m; i += 64) {
        const double vi = (i == 0) ? 1.0 : static_cast<double>(S[(k + 1 + i) * LD + k]);
        z[k + 1 + i] -= dot * vi;
      }
    }
    sign_of_largest(z, G, lane, &sSign[s]);
  }
  __syncthreads();

  // ---- 5. outputs (the first `skip` extracted pairs are dropped: MATRIX_SYM) ---------------------------------
  write_topk_outputs<kTdThreads, kSpecMaxG>(p, &sZ[0][0], sLam, sSign, skip);
}

int launch_tridiag_topk(const EigArgs& a, hipStream_t s) {
  (void)ensure_lds_cap<laplacian_tridiag_kernel>(kSpecMaxG * kTdLD * 4);
  hipLaunchKernelGGL(laplacian_tridiag_kernel, dim3(a.B), dim3(kTdThreads), sizeof(float) * kSpecMaxG * kTdLD, s, a);
  return static_cast<int>(hipGetLastError());
}

}  // namespace simamba
