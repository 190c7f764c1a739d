// Device steps shared by the spectral kernels: the graph weights of the two k-NN kernels (spectral.hip,
// spectral_large.hip), the Laplacian entry of the three eigen kernels, and every stage of the top-k solver that
// follows the Householder reduction in laplacian_tridiag_kernel and laplacian_large_kernel.  Storage comes in as
// pointers; vector pitch and workgroup size are template parameters.  The including files are compiled with
// -ffp-contract=off, so the operand order written here IS the arithmetic of every kernel that calls it.
#pragma once
#include "spectral_common.h"

namespace simamba {

// ---- k-NN graph -------------------------------------------------------------------------------------------------
// Euclidean distance of points i and j of an [n][F] array, summed in feature order like the reference's cdist
__device__ __forceinline__ float point_dist(const float* P, int i, int j, int F) {
  float d2 = 0.f;
  for (int f = 0; f < F; ++f) {
    const float df = P[i * F + f] - P[j * F + f];
    d2 = d2 + df * df;
  }
  return sqrtf(d2);
}

// SIGMA_MEAN: 2 sigma^2 with sigma the mean pairwise distance of the batch (dist_sum_kernel); 0 otherwise
__device__ __forceinline__ float knn_inv2s2(unsigned flags, const double* dist_sum, int B, int G) {
  float inv2s2 = 0.f;
  if (flags & SIMAMBA_SPEC_SIGMA_MEAN) {
    const float sigma = static_cast<float>(*dist_sum / (static_cast<double>(B) * G * G));
    inv2s2 = 2.f * (sigma * sigma);
  }
  return inv2s2;
}

__device__ __forceinline__ float knn_edge_weight(unsigned flags, float dist, float alpha, float inv2s2) {
  float w = 1.f;
  if (!(flags & SIMAMBA_SPEC_BINARY)) {
    const float dd = dist * dist;
    w = (flags & SIMAMBA_SPEC_SIGMA_MEAN) ? expf(-dd / inv2s2) : expf(-1.f * alpha * dd);
  }
  return w;
}

// lexicographic (value, index) order: ties go to the lower index like a stable sort
__device__ __forceinline__ bool knn_take(float ov, int oi, float v, int i) {
  return (ov < v) || (ov == v && static_cast<unsigned>(oi) < static_cast<unsigned>(i));
}

// ---- Laplacian --------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sym_adj(const float* A, int G, int i, int j) {
  return (A[i * G + j] + A[j * G + i]) / 2.f;
}

// degree of node i in (A + A^T)/2
__device__ __forceinline__ float degree_sum(const float* A, int G, int i) {
  float s = 0.f;
  for (int j = 0; j < G; ++j) s = s + sym_adj(A, G, i, j);
  return s;
}

// entry (i, j), i >= j, of I - D^-1 A (or, MATRIX_SYM, of I - D^-1/2 A D^-1/2), rounding like the reference's torch
// ops.  eigh(UPLO='L') reads only the lower triangle of the (unsymmetric) L: callers mirror this value.
__device__ __forceinline__ float laplacian_entry(float aij, float deg_i, float deg_j, bool diag, bool msym) {
  if (msym) {
    const float di = powf(deg_i, -0.5f), dj = powf(deg_j, -0.5f);
    return (diag ? 1.f : 0.f) - (di * aij) * dj;
  }
  const float dinv = 1.0f / (deg_i + 1e-6f);
  return (diag ? 1.f : 0.f) - dinv * aij;
}

// ---- Householder ------------------------------------------------------------------------------------------------
// reflector H = I - tau v v^T (v_0 = 1, v_i = x_i * scale) that maps x to (beta, 0, ...); nrm2 = |x|^2.
// tau = 0 (beta = x0) when the tail of x is negligible.  Every lane derives the same values.
__device__ __forceinline__ void householder_params(float nrm2, float x0, float* beta, float* tau, float* scale) {
  const float rest = nrm2 - x0 * x0;
  *tau = 0.f; *scale = 0.f; *beta = x0;
  if (rest > 1e-30f && rest > 1e-12f * nrm2) {
    *beta = -copysignf(sqrtf(nrm2), x0);
    *tau = (*beta - x0) / *beta;
    *scale = 1.0f / (x0 - *beta);
  }
}

// ---- fp64 stages on the tridiagonal T = (d, e) --------------------------------------------------------------------
// 1/x to ~1 ulp: hardware v_rcp_f64 seed + one Newton step (the IEEE division sequence is ~30 dependent
// instructions; the recurrences below are pure latency chains of divisions)
__device__ __forceinline__ double rcp_f64(double x) {
  double r = __builtin_amdgcn_rcp(x);
  return fma(fma(-x, r, 1.0), r, r);
}

// number of eigenvalues of T below sigma (e2 = e squared)
__device__ __forceinline__ int sturm_count(const double* d, const double* e2, int n, double sigma, double pivmin) {
  double q = d[0] - sigma;
  if (fabs(q) < pivmin) q = -pivmin;
  int cnt = q < 0.0;
  for (int i = 1; i < n; ++i) {
    q = d[i] - sigma - e2[i - 1] * rcp_f64(q);
    if (fabs(q) < pivmin) q = -pivmin;
    cnt += q < 0.0;
  }
  return cnt;
}

// Gershgorin range of T and its largest e^2, first half: lane tid < G takes disc tid, each wave reduces its own.
__device__ __forceinline__ void gershgorin_wave(const double* d, const double* e, int G, int tid, double* glo,
                                                double* ghi, double* emax) {
  *glo = 1e300; *ghi = -1e300; *emax = 0.0;
  if (tid < G) {
    const double el = tid > 0 ? fabs(e[tid - 1]) : 0.0, er = tid + 1 < G ? fabs(e[tid]) : 0.0;
    *glo = d[tid] - el - er;
    *ghi = d[tid] + el + er;
    *emax = er * er;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    *glo = fmin(*glo, __shfl_xor(*glo, off));
    *ghi = fmax(*ghi, __shfl_xor(*ghi, off));
    *emax = fmax(*emax, __shfl_xor(*emax, off));
  }
}

// Second half (one barrier inside): the per-wave results meet in the lent arrays (kThreads / 64 doubles each; waves
// without a disc hold the neutral elements); every lane leaves with the range widened by 1e-12 |T|, tnorm = |T|
// and the pivmin of the Sturm recurrence.
template <int kThreads>
__device__ __forceinline__ void gershgorin_block(double* red_lo, double* red_hi, double* red_max, int tid,
                                                 double* glo, double* ghi, double emax, double* tnorm,
                                                 double* pivmin) {
  if ((tid & 63) == 0) { red_lo[tid >> 6] = *glo; red_hi[tid >> 6] = *ghi; red_max[tid >> 6] = emax; }
  __syncthreads();
  *glo = red_lo[0]; *ghi = red_hi[0]; emax = red_max[0];
#pragma unroll
  for (int w = 1; w < kThreads / 64; ++w) {
    *glo = fmin(*glo, red_lo[w]); *ghi = fmax(*ghi, red_hi[w]); emax = fmax(emax, red_max[w]);
  }
  *tnorm = fmax(fabs(*glo), fabs(*ghi));
  *pivmin = fmax(emax, 1.0) * 2.2250738585072014e-308 * 4.0 + 1e-290;
  *glo -= 1e-12 * *tnorm + 1e-300;
  *ghi += 1e-12 * *tnorm + 1e-300;
}

// Eigenvalue number `want` (ascending) of T by multisection: the calling wave evaluates 64 shifts per round and
// narrows [glo, ghi] 65-fold, 5 rounds (65^-5 ~ 1e-9 of the Gershgorin range).  Whole waves call this.
__device__ __forceinline__ double multisect_eigenvalue(const double* d, const double* e2, int G, int want,
                                                       double glo, double ghi, double pivmin, int lane) {
  double lo = glo, hi = ghi;
  for (int round = 0; round < 5; ++round) {
    const double step = (hi - lo) * (1.0 / 65.0);
    const double sigma = lo + step * (lane + 1);
    const int cnt = sturm_count(d, e2, G, sigma, pivmin);
    // lanes whose shift already has more than `want` eigenvalues below it; the first of them bounds lambda
    const unsigned long long above = __ballot(cnt > want);
    const int t = above ? __builtin_ctzll(above) : 64;
    const double nlo = lo + step * t;
    hi = (t == 64) ? hi : lo + step * (t + 1);
    lo = nlo;
  }
  return 0.5 * (lo + hi);
}

// start-vector seed of extracted pair s
__device__ __forceinline__ unsigned inverse_iteration_seed(int s) { return 12345u + 977u * s; }

// Eigenvector of T for the eigenvalue lam by inverse iteration, ONE lane: pivoted LU of (T - lam I) with row
// interchanges between neighbours (U = (1/ra, ub, uc), L = l, P = piv), a deterministic LCG start vector in (-1, 1)
// from `seed`, three solves, each normalised -> z.  All recurrences carry their running values in registers, so the
// LDS traffic (d, e in; factors out) is off the dependent chain; the pivots are stored as reciprocals so the
// back-substitution has no division.
__device__ __forceinline__ void tridiag_inverse_iteration(int n, double lam, double tnorm, unsigned seed,
                                                          const double* d, const double* e, double* ra, double* ub,
                                                          double* uc, double* l, unsigned char* piv, double* z) {
  const double tiny = fmax(tnorm, 1.0) * 1.1e-16;
  double ai = d[0] - lam;                           // running diagonal / super-diagonal of row i
  double bi = (n > 1) ? e[0] : 0.0;
  for (int i = 0; i + 1 < n; ++i) {
    const double sub = e[i];
    const double a1 = d[i + 1] - lam;
    const double b1 = (i + 2 < n) ? e[i + 1] : 0.0;
    if (fabs(ai) >= fabs(sub)) {
      if (fabs(ai) < tiny) ai = tiny;
      const double r = rcp_f64(ai);
      const double mult = sub * r;
      ra[i] = r; ub[i] = bi; uc[i] = 0.0; l[i] = mult; piv[i] = 0;
      ai = a1 - mult * bi;
      bi = b1;
    } else {
      const double r = rcp_f64(sub);
      const double mult = ai * r;
      ra[i] = r; ub[i] = a1; uc[i] = b1; l[i] = mult; piv[i] = 1;      // row i <- old row i+1
      ai = bi - mult * a1;                                                // row i+1 <- old row i - mult * it
      bi = -mult * b1;
    }
  }
  if (fabs(ai) < tiny) ai = tiny;
  ra[n - 1] = rcp_f64(ai); ub[n - 1] = 0.0; uc[n - 1] = 0.0;
  unsigned rng = seed;
  for (int i = 0; i < n; ++i) {
    rng = rng * 1664525u + 1013904223u;
    z[i] = (static_cast<double>(rng >> 8) / 8388608.0) - 1.0;
  }
  for (int it = 0; it < 3; ++it) {
    double zi = z[0];                               // forward: apply P, L^-1
    for (int i = 0; i + 1 < n; ++i) {
      double zn = z[i + 1];
      if (piv[i]) { const double t = zi; zi = zn; zn = t; }
      z[i] = zi;
      zi = zn - l[i] * zi;
    }
    double z1 = zi * ra[n - 1], z2 = 0.0, nr = z1 * z1;   // backward: U z = rhs (two super-diagonals)
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

// modified Gram-Schmidt among the ntot vectors sZ[s * kPitch + i], wave 0 only (tid < 64); exact eigenvectors are
// orthogonal already
template <int kPitch>
__device__ __forceinline__ void gram_schmidt_wave0(double* sZ, int ntot, int G, int tid) {
  for (int s = 1; s < ntot; ++s) {
    double* zs = sZ + s * kPitch;
    for (int t = 0; t < s; ++t) {
      const double* zt = sZ + t * kPitch;
      double dot = 0.0;
      for (int i = tid; i < G; i += 64) dot += zs[i] * zt[i];
      dot = wave_xor_sum(dot);
      for (int i = tid; i < G; i += 64) zs[i] -= dot * zt[i];
    }
    double nr = 0.0;
    for (int i = tid; i < G; i += 64) nr += zs[i] * zs[i];
    nr = 1.0 / sqrt(wave_xor_sum(nr));
    for (int i = tid; i < G; i += 64) zs[i] *= nr;
  }
}

// sign convention, one wave: the component of largest magnitude (as rounded to fp32; first such index on ties)
// becomes positive.  Lane 0 writes +-1 to *sign.
__device__ __forceinline__ void sign_of_largest(const double* z, int G, int lane, float* sign) {
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
  if (lane == 0) *sign = z[bi] < 0.0 ? -1.f : 1.f;
}

// evals (B,k), evecs (B,G,k) and the rank-sort argsort `order` (B,k,G) of the signed vectors; the first `skip`
// extracted pairs are dropped (MATRIX_SYM)
template <int kThreads, int kPitch>
__device__ __forceinline__ void write_topk_outputs(const EigArgs& p, const double* sZ, const double* sLam,
                                                   const float* sSign, int skip) {
  const int G = p.G, nsel = p.k, tid = threadIdx.x;
  if (p.evals && tid < nsel)
    p.evals[static_cast<size_t>(blockIdx.x) * nsel + tid] = static_cast<float>(sLam[tid + skip]);
  if (p.evecs) {
    float* out = p.evecs + static_cast<size_t>(blockIdx.x) * G * nsel;
    for (int e = tid; e < G * nsel; e += kThreads) {
      const int i = e / nsel, mm = e - i * nsel;
      out[e] = static_cast<float>(sZ[(mm + skip) * kPitch + i]) * sSign[mm + skip];
    }
  }
  if (p.order) {
    long long* out = p.order + static_cast<size_t>(blockIdx.x) * nsel * G;
    for (int e = tid; e < G * nsel; e += kThreads) {
      const int mm = e / G, i = e - mm * G;
      const double* z = sZ + (mm + skip) * kPitch;
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

}  // namespace simamba
