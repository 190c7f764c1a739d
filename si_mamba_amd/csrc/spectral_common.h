// Shared host declarations of the spectral kernels (spectral.hip, spectral_tridiag.hip, spectral_large.hip); the
// device steps they share are in spectral_device.h.
#pragma once
#include "host_common.h"   // ensure_lds_cap

namespace simamba {

constexpr int kSpecMaxG = 128;       // LDS-resident kernels (spectral.hip, spectral_tridiag.hip)
constexpr int kSpecMaxGLarge = 512;  // global-workspace kernels (spectral_large.hip), 128 < G <= 512
constexpr int kKnnMaxK = 32;         // knn + 1 <= 32 list entries per node
constexpr int kTdMaxSel = 8;      // eigenpairs the tridiagonal path extracts at most (k, +1 for MATRIX_SYM)

struct EigArgs {
  const float* adj;
  float* evals;
  float* evecs;
  long long* order;
  float* all_evals;
  float* all_evecs;
  int B, G, k;
  unsigned flags;
};

int launch_tridiag_topk(const EigArgs& a, hipStream_t s);
// large-G paths: adjacency in the caller's adj (zero-filled here); the Laplacian in `ws` (B*G*G floats)
int launch_knn_graph_large(const float* pts, float* adj, const double* dist_sum, int B, int G, int F, int knn,
                           float alpha, unsigned flags, hipStream_t s);
int launch_laplacian_large_topk(const EigArgs& a, float* ws, hipStream_t s);

}  // namespace simamba
