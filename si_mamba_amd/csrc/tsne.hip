// Exact t-SNE in two dimensions (the reference's map of the classifier's pooled features, tools/runner_finetune.py:
// 605-612: scikit-learn's TSNE(n_components=2, init='pca')) without the host.  Storage is fp32; fp64 only where a sum
// runs over a whole row of exp terms (the perplexity search) or over the whole grid (Z, the squared gradient norm, KL).
//
// tsne_calibrate_kernel: one 256-lane workgroup per row i of the squared distances, the row staged in LDS less its
// smallest off-diagonal entry (the normalised row does not change, the largest term of every sum is exactly 1, and no
// beta underflows a whole row).  scikit-learn's search for beta_i: start at 1, double or halve until bracketed, then
// bisect; at most 100 steps; stop at |H - log perplexity| <= 1e-5, H = log S + beta T / S with S = sum p, T = sum d p
// accumulated in fp64.  Every lane forms H from the same LDS values, so all waves leave the loop in the same step.
//
// tsne_forces_kernel: thread <-> point i of a 256-row tile, a loop over the columns j of one chunk whose Y sits in LDS.
// P is symmetric, so P[j][i0 .. i0 + 255] is read coalesced and nothing crosses lanes inside the loop.  Each (chunk, i)
// writes its partial A = sum p w (yi - yj) and R = sum w^2 (yi - yj) to the workspace; each (row tile, chunk) writes
// its partial Z = sum w (and, on error launches, E = sum p log(1 + d^2)) in fp64.  No float atomics.
//
// tsne_update_kernel: every workgroup re-sums the (row tiles x chunks) Z partials in the same order, then a thread per
// point sums its chunk partials in ascending chunk order (fp64), forms g = 4 (alpha A - R / Z) and applies
// scikit-learn's gains / momentum rule.  On check launches each workgroup leaves its share of |gains g|^2;
// tsne_status_kernel (one workgroup, launched on those iterations only) finishes KL and the gradient norm and keeps
// scikit-learn's _gradient_descent stop rule in the status record.  Once `stopped` is set every later launch returns at
// once, so the host never looks inside the loop.  No grid-wide barrier, no cooperative launch.
#include <math.h>

#include "host_common.h"

namespace simamba {

constexpr int kTsneThreads = 256;
constexpr int kTsneWaves = kTsneThreads / 64;
constexpr int kTsneMaxN = 16384;
constexpr int kTsneTile = 256;                           // rows of a forces / update workgroup
constexpr int kTsneChunkUnit = 64;                       // a column chunk is a multiple of this
constexpr int kTsneChunkSpan = 40;                       // about this many chunks, so that N = 2 468 covers 256 CUs
constexpr int kTsneMaxChunk = kTsneChunkUnit * ((kTsneMaxN + kTsneChunkUnit * kTsneChunkSpan - 1) /
                                                (kTsneChunkUnit * kTsneChunkSpan));
constexpr int kTsneCheck = 50;                           // scikit-learn's n_iter_check
constexpr int kTsneMaxSteps = 100;
constexpr double kTsneTol = 1e-5;

// status record (doubles): what simamba.h documents
enum { kStKl = 0, kStGradNorm, kStBestError, kStBestIter, kStIters, kStStopped, kStFloats = 8 };

struct TsneGeom {
  int tiles, chunk, chunks;
};
inline TsneGeom tsne_geom(int n) {
  TsneGeom g;
  g.tiles = (n + kTsneTile - 1) / kTsneTile;
  g.chunk = kTsneChunkUnit * ((n + kTsneChunkUnit * kTsneChunkSpan - 1) / (kTsneChunkUnit * kTsneChunkSpan));
  g.chunks = (n + g.chunk - 1) / g.chunk;
  return g;
}
// workspace: [zpart tiles*chunks | epart tiles*chunks | gnpart tiles] doubles, then part[chunks][4][n] floats
inline long long tsne_ws_doubles(const TsneGeom& g) { return 2ll * g.tiles * g.chunks + g.tiles; }
inline long long tsne_ws_floats(int n) {
  const TsneGeom g = tsne_geom(n);
  return 2 * tsne_ws_doubles(g) + 4ll * g.chunks * n;
}

// the sum of v over the workgroup in a fixed order, the same value in every lane; `s` holds kTsneWaves doubles
__device__ __forceinline__ double tsne_block_sum(double v, double* s) {
  v = wave_xor_sum(v);
  __syncthreads();                                       // s is free again
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = s[0];
#pragma unroll
  for (int w = 1; w < kTsneWaves; ++w) t += s[w];
  return t;
}
__device__ __forceinline__ float tsne_block_min(float v, float* s) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fminf(v, __shfl_xor(v, off));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = s[0];
#pragma unroll
  for (int w = 1; w < kTsneWaves; ++w) t = fminf(t, s[w]);
  return t;
}

__global__ __launch_bounds__(kTsneThreads) void tsne_calibrate_kernel(
    const float* __restrict__ d2, float* __restrict__ cond, double* __restrict__ beta_out, int n, double log_perp) {
  extern __shared__ float tsne_row[];                    // n floats: d2[i][.] - min
  __shared__ double sD[kTsneWaves];
  __shared__ float sF[kTsneWaves];
  const int tid = threadIdx.x, i = blockIdx.x;
  if (i >= n) return;                                    // the whole workgroup
  const float* __restrict__ row = d2 + static_cast<size_t>(i) * n;
  float mn = __builtin_huge_valf();
  for (int j = tid; j < n; j += kTsneThreads) {
    const float v = row[j];
    tsne_row[j] = v;
    if (j != i) mn = fminf(mn, v);
  }
  mn = tsne_block_min(mn, sF);
  if (!(mn < __builtin_huge_valf())) mn = 0.f;           // a row of NaN or inf: stays what it is, in bounds
  for (int j = tid; j < n; j += kTsneThreads) tsne_row[j] -= mn;      // each lane its own entries
  double beta = 1.0, lo = -__builtin_huge_val(), hi = __builtin_huge_val(), S = 1.0;
  for (int step = 0; step < kTsneMaxSteps; ++step) {
    const float b2 = static_cast<float>(beta * 1.4426950408889634);
    double s = 0.0, t = 0.0;
    for (int j = tid; j < n; j += kTsneThreads) {
      if (j == i) continue;
      const float d = tsne_row[j];
      const double p = static_cast<double>(fast_exp2(-b2 * d));
      s += p;
      t += static_cast<double>(d) * p;
    }
    S = tsne_block_sum(s, sD);
    const double T = tsne_block_sum(t, sD);
    const double diff = log(S) + beta * T / S - log_perp;
    if (fabs(diff) <= kTsneTol) break;                   // the same S, T in every lane: every wave leaves here together
    if (diff > 0.0) {
      lo = beta;
      beta = hi == __builtin_huge_val() ? beta * 2.0 : (beta + hi) / 2.0;
    } else {                                             // a NaN lands here too: beta halves, the loop still ends
      hi = beta;
      beta = lo == -__builtin_huge_val() ? beta / 2.0 : (beta + lo) / 2.0;
    }
  }
  // the row at the beta the loop left with (after 100 steps: the next candidate, as scikit-learn's last P is not)
  const float b2 = static_cast<float>(beta * 1.4426950408889634);
  double s = 0.0;
  for (int j = tid; j < n; j += kTsneThreads)
    if (j != i) s += static_cast<double>(fast_exp2(-b2 * tsne_row[j]));
  S = tsne_block_sum(s, sD);
  const float inv = static_cast<float>(1.0 / S);
  float* __restrict__ out = cond + static_cast<size_t>(i) * n;
  for (int j = tid; j < n; j += kTsneThreads) out[j] = j == i ? 0.f : fast_exp2(-b2 * tsne_row[j]) * inv;
  if (tid == 0) beta_out[i] = beta;
}

template <bool kError>
__global__ __launch_bounds__(kTsneThreads) void tsne_forces_kernel(
    const float* __restrict__ P, const float* __restrict__ Y, const double* __restrict__ status,
    double* __restrict__ zpart, double* __restrict__ epart, float* __restrict__ part, int n, int chunk, int chunks) {
  __shared__ float sYx[kTsneMaxChunk], sYy[kTsneMaxChunk];
  __shared__ double sD[kTsneWaves];
  if (status && status[kStStopped] != 0.0) return;       // the same word for every lane: the whole grid leaves
  const int tid = threadIdx.x, i = blockIdx.x * kTsneTile + tid, c = blockIdx.y;
  const int j0 = c * chunk;
  const int cols = min(chunk, n - j0);                   // >= 1: chunks = ceil(n / chunk)
  for (int t = tid; t < cols; t += kTsneThreads) {
    sYx[t] = Y[2 * (j0 + t)];
    sYy[t] = Y[2 * (j0 + t) + 1];
  }
  __syncthreads();
  float z = 0.f, ax = 0.f, ay = 0.f, rx = 0.f, ry = 0.f, e = 0.f;
  if (i < n) {
    const float yx = Y[2 * i], yy = Y[2 * i + 1];
    const float* __restrict__ pcol = P + static_cast<size_t>(j0) * n + i;
    for (int t = 0; t < cols; ++t) {
      const float p = pcol[static_cast<size_t>(t) * n];
      const float dx = yx - sYx[t], dy = yy - sYy[t];
      const float dd = dx * dx + dy * dy;
      float w = fast_rcp(1.f + dd);
      w = (j0 + t == i) ? 0.f : w;                       // Z runs over j != i; A and R vanish there by dx = dy = 0
      const float pw = p * w, w2 = w * w;
      z += w;
      ax = fmaf(pw, dx, ax);
      ay = fmaf(pw, dy, ay);
      rx = fmaf(w2, dx, rx);
      ry = fmaf(w2, dy, ry);
      if (kError) e = fmaf(p, log1pf(dd), e);
    }
    float* __restrict__ o = part + static_cast<size_t>(c) * 4 * n + i;
    o[0] = ax;
    o[n] = ay;
    o[2 * static_cast<size_t>(n)] = rx;
    o[3 * static_cast<size_t>(n)] = ry;
  }
  const double zs = tsne_block_sum(static_cast<double>(z), sD);
  double es = 0.0;
  if (kError) es = tsne_block_sum(static_cast<double>(e), sD);
  if (tid == 0) {
    zpart[blockIdx.x * chunks + c] = zs;
    if (kError) epart[blockIdx.x * chunks + c] = es;
  }
}

// sum of m doubles in a fixed order, the same in every workgroup and lane
__device__ __forceinline__ double tsne_sum_parts(const double* __restrict__ v, int m, double* s) {
  double a = 0.0;
  for (int t = threadIdx.x; t < m; t += kTsneThreads) a += v[t];
  return tsne_block_sum(a, s);
}

// g_i = 4 (alpha A_i - R_i / Z) from the chunk partials, summed in ascending chunk order in fp64
__device__ __forceinline__ void tsne_point_grad(const float* __restrict__ part, int i, int n, int chunks, double alpha,
                                                double z, float& gx, float& gy) {
  double ax = 0.0, ay = 0.0, rx = 0.0, ry = 0.0;
  // eight chunks' loads in flight at a time: with ten workgroups on the chip this loop is a chain of load latencies
  // (15.8 us of a 24.8 us iteration at N = 2 468 before the unroll); the adds keep their order
#pragma unroll 8
  for (int c = 0; c < chunks; ++c) {
    const float* __restrict__ o = part + static_cast<size_t>(c) * 4 * n + i;
    ax += o[0];
    ay += o[n];
    rx += o[2 * static_cast<size_t>(n)];
    ry += o[3 * static_cast<size_t>(n)];
  }
  gx = static_cast<float>(4.0 * (alpha * ax - rx / z));
  gy = static_cast<float>(4.0 * (alpha * ay - ry / z));
}

__global__ __launch_bounds__(kTsneThreads) void tsne_gradient_kernel(
    const float* __restrict__ part, const double* __restrict__ zpart, const double* __restrict__ epart,
    const double* __restrict__ sum_plogp, float* __restrict__ grad, double* __restrict__ kl, int n, int tiles,
    int chunks, float alpha) {
  __shared__ double sD[kTsneWaves];
  const double z = tsne_sum_parts(zpart, tiles * chunks, sD);
  const int i = blockIdx.x * kTsneTile + threadIdx.x;
  if (i < n) {
    float gx, gy;
    tsne_point_grad(part, i, n, chunks, static_cast<double>(alpha), z, gx, gy);
    grad[2 * i] = gx;
    grad[2 * i + 1] = gy;
  }
  if (blockIdx.x == 0) {                                 // the whole workgroup
    const double e = tsne_sum_parts(epart, tiles * chunks, sD);
    if (threadIdx.x == 0) kl[0] = sum_plogp[0] + e + log(z);
  }
}

template <bool kCheck>
__global__ __launch_bounds__(kTsneThreads) void tsne_update_kernel(
    const float* __restrict__ part, const double* __restrict__ zpart, double* __restrict__ gnpart,
    const double* __restrict__ status, float* __restrict__ Y, float* __restrict__ update, float* __restrict__ gains,
    int n, int tiles, int chunks, float alpha, float momentum, float lr) {
  __shared__ double sD[kTsneWaves];
  if (status[kStStopped] != 0.0) return;
  const double z = tsne_sum_parts(zpart, tiles * chunks, sD);
  const int i = blockIdx.x * kTsneTile + threadIdx.x;
  double gn = 0.0;
  if (i < n) {
    float g[2];
    tsne_point_grad(part, i, n, chunks, static_cast<double>(alpha), z, g[0], g[1]);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int o = 2 * i + k;
      float u = update[o], ga = gains[o];
      ga = (u * g[k] < 0.f) ? ga + 0.2f : ga * 0.8f;
      ga = fmaxf(ga, 0.01f);
      const float gg = g[k] * ga;
      u = momentum * u - lr * gg;
      gains[o] = ga;
      update[o] = u;
      Y[o] += u;
      gn += static_cast<double>(gg) * gg;                // scikit-learn's norm is taken after grad *= gains
    }
  }
  if (kCheck) {
    gn = tsne_block_sum(gn, sD);
    if (threadIdx.x == 0) gnpart[blockIdx.x] = gn;
  }
}

// One workgroup, on the iterations that compute the error: KL of the iteration's (exaggerated) P, and on check
// iterations scikit-learn's stop rule.
__global__ __launch_bounds__(kTsneThreads) void tsne_status_kernel(
    const double* __restrict__ zpart, const double* __restrict__ epart, const double* __restrict__ gnpart,
    const double* __restrict__ sum_plogp, double* __restrict__ status, int tiles, int chunks, int it, int check,
    int window, double alpha, double min_grad_norm) {
  __shared__ double sD[kTsneWaves];
  if (status[kStStopped] != 0.0) return;
  const double z = tsne_sum_parts(zpart, tiles * chunks, sD);
  const double e = tsne_sum_parts(epart, tiles * chunks, sD);
  const double g2 = tsne_sum_parts(gnpart, tiles, sD);
  if (threadIdx.x != 0) return;
  // sum_ij (alpha p) log(alpha p / q), q = w / Z, sum p = 1
  const double kl = alpha * (sum_plogp[0] + e + log(alpha) + log(z));
  status[kStKl] = kl;
  status[kStIters] = static_cast<double>(it + 1);
  if (!check) return;
  const double gnorm = sqrt(g2);
  status[kStGradNorm] = gnorm;
  bool stop = false;
  if (kl < status[kStBestError]) {
    status[kStBestError] = kl;
    status[kStBestIter] = static_cast<double>(it);
  } else if (static_cast<double>(it) - status[kStBestIter] > static_cast<double>(window)) {
    stop = true;
  }
  if (gnorm <= min_grad_norm) stop = true;
  if (stop) status[kStStopped] = 1.0;
}

template <bool kError>
static void tsne_launch_forces(const float* p, const float* y, const double* status, float* ws, int n,
                               hipStream_t stream) {
  const TsneGeom g = tsne_geom(n);
  double* wd = reinterpret_cast<double*>(ws);
  double* zpart = wd;
  double* epart = wd + static_cast<size_t>(g.tiles) * g.chunks;
  float* part = ws + 2 * tsne_ws_doubles(g);
  hipLaunchKernelGGL(tsne_forces_kernel<kError>, dim3(g.tiles, g.chunks), dim3(kTsneThreads), 0, stream, p, y, status,
                     zpart, epart, part, n, g.chunk, g.chunks);
}

}  // namespace simamba

using namespace simamba;

extern "C" int simamba_tsne_calibrate(const float* d2, float* cond, double* beta, int n, float perplexity,
                                      void* stream) {
  if (n < 2 || n > kTsneMaxN) return SIMAMBA_E_SHAPE;
  if (!(perplexity > 0.f) || !(perplexity < static_cast<float>(n))) return SIMAMBA_E_SHAPE;
  if (!d2 || !cond || !beta) return SIMAMBA_E_NULLPTR;
  if (const hipError_t e = ensure_lds_cap<tsne_calibrate_kernel>(kTsneMaxN * 4)) return static_cast<int>(e);
  hipLaunchKernelGGL(tsne_calibrate_kernel, dim3(n), dim3(kTsneThreads), static_cast<size_t>(n) * 4,
                     static_cast<hipStream_t>(stream), d2, cond, beta, n, log(static_cast<double>(perplexity)));
  return static_cast<int>(hipGetLastError());
}

extern "C" long long simamba_tsne_workspace_floats(int n) {
  if (n < 2 || n > kTsneMaxN) return SIMAMBA_E_SHAPE;
  return tsne_ws_floats(n);
}

extern "C" int simamba_tsne_gradient(const float* p, const float* y, float* grad, double* kl, float* ws,
                                     const double* sum_plogp, int n, float exaggeration, void* stream) {
  if (n < 2 || n > kTsneMaxN) return SIMAMBA_E_SHAPE;
  if (!(exaggeration > 0.f) || !(exaggeration < __builtin_huge_valf())) return SIMAMBA_E_SHAPE;
  if (!p || !y || !grad || !kl || !sum_plogp) return SIMAMBA_E_NULLPTR;
  if (!ws) return SIMAMBA_E_WORKSPACE;
  if (!aligned16(ws)) return SIMAMBA_E_ALIGN;
  const TsneGeom g = tsne_geom(n);
  hipStream_t s = static_cast<hipStream_t>(stream);
  tsne_launch_forces<true>(p, y, nullptr, ws, n, s);
  double* wd = reinterpret_cast<double*>(ws);
  hipLaunchKernelGGL(tsne_gradient_kernel, dim3(g.tiles), dim3(kTsneThreads), 0, s, ws + 2 * tsne_ws_doubles(g), wd,
                     wd + static_cast<size_t>(g.tiles) * g.chunks, sum_plogp, grad, kl, n, g.tiles, g.chunks,
                     exaggeration);
  return static_cast<int>(hipGetLastError());
}

extern "C" int simamba_tsne_run(const float* p, float* y, float* update, float* gains, double* status, float* ws,
                                const double* sum_plogp, const double* params, int n, int first_iter, int n_iter,
                                int window, void* stream) {
  if (n < 2 || n > kTsneMaxN) return SIMAMBA_E_SHAPE;
  if (first_iter < 0 || n_iter < 0 || window < 0 || first_iter > 0x7fffffff - n_iter) return SIMAMBA_E_SHAPE;
  double alpha = 0.0, momentum = 0.0, lr = 0.0, min_grad_norm = 0.0;
  if (params) {                                          // a HOST array: the ABI passes no double by value
    alpha = params[0];
    momentum = params[1];
    lr = params[2];
    min_grad_norm = params[3];
    if (!(alpha > 0.0) || !(alpha < 3e38) || !(momentum >= 0.0) || !(momentum < 1.0) || !(lr > 0.0) || !(lr < 3e38) ||
        !(min_grad_norm >= 0.0))
      return SIMAMBA_E_SHAPE;
  }
  if (!p || !y || !update || !gains || !status || !sum_plogp || !params) return SIMAMBA_E_NULLPTR;
  if (!ws) return SIMAMBA_E_WORKSPACE;
  if (!aligned16(ws)) return SIMAMBA_E_ALIGN;
  const TsneGeom g = tsne_geom(n);
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* wd = reinterpret_cast<double*>(ws);
  double* zpart = wd;
  double* epart = wd + static_cast<size_t>(g.tiles) * g.chunks;
  double* gnpart = epart + static_cast<size_t>(g.tiles) * g.chunks;
  float* part = ws + 2 * tsne_ws_doubles(g);
  const float fa = static_cast<float>(alpha), fm = static_cast<float>(momentum), fl = static_cast<float>(lr);
  const int last = first_iter + n_iter - 1;
  for (int it = first_iter; it <= last; ++it) {
    const bool check = (it + 1) % kTsneCheck == 0;
    const bool error = check || it == last;              // scikit-learn computes the error on the last iteration too
    if (error) {
      tsne_launch_forces<true>(p, y, status, ws, n, s);
      hipLaunchKernelGGL(tsne_update_kernel<true>, dim3(g.tiles), dim3(kTsneThreads), 0, s, part, zpart, gnpart,
                         status, y, update, gains, n, g.tiles, g.chunks, fa, fm, fl);
      hipLaunchKernelGGL(tsne_status_kernel, dim3(1), dim3(kTsneThreads), 0, s, zpart, epart, gnpart, sum_plogp,
                         status, g.tiles, g.chunks, it, check ? 1 : 0, window, alpha, min_grad_norm);
    } else {
      tsne_launch_forces<false>(p, y, status, ws, n, s);
      hipLaunchKernelGGL(tsne_update_kernel<false>, dim3(g.tiles), dim3(kTsneThreads), 0, s, part, zpart, gnpart,
                         status, y, update, gains, n, g.tiles, g.chunks, fa, fm, fl);
    }
  }
  return static_cast<int>(hipGetLastError());
}
