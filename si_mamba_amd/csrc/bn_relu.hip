// BatchNorm1d (+ per-group additive term) + ReLU, and the max over a group's points, for the patch encoder
// (reference models/point_mamba.py:46-73: Conv1d - BatchNorm1d - ReLU - Conv1d, max over the n points of a patch,
// concat [global, local] - Conv1d - BatchNorm1d - ReLU - Conv1d, max).  HBM-bound streaming kernels over the
// token-major (rows, C) activations the 1x1 convolutions produce as GEMMs:
//
//   * forward   : pass 1 per-channel shifted sums (one read), finalize (mean, 1/std, running statistics),
//                 pass 2 y = relu((x + g - mean) * invstd * w + b) (one read, one write): 3 passes instead of the 5
//                 of stock batch_norm + relu;
//   * backward  : pass 1 sums of dy*mask and dy*mask*xhat (two reads), finalize (dweight, dbias),
//                 pass 2 dx (two reads, one write) and the per-group sum of dx (the gradient of the additive
//                 term): 5 passes instead of 8;
//   * the additive term g[r / group][c] is the "global feature" half of the encoder's second convolution:
//     cat([max_n f, f]) @ W^T == f @ W_local^T + (max_n f) @ W_global^T, the second product having one row per
//     patch instead of one per point -- the 537 MB concat tensor and a quarter of the GEMM flops disappear.
//
// A thread owns 4 consecutive channels (one 16-byte access fp32 / 8-byte bf16) for the whole kernel, so the
// per-channel constants sit in registers; a workgroup is TPR = C / 4 lanes per row x RL row lanes and walks a
// chunk of kBnChunk rows.  Per-workgroup partial sums go to a (grid, 2, C) buffer and are combined in fp64 by
// a one-workgroup finalize kernel: deterministic, no atomics.  Sums are taken about the first row's value
// (shifted data), which removes the cancellation in E[x^2] - E[x]^2.
//
// Cross-rank statistics (nn.SyncBatchNorm): the same kernels, entered stage by stage so that a collective fits between
// the passes.  simamba_bn_stats_local leaves this rank's (count, mean, M2 = sum (x - mean)^2) per channel in fp64 -- free
// of the rank's own shift -- simamba_bn_stats_merge combines the all-gathered (W, 3, C) block in rank order with the
// pairwise update of Chan et al. (every rank gets the same bits), simamba_bn_relu_apply is pass 2 with those
// statistics; simamba_bn_relu_bwd_sums leaves the rank's (sum dy*mask, sum dy*mask*xhat), the caller all-reduces them,
// simamba_bn_relu_bwd_dx is the backward's pass 2 with the global sums and the global row count (read from the device
// buffer the merge wrote: no host read anywhere).
#include "host_common.h"

namespace simamba {

constexpr int kBnChunk = 256;        // rows per workgroup (a multiple of the group size)
constexpr int kBnMaxThreads = 256;

struct BnArgs {
  const void* x;
  const float* gterm;
  const float* weight;
  const float* bias;
  const float* mean;
  const float* invstd;
  const void* dy;
  void* y;            // forward output / backward dx
  float* dgterm;
  float* partial;     // (grid, 2, C)
  const double* count;  // staged backward: the row count of all ranks (device); NULL: rows
  long long rows;
  long long ld;       // row stride (elements) of x / y / dy / dx: channel slices of a wider tensor are processed in place
  int C, group, dgroup, training;
};

template <typename T>
__device__ __forceinline__ void load_c4(const T* p, float (&v)[4]) {
  const Pack<T, 4> pk = *reinterpret_cast<const Pack<T, 4>*>(p);
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = to_f32<T>(pk.v[i]);
}
template <typename T>
__device__ __forceinline__ void store_c4(T* p, const float (&v)[4]) {
  Pack<T, 4> pk;
#pragma unroll
  for (int i = 0; i < 4; ++i) pk.v[i] = from_f32<T>(v[i]);
  *reinterpret_cast<Pack<T, 4>*>(p) = pk;
}

// this thread's 4 channels of row r: v += gterm[r / group]
__device__ __forceinline__ void add_gterm(const float* gterm, int group, int C, long long r, int cl, float (&v)[4]) {
  if (gterm) {
    const float4 g = *reinterpret_cast<const float4*>(gterm + (r / group) * C + 4 * cl);
    v[0] += g.x; v[1] += g.y; v[2] += g.z; v[3] += g.w;
  }
}

// the rows [r0, r1) of this workgroup
__device__ __forceinline__ long long chunk_begin() { return static_cast<long long>(blockIdx.x) * kBnChunk; }
__device__ __forceinline__ long long chunk_end(long long r0, long long rows) { return min(r0 + kBnChunk, rows); }

// combine the RL row lanes of a workgroup: s0 / s1 hold this thread's two 4-channel sums
__device__ __forceinline__ void reduce_row_lanes(float (&s0)[4], float (&s1)[4], float* sm, int tpr, int rl,
                                                 int cl, int rlane, float* out, int C) {
  // sm: [rl][2][C]
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    sm[(rlane * 2 + 0) * C + 4 * cl + i] = s0[i];
    sm[(rlane * 2 + 1) * C + 4 * cl + i] = s1[i];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 2 * C; e += blockDim.x) {
    float acc = 0.f;
    for (int r = 0; r < rl; ++r) acc += sm[r * 2 * C + e];
    out[e] = acc;
  }
}

// ---- forward pass 1: shifted sums -----------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBnMaxThreads) void bn_stats_kernel(BnArgs p) {
  extern __shared__ float sm[];
  const int C = p.C, tpr = C / 4, rl = blockDim.x / tpr;
  const int cl = threadIdx.x % tpr, rlane = threadIdx.x / tpr;
  const T* __restrict__ x = static_cast<const T*>(p.x);
  float K[4];
  load_c4<T>(x + 4 * cl, K);                                   // shift: the first row (same for every workgroup)
  if (p.gterm) {
#pragma unroll
    for (int i = 0; i < 4; ++i) K[i] += p.gterm[4 * cl + i];
  }
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  const long long r0 = chunk_begin(), r1 = chunk_end(r0, p.rows);
#pragma unroll 4
  for (long long r = r0 + rlane; r < r1; r += rl) {
    float v[4];
    load_c4<T>(x + r * p.ld + 4 * cl, v);
    add_gterm(p.gterm, p.group, C, r, cl, v);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float d = v[i] - K[i];
      s1[i] += d;
      s2[i] = fmaf(d, d, s2[i]);
    }
  }
  reduce_row_lanes(s1, s2, sm, tpr, rl, cl, rlane, p.partial + static_cast<size_t>(blockIdx.x) * 2 * C, C);
}

// finalize: fp64 combination of the per-workgroup partials.  A workgroup of 256 threads owns kFinCh channels:
// thread (pl, c) sums partials pl, pl + kFinPl, ... of channel c, the kFinPl lanes are combined through LDS.
constexpr int kFinCh = 16, kFinPl = 16;

__device__ __forceinline__ void finalize_sums(const float* __restrict__ partial, int grid, int C, int c, int pl,
                                              bool valid, double (*sm)[kFinPl][kFinCh], double& S1, double& S2) {
  double a1 = 0.0, a2 = 0.0;
  if (valid) {
#pragma unroll 4
    for (int g = pl; g < grid; g += kFinPl) {
      a1 += partial[(static_cast<size_t>(g) * 2 + 0) * C + c];
      a2 += partial[(static_cast<size_t>(g) * 2 + 1) * C + c];
    }
  }
  const int cl = threadIdx.x % kFinCh;
  sm[0][pl][cl] = a1;
  sm[1][pl][cl] = a2;
  __syncthreads();
  S1 = 0.0; S2 = 0.0;
  for (int k = 0; k < kFinPl; ++k) { S1 += sm[0][k][cl]; S2 += sm[1][k][cl]; }
}

template <typename T>
__global__ __launch_bounds__(kFinCh * kFinPl) void bn_stats_finalize_kernel(
    const void* x, const float* gterm, const float* partial, int grid, long long rows, int C, float eps,
    float momentum, float* mean, float* invstd, float* running_mean, float* running_var) {
  __shared__ double sm[2][kFinPl][kFinCh];
  const int c = blockIdx.x * kFinCh + threadIdx.x % kFinCh, pl = threadIdx.x / kFinCh;
  double S1, S2;
  finalize_sums(partial, grid, C, c, pl, c < C, sm, S1, S2);
  if (c >= C || pl != 0) return;
  float K = to_f32<T>(static_cast<const T*>(x)[c]);
  if (gterm) K += gterm[c];
  const double n = static_cast<double>(rows);
  const double m1 = S1 / n;
  double var = S2 / n - m1 * m1;
  var = var < 0.0 ? 0.0 : var;
  const double mu = static_cast<double>(K) + m1;
  mean[c] = static_cast<float>(mu);
  invstd[c] = static_cast<float>(1.0 / sqrt(var + static_cast<double>(eps)));
  if (running_mean) running_mean[c] = static_cast<float>((1.0 - momentum) * running_mean[c] + momentum * mu);
  if (running_var) {
    const double unbiased = rows > 1 ? var * n / (n - 1.0) : var;
    running_var[c] = static_cast<float>((1.0 - momentum) * running_var[c] + momentum * unbiased);
  }
}

// staged form of the finalize: this rank's (count, mean, M2) per channel in fp64, rows of a (3, C) block with row stride
// sld.  M2 = sum (x - mean)^2 = S2 - S1^2 / n does not depend on the shift K, so blocks of ranks with different first
// rows can be merged.  No running statistics here: they belong to the merged result.
template <typename T>
__global__ __launch_bounds__(kFinCh * kFinPl) void bn_stats_local_finalize_kernel(
    const void* x, const float* gterm, const float* partial, int grid, long long rows, int C, double* stats,
    long long sld) {
  __shared__ double sm[2][kFinPl][kFinCh];
  const int c = blockIdx.x * kFinCh + threadIdx.x % kFinCh, pl = threadIdx.x / kFinCh;
  double S1, S2;
  finalize_sums(partial, grid, C, c, pl, c < C, sm, S1, S2);
  if (c >= C || pl != 0) return;
  float K = to_f32<T>(static_cast<const T*>(x)[c]);
  if (gterm) K += gterm[c];
  const double n = static_cast<double>(rows);
  double m2 = S2 - S1 * S1 / n;
  m2 = m2 < 0.0 ? 0.0 : m2;
  stats[c] = n;
  stats[sld + c] = static_cast<double>(K) + S1 / n;
  stats[2 * sld + c] = m2;
}

// merge of the all-gathered (W, 3, C) block, one thread per channel, ranks in the order 0 .. W-1 (a fixed order: every
// rank computes the same bits).  Pairwise update: n = na + nb, d = mb - ma, mean = ma + d nb / n,
// M2 = M2a + M2b + d^2 na nb / n.  Never E[x^2] - E[x]^2.
__global__ void bn_stats_merge_kernel(const double* __restrict__ stats, int W, int C, float eps, float momentum,
                                      float* mean, float* invstd, double* count, float* running_mean,
                                      float* running_var) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double n = 0.0, mu = 0.0, m2 = 0.0;
  for (int w = 0; w < W; ++w) {
    const double* b = stats + static_cast<size_t>(w) * 3 * C;
    const double nb = b[c];
    if (!(nb > 0.0)) continue;                        // a rank without rows adds nothing
    if (n == 0.0) { n = nb; mu = b[C + c]; m2 = b[2 * C + c]; continue; }
    const double nn = n + nb, d = b[C + c] - mu;
    mu += d * (nb / nn);
    m2 += b[2 * C + c] + d * d * (n * nb / nn);
    n = nn;
  }
  double var = n > 0.0 ? m2 / n : 0.0;
  var = var < 0.0 ? 0.0 : var;
  mean[c] = static_cast<float>(mu);
  invstd[c] = static_cast<float>(1.0 / sqrt(var + static_cast<double>(eps)));
  if (running_mean) running_mean[c] = static_cast<float>((1.0 - momentum) * running_mean[c] + momentum * mu);
  if (running_var) {
    const double unbiased = n > 1.0 ? var * n / (n - 1.0) : var;
    running_var[c] = static_cast<float>((1.0 - momentum) * running_var[c] + momentum * unbiased);
  }
  if (c == 0) *count = n;
}

// eval mode: statistics are the running ones
__global__ void bn_eval_stats_kernel(const float* running_mean, const float* running_var, float eps, int C,
                                     float* mean, float* invstd) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  mean[c] = running_mean[c];
  invstd[c] = 1.0f / sqrtf(running_var[c] + eps);
}

// ---- forward pass 2: normalise + ReLU ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBnMaxThreads) void bn_relu_apply_kernel(BnArgs p) {
  const int C = p.C, tpr = C / 4, rl = blockDim.x / tpr;
  const int cl = threadIdx.x % tpr, rlane = threadIdx.x / tpr;
  const T* __restrict__ x = static_cast<const T*>(p.x);
  T* __restrict__ y = static_cast<T*>(p.y);
  float scale[4], shift[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = 4 * cl + i;
    scale[i] = p.invstd[c] * (p.weight ? p.weight[c] : 1.f);
    shift[i] = (p.bias ? p.bias[c] : 0.f) - p.mean[c] * scale[i];
  }
  const long long r0 = chunk_begin(), r1 = chunk_end(r0, p.rows);
#pragma unroll 4
  for (long long r = r0 + rlane; r < r1; r += rl) {
    float v[4];
    load_c4<T>(x + r * p.ld + 4 * cl, v);
    add_gterm(p.gterm, p.group, C, r, cl, v);
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = fmaxf(fmaf(v[i], scale[i], shift[i]), 0.f);
    store_c4<T>(y + r * p.ld + 4 * cl, o);
  }
}

// ---- backward pass 1: sum dy*mask, sum dy*mask*xhat ---------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBnMaxThreads) void bn_relu_bwd_reduce_kernel(BnArgs p) {
  extern __shared__ float sm[];
  const int C = p.C, tpr = C / 4, rl = blockDim.x / tpr;
  const int cl = threadIdx.x % tpr, rlane = threadIdx.x / tpr;
  const T* __restrict__ x = static_cast<const T*>(p.x);
  const T* __restrict__ dy = static_cast<const T*>(p.dy);
  float scale[4], shift[4], mu[4], is[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = 4 * cl + i;
    mu[i] = p.mean[c]; is[i] = p.invstd[c];
    scale[i] = is[i] * (p.weight ? p.weight[c] : 1.f);
    shift[i] = (p.bias ? p.bias[c] : 0.f) - mu[i] * scale[i];
  }
  float sb[4] = {0.f, 0.f, 0.f, 0.f}, sw[4] = {0.f, 0.f, 0.f, 0.f};
  const long long r0 = chunk_begin(), r1 = chunk_end(r0, p.rows);
#pragma unroll 4
  for (long long r = r0 + rlane; r < r1; r += rl) {
    float v[4], d[4];
    load_c4<T>(x + r * p.ld + 4 * cl, v);
    load_c4<T>(dy + r * p.ld + 4 * cl, d);
    add_gterm(p.gterm, p.group, C, r, cl, v);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float dr = fmaf(v[i], scale[i], shift[i]) > 0.f ? d[i] : 0.f;
      sb[i] += dr;
      sw[i] = fmaf(dr, (v[i] - mu[i]) * is[i], sw[i]);
    }
  }
  reduce_row_lanes(sb, sw, sm, tpr, rl, cl, rlane, p.partial + static_cast<size_t>(blockIdx.x) * 2 * C, C);
}

__global__ __launch_bounds__(kFinCh * kFinPl) void bn_bwd_finalize_kernel(const float* partial, int grid, int C,
                                                                             float* dweight, float* dbias) {
  __shared__ double sm[2][kFinPl][kFinCh];
  const int c = blockIdx.x * kFinCh + threadIdx.x % kFinCh, pl = threadIdx.x / kFinCh;
  double Sb, Sw;
  finalize_sums(partial, grid, C, c, pl, c < C, sm, Sb, Sw);
  if (c >= C || pl != 0) return;
  dbias[c] = static_cast<float>(Sb);
  dweight[c] = static_cast<float>(Sw);
}

// ---- backward pass 2: dx, and the per-group sum of dx -------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBnMaxThreads) void bn_relu_bwd_dx_kernel(BnArgs p, const float* dweight,
                                                                        const float* dbias) {
  extern __shared__ float sm[];                    // [rl][C] for the group sums
  const int C = p.C, tpr = C / 4, rl = blockDim.x / tpr;
  const int cl = threadIdx.x % tpr, rlane = threadIdx.x / tpr;
  const T* __restrict__ x = static_cast<const T*>(p.x);
  const T* __restrict__ dy = static_cast<const T*>(p.dy);
  T* __restrict__ dx = static_cast<T*>(p.y);
  float scale[4], shift[4], mu[4], is[4], kb[4], kw[4];
  const float inv_n = 1.f / (p.count ? static_cast<float>(*p.count) : static_cast<float>(p.rows));
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = 4 * cl + i;
    mu[i] = p.mean[c]; is[i] = p.invstd[c];
    scale[i] = is[i] * (p.weight ? p.weight[c] : 1.f);
    shift[i] = (p.bias ? p.bias[c] : 0.f) - mu[i] * scale[i];
    kb[i] = p.training ? dbias[c] * inv_n : 0.f;
    kw[i] = p.training ? dweight[c] * inv_n : 0.f;
  }
  const long long r0 = chunk_begin(), r1 = chunk_end(r0, p.rows);
  const int group = p.dgterm ? p.dgroup : kBnChunk;
  for (long long gbase = r0; gbase < r1; gbase += group) {
    float gs[4] = {0.f, 0.f, 0.f, 0.f};
    const long long gend = min(gbase + group, r1);
#pragma unroll 4
    for (long long r = gbase + rlane; r < gend; r += rl) {
      float v[4], d[4], o[4];
      load_c4<T>(x + r * p.ld + 4 * cl, v);
      load_c4<T>(dy + r * p.ld + 4 * cl, d);
      add_gterm(p.gterm, p.group, C, r, cl, v);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float dr = fmaf(v[i], scale[i], shift[i]) > 0.f ? d[i] : 0.f;
        const float xh = (v[i] - mu[i]) * is[i];
        o[i] = scale[i] * (dr - kb[i] - xh * kw[i]);
        gs[i] += o[i];
      }
      store_c4<T>(dx + r * p.ld + 4 * cl, o);
    }
    if (p.dgterm) {
      __syncthreads();                              // previous group's reads of sm are done
#pragma unroll
      for (int i = 0; i < 4; ++i) sm[rlane * C + 4 * cl + i] = gs[i];
      __syncthreads();
      for (int e = threadIdx.x; e < C; e += blockDim.x) {
        float acc = 0.f;
        for (int r = 0; r < rl; ++r) acc += sm[r * C + e];
        p.dgterm[(gbase / p.dgroup) * C + e] = acc;
      }
    }
  }
}

// ---- max over the n points of a group ------------------------------------------------------------------------------
template <typename T>
__global__ void group_max_fwd_kernel(const T* __restrict__ x, T* __restrict__ out, unsigned char* __restrict__ idx,
                                     long long groups, int n, int C) {
  const long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;   // (group, channel quad)
  const int cq = C / 4;
  if (e >= groups * cq) return;
  const long long g = e / cq;
  const int c = static_cast<int>(e - g * cq) * 4;
  const T* base = x + g * n * C + c;
  float best[4];
  int bi[4] = {0, 0, 0, 0};
  load_c4<T>(base, best);
  for (int r = 1; r < n; ++r) {
    float v[4];
    load_c4<T>(base + static_cast<long long>(r) * C, v);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool take = (v[i] > best[i]) || (v[i] != v[i] && best[i] == best[i]);   // first max; NaN wins
      best[i] = take ? v[i] : best[i];
      bi[i] = take ? r : bi[i];
    }
  }
  store_c4<T>(out + g * C + c, best);
  *reinterpret_cast<uchar4*>(idx + g * C + c) = make_uchar4(bi[0], bi[1], bi[2], bi[3]);
}

// same (group, channel quad) -> lane map as the forward: a lane walks the n rows of its group and writes dout to the
// arg-max row, zeros elsewhere (no per-element index arithmetic; the (group, row, quad) map of the first version
// spent its time in 64-bit divisions and reached 2.6 TB/s)
template <typename T>
__global__ void group_max_bwd_kernel(const T* __restrict__ dout, const unsigned char* __restrict__ idx,
                                     T* __restrict__ dx, long long groups, int n, int C) {
  const long long e = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;   // (group, channel quad)
  const int cq = C / 4;
  if (e >= groups * cq) return;
  const long long g = e / cq;
  const int c = static_cast<int>(e - g * cq) * 4;
  float d[4];
  load_c4<T>(dout + g * C + c, d);
  const uchar4 id = *reinterpret_cast<const uchar4*>(idx + g * C + c);
  T* base = dx + g * n * C + c;
#pragma unroll 4
  for (int r = 0; r < n; ++r) {
    float o[4];
    o[0] = id.x == r ? d[0] : 0.f; o[1] = id.y == r ? d[1] : 0.f;
    o[2] = id.z == r ? d[2] : 0.f; o[3] = id.w == r ? d[3] : 0.f;
    store_c4<T>(base + static_cast<long long>(r) * C, o);
  }
}

static bool bn_shape_ok(long long rows, int C, long long ld, int group, bool has_g) {
  if (rows <= 0 || C < 4 || C > 4 * kBnMaxThreads || (C % 4) != 0 || ld < C || (ld % 4) != 0) return false;
  if (has_g && (group <= 0 || (rows % group) != 0)) return false;
  return true;
}

// ---- argument checks ------------------------------------------------------------------------------------------------
constexpr int kNothingToDo = 1;       // an empty problem: the entry point answers SIMAMBA_OK without a launch
static int entry_result(int rc) { return rc == kNothingToDo ? SIMAMBA_OK : rc; }

// What every entry point that walks (rows, C) activations does first, in the order they report: dtype, empty, the
// "0 = contiguous" row stride, shape.  Each entry point's own null pointers come after it.
static int bn_check(int io_dtype, long long rows, int C, long long& ld, int group, const float* gterm) {
  if (const int rc = check_io_dtype(io_dtype)) return rc;
  if (rows == 0) return kNothingToDo;
  if (ld == 0) ld = C;
  return bn_shape_ok(rows, C, ld, group, gterm != nullptr) ? SIMAMBA_OK : SIMAMBA_E_SHAPE;
}

// The backward's pointers and its per-group sums of dx: dgroup > 0 divides kBnChunk and the rows (shape, before any
// pointer), `required` = the entry point's own pointers are all there, and dgterm needs the gterm it is the gradient of.
static int bn_check_dgterm(const float* dgterm, int dgroup, long long rows, const float* gterm, bool required) {
  if (dgterm && (dgroup <= 0 || (kBnChunk % dgroup) != 0 || (rows % dgroup) != 0)) return SIMAMBA_E_SHAPE;
  if (!required || (dgterm && !gterm)) return SIMAMBA_E_NULLPTR;
  return SIMAMBA_OK;
}

// ---- the passes: grid, block, LDS bytes and the I/O type of each, in one place ----------------------------------------
// the fields every route sets; the routes add their outputs (and the fused ones their `training`, the backward `dgroup`)
static BnArgs bn_args(const void* x, const float* gterm, int group, const float* weight, const float* bias,
                      const float* mean, const float* invstd, long long rows, int C, long long ld) {
  BnArgs a{};
  a.x = x; a.gterm = gterm; a.weight = weight; a.bias = bias; a.mean = mean; a.invstd = invstd;
  a.rows = rows; a.ld = ld; a.C = C; a.group = group; a.dgroup = group; a.training = 1;
  return a;
}
static dim3 bn_grid(const BnArgs& a) { return dim3(simamba_bn_relu_grid(a.rows)); }
static dim3 bn_block(int C) {
  const int tpr = C / 4;
  const int rl = kBnMaxThreads / tpr > 0 ? kBnMaxThreads / tpr : 1;
  return dim3(tpr * rl);
}
// `planes` planes of (row lanes, C) floats
static size_t bn_lds(int C, int planes) { return sizeof(float) * planes * C * (bn_block(C).x / (C / 4)); }
static dim3 fin_grid(int C) { return dim3((C + kFinCh - 1) / kFinCh); }
static dim3 fin_block() { return dim3(kFinCh * kFinPl); }

// where the batch statistics go: the fused finalize (mean, invstd, running statistics) or, with `stats`, this rank's
// (count, mean, M2) block
struct BnStatsOut {
  float eps, momentum;
  float *mean, *invstd, *running_mean, *running_var;
  double* stats;
  long long stats_ld;
};

static void launch_stats(const BnArgs& a, int io_dtype, hipStream_t s, const BnStatsOut& o) {
  const dim3 grid = bn_grid(a);
  with_io_type(io_dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(bn_stats_kernel<T>, grid, bn_block(a.C), bn_lds(a.C, 2), s, a);
    if (o.stats)
      hipLaunchKernelGGL(bn_stats_local_finalize_kernel<T>, fin_grid(a.C), fin_block(), 0, s, a.x, a.gterm, a.partial,
                         static_cast<int>(grid.x), a.rows, a.C, o.stats, o.stats_ld);
    else
      hipLaunchKernelGGL(bn_stats_finalize_kernel<T>, fin_grid(a.C), fin_block(), 0, s, a.x, a.gterm, a.partial,
                         static_cast<int>(grid.x), a.rows, a.C, o.eps, o.momentum, o.mean, o.invstd, o.running_mean,
                         o.running_var);
  });
}

static void launch_eval_stats(const BnArgs& a, hipStream_t s, const float* running_mean, const float* running_var,
                              float eps, float* mean, float* invstd) {
  hipLaunchKernelGGL(bn_eval_stats_kernel, dim3((a.C + 127) / 128), dim3(128), 0, s, running_mean, running_var, eps,
                     a.C, mean, invstd);
}

static void launch_apply(const BnArgs& a, int io_dtype, hipStream_t s) {
  with_io_type(io_dtype, [&](auto tag) {
    hipLaunchKernelGGL(bn_relu_apply_kernel<decltype(tag)>, bn_grid(a), bn_block(a.C), 0, s, a);
  });
}

static void launch_bwd_sums(const BnArgs& a, int io_dtype, hipStream_t s, float* dweight, float* dbias) {
  const dim3 grid = bn_grid(a);
  with_io_type(io_dtype, [&](auto tag) {
    hipLaunchKernelGGL(bn_relu_bwd_reduce_kernel<decltype(tag)>, grid, bn_block(a.C), bn_lds(a.C, 2), s, a);
  });
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, fin_grid(a.C), fin_block(), 0, s, a.partial, static_cast<int>(grid.x), a.C,
                     dweight, dbias);
}

static void launch_bwd_dx(const BnArgs& a, int io_dtype, hipStream_t s, const float* dweight, const float* dbias) {
  with_io_type(io_dtype, [&](auto tag) {
    hipLaunchKernelGGL(bn_relu_bwd_dx_kernel<decltype(tag)>, bn_grid(a), bn_block(a.C), bn_lds(a.C, 1), s, a, dweight,
                       dbias);
  });
}

// dtype, no groups, shape, pointers, and a grid that fits 32 bits
static int group_max_check(int io_dtype, long long groups, int n, int C, bool pointers, dim3& grid) {
  if (const int rc = check_io_dtype(io_dtype)) return rc;
  if (groups == 0) return kNothingToDo;
  if (groups < 0 || n < 1 || n > 256 || C < 4 || (C % 4) != 0) return SIMAMBA_E_SHAPE;
  if (!pointers) return SIMAMBA_E_NULLPTR;
  const long long total = groups * (C / 4);
  if (total > 0x7fffffffll * 256) return SIMAMBA_E_SHAPE;
  grid = dim3(static_cast<unsigned>((total + 255) / 256));
  return SIMAMBA_OK;
}

}  // namespace simamba

using namespace simamba;

extern "C" int simamba_bn_relu_grid(long long rows) {
  return rows <= 0 ? 0 : static_cast<int>((rows + kBnChunk - 1) / kBnChunk);
}

extern "C" int simamba_bn_relu_fwd(const void* x, const float* gterm, int group, const float* weight,
                                   const float* bias, float* running_mean, float* running_var, float momentum,
                                   float eps, int training, void* y, float* mean, float* invstd, float* partial,
                                   long long rows, int C, long long ld, int io_dtype, void* stream) {
  if (const int rc = bn_check(io_dtype, rows, C, ld, group, gterm)) return entry_result(rc);
  if (!x || !y || !mean || !invstd) return SIMAMBA_E_NULLPTR;
  if (training && !partial) return SIMAMBA_E_NULLPTR;
  if (!training && (!running_mean || !running_var)) return SIMAMBA_E_NULLPTR;
  hipStream_t s = static_cast<hipStream_t>(stream);
  BnArgs a = bn_args(x, gterm, group, weight, bias, mean, invstd, rows, C, ld);
  a.y = y; a.partial = partial; a.training = training;
  if (training) launch_stats(a, io_dtype, s, {eps, momentum, mean, invstd, running_mean, running_var, nullptr, 0});
  else launch_eval_stats(a, s, running_mean, running_var, eps, mean, invstd);
  launch_apply(a, io_dtype, s);
  return static_cast<int>(hipGetLastError());
}

extern "C" int simamba_bn_relu_bwd(const void* dy, const void* x, const float* gterm, int group,
                                   const float* weight, const float* bias, const float* mean, const float* invstd,
                                   void* dx, float* dgterm, int dgroup, float* dweight, float* dbias, float* partial,
                                   long long rows, int C, long long ld, int io_dtype, int training, void* stream) {
  if (const int rc = bn_check(io_dtype, rows, C, ld, group, gterm)) return entry_result(rc);
  if (const int rc = bn_check_dgterm(dgterm, dgroup, rows, gterm,
                                     dy && x && mean && invstd && dx && dweight && dbias && partial))
    return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  BnArgs a = bn_args(x, gterm, group, weight, bias, mean, invstd, rows, C, ld);
  a.dy = dy; a.y = dx; a.dgterm = dgterm; a.partial = partial; a.dgroup = dgroup; a.training = training;
  launch_bwd_sums(a, io_dtype, s, dweight, dbias);
  launch_bwd_dx(a, io_dtype, s, dweight, dbias);
  return static_cast<int>(hipGetLastError());
}

// ---- staged entry points (cross-rank statistics): one pass each ------------------------------------------------------
extern "C" int simamba_bn_stats_local(const void* x, const float* gterm, int group, double* stats, long long stats_ld,
                                      float* partial, long long rows, int C, long long ld, int io_dtype,
                                      void* stream) {
  if (const int rc = bn_check(io_dtype, rows, C, ld, group, gterm)) return entry_result(rc);
  if (stats_ld == 0) stats_ld = C;
  if (stats_ld < C) return SIMAMBA_E_SHAPE;
  if (!x || !stats || !partial) return SIMAMBA_E_NULLPTR;
  BnArgs a = bn_args(x, gterm, group, nullptr, nullptr, nullptr, nullptr, rows, C, ld);
  a.partial = partial;
  launch_stats(a, io_dtype, static_cast<hipStream_t>(stream),
               {0.f, 0.f, nullptr, nullptr, nullptr, nullptr, stats, stats_ld});
  return static_cast<int>(hipGetLastError());
}

extern "C" int simamba_bn_stats_merge(const double* stats, int world, float* running_mean, float* running_var,
                                      float momentum, float eps, float* mean, float* invstd, double* count, int C,
                                      void* stream) {
  if (C == 0) return SIMAMBA_OK;
  if (world < 1 || C < 0) return SIMAMBA_E_SHAPE;
  if (!stats || !mean || !invstd || !count) return SIMAMBA_E_NULLPTR;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(bn_stats_merge_kernel, dim3((C + 127) / 128), dim3(128), 0, s, stats, world, C, eps, momentum,
                     mean, invstd, count, running_mean, running_var);
  return static_cast<int>(hipGetLastError());
}

extern "C" int simamba_bn_relu_apply(const void* x, const float* gterm, int group, const float* weight,
                                     const float* bias, const float* mean, const float* invstd, void* y,
                                     long long rows, int C, long long ld, int io_dtype, void* stream) {
  if (const int rc = bn_check(io_dtype, rows, C, ld, group, gterm)) return entry_result(rc);
  if (!x || !y || !mean || !invstd) return SIMAMBA_E_NULLPTR;
  BnArgs a = bn_args(x, gterm, group, weight, bias, mean, invstd, rows, C, ld);
  a.y = y;
  launch_apply(a, io_dtype, static_cast<hipStream_t>(stream));
  return static_cast<int>(hipGetLastError());
}

extern "C" int simamba_bn_relu_bwd_sums(const void* dy, const void* x, const float* gterm, int group,
                                        const float* weight, const float* bias, const float* mean,
                                        const float* invstd, float* dweight, float* dbias, float* partial,
                                        long long rows, int C, long long ld, int io_dtype, void* stream) {
  if (const int rc = bn_check(io_dtype, rows, C, ld, group, gterm)) return entry_result(rc);
  if (!dy || !x || !mean || !invstd || !dweight || !dbias || !partial) return SIMAMBA_E_NULLPTR;
  BnArgs a = bn_args(x, gterm, group, weight, bias, mean, invstd, rows, C, ld);
  a.dy = dy; a.partial = partial;
  launch_bwd_sums(a, io_dtype, static_cast<hipStream_t>(stream), dweight, dbias);
  return static_cast<int>(hipGetLastError());
}

extern "C" int simamba_bn_relu_bwd_dx(const void* dy, const void* x, const float* gterm, int group,
                                      const float* weight, const float* bias, const float* mean, const float* invstd,
                                      const float* sum_dweight, const float* sum_dbias, const double* count, void* dx,
                                      float* dgterm, int dgroup, long long rows, int C, long long ld, int io_dtype,
                                      void* stream) {
  if (const int rc = bn_check(io_dtype, rows, C, ld, group, gterm)) return entry_result(rc);
  if (const int rc = bn_check_dgterm(dgterm, dgroup, rows, gterm,
                                     dy && x && mean && invstd && dx && sum_dweight && sum_dbias && count))
    return rc;
  BnArgs a = bn_args(x, gterm, group, weight, bias, mean, invstd, rows, C, ld);
  a.dy = dy; a.y = dx; a.dgterm = dgterm; a.count = count; a.dgroup = dgroup;
  launch_bwd_dx(a, io_dtype, static_cast<hipStream_t>(stream), sum_dweight, sum_dbias);
  return static_cast<int>(hipGetLastError());
}

extern "C" int simamba_group_max_fwd(const void* x, void* out, unsigned char* idx, long long groups, int n, int C,
                                     int io_dtype, void* stream) {
  dim3 grid;
  if (const int rc = group_max_check(io_dtype, groups, n, C, x && out && idx, grid)) return entry_result(rc);
  with_io_type(io_dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(group_max_fwd_kernel<T>, grid, dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const T*>(x), static_cast<T*>(out), idx, groups, n, C);
  });
  return static_cast<int>(hipGetLastError());
}

extern "C" int simamba_group_max_bwd(const void* dout, const unsigned char* idx, void* dx, long long groups, int n,
                                     int C, int io_dtype, void* stream) {
  dim3 grid;
  if (const int rc = group_max_check(io_dtype, groups, n, C, dout && idx && dx, grid)) return entry_result(rc);
  with_io_type(io_dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(group_max_bwd_kernel<T>, grid, dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const T*>(dout), idx, static_cast<T*>(dx), groups, n, C);
  });
  return static_cast<int>(hipGetLastError());
}
