// Debiased Sinkhorn divergence between point sets of unequal size (1 <= n, m <= 8192 per set), with gradients for both
// sets: the entropic counterpart of emd.hip, on the tiling of chamfer_large.hip.  Per pair, with nx, ny valid points,
// uniform masses a = 1/nx, b = 1/ny and costs C_ij = (dx*dx + dy*dy) + dz*dz (this file is built with
// -ffp-contract=off):
//   diam2  = squared diagonal of the bounding box of the pair's nx + ny points, at least 1e-30
//   eps_t  = diam2 * 2^-t for t < S = ceil(log2(1 / eps_rel)), then `iters` steps at diam2 * eps_rel
//   a step = f_i <- -eps log sum_j b_j exp((g_j - C_ij) / eps), then g_j <- -eps log sum_i a_i exp((f_i - C_ij) / eps)
//   OT(x, y) = sum_i a_i f_i + sum_j b_j g_j ;  div = OT(x, y) - OT(x, x) / 2 - OT(y, y) / 2
// The three problems share the pair's diam2 and the schedule, and run in the same launches.
//
//   * sinkhorn_diam2_kernel: one workgroup per pair, O(n + m).
//   * sinkhorn_softmin_kernel: one half-step of all three problems.  A workgroup owns 64 rows of one problem of one
//     pair, one per lane and in registers, held by all four of its waves; it walks the other set in LDS tiles of kSkTile
//     points staged as (x, y, z, potential), every lane reading the same address (a broadcast).  The log-sum-exp is
//     online in base 2, eight columns at a time: t_c = (potential_c - C_c) k with k = 1 / (eps ln 2) formed once per
//     row (the difference first: it is small for the columns that carry the sum), the running maximum M and the sum s
//     rescaled once per eight columns: one v_exp_f32 per cost plus one per eight.  Wave w takes chunks w, w + 4, ... of
//     every tile and the four (M, s) are merged through LDS in wave order, so a row's bits depend on its columns alone,
//     and (1, 8192, 8192) still fills the chip: 384 workgroups per half-step.  A tile is padded to a multiple of eight
//     with columns of potential -inf, which add exactly 0.  The caller swaps the roles for the other half-step.  The
//     same kernel in its `mrow` form leaves |1 - exp((f_i - f_i+) / eps)| per row of (x, y), f+ one further update that
//     is not stored: the row-marginal error of the plan.
//   * sinkhorn_final_kernel: one workgroup per pair: the six potential sums and the marginal error, fp64 partial sums in
//     a fixed order (thread t takes elements t, t + 256, ...; then block_tree_sum) as in chamfer_large_reduce_kernel.
//   * sinkhorn_grad_kernel: the same walk with the potentials held fixed, accumulating sum w and sum w (x_i - y_j):
//       dx_i = ddiv a_i 2 ( sum_j pi_xy(j|i) (x_i - y_j) - sum_k pi_xx(k|i) (x_i - x_k) ),
//     pi_xy(j|i) = softmax_j((g_xy_j - C_ij) / eps_fin), pi_xx from g_xx; dy_j from f_xy and f_yy.  The two sums are the
//     same instructions on different operands, so with y == x (where g_xx is g_xy and f_yy is f_xy, bit for bit) both
//     gradients are exactly 0, as the value is.
// Ragged batches as in chamfer_large.hip: lengths are clamped on the device and read once per workgroup, nothing at or
// behind a length is loaded, rows behind a length are written as 0, and a row's result does not depend on the padded
// sizes or on the other pairs.  No atomics, no data-dependent trip count: the same bits every call, and a NaN
// coordinate makes its own pair NaN and nothing else.
#include <cmath>

#include "host_common.h"
#include "pointset.h"

namespace simamba {

constexpr int kSkWave = 64;          // rows per workgroup: one per lane
constexpr int kSkWaves = 4;          // waves per workgroup: each takes every fourth chunk of the columns
constexpr int kSkThreads = kSkWave * kSkWaves;
constexpr int kSkTile = 1024;        // columns per LDS tile: 16 KB
constexpr int kSkChunk = 8;          // columns per rescale of the running sum
constexpr int kSkMaxPoints = 8192;
constexpr int kSkMaxSteps = 4096;
constexpr int kSkDebias = 1;         // `flags`
constexpr float kSkLn2 = 0.6931471805599453f;

struct SkArgs {
  const float* x; const float* y;
  const int* xlen; const int* ylen;
  const float* diam2;                // (pairs)
  float* f_xy; float* g_xy;          // (pairs, n), (pairs, m)
  float* f_xx; float* g_xx;          // (pairs, n) both
  float* f_yy; float* g_yy;          // (pairs, m) both
  int n, m, bx, by, debias;
};

// A row's running log-sum-exp, and with the gradient the weighted sum of (row - column)
struct SkAcc { float M, s, ax, ay, az; };
struct SkLds {
  float4 tile[kSkTile];
  float part[5][kSkWaves][kSkWave];   // M, s, ax, ay, az of every wave's share of a row
};

__device__ __forceinline__ float sk_exp2(float v) { return __builtin_amdgcn_exp2f(v); }

// Stage columns [t0, t0 + cnt) of `set` with .w = pot[t] (0 without pot), and pad to a multiple of kSkChunk
__device__ __forceinline__ void sk_stage(float4* sT, const float* __restrict__ set, const float* __restrict__ pot,
                                         int t0, int cnt) {
  stage_points<kSkThreads>(sT, set, t0, cnt);
  for (int t = threadIdx.x; t < cnt; t += kSkThreads) sT[t].w = pot ? pot[t0 + t] : 0.f;
  const int padded = (cnt + kSkChunk - 1) / kSkChunk * kSkChunk;
  for (int t = cnt + threadIdx.x; t < padded; t += kSkThreads) sT[t] = make_float4(0.f, 0.f, 0.f, -INFINITY);
}

// The walk of nc columns for the row (px, py, pz) of this lane: M + log2(s) = log2 sum_j 2^((pot_j - C_ij) k), and with
// GRAD a = sum_j 2^((pot_j - C_ij) k - M) (row - col_j).  The four waves of the workgroup hold the same 64 rows; wave w
// takes chunks w, w + 4, ... of every tile, and the four partial sums are merged in wave order, so a row's bits depend
// on its columns alone.  Every thread of the workgroup must call it (barriers), and every thread gets the result.
template <bool GRAD>
__device__ __forceinline__ SkAcc sk_walk(SkLds& lds, const float* __restrict__ cols, const float* __restrict__ pot,
                                         int nc, float k, float px, float py, float pz) {
  const int wave = threadIdx.x / kSkWave, lane = threadIdx.x % kSkWave;
  SkAcc a{-INFINITY, 0.f, 0.f, 0.f, 0.f};
  for (int t0 = 0; t0 < nc; t0 += kSkTile) {
    const int cnt = min(kSkTile, nc - t0);
    __syncthreads();
    sk_stage(lds.tile, cols, pot, t0, cnt);
    __syncthreads();
    for (int j0 = wave * kSkChunk; j0 < cnt; j0 += kSkWaves * kSkChunk) {
      float t[kSkChunk], dx[kSkChunk], dy[kSkChunk], dz[kSkChunk];
#pragma unroll
      for (int u = 0; u < kSkChunk; ++u) {
        const float4 c = lds.tile[j0 + u];
        dx[u] = px - c.x; dy[u] = py - c.y; dz[u] = pz - c.z;
        const float cost = (dx[u] * dx[u] + dy[u] * dy[u]) + dz[u] * dz[u];
        t[u] = (c.w - cost) * k;                                  // the difference first: it is small where it counts
      }
      float cm = t[0];
#pragma unroll
      for (int u = 1; u < kSkChunk; ++u) cm = fmaxf(cm, t[u]);
      const float Mn = fmaxf(a.M, cm);
      const float r = sk_exp2(a.M - Mn);
      float e[kSkChunk];
#pragma unroll
      for (int u = 0; u < kSkChunk; ++u) e[u] = sk_exp2(t[u] - Mn);
      float se = e[0];
#pragma unroll
      for (int u = 1; u < kSkChunk; ++u) se += e[u];
      a.s = __builtin_fmaf(a.s, r, se);
      a.M = Mn;
      if constexpr (GRAD) {
        float gx = e[0] * dx[0], gy = e[0] * dy[0], gz = e[0] * dz[0];
#pragma unroll
        for (int u = 1; u < kSkChunk; ++u) {
          gx = __builtin_fmaf(e[u], dx[u], gx); gy = __builtin_fmaf(e[u], dy[u], gy);
          gz = __builtin_fmaf(e[u], dz[u], gz);
        }
        a.ax = __builtin_fmaf(a.ax, r, gx); a.ay = __builtin_fmaf(a.ay, r, gy); a.az = __builtin_fmaf(a.az, r, gz);
      }
    }
  }
  // merge: wave 0 always holds a real column (chunk 0 of tile 0), so the maximum is finite for finite inputs, and a
  // wave that saw no chunk (M = -inf, s = 0) adds 0 * 2^-inf = 0
  lds.part[0][wave][lane] = a.M; lds.part[1][wave][lane] = a.s;
  if constexpr (GRAD) { lds.part[2][wave][lane] = a.ax; lds.part[3][wave][lane] = a.ay; lds.part[4][wave][lane] = a.az; }
  __syncthreads();
  float M = lds.part[0][0][lane];
#pragma unroll
  for (int w = 1; w < kSkWaves; ++w) M = fmaxf(M, lds.part[0][w][lane]);
  SkAcc o{M, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int w = 0; w < kSkWaves; ++w) {
    const float r = sk_exp2(lds.part[0][w][lane] - M);
    o.s = __builtin_fmaf(lds.part[1][w][lane], r, o.s);
    if constexpr (GRAD) {
      o.ax = __builtin_fmaf(lds.part[2][w][lane], r, o.ax); o.ay = __builtin_fmaf(lds.part[3][w][lane], r, o.ay);
      o.az = __builtin_fmaf(lds.part[4][w][lane], r, o.az);
    }
  }
  return o;
}

__global__ __launch_bounds__(kSkThreads) void sinkhorn_diam2_kernel(const float* __restrict__ x,
                                                                    const float* __restrict__ y,
                                                                    const int* __restrict__ xlen,
                                                                    const int* __restrict__ ylen,
                                                                    float* __restrict__ diam2, int n, int m) {
  __shared__ float sLo[3][kSkThreads], sHi[3][kSkThreads];
  const long long pr = blockIdx.x;
  const int nx = clamped_length(xlen, pr, n), ny = clamped_length(ylen, pr, m);
  const float* xs = x + pr * n * 3;
  const float* ys = y + pr * m * 3;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int i = threadIdx.x; i < nx + ny; i += kSkThreads) {
    const float* p = i < nx ? xs + 3 * i : ys + 3 * (i - nx);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = p[c];
      // a NaN coordinate must reach diam2: fminf / fmaxf would drop it
      lo[c] = (v < lo[c] || v != v) ? v : lo[c];
      hi[c] = (v > hi[c] || v != v) ? v : hi[c];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) { sLo[c][threadIdx.x] = lo[c]; sHi[c][threadIdx.x] = hi[c]; }
  __syncthreads();
  for (int w = kSkThreads / 2; w >= 1; w >>= 1) {
    if (threadIdx.x < w) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float a = sLo[c][threadIdx.x], b = sLo[c][threadIdx.x + w];
        sLo[c][threadIdx.x] = (b < a || b != b) ? b : a;
        const float d = sHi[c][threadIdx.x], e = sHi[c][threadIdx.x + w];
        sHi[c][threadIdx.x] = (e > d || e != e) ? e : d;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float ex = sHi[0][0] - sLo[0][0], ey = sHi[1][0] - sLo[1][0], ez = sHi[2][0] - sLo[2][0];
    const float d2 = (ex * ex + ey * ey) + ez * ez;
    diam2[pr] = d2 < 1e-30f ? 1e-30f : d2;                         // NaN stays NaN
  }
}

// half 0: the f half-step (rows of the first set against the second), half 1: the g half-step.  Blocks of a pair:
// [0, job0) the (x, y) problem, then bx blocks of (x, x) and by blocks of (y, y) with debias.  `first`: g is 0 and is
// not read.  mrow != NULL: only the f half-step of (x, y), nothing stored but mrow.
__global__ __launch_bounds__(kSkThreads) void sinkhorn_softmin_kernel(SkArgs a, int half, int first, float eps_scale,
                                                                      float* __restrict__ mrow) {
  __shared__ SkLds lds;
  const int job0 = half == 0 ? a.bx : a.by;
  const int per = job0 + ((a.debias && !mrow) ? a.bx + a.by : 0);
  const long long pr = blockIdx.x / per;
  int r = static_cast<int>(blockIdx.x - pr * per);
  const int job = r < job0 ? 0 : (r < job0 + a.bx ? 1 : 2);      // workgroup-uniform
  r -= job == 0 ? 0 : (job == 1 ? job0 : job0 + a.bx);
  const int nx = clamped_length(a.xlen, pr, a.n), ny = clamped_length(a.ylen, pr, a.m);
  const bool rows_x = job == 1 || (job == 0 && half == 0);
  const bool cols_x = job == 1 || (job == 0 && half == 1);
  const int nrp = rows_x ? a.n : a.m, ncp = cols_x ? a.n : a.m;   // padded sizes: the strides
  const int nr = rows_x ? nx : ny, nc = cols_x ? nx : ny;
  const float* rows = (rows_x ? a.x : a.y) + pr * nrp * 3;
  const float* cols = (cols_x ? a.x : a.y) + pr * ncp * 3;
  const float* fpot = job == 0 ? a.f_xy : (job == 1 ? a.f_xx : a.f_yy);
  float* gpot = job == 0 ? a.g_xy : (job == 1 ? a.g_xx : a.g_yy);
  float* fout = job == 0 ? a.f_xy : (job == 1 ? a.f_xx : a.f_yy);
  const float* pot = first ? nullptr : (half == 0 ? gpot : fpot) + pr * ncp;
  float* out = (mrow ? mrow : (half == 0 ? fout : gpot)) + pr * nrp;
  const bool writer = threadIdx.x < kSkWave;                      // the four waves hold the same rows: wave 0 stores
  const int i = r * kSkWave + static_cast<int>(threadIdx.x % kSkWave);
  if (r * kSkWave >= nr) {                                        // all padding: zeros, and out before any barrier
    if (writer && i < nrp) out[i] = 0.f;
    return;
  }
  const float eps = a.diam2[pr] * eps_scale;
  const float k = 1.f / (eps * kSkLn2);
  const int ic = min(i, nr - 1);                                  // lanes past the end repeat the last row
  const SkAcc acc = sk_walk<false>(lds, cols, pot, nc, k, rows[3 * ic], rows[3 * ic + 1], rows[3 * ic + 2]);
  if (!writer) return;
  const float lnc = logf(static_cast<float>(nc));                 // the uniform mass 1 / nc, taken out of the sum
  const float v = eps * (lnc - kSkLn2 * (acc.M + __builtin_amdgcn_logf(acc.s)));
  if (i < nr) out[i] = mrow ? fabsf(1.f - sk_exp2((fout[pr * nrp + i] - v) * k)) : v;
  else if (i < nrp) out[i] = 0.f;
}

__global__ __launch_bounds__(kSkThreads) void sinkhorn_final_kernel(SkArgs a, const float* __restrict__ mrow,
                                                                    float* __restrict__ div,
                                                                    float* __restrict__ ot_xy,
                                                                    float* __restrict__ merr) {
  __shared__ double sS[7][kSkThreads];
  const long long pr = blockIdx.x;
  const int nx = clamped_length(a.xlen, pr, a.n), ny = clamped_length(a.ylen, pr, a.m);
  const float* vx[4] = {a.f_xy + pr * a.n, a.debias ? a.f_xx + pr * a.n : nullptr,
                        a.debias ? a.g_xx + pr * a.n : nullptr, mrow ? mrow + pr * a.n : nullptr};
  const float* vy[3] = {a.g_xy + pr * a.m, a.debias ? a.f_yy + pr * a.m : nullptr,
                        a.debias ? a.g_yy + pr * a.m : nullptr};
  double t[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int v = 0; v < 4; ++v)
    if (vx[v])
      for (int i = threadIdx.x; i < nx; i += kSkThreads) t[v] += static_cast<double>(vx[v][i]);
#pragma unroll
  for (int v = 0; v < 3; ++v)
    if (vy[v])
      for (int j = threadIdx.x; j < ny; j += kSkThreads) t[4 + v] += static_cast<double>(vy[v][j]);
#pragma unroll
  for (int v = 0; v < 7; ++v) sS[v][threadIdx.x] = t[v];
  block_tree_sum(sS);
  if (threadIdx.x == 0) {
    // x sums: 0 f_xy, 1 f_xx, 2 g_xx, 3 mrow ; y sums: 4 g_xy, 5 f_yy, 6 g_yy
    const double xy = sS[0][0] / nx + sS[4][0] / ny;
    ot_xy[pr] = static_cast<float>(xy);
    if (a.debias) {
      const double xx = sS[1][0] / nx + sS[2][0] / nx, yy = sS[5][0] / ny + sS[6][0] / ny;
      div[pr] = static_cast<float>(xy - 0.5 * xx - 0.5 * yy);
    } else {
      div[pr] = static_cast<float>(xy);
    }
    if (merr) merr[pr] = static_cast<float>(sS[3][0] / nx);
  }
}

// Blocks [0, bx) of a pair write dx, blocks [bx, bx + by) dy; bx or by is 0 when that gradient is not wanted.
__global__ __launch_bounds__(kSkThreads) void sinkhorn_grad_kernel(SkArgs a, const float* __restrict__ ddiv,
                                                                   float* __restrict__ dx, float* __restrict__ dy,
                                                                   float eps_scale) {
  __shared__ SkLds lds;
  const long long pr = blockIdx.x / (a.bx + a.by);
  const int r = static_cast<int>(blockIdx.x - pr * (a.bx + a.by));
  const bool forx = r < a.bx;
  const int nx = clamped_length(a.xlen, pr, a.n), ny = clamped_length(a.ylen, pr, a.m);
  const int nsp = forx ? a.n : a.m, nop = forx ? a.m : a.n;
  const int ns = forx ? nx : ny, no = forx ? ny : nx;
  const float* self = (forx ? a.x : a.y) + pr * nsp * 3;
  const float* other = (forx ? a.y : a.x) + pr * nop * 3;
  const float* pot_other = (forx ? a.g_xy : a.f_xy) + pr * nop;   // the (x, y) potential that lives on the other set
  const float* pot_self = a.debias ? (forx ? a.g_xx : a.f_yy) + pr * nsp : nullptr;
  float* out = (forx ? dx : dy) + pr * nsp * 3;
  const int r0 = (forx ? r : r - a.bx) * kSkWave;
  const bool writer = threadIdx.x < kSkWave;
  const int i = r0 + static_cast<int>(threadIdx.x % kSkWave);
  if (r0 >= ns) {
    if (writer && i < nsp) { out[3 * i] = 0.f; out[3 * i + 1] = 0.f; out[3 * i + 2] = 0.f; }
    return;
  }
  const float eps = a.diam2[pr] * eps_scale;
  const float k = 1.f / (eps * kSkLn2);
  const float coef = 2.f * ddiv[pr] / static_cast<float>(ns);
  const int ic = min(i, ns - 1);
  const float px = self[3 * ic], py = self[3 * ic + 1], pz = self[3 * ic + 2];
  const SkAcc to = sk_walk<true>(lds, other, pot_other, no, k, px, py, pz);
  float gx = to.ax / to.s, gy = to.ay / to.s, gz = to.az / to.s;
  if (pot_self) {
    const SkAcc ts = sk_walk<true>(lds, self, pot_self, ns, k, px, py, pz);
    gx -= ts.ax / ts.s; gy -= ts.ay / ts.s; gz -= ts.az / ts.s;
  }
  if (!writer) return;
  if (i < ns) { out[3 * i] = coef * gx; out[3 * i + 1] = coef * gy; out[3 * i + 2] = coef * gz; }
  else if (i < nsp) { out[3 * i] = 0.f; out[3 * i + 1] = 0.f; out[3 * i + 2] = 0.f; }
}

// S = ceil(log2(1 / eps_rel)) for 0 < eps_rel <= 1: the first S with 2^-S <= eps_rel (at most 149 for a float)
inline int sk_scaling_steps(float eps_rel) {
  int s = 0;
  while (std::ldexp(1.0, -s) > static_cast<double>(eps_rel)) ++s;
  return s;
}

inline int sk_check(long long pairs, int n, int m, float eps_rel, int flags) {
  if (flags & ~kSkDebias) return SIMAMBA_E_VARIANT;
  if (pairs < 1 || n < 1 || m < 1 || n > kSkMaxPoints || m > kSkMaxPoints) return SIMAMBA_E_SHAPE;
  if (!(eps_rel > 0.f && eps_rel <= 1.f)) return SIMAMBA_E_SHAPE;
  // the largest grid of either call: every problem's blocks
  const long long bx = (n + kSkWave - 1) / kSkWave, by = (m + kSkWave - 1) / kSkWave;
  if (pairs > 0x7fffffffll / (2 * (bx + by))) return SIMAMBA_E_SHAPE;
  return SIMAMBA_OK;
}

inline size_t sk_workspace_floats(long long pairs, int n, int debias) {
  return static_cast<size_t>(pairs) * (1 + static_cast<size_t>(n) * (debias ? 2 : 1));
}

}  // namespace simamba

using namespace simamba;

extern "C" size_t simamba_sinkhorn_workspace_bytes(long long pairs, int n, int m, int flags) {
  if (sk_check(pairs, n, m, 1.f, flags)) return 0;
  return sizeof(float) * sk_workspace_floats(pairs, n, flags & kSkDebias);
}

extern "C" int simamba_sinkhorn_fwd(const float* x, const float* y, const int* xlen, const int* ylen, float* div,
                                    float* ot_xy, float* merr, float* f_xy, float* g_xy, float* g_xx, float* g_yy,
                                    float* f_yy, long long pairs, int n, int m, float eps_rel, int iters, int flags,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  if (const int rc = sk_check(pairs, n, m, eps_rel, flags)) return rc;
  if (iters < 0) return SIMAMBA_E_SHAPE;
  const int S = sk_scaling_steps(eps_rel);
  if (iters > kSkMaxSteps || S + iters < 1 || S + iters > kSkMaxSteps) return SIMAMBA_E_SHAPE;
  const int debias = flags & kSkDebias;
  if (!x || !y || !div || !ot_xy || !f_xy || !g_xy || (debias && (!g_xx || !g_yy || !f_yy))) return SIMAMBA_E_NULLPTR;
  if (!workspace || workspace_bytes < simamba_sinkhorn_workspace_bytes(pairs, n, m, flags)) return SIMAMBA_E_WORKSPACE;
  if (!aligned16(workspace)) return SIMAMBA_E_ALIGN;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  // workspace: diam2 (pairs), the per-row marginal errors (pairs, n), f_xx (pairs, n)
  float* ws = static_cast<float*>(workspace);
  float* diam2 = ws;
  float* mrow = ws + pairs;
  float* f_xx = debias ? mrow + pairs * n : nullptr;
  const int bx = (n + kSkWave - 1) / kSkWave, by = (m + kSkWave - 1) / kSkWave;
  const SkArgs a{x, y, xlen, ylen, diam2, f_xy, g_xy, f_xx, g_xx, f_yy, g_yy, n, m, bx, by, debias};
  const dim3 b(kSkThreads);
  hipLaunchKernelGGL(sinkhorn_diam2_kernel, dim3(static_cast<unsigned>(pairs)), b, 0, st, x, y, xlen, ylen, diam2, n, m);
  if (const hipError_t e = hipGetLastError()) return static_cast<int>(e);
  const long long both = debias ? bx + by : 0;
  const dim3 gf(static_cast<unsigned>(pairs * (bx + both))), gg(static_cast<unsigned>(pairs * (by + both)));
  hipError_t err = hipSuccess;
  for (int t = 0; t < S + iters && err == hipSuccess; ++t) {
    const float scale = t < S ? static_cast<float>(std::ldexp(1.0, -t)) : eps_rel;
    hipLaunchKernelGGL(sinkhorn_softmin_kernel, gf, b, 0, st, a, 0, t == 0 ? 1 : 0, scale, nullptr);
    hipLaunchKernelGGL(sinkhorn_softmin_kernel, gg, b, 0, st, a, 1, 0, scale, nullptr);
    err = hipGetLastError();
  }
  if (merr && err == hipSuccess) {
    hipLaunchKernelGGL(sinkhorn_softmin_kernel, dim3(static_cast<unsigned>(pairs * bx)), b, 0, st, a, 0, 0, eps_rel,
                       mrow);
    err = hipGetLastError();
  }
  if (err) return static_cast<int>(err);
  hipLaunchKernelGGL(sinkhorn_final_kernel, dim3(static_cast<unsigned>(pairs)), b, 0, st, a, merr ? mrow : nullptr, div,
                     ot_xy, merr);
  return static_cast<int>(hipGetLastError());
}

extern "C" int simamba_sinkhorn_bwd(const float* x, const float* y, const int* xlen, const int* ylen,
                                    const float* ddiv, const float* f_xy, const float* g_xy, const float* g_xx,
                                    const float* f_yy, float* dx, float* dy, long long pairs, int n, int m,
                                    float eps_rel, int flags, void* workspace, size_t workspace_bytes, void* stream) {
  if (const int rc = sk_check(pairs, n, m, eps_rel, flags)) return rc;
  const int debias = flags & kSkDebias;
  if (!x || !y || !ddiv || (dx && (!g_xy || (debias && !g_xx))) || (dy && (!f_xy || (debias && !f_yy))))
    return SIMAMBA_E_NULLPTR;
  if (!workspace || workspace_bytes < sizeof(float) * static_cast<size_t>(pairs)) return SIMAMBA_E_WORKSPACE;
  if (!aligned16(workspace)) return SIMAMBA_E_ALIGN;
  if (!dx && !dy) return SIMAMBA_OK;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  float* diam2 = static_cast<float*>(workspace);
  const int bx = dx ? (n + kSkWave - 1) / kSkWave : 0, by = dy ? (m + kSkWave - 1) / kSkWave : 0;
  const SkArgs a{x, y, xlen, ylen, diam2, const_cast<float*>(f_xy), const_cast<float*>(g_xy), nullptr,
                 const_cast<float*>(g_xx), const_cast<float*>(f_yy), nullptr, n, m, bx, by, debias};
  const dim3 b(kSkThreads);
  hipLaunchKernelGGL(sinkhorn_diam2_kernel, dim3(static_cast<unsigned>(pairs)), b, 0, st, x, y, xlen, ylen, diam2, n, m);
  if (const hipError_t e = hipGetLastError()) return static_cast<int>(e);
  hipLaunchKernelGGL(sinkhorn_grad_kernel, dim3(static_cast<unsigned>(pairs * (bx + by))), b, 0, st, a, ddiv, dx, dy,
                     eps_rel);
  return static_cast<int>(hipGetLastError());
}
