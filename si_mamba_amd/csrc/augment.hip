// Point-cloud sampling and augmentation in front of a training step (the reference's tools/runner_finetune.py:191-194
// and datasets/data_transforms.py, without their per-cloud Python loops, host draws and host-to-device copies):
//   out[b][i] = chain(points[b][idx[b][sel[i]]])
// in one launch, the chain being up to 8 of rotate / scale / translate / scale-and-translate / jitter / dropout / flip.
//
// One workgroup per cloud, the cloud in registers: lane t of T holds rows t, t + T, ... (at most 8 at T = 1024, so a
// cloud has at most 8192 rows, the limit of the other point kernels here).  The chain runs in order on the registers;
// the workgroup meets only where a transform asks for the whole cloud: flip's per-axis maximum (wave shuffles, then one
// LDS row per axis) and dropout's current row 0 (lane 0 holds it).  The work is a few microseconds of latency per batch
// and nothing here is tuned beyond that: plain C++, every lane redoes the per-cloud draws instead of sharing them.
//
// Random numbers are counter based (Philox4x32-10, philox.h), so nothing is read on the host, the call can sit in a
// captured graph, and a value depends only on (seed, step, cloud, row, position in the chain); the counter layout is
// part of the contract and stated in include/simamba.h.  `step` lives on the device and a one-lane kernel adds 1 to it
// behind every launch, in stream order.
//
// Rounding: built with -ffp-contract=off, and every product and sum a draw or a transform consists of is spelled
// __fmul_rn / __fadd_rn, so each is one correctly rounded fp32 operation and a numpy float32 restatement reproduces the
// drawn parameters and the keep / flip decisions bit for bit.  cos / sin / log are the device library's.
#include "host_common.h"
#include "philox_draws.h"
#include "pointset.h"

namespace simamba {

constexpr int kAugMaxOps = SIMAMBA_AUG_MAX_OPS;
constexpr int kAugMaxPoints = 8192;
constexpr int kAugMaxThreads = 1024;
constexpr int kAugPerLane = kAugMaxPoints / kAugMaxThreads;
constexpr int kAugMaxWaves = kAugMaxThreads / 64;
constexpr int kAugDraws = SIMAMBA_AUG_CLOUD_PARAMS;      // floats emitted per (cloud, op)
constexpr float kAugTwoPi = 6.2831854820251465f;         // fp32(2 pi)

struct AugChain {                                        // by value in the kernel arguments
  int n;
  int op[kAugMaxOps];
  float p[kAugMaxOps][4];
};

struct AugRng {
  uint32_t k0, k1, cloud, step_lo, step_hi;
};

__device__ __forceinline__ AugRng aug_rng(const long long* __restrict__ state, unsigned cloud) {
  const unsigned long long seed = static_cast<unsigned long long>(state[0]);
  const unsigned long long step = static_cast<unsigned long long>(state[1]);
  return AugRng{static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), cloud, static_cast<uint32_t>(step),
                static_cast<uint32_t>(step >> 32)};
}

// the Philox block `index` of stream (cloud, step, chain position, per-cloud | per-point): the layout of simamba.h
__device__ __forceinline__ Philox4 aug_block(const AugRng& r, int pos, bool per_point, uint32_t index) {
  const uint32_t c3 = (r.step_hi & 0x0FFFFFFFu) | (static_cast<uint32_t>(pos) << 28) | (per_point ? 0x80000000u : 0u);
  return philox4x32_10(r.k0, r.k1, index, r.cloud, r.step_lo, c3);
}

// aug_uniform and the Box-Muller normals: philox_draws.h, shared with corrupt.hip
__device__ __forceinline__ void aug_point_normals(const AugRng& r, int pos, int i, float& n0, float& n1, float& n2) {
  aug_block_normals(aug_block(r, pos, true, static_cast<uint32_t>(i)), n0, n1, n2);
}

__device__ __forceinline__ float aug_point_uniform(const AugRng& r, int pos, int i) {
  return aug_uniform(aug_block(r, pos, true, static_cast<uint32_t>(i)).w[0]);
}

// What an op draws once per cloud, in the order simamba_augment_params writes it (simamba.h); unused slots are 0.
struct AugDraw {
  float v[kAugDraws];
};

__device__ __forceinline__ AugDraw aug_draw_cloud(const AugRng& r, int pos, int op, const float* __restrict__ p) {
  AugDraw d;
#pragma unroll
  for (int k = 0; k < kAugDraws; ++k) d.v[k] = 0.f;
  const Philox4 q = aug_block(r, pos, false, 0u);
  const float u0 = aug_uniform(q.w[0]), u1 = aug_uniform(q.w[1]), u2 = aug_uniform(q.w[2]);
  switch (op) {
    case SIMAMBA_AUG_ROTATE: {
      d.v[0] = __fmul_rn(u0, kAugTwoPi);
      sincosf(d.v[0], &d.v[2], &d.v[1]);
      break;
    }
    case SIMAMBA_AUG_SCALE:
    case SIMAMBA_AUG_SCALE_TRANSLATE: {
      const float lo = p[0], range = __fsub_rn(p[1], p[0]);
      d.v[0] = __fadd_rn(lo, __fmul_rn(u0, range));
      d.v[1] = __fadd_rn(lo, __fmul_rn(u1, range));
      d.v[2] = __fadd_rn(lo, __fmul_rn(u2, range));
      if (op == SIMAMBA_AUG_SCALE_TRANSLATE) {
        const Philox4 q1 = aug_block(r, pos, false, 1u);
        const float tr = p[2], span = __fmul_rn(2.f, tr);
        d.v[3] = __fadd_rn(-tr, __fmul_rn(aug_uniform(q1.w[0]), span));
        d.v[4] = __fadd_rn(-tr, __fmul_rn(aug_uniform(q1.w[1]), span));
        d.v[5] = __fadd_rn(-tr, __fmul_rn(aug_uniform(q1.w[2]), span));
      }
      break;
    }
    case SIMAMBA_AUG_TRANSLATE: {
      const float tr = p[0], span = __fmul_rn(2.f, tr);
      d.v[0] = __fadd_rn(-tr, __fmul_rn(u0, span));
      d.v[1] = __fadd_rn(-tr, __fmul_rn(u1, span));
      d.v[2] = __fadd_rn(-tr, __fmul_rn(u2, span));
      break;
    }
    case SIMAMBA_AUG_JITTER: {
      d.v[0] = p[0];
      d.v[1] = p[1];
      break;
    }
    case SIMAMBA_AUG_DROPOUT: {
      d.v[0] = __fmul_rn(u0, p[0]);
      break;
    }
    case SIMAMBA_AUG_FLIP: {
      const int up = static_cast<int>(p[0]);                         // 0, 1 or 2: checked on the host
      const bool gate = u0 < 0.95f;
      const float ua[2] = {u1, u2};                                  // the horizontal axes in ascending order
      int h = 0;
      d.v[0] = gate ? 1.f : 0.f;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        if (a == up) continue;
        d.v[1 + a] = (gate && ua[h] < 0.5f) ? 1.f : 0.f;
        ++h;
      }
      break;
    }
    default: break;
  }
  return d;
}

template <typename IdxT>
__global__ __launch_bounds__(kAugMaxThreads) void augment_points_kernel(
    const float* points, const IdxT* __restrict__ idx, const long long* __restrict__ sel,
    const long long* __restrict__ lengths, float* out, const AugChain chain, const long long* __restrict__ state,
    int N, int M, int K) {
  __shared__ float sMax[3][kAugMaxWaves];
  __shared__ float sFirst[3];
  const long long b = blockIdx.x;
  const int T = blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = T >> 6;
  const int len = clamped_length(lengths, b, K);
  const AugRng rng = aug_rng(state, blockIdx.x);

  // rows >= len stay 0 and are never looked up; every index is forced into its range before it is used
  float x[kAugPerLane], y[kAugPerLane], z[kAugPerLane];
#pragma unroll
  for (int j = 0; j < kAugPerLane; ++j) {
    const int i = tid + j * T;
    x[j] = y[j] = z[j] = 0.f;
    if (i < len) {
      long long s = sel ? sel[i] : i;
      s = s < 0 ? 0 : (s > M - 1 ? M - 1 : s);
      long long row = idx ? static_cast<long long>(idx[b * M + s]) : s;
      row = row < 0 ? 0 : (row > N - 1 ? N - 1 : row);
      const float* p = points + (b * N + row) * 3;
      x[j] = p[0];
      y[j] = p[1];
      z[j] = p[2];
    }
  }

  for (int o = 0; o < chain.n; ++o) {
    const int op = chain.op[o];
    const AugDraw d = aug_draw_cloud(rng, o, op, chain.p[o]);
    switch (op) {                                                    // uniform over the workgroup
      case SIMAMBA_AUG_ROTATE: {
        const float c = d.v[1], s = d.v[2];
#pragma unroll
        for (int j = 0; j < kAugPerLane; ++j) {
          const float nx = __fsub_rn(__fmul_rn(x[j], c), __fmul_rn(z[j], s));
          const float nz = __fadd_rn(__fmul_rn(x[j], s), __fmul_rn(z[j], c));
          x[j] = nx;
          z[j] = nz;
        }
        break;
      }
      case SIMAMBA_AUG_SCALE: {
#pragma unroll
        for (int j = 0; j < kAugPerLane; ++j) {
          x[j] = __fmul_rn(x[j], d.v[0]);
          y[j] = __fmul_rn(y[j], d.v[1]);
          z[j] = __fmul_rn(z[j], d.v[2]);
        }
        break;
      }
      case SIMAMBA_AUG_TRANSLATE: {
#pragma unroll
        for (int j = 0; j < kAugPerLane; ++j) {
          x[j] = __fadd_rn(x[j], d.v[0]);
          y[j] = __fadd_rn(y[j], d.v[1]);
          z[j] = __fadd_rn(z[j], d.v[2]);
        }
        break;
      }
      case SIMAMBA_AUG_SCALE_TRANSLATE: {
#pragma unroll
        for (int j = 0; j < kAugPerLane; ++j) {
          x[j] = __fadd_rn(__fmul_rn(x[j], d.v[0]), d.v[3]);
          y[j] = __fadd_rn(__fmul_rn(y[j], d.v[1]), d.v[4]);
          z[j] = __fadd_rn(__fmul_rn(z[j], d.v[2]), d.v[5]);
        }
        break;
      }
      case SIMAMBA_AUG_JITTER: {
        const float sd = d.v[0], clip = d.v[1];
#pragma unroll
        for (int j = 0; j < kAugPerLane; ++j) {
          const int i = tid + j * T;
          if (i < len) {
            float n0, n1, n2;
            aug_point_normals(rng, o, i, n0, n1, n2);
            x[j] = __fadd_rn(x[j], fminf(fmaxf(__fmul_rn(sd, n0), -clip), clip));
            y[j] = __fadd_rn(y[j], fminf(fmaxf(__fmul_rn(sd, n1), -clip), clip));
            z[j] = __fadd_rn(z[j], fminf(fmaxf(__fmul_rn(sd, n2), -clip), clip));
          }
        }
        break;
      }
      case SIMAMBA_AUG_DROPOUT: {
        if (tid == 0) {                                              // row 0 is lane 0's first row; len >= 1
          sFirst[0] = x[0];
          sFirst[1] = y[0];
          sFirst[2] = z[0];
        }
        __syncthreads();
        const float fx = sFirst[0], fy = sFirst[1], fz = sFirst[2], ratio = d.v[0];
#pragma unroll
        for (int j = 0; j < kAugPerLane; ++j) {
          const int i = tid + j * T;
          if (i < len && aug_point_uniform(rng, o, i) <= ratio) {
            x[j] = fx;
            y[j] = fy;
            z[j] = fz;
          }
        }
        __syncthreads();                                             // sFirst may be written again by a later op
        break;
      }
      case SIMAMBA_AUG_FLIP: {
        const bool bx = d.v[1] != 0.f, by = d.v[2] != 0.f, bz = d.v[3] != 0.f;
        if (!(bx || by || bz)) break;
        float mx = -INFINITY, my = -INFINITY, mz = -INFINITY;        // over the rows < len; a NaN is passed over
#pragma unroll
        for (int j = 0; j < kAugPerLane; ++j) {
          if (tid + j * T < len) {
            mx = fmaxf(mx, x[j]);
            my = fmaxf(my, y[j]);
            mz = fmaxf(mz, z[j]);
          }
        }
        mx = wave_xor_max(mx);
        my = wave_xor_max(my);
        mz = wave_xor_max(mz);
        if (lane == 0) {
          sMax[0][wave] = mx;
          sMax[1][wave] = my;
          sMax[2][wave] = mz;
        }
        __syncthreads();
        mx = sMax[0][0];
        my = sMax[1][0];
        mz = sMax[2][0];
        for (int w = 1; w < waves; ++w) {
          mx = fmaxf(mx, sMax[0][w]);
          my = fmaxf(my, sMax[1][w]);
          mz = fmaxf(mz, sMax[2][w]);
        }
        __syncthreads();                                             // sMax may be written again by a later flip
#pragma unroll
        for (int j = 0; j < kAugPerLane; ++j) {
          if (bx) x[j] = __fsub_rn(mx, x[j]);
          if (by) y[j] = __fsub_rn(my, y[j]);
          if (bz) z[j] = __fsub_rn(mz, z[j]);
        }
        break;
      }
      default: break;
    }
  }

#pragma unroll
  for (int j = 0; j < kAugPerLane; ++j) {
    const int i = tid + j * T;
    if (i < K) {
      float* q = out + (b * K + i) * 3;
      const bool valid = i < len;
      q[0] = valid ? x[j] : 0.f;
      q[1] = valid ? y[j] : 0.f;
      q[2] = valid ? z[j] : 0.f;
    }
  }
}

__global__ void augment_step_kernel(long long* state) {
  state[1] = static_cast<long long>(static_cast<unsigned long long>(state[1]) + 1ull);
}

// the values augment_points_kernel draws for the same chain and state, and no points
__global__ __launch_bounds__(kAugMaxThreads) void augment_params_kernel(
    const long long* __restrict__ lengths, const AugChain chain, const long long* __restrict__ state,
    float* __restrict__ cloud_params, float* __restrict__ noise, unsigned char* __restrict__ keep, int K) {
  const long long b = blockIdx.x;
  const int T = blockDim.x, tid = threadIdx.x;
  const int len = clamped_length(lengths, b, K);
  const AugRng rng = aug_rng(state, blockIdx.x);
  int jitter_at = -1, dropout_at = -1;                               // the chain's first of each
  float ratio = 0.f;
  for (int o = 0; o < chain.n; ++o) {
    const int op = chain.op[o];
    const AugDraw d = aug_draw_cloud(rng, o, op, chain.p[o]);
    if (tid == 0) {
#pragma unroll
      for (int k = 0; k < kAugDraws; ++k) cloud_params[(b * chain.n + o) * kAugDraws + k] = d.v[k];
    }
    if (op == SIMAMBA_AUG_JITTER && jitter_at < 0) jitter_at = o;
    if (op == SIMAMBA_AUG_DROPOUT && dropout_at < 0) {
      dropout_at = o;
      ratio = d.v[0];
    }
  }
  for (int i = tid; i < K; i += T) {
    if (noise) {
      float n0 = 0.f, n1 = 0.f, n2 = 0.f;
      if (i < len && jitter_at >= 0) aug_point_normals(rng, jitter_at, i, n0, n1, n2);
      float* q = noise + (b * K + i) * 3;
      q[0] = n0;
      q[1] = n1;
      q[2] = n2;
    }
    if (keep) {
      bool kept = i < len;
      if (kept && dropout_at >= 0) kept = !(aug_point_uniform(rng, dropout_at, i) <= ratio);
      keep[b * K + i] = kept ? 1 : 0;
    }
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------
static int aug_check_chain(const int* ops, const float* op_params, int n_ops, AugChain& chain) {
  chain.n = n_ops;
  for (int o = 0; o < kAugMaxOps; ++o) {
    chain.op[o] = 0;
    for (int k = 0; k < 4; ++k) chain.p[o][k] = 0.f;
  }
  for (int o = 0; o < n_ops; ++o) {
    const int op = ops[o];
    if (op < SIMAMBA_AUG_ROTATE || op > SIMAMBA_AUG_FLIP) return SIMAMBA_E_VARIANT;
    const float* p = op_params + 4 * o;
    if (op == SIMAMBA_AUG_FLIP && !(p[0] == 0.f || p[0] == 1.f || p[0] == 2.f)) return SIMAMBA_E_VARIANT;
    chain.op[o] = op;
    for (int k = 0; k < 4; ++k) chain.p[o][k] = p[k];
  }
  return SIMAMBA_OK;
}

static int aug_threads(int K) {
  const int t = (K + 63) / 64 * 64;
  return t > kAugMaxThreads ? kAugMaxThreads : t;
}

static bool aug_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + nb && pb < pa + na;
}

}  // namespace simamba

using namespace simamba;

extern "C" int simamba_augment_points(const float* points, const void* idx, int idx_is_64, const long long* sel,
                                      const long long* lengths, float* out, const int* ops, const float* op_params,
                                      int n_ops, long long* state, long long B, int N, int M, int K, void* stream) {
  if (B < 1 || B > 0x7fffffffll || N < 1 || N > kAugMaxPoints || M < 1 || M > kAugMaxPoints || K < 1 ||
      K > kAugMaxPoints || n_ops < 0 || n_ops > kAugMaxOps)
    return SIMAMBA_E_SHAPE;
  if ((!idx && M != N) || (!sel && K != M)) return SIMAMBA_E_SHAPE;
  if (!points || !out || !state || (n_ops > 0 && (!ops || !op_params))) return SIMAMBA_E_NULLPTR;
  AugChain chain;
  if (const int rc = aug_check_chain(ops, op_params, n_ops, chain)) return rc;
  // in place only row for row: a gather or a subset reads rows that other lanes, or other clouds' workgroups, write
  const size_t in_bytes = static_cast<size_t>(B) * N * 12, out_bytes = static_cast<size_t>(B) * K * 12;
  if (aug_overlap(points, in_bytes, out, out_bytes) && (idx || sel || static_cast<const void*>(points) != out))
    return SIMAMBA_E_VARIANT;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>(B)), block(aug_threads(K));
  if (idx && idx_is_64)
    hipLaunchKernelGGL(augment_points_kernel<long long>, grid, block, 0, st, points, static_cast<const long long*>(idx),
                       sel, lengths, out, chain, state, N, M, K);
  else
    hipLaunchKernelGGL(augment_points_kernel<int>, grid, block, 0, st, points, static_cast<const int*>(idx), sel,
                       lengths, out, chain, state, N, M, K);
  if (const hipError_t e = hipGetLastError()) return static_cast<int>(e);
  hipLaunchKernelGGL(augment_step_kernel, dim3(1), dim3(1), 0, st, state);
  return static_cast<int>(hipGetLastError());
}

extern "C" int simamba_augment_params(const long long* lengths, const int* ops, const float* op_params, int n_ops,
                                      const long long* state, float* cloud_params, float* noise, unsigned char* keep,
                                      long long B, int K, void* stream) {
  if (B < 1 || B > 0x7fffffffll || K < 1 || K > kAugMaxPoints || n_ops < 0 || n_ops > kAugMaxOps)
    return SIMAMBA_E_SHAPE;
  if (!state || (n_ops > 0 && (!ops || !op_params || !cloud_params))) return SIMAMBA_E_NULLPTR;
  AugChain chain;
  if (const int rc = aug_check_chain(ops, op_params, n_ops, chain)) return rc;
  hipLaunchKernelGGL(augment_params_kernel, dim3(static_cast<unsigned>(B)), dim3(aug_threads(K)), 0,
                     static_cast<hipStream_t>(stream), lengths, chain, state, cloud_params, noise, keep, K);
  return static_cast<int>(hipGetLastError());
}

extern "C" int simamba_philox4x32_10(long long seed, unsigned c0, unsigned c1, unsigned c2, unsigned c3,
                                     unsigned* out) {
  if (!out) return SIMAMBA_E_NULLPTR;
  const unsigned long long s = static_cast<unsigned long long>(seed);
  const Philox4 q = philox4x32_10(static_cast<uint32_t>(s), static_cast<uint32_t>(s >> 32), c0, c1, c2, c3);
  for (int k = 0; k < 4; ++k) out[k] = q.w[k];
  return SIMAMBA_OK;
}
