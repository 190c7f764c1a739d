// Damage to a batch of clouds, the kinds robustness suites score a classifier on (after ModelNet-C, Ren et al. 2022):
//   drop points globally | drop k-NN clusters | add uniform outliers | add Gaussian clusters on the surface |
//   bounded 3-axis rotation | anisotropic scale | jitter,   each optionally followed by the unit-sphere normalisation
// in one launch, one kind per call, followed by a one-lane kernel that adds 1 to the step.  Unlike augment.hip the cloud
// changes its size: out_lengths (B) is what PointMamba.forward(..., lengths=) takes, src (B, K) says where a row came from.
//
// One workgroup per cloud, the cloud in registers: lane t holds the 8 consecutive rows 8 t .. 8 t + 7 (T = ceil(K / 8)
// lanes rounded up to whole waves, K <= 8192), so the index order of the rows is the order (lane, slot) and compaction
// is a prefix sum over the lanes' alive counts.  Added points take the rows n .. behind the cloud's own.
//
// The m smallest of up to 8192 keys: every key is (32 bits of rank) << 13 | row, so keys are distinct and ties go to the
// lower row by construction; the m-th smallest is found bit by bit from the top (45 counting passes over the registers,
// one workgroup sum each) and the rows at or below it are removed.  No sort and no LDS beyond a row per wave: a
// bitonic sort of the same keys (curve_order.hip) is 91 barrier stages over 64 KB of LDS.  The bits of a
// non-negative fp32 d^2 order as unsigned integers.
//
// Random numbers are augment.hip's (Philox4x32-10, its counter layout at chain position 0) under a key of its own,
// (seed & 0xffffffff, (seed >> 32) ^ 0x434F5252), so one AugmentState feeds both kernels without sharing a stream.
// Nothing is read on the host; the call can sit in a captured graph.
//
// Rounding: built with -ffp-contract=off, every product and sum spelled __fmul_rn / __fadd_rn / ...: each discrete
// decision (how many rows go, which seed, which cluster, the angles, the scale factors) is a chain of single correctly
// rounded fp32 operations and integer arithmetic that a numpy restatement (tests/corrupt_ref.py) reproduces bit for bit.
// cos / sin / cbrt / log are the device library's.
#include <limits.h>

#include "cloud_regs.h"
#include "host_common.h"
#include "unit_sphere.h"

namespace simamba {

constexpr int kCorMaxClusters = SIMAMBA_CORRUPT_MAX_CLUSTERS;
constexpr float kCorTwoPi = 6.2831854820251465f;           // fp32(2 pi)

struct CorArgs {                                           // by value in the kernel arguments
  const float* points;
  const long long* lengths;
  float* out;
  long long* out_lengths;
  int* src;
  const long long* state;
  int N, K, kind, flags;
  int count, cmax;                                         // DROP_LOCAL / ADD_*: p[0] and p[1] as integers
  float p[4];
};

// C = min(1 + (int)(u * float(Cmax)), Cmax)
__device__ __forceinline__ int cor_clusters(const Philox4& q0, int cmax) {
  const int c = 1 + static_cast<int>(__fmul_rn(aug_uniform(q0.w[0]), static_cast<float>(cmax)));
  return c < cmax ? c : cmax;
}

__global__ __launch_bounds__(kCorMaxThreads) void corrupt_points_kernel(const CorArgs a) {
  __shared__ float sRed[kCorMaxWaves];
  __shared__ int sCnt[kCorMaxWaves];
  __shared__ float sPt[3];
  const long long b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
  const int N = a.N, K = a.K;
  const int n = clamped_length(a.lengths, b, N);
  const unsigned long long seed = static_cast<unsigned long long>(a.state[0]);
  const unsigned long long step = static_cast<unsigned long long>(a.state[1]);
  const CorRng rng{static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32) ^ SIMAMBA_CORRUPT_KEY_TWEAK,
                   blockIdx.x, static_cast<uint32_t>(step), static_cast<uint32_t>(step >> 32)};
  const float* __restrict__ in = a.points + b * N * 3;

  // rows >= n are never read; a row is alive while it belongs to the result
  float x[kCorPerLane], y[kCorPerLane], z[kCorPerLane];
  int sr[kCorPerLane];
  unsigned alive = 0;
  const int row0 = tid * kCorPerLane;
#pragma unroll
  for (int j = 0; j < kCorPerLane; ++j) {
    const int i = row0 + j;
    x[j] = y[j] = z[j] = 0.f;
    sr[j] = INT_MIN;
    if (i < n) {
      x[j] = in[3 * i];
      y[j] = in[3 * i + 1];
      z[j] = in[3 * i + 2];
      sr[j] = i;
      alive |= 1u << j;
    }
  }

  const Philox4 q0 = cor_block(rng, false, 0u);
  switch (a.kind) {                                                  // uniform over the workgroup
    case SIMAMBA_CORRUPT_DROP_GLOBAL: {
      int m = static_cast<int>(__fmul_rn(static_cast<float>(n), a.p[0]));
      m = m < 0 ? 0 : (m > n - 1 ? n - 1 : m);
      if (m == 0) break;
      unsigned long long key[kCorPerLane];
#pragma unroll
      for (int j = 0; j < kCorPerLane; ++j) {
        const int i = row0 + j;
        key[j] = kCorDead;
        if (i < n)
          key[j] = static_cast<unsigned long long>(cor_block(rng, true, static_cast<uint32_t>(i)).w[0]) << kCorIndexBits |
                   static_cast<unsigned long long>(i);
      }
      cor_remove_smallest(key, m, alive, sCnt, lane, wave, waves);
      break;
    }
    case SIMAMBA_CORRUPT_DROP_LOCAL: {
      const int C = cor_clusters(q0, a.cmax);
      const int Tp = a.count < n - 1 ? a.count : n - 1;
      int left = n;                                                  // alive rows
      for (int c = 0; c < C; ++c) {
        const int size = Tp / C + (c < Tp % C ? 1 : 0);
        if (size == 0 || size >= left) continue;                     // size < left by construction: Tp <= n - 1
        // the seed: the alive row of rank r in index order
        const int r = cor_pick(cor_block(rng, false, static_cast<uint32_t>(1 + c)).w[0], left);
        int unused;
        const int mine = __popc(alive);
        const int base = cor_block_scan(mine, sCnt, lane, wave, waves, unused);
        if (r >= base && r < base + mine) {
          int k = r - base;
#pragma unroll
          for (int j = 0; j < kCorPerLane; ++j) {
            if (alive >> j & 1u) {
              if (k == 0) {
                sPt[0] = x[j];
                sPt[1] = y[j];
                sPt[2] = z[j];
              }
              --k;
            }
          }
        }
        __syncthreads();
        const float sx = sPt[0], sy = sPt[1], sz = sPt[2];
        unsigned long long key[kCorPerLane];
#pragma unroll
        for (int j = 0; j < kCorPerLane; ++j) {
          const float dx = __fsub_rn(x[j], sx), dy = __fsub_rn(y[j], sy), dz = __fsub_rn(z[j], sz);
          const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
          key[j] = (alive >> j & 1u) ? static_cast<unsigned long long>(__builtin_bit_cast(uint32_t, d2)) << kCorIndexBits |
                                           static_cast<unsigned long long>(row0 + j)
                                     : kCorDead;
        }
        cor_remove_smallest(key, size, alive, sCnt, lane, wave, waves);   // its barriers also free sPt for the next seed
        left -= size;
      }
      break;
    }
    case SIMAMBA_CORRUPT_ADD_GLOBAL: {
      const int Ab = a.count < K - n ? a.count : K - n;
      const float R = a.p[1];
#pragma unroll
      for (int j = 0; j < kCorPerLane; ++j) {
        const int t = row0 + j - n;
        if (t >= 0 && t < Ab) {
          const Philox4 q = cor_block(rng, true, static_cast<uint32_t>(t));
          const float al = __fmul_rn(2.f, aug_uniform(q.w[1]));
          const float zc = __fsub_rn(1.f, al);
          const float s = __fsqrt_rn(__fmul_rn(al, __fsub_rn(2.f, al)));
          float sn, cs;
          sincosf(__fmul_rn(kCorTwoPi, aug_uniform(q.w[2])), &sn, &cs);
          const float r = __fmul_rn(R, cbrtf(aug_uniform(q.w[0])));
          x[j] = __fmul_rn(r, __fmul_rn(s, cs));
          y[j] = __fmul_rn(r, __fmul_rn(s, sn));
          z[j] = __fmul_rn(r, zc);
          sr[j] = -1;
          alive |= 1u << j;
        }
      }
      break;
    }
    case SIMAMBA_CORRUPT_ADD_LOCAL: {
      const int C = cor_clusters(q0, a.cmax);
      const int Tb = a.count < K - n ? a.count : K - n;
      const float lo = a.p[2], range = __fsub_rn(a.p[3], a.p[2]);
#pragma unroll
      for (int j = 0; j < kCorPerLane; ++j) {
        const int t = row0 + j - n;
        if (t >= 0 && t < Tb) {
          int c = 0, start = 0;                                      // the cluster whose prefix of sizes holds t
          for (; c < C - 1; ++c) {
            const int size = Tb / C + (c < Tb % C ? 1 : 0);
            if (t < start + size) break;
            start += size;
          }
          const Philox4 qc = cor_block(rng, false, static_cast<uint32_t>(1 + c));
          const int srow = cor_pick(qc.w[0], n);                     // < n: a row of the input that may be read
          const float sigma = __fadd_rn(lo, __fmul_rn(aug_uniform(qc.w[1]), range));
          float n0, n1, n2;
          aug_block_normals(cor_block(rng, true, static_cast<uint32_t>(t)), n0, n1, n2);
          x[j] = __fadd_rn(in[3 * srow], __fmul_rn(sigma, n0));
          y[j] = __fadd_rn(in[3 * srow + 1], __fmul_rn(sigma, n1));
          z[j] = __fadd_rn(in[3 * srow + 2], __fmul_rn(sigma, n2));
          sr[j] = -1 - c;
          alive |= 1u << j;
        }
      }
      break;
    }
    case SIMAMBA_CORRUPT_ROTATE3: {
      float sn[3], cs[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float ang = __fmul_rn(__fsub_rn(__fmul_rn(2.f, aug_uniform(q0.w[k])), 1.f), a.p[0]);
        sincosf(ang, &sn[k], &cs[k]);
      }
#pragma unroll
      for (int j = 0; j < kCorPerLane; ++j) {                        // Rx, then Ry, then Rz
        const float y1 = __fsub_rn(__fmul_rn(cs[0], y[j]), __fmul_rn(sn[0], z[j]));
        const float z1 = __fadd_rn(__fmul_rn(sn[0], y[j]), __fmul_rn(cs[0], z[j]));
        const float x2 = __fadd_rn(__fmul_rn(cs[1], x[j]), __fmul_rn(sn[1], z1));
        const float z2 = __fsub_rn(__fmul_rn(cs[1], z1), __fmul_rn(sn[1], x[j]));
        x[j] = __fsub_rn(__fmul_rn(cs[2], x2), __fmul_rn(sn[2], y1));
        y[j] = __fadd_rn(__fmul_rn(sn[2], x2), __fmul_rn(cs[2], y1));
        z[j] = z2;
      }
      break;
    }
    case SIMAMBA_CORRUPT_SCALE_AXES: {
      const float inv = __fdiv_rn(1.f, a.p[0]), range = __fsub_rn(a.p[0], inv);
      const float fx = __fadd_rn(inv, __fmul_rn(aug_uniform(q0.w[0]), range));
      const float fy = __fadd_rn(inv, __fmul_rn(aug_uniform(q0.w[1]), range));
      const float fz = __fadd_rn(inv, __fmul_rn(aug_uniform(q0.w[2]), range));
#pragma unroll
      for (int j = 0; j < kCorPerLane; ++j) {
        x[j] = __fmul_rn(x[j], fx);
        y[j] = __fmul_rn(y[j], fy);
        z[j] = __fmul_rn(z[j], fz);
      }
      break;
    }
    case SIMAMBA_CORRUPT_JITTER: {
      const float sd = a.p[0];
#pragma unroll
      for (int j = 0; j < kCorPerLane; ++j) {
        const int i = row0 + j;
        if (i < n) {
          float n0, n1, n2;
          aug_block_normals(cor_block(rng, true, static_cast<uint32_t>(i)), n0, n1, n2);
          x[j] = __fadd_rn(x[j], __fmul_rn(sd, n0));
          y[j] = __fadd_rn(y[j], __fmul_rn(sd, n1));
          z[j] = __fadd_rn(z[j], __fmul_rn(sd, n2));
        }
      }
      break;
    }
    default: break;
  }

  // where every alive row goes: its rank among the alive rows; the count is the output length (1 <= len <= K)
  int len;
  const int base = cor_block_scan(__popc(alive), sCnt, lane, wave, waves, len);
  len = len < 1 ? 1 : (len > K ? K : len);

  if (a.flags & SIMAMBA_CORRUPT_RENORM) {                            // uniform over the workgroup
    if (base == 0 && alive != 0) {                                   // the lane that holds output row 0
      const int j = __ffs(alive) - 1;
      float fx = 0.f, fy = 0.f, fz = 0.f;
#pragma unroll
      for (int k = 0; k < kCorPerLane; ++k) {
        if (k == j) {
          fx = x[k];
          fy = y[k];
          fz = z[k];
        }
      }
      sPt[0] = fx;
      sPt[1] = fy;
      sPt[2] = fz;
    }
    __syncthreads();
    unit_sphere_rows(x, y, z, alive, len, sPt[0], sPt[1], sPt[2], sRed, lane, wave, waves);
  }

  float* __restrict__ out = a.out + b * K * 3;
  int* __restrict__ src = a.src ? a.src + b * K : nullptr;
  for (int r = len + tid; r < K; r += blockDim.x) {                  // the tail: zeros, no source
    out[3 * r] = 0.f;
    out[3 * r + 1] = 0.f;
    out[3 * r + 2] = 0.f;
    if (src) src[r] = INT_MIN;
  }
  int d = base;
#pragma unroll
  for (int j = 0; j < kCorPerLane; ++j) {
    if (alive >> j & 1u) {
      const int r = d < len - 1 ? d : len - 1;                       // d < len; forced into range all the same
      out[3 * r] = x[j];
      out[3 * r + 1] = y[j];
      out[3 * r + 2] = z[j];
      if (src) src[r] = sr[j];
      ++d;
    }
  }
  if (tid == 0) a.out_lengths[b] = len;
}

__global__ void corrupt_step_kernel(long long* state) {
  state[1] = static_cast<long long>(static_cast<unsigned long long>(state[1]) + 1ull);
}

// a count parameter: >= 0 (a NaN fails), cut at the cloud limit, as an integer
static bool cor_count(float v, int& out) {
  if (!(v >= 0.f)) return false;
  out = v > static_cast<float>(kCorMaxPoints) ? kCorMaxPoints : static_cast<int>(v);
  return true;
}

static bool cor_cmax(float v, int& out) {
  if (!(v >= 1.f && v <= static_cast<float>(kCorMaxClusters)) || v != static_cast<float>(static_cast<int>(v)))
    return false;
  out = static_cast<int>(v);
  return true;
}

}  // namespace simamba

using namespace simamba;

extern "C" int simamba_corrupt_points(const float* points, const long long* lengths, float* out, long long* out_lengths,
                                      int* src, long long* state, int kind, int flags, const float* params, long long B,
                                      int N, int K, void* stream) {
  if (B < 1 || B > 0x7fffffffll || N < 1 || N > kCorMaxPoints || K < N || K > kCorMaxPoints) return SIMAMBA_E_SHAPE;
  if (!points || !out || !out_lengths || !state || !params) return SIMAMBA_E_NULLPTR;
  if (kind < SIMAMBA_CORRUPT_DROP_GLOBAL || kind > SIMAMBA_CORRUPT_JITTER || (flags & ~SIMAMBA_CORRUPT_RENORM))
    return SIMAMBA_E_VARIANT;
  CorArgs a{};
  for (int k = 0; k < 4; ++k) a.p[k] = params[k];
  a.cmax = 1;
  switch (kind) {
    case SIMAMBA_CORRUPT_DROP_GLOBAL:
      if (!(a.p[0] >= 0.f && a.p[0] < 1.f)) return SIMAMBA_E_VARIANT;
      break;
    case SIMAMBA_CORRUPT_DROP_LOCAL:
    case SIMAMBA_CORRUPT_ADD_LOCAL:
      if (!cor_count(a.p[0], a.count) || !cor_cmax(a.p[1], a.cmax)) return SIMAMBA_E_VARIANT;
      break;
    case SIMAMBA_CORRUPT_ADD_GLOBAL:
      if (!cor_count(a.p[0], a.count)) return SIMAMBA_E_VARIANT;
      break;
    case SIMAMBA_CORRUPT_SCALE_AXES:
      if (!(a.p[0] >= 1.f)) return SIMAMBA_E_VARIANT;
      break;
    default: break;
  }
  if (cor_overlap(points, static_cast<size_t>(B) * N * 12, out, static_cast<size_t>(B) * K * 12))
    return SIMAMBA_E_VARIANT;
  a.points = points;
  a.lengths = lengths;
  a.out = out;
  a.out_lengths = out_lengths;
  a.src = src;
  a.state = state;
  a.N = N;
  a.K = K;
  a.kind = kind;
  a.flags = flags;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(corrupt_points_kernel, dim3(static_cast<unsigned>(B)), dim3(cor_threads(K)), 0, st, a);
  if (const hipError_t e = hipGetLastError()) return static_cast<int>(e);
  hipLaunchKernelGGL(corrupt_step_kernel, dim3(1), dim3(1), 0, st, state);
  return static_cast<int>(hipGetLastError());
}
