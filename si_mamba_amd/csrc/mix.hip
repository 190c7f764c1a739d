// Training-time augmentations that corrupt.hip's score is lowered with (the ones the ModelNet-C study compares):
//   simamba_cutmix_points     PointCutMix-R / -K (Zhang et al. 2021): m rows of a cloud are replaced by m rows of a
//                             partner cloud of the batch, chosen at random (R) or nearest to a seed row (K)
//   simamba_pointwolf_points  locally weighted deformation after PointWOLF (Kim et al. 2021): M anchors by farthest-point
//                             sampling, a random rotation / scale / translation about each, blended by a Gaussian of the
//                             distance to the anchor.  Written from the paper's description, not a reproduction of its
//                             draws.
//   simamba_mix_draw          the partner map and the lambdas the first draws when it is given none, for the caller's
//                             label arithmetic
// The first two are one launch, one workgroup per output cloud, followed by a one-lane kernel that adds 1 to the step.
//
// The cloud is in registers as in corrupt.hip (cloud_regs.h): lane t holds rows 8 t .. 8 t + 7, the m smallest keys are
// found by the 45-pass counting select, compaction is a prefix sum.  cutmix handles the partner's rows and then the
// cloud's own, so only one cloud's keys are live at a time; it copies rows and never computes with them, so its
// coordinates pass through the registers only on their way from points to out.
//
// Random numbers are augment.hip's (Philox4x32-10, its counter layout at chain position 0) under a key of its own,
// (seed & 0xffffffff, (seed >> 32) ^ SIMAMBA_MIX_KEY_TWEAK): one AugmentState feeds augment, corrupt and mix without
// sharing a stream.  Nothing is read on the host; the calls can sit in a captured graph.
//
// Rounding: built with -ffp-contract=off, every product, sum and quotient spelled __fmul_rn / __fadd_rn / ...: each
// discrete decision (lambda, m, the seeds, the selected rows, the anchors, the angles, factors and shifts, the argument
// of every exponential) is a chain of single correctly rounded fp32 operations and integer arithmetic that a numpy
// restatement (tests/mix_ref.py) reproduces bit for bit.  cos / sin / exp are the device library's.
#include <limits.h>

#include <cmath>

#include "cloud_regs.h"
#include "host_common.h"
#include "keyed_perm.h"
#include "unit_sphere.h"

namespace simamba {

constexpr int kWolfMaxAnchors = SIMAMBA_WOLF_MAX_ANCHORS;
constexpr int kWolfParams = 16;                            // floats per anchor in LDS: cos, sin, f, a, t (3 each), pad

__device__ __forceinline__ CorRng mix_rng(const long long* state, uint32_t cloud) {
  const unsigned long long seed = static_cast<unsigned long long>(state[0]);
  const unsigned long long step = static_cast<unsigned long long>(state[1]);
  return CorRng{static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32) ^ SIMAMBA_MIX_KEY_TWEAK, cloud,
                static_cast<uint32_t>(step), static_cast<uint32_t>(step >> 32)};
}

// the partner of cloud b: the caller's, forced into [0, B), or perm(B, key, stream = step, b)
__device__ __forceinline__ long long mix_partner(const long long* partner, const CorRng& r, long long b, long long B) {
  if (partner) {
    const long long q = partner[b];
    return q < 0 ? 0 : (q > B - 1 ? B - 1 : q);
  }
  const KeyedPerm plan = keyed_perm_plan(static_cast<uint32_t>(B));
  return keyed_perm(plan, r.k0, r.k1, r.step_lo, r.step_hi, static_cast<uint32_t>(b));
}

// lambda of cloud b: the caller's, forced into [0, 1] (a NaN becomes 0), or u(cloud block 0, w0)
__device__ __forceinline__ float mix_lambda(const float* lam, const CorRng& r, long long b) {
  if (lam) {
    const float l = lam[b];
    return l > 0.f ? (l < 1.f ? l : 1.f) : 0.f;
  }
  return aug_uniform(cor_block(r, false, 0u).w[0]);
}

// d2 = (dx dx + dy dy) + dz dz by direct differences: DROP_LOCAL's rule
__device__ __forceinline__ float mix_d2(float x, float y, float z, float sx, float sy, float sz) {
  const float dx = __fsub_rn(x, sx), dy = __fsub_rn(y, sy), dz = __fsub_rn(z, sz);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// Which m of the rows [0, n) of `in` have the smallest keys: they leave `alive`, which starts as `valid`.
// mode R: (word `word` of per-point block i, i); mode K: (d2 from row `seed`, i).  m == 0: nothing is selected.
// The coordinates are dead when the select begins: its 45 passes hold the keys alone.
__device__ __forceinline__ void mix_select(const float* __restrict__ in, int n, int m, int mode, int word, int seed,
                                           const CorRng& rng, unsigned& valid, unsigned& alive, int* sCnt, int row0,
                                           int lane, int wave, int waves) {
  valid = 0;
#pragma unroll
  for (int j = 0; j < kCorPerLane; ++j)
    if (row0 + j < n) valid |= 1u << j;
  alive = valid;
  if (m == 0) return;                                                // uniform over the workgroup
  unsigned long long key[kCorPerLane];
  if (mode == SIMAMBA_MIX_CUT_R) {
#pragma unroll
    for (int j = 0; j < kCorPerLane; ++j) {
      const int i = row0 + j;
      key[j] = kCorDead;
      if (i < n) {
        const Philox4 q = cor_block(rng, true, static_cast<uint32_t>(i));
        key[j] = static_cast<unsigned long long>(word ? q.w[1] : q.w[0]) << kCorIndexBits |
                 static_cast<unsigned long long>(i);
      }
    }
  } else {
    const float sx = in[3 * seed], sy = in[3 * seed + 1], sz = in[3 * seed + 2];   // seed < n: a row that may be read
#pragma unroll
    for (int j = 0; j < kCorPerLane; ++j) {
      const int i = row0 + j;
      key[j] = kCorDead;
      if (i < n) {                                                   // rows >= n are never read
        const float d2 = mix_d2(in[3 * i], in[3 * i + 1], in[3 * i + 2], sx, sy, sz);
        key[j] = static_cast<unsigned long long>(__builtin_bit_cast(uint32_t, d2)) << kCorIndexBits |
                 static_cast<unsigned long long>(i);
      }
    }
  }
  cor_remove_smallest(key, m, alive, sCnt, lane, wave, waves);
}

// the rows of `mask` (all below the cloud's length) from `in` to out rows first, first + 1, ... in index order, every
// row forced below `limit`
__device__ __forceinline__ void mix_store(const float* __restrict__ in, float* __restrict__ out, int* __restrict__ src,
                                          unsigned mask, int first, int limit, bool partner, int* sCnt, int row0,
                                          int lane, int wave, int waves) {
  int unused;
  int d = first + cor_block_scan(__popc(mask), sCnt, lane, wave, waves, unused);
#pragma unroll
  for (int j = 0; j < kCorPerLane; ++j) {
    if (mask >> j & 1u) {
      const int i = row0 + j;
      const int r = d < limit - 1 ? d : limit - 1;                   // d < limit; forced into range all the same
      out[3 * r] = in[3 * i];
      out[3 * r + 1] = in[3 * i + 1];
      out[3 * r + 2] = in[3 * i + 2];
      if (src) src[r] = partner ? -1 - i : i;
      ++d;
    }
  }
}

struct CutArgs {                                           // by value in the kernel arguments
  const float* points;
  const long long* lengths;
  const long long* partner;
  const float* lam;
  float* out;
  float* ratio;
  int* src;
  const long long* state;
  long long B;
  int N, mode;
};

__global__ __launch_bounds__(kCorMaxThreads) void cutmix_points_kernel(const CutArgs a) {
  __shared__ int sCnt[kCorMaxWaves];
  const long long b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
  const int N = a.N;
  const CorRng rng = mix_rng(a.state, blockIdx.x);
  const long long q = mix_partner(a.partner, rng, b, a.B);
  const int nb = clamped_length(a.lengths, b, N), nq = clamped_length(a.lengths, q, N);
  const float lambda = mix_lambda(a.lam, rng, b);
  int m = static_cast<int>(__fmul_rn(static_cast<float>(nb), lambda));
  m = m < 0 ? 0 : m;
  m = m < nb ? m : nb;
  m = m < nq ? m : nq;
  const Philox4 q1 = cor_block(rng, false, 1u);                      // the seeds of mode K
  const int row0 = tid * kCorPerLane;
  float* __restrict__ out = a.out + b * N * 3;
  int* __restrict__ src = a.src ? a.src + b * N : nullptr;

  const float* __restrict__ own = a.points + b * N * 3;
  const float* __restrict__ other = a.points + q * N * 3;
  unsigned valid, alive;
  if (m > 0) {                                                       // the partner's m rows, behind the survivors
    mix_select(other, nq, m, a.mode, 1, cor_pick(q1.w[1], nq), rng, valid, alive, sCnt, row0, lane, wave, waves);
    mix_store(other, out, src, valid & ~alive, nb - m, nb, true, sCnt, row0, lane, wave, waves);
  }
  if (m < nb) {                                                      // the cloud's own n_b - m survivors, in front
    mix_select(own, nb, m, a.mode, 0, cor_pick(q1.w[0], nb), rng, valid, alive, sCnt, row0, lane, wave, waves);
    mix_store(own, out, src, alive, 0, nb - m, false, sCnt, row0, lane, wave, waves);
  }

  for (int r = nb + tid; r < N; r += blockDim.x) {                   // the tail: zeros, no source
    out[3 * r] = 0.f;
    out[3 * r + 1] = 0.f;
    out[3 * r + 2] = 0.f;
    if (src) src[r] = INT_MIN;
  }
  if (tid == 0) a.ratio[b] = __fdiv_rn(static_cast<float>(m), static_cast<float>(nb));
}

__global__ void mix_draw_kernel(long long* partner, float* lam, const long long* state, long long B) {
  const long long b = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const CorRng rng = mix_rng(state, static_cast<uint32_t>(b));
  if (partner) partner[b] = mix_partner(nullptr, rng, b, B);
  if (lam) lam[b] = mix_lambda(nullptr, rng, b);
}

__global__ void mix_step_kernel(long long* state) {
  state[1] = static_cast<long long>(static_cast<unsigned long long>(state[1]) + 1ull);
}

// the largest v over the workgroup, in every lane
__device__ __forceinline__ unsigned long long mix_block_max(unsigned long long v, unsigned long long* s, int lane,
                                                            int wave, int waves) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long t = __shfl_xor(v, off);
    v = t > v ? t : v;
  }
  __syncthreads();                                         // the row may still be read from the call before
  if (lane == 0) s[wave] = v;
  __syncthreads();
  unsigned long long t = s[0];
  for (int w = 1; w < waves; ++w) t = s[w] > t ? s[w] : t;
  return t;
}

struct WolfArgs {                                          // by value in the kernel arguments
  const float* points;
  const long long* lengths;
  float* out;
  int* anchors;
  const long long* state;
  int N, M, flags;
  float c, rot, scale, trans;
};

__global__ __launch_bounds__(kCorMaxThreads) void pointwolf_points_kernel(const WolfArgs a) {
  __shared__ float sRed[kCorMaxWaves];
  __shared__ unsigned long long sKey[kCorMaxWaves];
  __shared__ float sT[kWolfMaxAnchors][kWolfParams];
  __shared__ float sPt[3];
  const long long b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
  const int N = a.N, M = a.M;
  const int n = clamped_length(a.lengths, b, N);
  const CorRng rng = mix_rng(a.state, blockIdx.x);
  const float* in = a.points + b * N * 3;                            // may be the output: every read is in front of the
  float* out = a.out + b * N * 3;                                    // barriers that precede the first store

  float x[kCorPerLane], y[kCorPerLane], z[kCorPerLane];
  unsigned valid = 0;
  const int row0 = tid * kCorPerLane;
#pragma unroll
  for (int j = 0; j < kCorPerLane; ++j) {
    const int i = row0 + j;
    x[j] = y[j] = z[j] = 0.f;
    if (i < n) {
      x[j] = in[3 * i];
      y[j] = in[3 * i + 1];
      z[j] = in[3 * i + 2];
      valid |= 1u << j;
    }
  }

  // anchors: a drawn row, then farthest-point sampling on the registers; a row's key is (bits of its smallest d2 to
  // the anchors so far) << 13 | (8191 - row), so the largest key is the farthest row and the lower row on a tie
  float mind[kCorPerLane];
  int anchor = cor_pick(cor_block(rng, false, 0u).w[0], n);
  for (int k = 0; k < M; ++k) {                                      // uniform over the workgroup
    anchor = anchor < 0 ? 0 : (anchor > n - 1 ? n - 1 : anchor);     // < n by construction; forced all the same
    const float ax = in[3 * anchor], ay = in[3 * anchor + 1], az = in[3 * anchor + 2];
    if (tid == 0) {
      sT[k][9] = ax;
      sT[k][10] = ay;
      sT[k][11] = az;
      if (a.anchors) a.anchors[b * M + k] = anchor;
    }
    if (k + 1 == M) break;
    unsigned long long best = 0;
#pragma unroll
    for (int j = 0; j < kCorPerLane; ++j) {
      const float d2 = mix_d2(x[j], y[j], z[j], ax, ay, az);
      mind[j] = (k == 0 || d2 < mind[j]) ? d2 : mind[j];
      const unsigned long long key = static_cast<unsigned long long>(__builtin_bit_cast(uint32_t, mind[j]))
                                         << kCorIndexBits |
                                     static_cast<unsigned long long>(kCorMaxPoints - 1 - (row0 + j));
      if ((valid >> j & 1u) && key > best) best = key;
    }
    best = mix_block_max(best, sKey, lane, wave, waves);
    anchor = kCorMaxPoints - 1 - static_cast<int>(best & static_cast<unsigned long long>(kCorMaxPoints - 1));
  }

  // the local transform of anchor j, by lane j: cos, sin (x, y, z), the factors, the shifts
  if (tid < M) {
    const Philox4 qa = cor_block(rng, false, static_cast<uint32_t>(1 + tid));
    const Philox4 qs = cor_block(rng, false, static_cast<uint32_t>(9 + tid));
    const Philox4 qt = cor_block(rng, false, static_cast<uint32_t>(17 + tid));
    const float range = __fsub_rn(a.scale, 1.f);
    const bool invert = qs.w[3] >> 31 != 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float ang = __fmul_rn(__fsub_rn(__fmul_rn(2.f, aug_uniform(qa.w[k])), 1.f), a.rot);
      float sn, cs;
      sincosf(ang, &sn, &cs);
      sT[tid][k] = cs;
      sT[tid][3 + k] = sn;
      const float f = __fadd_rn(1.f, __fmul_rn(aug_uniform(qs.w[k]), range));
      sT[tid][6 + k] = invert ? __fdiv_rn(1.f, f) : f;
      sT[tid][12 + k] = __fmul_rn(__fsub_rn(__fmul_rn(2.f, aug_uniform(qt.w[k])), 1.f), a.trans);
    }
  }
  __syncthreads();

#pragma unroll
  for (int j = 0; j < kCorPerLane; ++j) {
    if (!(valid >> j & 1u)) continue;
    float dmin = 0.f;
    for (int k = 0; k < M; ++k) {
      const float d2 = mix_d2(x[j], y[j], z[j], sT[k][9], sT[k][10], sT[k][11]);
      dmin = (k == 0 || d2 < dmin) ? d2 : dmin;
    }
    float sw = 0.f, px = 0.f, py = 0.f, pz = 0.f;
    for (int k = 0; k < M; ++k) {
      const float* t = sT[k];
      const float dx = __fsub_rn(x[j], t[9]), dy = __fsub_rn(y[j], t[10]), dz = __fsub_rn(z[j], t[11]);
      const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
      const float w = expf(-__fmul_rn(__fsub_rn(d2, dmin), a.c));
      const float vx = __fmul_rn(dx, t[6]), vy = __fmul_rn(dy, t[7]), vz = __fmul_rn(dz, t[8]);
      // Rx, then Ry, then Rz: corrupt.hip's ROTATE3
      const float y1 = __fsub_rn(__fmul_rn(t[0], vy), __fmul_rn(t[3], vz));
      const float z1 = __fadd_rn(__fmul_rn(t[3], vy), __fmul_rn(t[0], vz));
      const float x2 = __fadd_rn(__fmul_rn(t[1], vx), __fmul_rn(t[4], z1));
      const float z2 = __fsub_rn(__fmul_rn(t[1], z1), __fmul_rn(t[4], vx));
      const float x3 = __fsub_rn(__fmul_rn(t[2], x2), __fmul_rn(t[5], y1));
      const float y3 = __fadd_rn(__fmul_rn(t[5], x2), __fmul_rn(t[2], y1));
      const float qx = __fadd_rn(__fadd_rn(x3, t[9]), t[12]);
      const float qy = __fadd_rn(__fadd_rn(y3, t[10]), t[13]);
      const float qz = __fadd_rn(__fadd_rn(z2, t[11]), t[14]);
      sw = __fadd_rn(sw, w);
      px = __fadd_rn(px, __fmul_rn(w, qx));
      py = __fadd_rn(py, __fmul_rn(w, qy));
      pz = __fadd_rn(pz, __fmul_rn(w, qz));
    }
    x[j] = __fdiv_rn(px, sw);                                        // sw >= 1: the nearest anchor's weight is exp(0)
    y[j] = __fdiv_rn(py, sw);
    z[j] = __fdiv_rn(pz, sw);
  }

  if (a.flags & SIMAMBA_WOLF_RENORM) {                               // uniform over the workgroup
    if (tid == 0) {                                                  // row 0 is valid: n >= 1
      sPt[0] = x[0];
      sPt[1] = y[0];
      sPt[2] = z[0];
    }
    __syncthreads();
    unit_sphere_rows(x, y, z, valid, n, sPt[0], sPt[1], sPt[2], sRed, lane, wave, waves);
  }

  for (int r = n + tid; r < N; r += blockDim.x) {                    // the tail: zeros
    out[3 * r] = 0.f;
    out[3 * r + 1] = 0.f;
    out[3 * r + 2] = 0.f;
  }
#pragma unroll
  for (int j = 0; j < kCorPerLane; ++j) {
    const int i = row0 + j;
    if (i < n) {
      out[3 * i] = x[j];
      out[3 * i + 1] = y[j];
      out[3 * i + 2] = z[j];
    }
  }
}

}  // namespace simamba

using namespace simamba;

extern "C" int simamba_cutmix_points(const float* points, const long long* lengths, const long long* partner,
                                     const float* lam, float* out, float* ratio, int* src, long long* state, int mode,
                                     long long B, int N, void* stream) {
  if (B < 1 || B > 0x7fffffffll || N < 1 || N > kCorMaxPoints) return SIMAMBA_E_SHAPE;
  if (!points || !out || !ratio || !state) return SIMAMBA_E_NULLPTR;
  if (mode != SIMAMBA_MIX_CUT_R && mode != SIMAMBA_MIX_CUT_K) return SIMAMBA_E_VARIANT;
  const size_t bytes = static_cast<size_t>(B) * N * 12;
  if (cor_overlap(points, bytes, out, bytes)) return SIMAMBA_E_VARIANT;
  const CutArgs a{points, lengths, partner, lam, out, ratio, src, state, B, N, mode};
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(cutmix_points_kernel, dim3(static_cast<unsigned>(B)), dim3(cor_threads(N)), 0, st, a);
  if (const hipError_t e = hipGetLastError()) return static_cast<int>(e);
  hipLaunchKernelGGL(mix_step_kernel, dim3(1), dim3(1), 0, st, state);
  return static_cast<int>(hipGetLastError());
}

extern "C" int simamba_mix_draw(long long* partner, float* lam, const long long* state, long long B, void* stream) {
  if (B < 1 || B > 0x7fffffffll) return SIMAMBA_E_SHAPE;
  if (!state || (!partner && !lam)) return SIMAMBA_E_NULLPTR;
  const unsigned blocks = static_cast<unsigned>((B + 255) / 256);
  hipLaunchKernelGGL(mix_draw_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), partner, lam, state,
                     B);
  return static_cast<int>(hipGetLastError());
}

extern "C" int simamba_pointwolf_points(const float* points, const long long* lengths, float* out, int* anchors_out,
                                        long long* state, int M, const float* params, int flags, long long B, int N,
                                        void* stream) {
  if (B < 1 || B > 0x7fffffffll || N < 1 || N > kCorMaxPoints || M < 1 || M > kWolfMaxAnchors) return SIMAMBA_E_SHAPE;
  if (!points || !out || !state || !params) return SIMAMBA_E_NULLPTR;
  if (flags & ~SIMAMBA_WOLF_RENORM) return SIMAMBA_E_VARIANT;
  const float sigma = params[0], rot = params[1], scale = params[2], trans = params[3];
  const float c = static_cast<float>(1.0 / (2.0 * static_cast<double>(sigma) * static_cast<double>(sigma)));
  if (!(sigma > 0.f) || !std::isfinite(sigma) || !std::isfinite(c) || !(rot >= 0.f) || !std::isfinite(rot) || !(scale >= 1.f) ||
      !std::isfinite(scale) || !(trans >= 0.f) || !std::isfinite(trans))
    return SIMAMBA_E_VARIANT;
  const size_t bytes = static_cast<size_t>(B) * N * 12;
  if (out != points && cor_overlap(points, bytes, out, bytes)) return SIMAMBA_E_VARIANT;
  const WolfArgs a{points, lengths, out, anchors_out, state, N, M, flags, c, rot, scale, trans};
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(pointwolf_points_kernel, dim3(static_cast<unsigned>(B)), dim3(cor_threads(N)), 0, st, a);
  if (const hipError_t e = hipGetLastError()) return static_cast<int>(e);
  hipLaunchKernelGGL(mix_step_kernel, dim3(1), dim3(1), 0, st, state);
  return static_cast<int>(hipGetLastError());
}
