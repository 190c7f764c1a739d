// The optimizer tail of a training step in three launches, for any number of parameter tensors: the squared gradient
// norm, one workgroup that prepares every scalar the update needs, and decoupled AdamW (torch.optim.AdamW's
// formulation; the clip is torch.nn.utils.clip_grad_norm_'s).  The reference composes the same from torch multi-tensor
// ops (tools/builder.py:58-95, tools/runner_finetune.py:200-215).
//
// The kernels work from two tables in device memory.  A segment (simamba_optim_segment, 64 bytes) is one parameter
// tensor: the addresses of p, g, exp_avg and exp_avg_sq, the element count, the group and the tensor's own step count.
// A chunk entry maps a workgroup to (segment, chunk inside the segment); a chunk is SIMAMBA_OPTIM_CHUNK elements, so
// one launch covers every tensor and a workgroup never straddles two of them.  A segment whose g is NULL took no
// gradient: its workgroups write a zero partial and leave.
//
// The gradient addresses are the one column of the table that changes from step to step (autograd hands out a fresh
// tensor after zero_grad(set_to_none=True), and inside a graph capture one whose address no eager step has seen), so
// they do not come from the host's copy of the table: the call takes them as a HOST array and the first kernel
// receives them BY VALUE, kOptGradArgs to a launch, reads its own g from the argument and leaves it in the table for
// the other two.  A captured launch keeps its arguments, so a replay restores the column the capture saw.
//
// optim_sumsq_kernel:   partial[chunk] = sum (grad_scale g)^2, accumulated in fp64; segment.g = the argument.  No atomics.
// optim_prepare_kernel: one workgroup.  grad_norm = sqrt(sum of the partials in a fixed order); coef = clip /
//                       (grad_norm + 1e-6) clamped above at 1 with NaN propagating; the update count and the step of
//                       every segment with a gradient advance; each group's learning rate comes from the schedule
//                       table (and is written back to the group's device lr) or from the device lr as it stands; per
//                       segment lr / (1 - beta1^t), sqrt(1 - beta2^t) and 1 - lr wd, the powers and quotients in fp64.
// optim_adamw_kernel:   p *= 1 - lr wd;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;
//                       p -= step_size m / (sqrt(v) / sqrt(bc2) + eps),  g' = grad_scale coef g;  optionally g = 0.
//
// Each of the four arrays of a segment is read and written with 16-byte accesses when its own address is 16-byte
// aligned and dword by dword when it is not (a slice of a flat gradient buffer, a view into a flat parameter buffer):
// the four decide independently, the branch is uniform over the workgroup.  Every sum runs in a fixed order: the same
// bits on every call.
#include <math.h>

#include "host_common.h"

namespace simamba {

constexpr int kOptThreads = 256;
constexpr int kOptWaves = kOptThreads / 64;
constexpr int kOptChunk = SIMAMBA_OPTIM_CHUNK;
constexpr int kOptIters = kOptChunk / (kOptThreads * 4);     // float4 groups per lane and chunk
static_assert(kOptChunk % (kOptThreads * 4) == 0, "a chunk is whole rounds of one float4 per lane");
constexpr int kOptMaxSegments = SIMAMBA_OPTIM_MAX_SEGMENTS;
constexpr int kOptMaxChunks = SIMAMBA_OPTIM_MAX_CHUNKS;
constexpr int kOptMaxGroups = SIMAMBA_OPTIM_MAX_GROUPS;
constexpr int kOptMaxSchedule = 1 << 20;
constexpr int kOptGradArgs = 448;                            // 3 584 of the 4 096 bytes a kernel's arguments may take

using OptSegment = simamba_optim_segment;
using OptGroup = simamba_optim_group;
static_assert(sizeof(OptSegment) == 64 && sizeof(OptGroup) == 64, "the tables are built by the caller, word by word");

struct OptGradArgs {
  float* g[kOptGradArgs];
};

struct alignas(16) OptCoef {
  float step_size, bc2_sqrt, decay, eps;
};

// workspace: [gscale and 12 unused bytes | partials: chunks doubles, rounded up to 16 bytes | coefs: segments x 16 bytes]
inline size_t opt_partials_bytes(int n_chunks) { return 16 * ((static_cast<size_t>(n_chunks) + 1) / 2); }
inline size_t opt_ws_bytes(int n_segments, int n_chunks) {
  return 16 + opt_partials_bytes(n_chunks) + sizeof(OptCoef) * static_cast<size_t>(n_segments);
}

__device__ __forceinline__ bool opt_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__device__ __forceinline__ float4 opt_load4(const float* __restrict__ p, bool vec) {
  if (vec) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}
__device__ __forceinline__ void opt_store4(float* __restrict__ p, bool vec, float4 x) {
  if (vec) {
    *reinterpret_cast<float4*>(p) = x;
  } else {
    p[0] = x.x;
    p[1] = x.y;
    p[2] = x.z;
    p[3] = x.w;
  }
}

// the sum of v over the workgroup in a fixed order, the same value in every lane; `s` holds kOptWaves doubles
__device__ __forceinline__ double opt_block_sum(double v, double* s) {
  v = wave_xor_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = s[0];
#pragma unroll
  for (int w = 1; w < kOptWaves; ++w) t += s[w];
  return t;
}

// the elements of chunk `c` of a segment of n elements: 0 for a table that names a chunk past the end
__device__ __forceinline__ int opt_chunk_count(long long n, int c) {
  const long long left = n - static_cast<long long>(c) * kOptChunk;
  return left <= 0 ? 0 : (left < kOptChunk ? static_cast<int>(left) : kOptChunk);
}

__global__ __launch_bounds__(kOptThreads) void optim_sumsq_kernel(OptSegment* __restrict__ segs,
                                                                   const int2* __restrict__ chunks,
                                                                   double* __restrict__ partials, int seg_base,
                                                                   int seg_count, int chunk_base, float grad_scale,
                                                                   const OptGradArgs grads) {
  __shared__ double sD[kOptWaves];
  const int k = chunk_base + blockIdx.x;
  const int2 c = chunks[k];
  const int local = c.x - seg_base;
  const bool known = local >= 0 && local < seg_count;        // an entry this launch cannot mean: a zero partial
  const float* __restrict__ g = known ? grads.g[local] : nullptr;
  if (known && c.y == 0 && threadIdx.x == 0) segs[c.x].g = const_cast<float*>(g);    // one writer per segment
  double acc = 0.0;
  if (g) {                                                   // the same word for the whole workgroup
    const int cnt = opt_chunk_count(segs[c.x].n, c.y);
    g += static_cast<long long>(c.y) * kOptChunk;
    const bool vec = opt_aligned16(g);
#pragma unroll
    for (int it = 0; it < kOptIters; ++it) {
      const int e = (it * kOptThreads + threadIdx.x) * 4;
      if (e + 4 <= cnt) {
        const float4 x = opt_load4(g + e, vec);
        const double a = grad_scale * x.x, b = grad_scale * x.y, d = grad_scale * x.z, f = grad_scale * x.w;
        acc = fma(a, a, acc);
        acc = fma(b, b, acc);
        acc = fma(d, d, acc);
        acc = fma(f, f, acc);
      } else {
        for (int k = e; k < cnt; ++k) {
          const double a = grad_scale * g[k];
          acc = fma(a, a, acc);
        }
      }
    }
  }
  acc = opt_block_sum(acc, sD);
  if (threadIdx.x == 0) partials[k] = acc;
}

__global__ __launch_bounds__(kOptThreads) void optim_prepare_kernel(
    OptSegment* __restrict__ segs, const OptGroup* __restrict__ groups, long long* __restrict__ updates,
    const double* __restrict__ sched, const double* __restrict__ partials, OptCoef* __restrict__ coefs,
    float* __restrict__ gscale, float* __restrict__ grad_norm, int n_segments, int n_chunks, int n_groups, int sched_n,
    int steps_per_epoch, float max_norm, float grad_scale) {
  __shared__ double sD[kOptWaves];
  __shared__ float sLr[kOptMaxGroups];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int k = tid; k < n_chunks; k += kOptThreads) acc += partials[k];
  const double norm = sqrt(opt_block_sum(acc, sD));
  const long long done = updates[0];                         // every lane reads it before lane 0 advances it
  if (tid < n_groups) {
    float lr;
    if (sched_n > 0) {
      const long long epoch = done / steps_per_epoch;
      const int idx = epoch < 0 ? 0 : (epoch < sched_n - 1 ? static_cast<int>(epoch) : sched_n - 1);
      lr = static_cast<float>(sched[idx] * groups[tid].lr_scale);
      groups[tid].lr[0] = lr;
    } else {
      lr = groups[tid].lr[0];
    }
    sLr[tid] = lr;
  }
  __syncthreads();                                           // sLr is whole; `done` is in every lane's register
  if (tid == 0) {
    double coef = 1.0;
    if (max_norm >= 0.f) {
      coef = static_cast<double>(max_norm) / (norm + 1e-6);
      if (coef > 1.0) coef = 1.0;                            // torch.clamp(max=1): a NaN fails the test and stays NaN
    }
    gscale[0] = static_cast<float>(static_cast<double>(grad_scale) * coef);
    grad_norm[0] = static_cast<float>(norm);
    updates[0] = done + 1;
  }
  for (int s = tid; s < n_segments; s += kOptThreads) {
    if (!segs[s].g) continue;
    const int gi = segs[s].group;
    if (gi < 0 || gi >= n_groups) continue;                  // a table this call did not build: the update skips it too
    const OptGroup& G = groups[gi];
    const float t = segs[s].step + 1.f;
    segs[s].step = t;
    const double lr = static_cast<double>(sLr[gi]);
    const double bc1 = 1.0 - pow(G.beta1, static_cast<double>(t));
    const double bc2 = 1.0 - pow(G.beta2, static_cast<double>(t));
    OptCoef c;
    c.step_size = static_cast<float>(lr / bc1);
    c.bc2_sqrt = static_cast<float>(sqrt(bc2));
    c.decay = static_cast<float>(1.0 - lr * G.weight_decay);
    c.eps = static_cast<float>(G.eps);
    coefs[s] = c;
  }
}

__device__ __forceinline__ void opt_adamw_one(float& p, float g, float& m, float& v, float gs, float b1, float omb1,
                                              float b2, float omb2, const OptCoef& c) {
  g *= gs;
  p *= c.decay;
  m = b1 * m + omb1 * g;
  v = b2 * v + omb2 * (g * g);
  const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
  p -= c.step_size * (m / denom);
}

template <bool kZero>
__global__ __launch_bounds__(kOptThreads) void optim_adamw_kernel(const OptSegment* __restrict__ segs,
                                                                   const int2* __restrict__ chunks,
                                                                   const OptGroup* __restrict__ groups,
                                                                   const OptCoef* __restrict__ coefs,
                                                                   const float* __restrict__ gscale, int n_segments,
                                                                   int n_groups) {
  const int2 ce = chunks[blockIdx.x];
  if (ce.x < 0 || ce.x >= n_segments) return;
  const OptSegment& S = segs[ce.x];
  if (!S.g) return;                                          // the whole workgroup
  const int gi = S.group;
  if (gi < 0 || gi >= n_groups) return;
  const int cnt = opt_chunk_count(S.n, ce.y);
  const long long first = static_cast<long long>(ce.y) * kOptChunk;
  float* __restrict__ p = S.p + first;
  float* __restrict__ g = S.g + first;
  float* __restrict__ m = S.exp_avg + first;
  float* __restrict__ v = S.exp_avg_sq + first;
  const bool vp = opt_aligned16(p), vg = opt_aligned16(g), vm = opt_aligned16(m), vv = opt_aligned16(v);
  const OptCoef c = coefs[ce.x];
  const float gs = gscale[0];
  const float b1 = static_cast<float>(groups[gi].beta1), omb1 = static_cast<float>(1.0 - groups[gi].beta1);
  const float b2 = static_cast<float>(groups[gi].beta2), omb2 = static_cast<float>(1.0 - groups[gi].beta2);
#pragma unroll 2
  for (int it = 0; it < kOptIters; ++it) {
    const int e = (it * kOptThreads + threadIdx.x) * 4;
    if (e + 4 <= cnt) {
      float4 P = opt_load4(p + e, vp), M = opt_load4(m + e, vm), V = opt_load4(v + e, vv);
      const float4 G = opt_load4(g + e, vg);
      opt_adamw_one(P.x, G.x, M.x, V.x, gs, b1, omb1, b2, omb2, c);
      opt_adamw_one(P.y, G.y, M.y, V.y, gs, b1, omb1, b2, omb2, c);
      opt_adamw_one(P.z, G.z, M.z, V.z, gs, b1, omb1, b2, omb2, c);
      opt_adamw_one(P.w, G.w, M.w, V.w, gs, b1, omb1, b2, omb2, c);
      opt_store4(p + e, vp, P);
      opt_store4(m + e, vm, M);
      opt_store4(v + e, vv, V);
      if (kZero) opt_store4(g + e, vg, make_float4(0.f, 0.f, 0.f, 0.f));
    } else {
      for (int k = e; k < cnt; ++k) {
        float P = p[k], M = m[k], V = v[k];
        opt_adamw_one(P, g[k], M, V, gs, b1, omb1, b2, omb2, c);
        p[k] = P;
        m[k] = M;
        v[k] = V;
        if (kZero) g[k] = 0.f;
      }
    }
  }
}

}  // namespace simamba

using namespace simamba;

extern "C" size_t simamba_optim_workspace_bytes(int n_segments, int n_chunks) {
  if (n_segments < 0 || n_segments > kOptMaxSegments || n_chunks < 0 || n_chunks > kOptMaxChunks) return 0;
  return opt_ws_bytes(n_segments, n_chunks);
}

extern "C" int simamba_optim_adamw_step(void* segments, const int* chunks, const void* groups, long long* updates,
                                        const double* schedule, float* grad_norm, const void* const* grads,
                                        const int* first_chunk, void* workspace,
                                        size_t workspace_bytes, int n_segments, int n_chunks, int n_groups,
                                        int schedule_n, int steps_per_epoch, float max_norm, float grad_scale,
                                        int flags, void* stream) {
  if (flags & ~SIMAMBA_OPTIM_ZERO_GRADS) return SIMAMBA_E_VARIANT;
  if (n_segments < 1 || n_segments > kOptMaxSegments || n_chunks < 1 || n_chunks > kOptMaxChunks ||
      n_groups < 1 || n_groups > kOptMaxGroups)
    return SIMAMBA_E_SHAPE;
  if (schedule_n < 0 || schedule_n > kOptMaxSchedule || (schedule_n > 0 && steps_per_epoch < 1)) return SIMAMBA_E_SHAPE;
  if (max_norm != max_norm || !(grad_scale > -3e38f && grad_scale < 3e38f)) return SIMAMBA_E_SHAPE;
  if (first_chunk) {                                         // a HOST array: segment s owns chunks [first[s], first[s+1])
    if (first_chunk[0] != 0 || first_chunk[n_segments] != n_chunks) return SIMAMBA_E_SHAPE;
    for (int i = 0; i < n_segments; ++i)
      if (first_chunk[i] > first_chunk[i + 1]) return SIMAMBA_E_SHAPE;
  }
  if (!segments || !chunks || !groups || !updates || !grad_norm || !grads || !first_chunk ||
      (schedule_n > 0 && !schedule))
    return SIMAMBA_E_NULLPTR;
  if (!workspace || workspace_bytes < opt_ws_bytes(n_segments, n_chunks)) return SIMAMBA_E_WORKSPACE;
  if (!aligned16(workspace) || !aligned16(segments) || !aligned16(groups) ||
      (reinterpret_cast<uintptr_t>(chunks) & 7u) || (reinterpret_cast<uintptr_t>(updates) & 7u) ||
      (reinterpret_cast<uintptr_t>(schedule) & 7u) || (reinterpret_cast<uintptr_t>(grad_norm) & 3u))
    return SIMAMBA_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  OptSegment* segs = static_cast<OptSegment*>(segments);
  const OptGroup* grp = static_cast<const OptGroup*>(groups);
  const int2* chk = reinterpret_cast<const int2*>(chunks);
  char* ws = static_cast<char*>(workspace);
  float* gscale = reinterpret_cast<float*>(ws);
  double* partials = reinterpret_cast<double*>(ws + 16);
  OptCoef* coefs = reinterpret_cast<OptCoef*>(ws + 16 + opt_partials_bytes(n_chunks));
  for (int base = 0; base < n_segments; base += kOptGradArgs) {
    const int count = n_segments - base < kOptGradArgs ? n_segments - base : kOptGradArgs;
    const int c0 = first_chunk[base], c1 = first_chunk[base + count];
    if (c1 == c0) continue;                                  // empty tensors only
    OptGradArgs a;
    for (int i = 0; i < count; ++i) a.g[i] = static_cast<float*>(const_cast<void*>(grads[base + i]));
    for (int i = count; i < kOptGradArgs; ++i) a.g[i] = nullptr;
    hipLaunchKernelGGL(optim_sumsq_kernel, dim3(c1 - c0), dim3(kOptThreads), 0, s, segs, chk, partials, base, count,
                       c0, grad_scale, a);
  }
  hipLaunchKernelGGL(optim_prepare_kernel, dim3(1), dim3(kOptThreads), 0, s, segs, grp, updates, schedule, partials,
                     coefs, gscale, grad_norm, n_segments, n_chunks, n_groups, schedule_n, steps_per_epoch, max_norm,
                     grad_scale);
  if (flags & SIMAMBA_OPTIM_ZERO_GRADS)
    hipLaunchKernelGGL(optim_adamw_kernel<true>, dim3(n_chunks), dim3(kOptThreads), 0, s, segs, chk, grp, coefs,
                       gscale, n_segments, n_groups);
  else
    hipLaunchKernelGGL(optim_adamw_kernel<false>, dim3(n_chunks), dim3(kOptThreads), 0, s, segs, chk, grp, coefs,
                       gscale, n_segments, n_groups);
  return static_cast<int>(hipGetLastError());
}
