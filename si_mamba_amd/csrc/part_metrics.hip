// Part-segmentation scoring (the reference's evaluation loop, part_segmentation/main.py:269-334, without the host):
// per point the argmax of the scores restricted to the label range [first, first + count) of the shape's category,
// and from it every count the four ShapeNetPart numbers are made of.  Integers until the last division.
//
// One 256-lane workgroup per shape, lanes striding over the points.  A lane keeps inter / uni of the (at most 16) parts
// and its correct count in registers; they are summed over the wave with shuffles and over the four waves through LDS,
// and lane 0 finishes shape_iou in double.  seen_class is an LDS histogram (integer LDS atomics) of the shape, added to
// the caller's (C) totals with one 64-bit integer atomic per label that occurred; correct_class[first + k] is inter[k]
// (a target outside the category never matches a prediction).  These two are the only sums across workgroups, and no
// float or double atomic exists here: the same bits every call.
//
// The argmax is np.argmax's: the first maximum, a NaN greater than every number, the first NaN wins; +-inf order as
// numbers.  No index is derived from a score, and a target label indexes LDS only after the check 0 <= t < C.
#include "host_common.h"
#include "pointset.h"

namespace simamba {

constexpr int kPartMaxParts = 16;       // parts per category
constexpr int kPartMaxLabels = 256;     // C
constexpr int kPartThreads = 256;
constexpr int kPartWaves = kPartThreads / 64;
constexpr int kPartSums = 2 * kPartMaxParts + 1;   // inter[16], uni[16], correct

template <typename T>
__global__ __launch_bounds__(kPartThreads) void part_seg_eval_kernel(
    const T* __restrict__ scores, const long long* __restrict__ target, const int* __restrict__ part_first,
    const int* __restrict__ part_count, const long long* __restrict__ lengths, long long* __restrict__ pred,
    int* __restrict__ inter_out, int* __restrict__ uni_out, double* __restrict__ shape_iou, int* __restrict__ correct_out,
    unsigned long long* __restrict__ seen_class, unsigned long long* __restrict__ correct_class, int n, int c) {
  __shared__ unsigned int sSeen[kPartMaxLabels];
  __shared__ int sSum[kPartWaves][kPartSums];
  const long long b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // the category's label range, forced inside [0, C): 1 <= count <= min(16, C), 0 <= first <= C - count
  const int cmax = c < kPartMaxParts ? c : kPartMaxParts;
  int count = part_count[b];
  count = count < 1 ? 1 : (count > cmax ? cmax : count);
  int first = part_first[b];
  first = first < 0 ? 0 : (first > c - count ? c - count : first);
  const int len = clamped_length(lengths, b, n);

  if (tid < c) sSeen[tid] = 0u;                    // c <= 256 = the workgroup
  __syncthreads();

  int inter[kPartMaxParts], uni[kPartMaxParts];
#pragma unroll
  for (int k = 0; k < kPartMaxParts; ++k) inter[k] = uni[k] = 0;
  int correct = 0;

  const T* __restrict__ srow = scores + b * n * c + first;
  const long long* __restrict__ trow = target + b * n;
  long long* __restrict__ prow = pred ? pred + b * n : nullptr;
  for (int i = tid; i < n; i += kPartThreads) {
    if (i >= len) {                                // padding: written, never read
      if (prow) prow[i] = -1;
      continue;
    }
    const T* __restrict__ s = srow + static_cast<long long>(i) * c;
    float v[kPartMaxParts];
#pragma unroll
    for (int k = 0; k < kPartMaxParts; ++k) v[k] = k < count ? to_f32<T>(s[k]) : 0.f;   // all loads in flight at once
    float best = v[0];
    int pk = 0;
#pragma unroll
    for (int k = 1; k < kPartMaxParts; ++k) {
      // v > best, or the first NaN: once best is a NaN neither comparison holds again
      const bool take = k < count && (v[k] > best || (v[k] != v[k] && best == best));
      best = take ? v[k] : best;
      pk = take ? k : pk;
    }
    const long long t = trow[i];
    const int tk = (t >= first && t < first + count) ? static_cast<int>(t - first) : -1;
    if (prow) prow[i] = first + pk;
    if (t >= 0 && t < c) atomicAdd(&sSeen[static_cast<int>(t)], 1u);
    correct += tk == pk;
#pragma unroll
    for (int k = 0; k < kPartMaxParts; ++k) {
      const bool tp = tk == k, pp = pk == k;
      inter[k] += tp && pp;
      uni[k] += tp || pp;
    }
  }

#pragma unroll
  for (int k = 0; k < kPartMaxParts; ++k) {
    inter[k] = wave_xor_sum(inter[k]);
    uni[k] = wave_xor_sum(uni[k]);
  }
  correct = wave_xor_sum(correct);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kPartMaxParts; ++k) {
      sSum[wave][k] = inter[k];
      sSum[wave][kPartMaxParts + k] = uni[k];
    }
    sSum[wave][2 * kPartMaxParts] = correct;
  }
  __syncthreads();                                 // also: every LDS atomic on sSeen has landed
  if (tid < kPartSums) {
    int t = sSum[0][tid];
#pragma unroll
    for (int w = 1; w < kPartWaves; ++w) t += sSum[w][tid];
    sSum[0][tid] = t;                              // column tid belongs to this lane alone
  }
  __syncthreads();

  if (tid < kPartMaxParts) {                       // columns >= count counted nothing: 0
    const int in = sSum[0][tid];
    inter_out[b * kPartMaxParts + tid] = in;
    uni_out[b * kPartMaxParts + tid] = sSum[0][kPartMaxParts + tid];
    if (in > 0) atomicAdd(&correct_class[first + tid], static_cast<unsigned long long>(in));
  }
  if (tid < c) {
    const unsigned int sn = sSeen[tid];
    if (sn != 0u) atomicAdd(&seen_class[tid], static_cast<unsigned long long>(sn));
  }
  if (tid == 0) {
    correct_out[b] = sSum[0][2 * kPartMaxParts];
    double sum = 0.0;                              // divide, add in part order, divide by count
    for (int k = 0; k < count; ++k) {
      const int u = sSum[0][kPartMaxParts + k];
      sum += u == 0 ? 1.0 : static_cast<double>(sSum[0][k]) / static_cast<double>(u);
    }
    shape_iou[b] = sum / static_cast<double>(count);
  }
}

}  // namespace simamba

using namespace simamba;

extern "C" int simamba_part_seg_eval(const void* scores, const long long* target, const int* part_first,
                                     const int* part_count, const long long* lengths, long long* pred, int* inter,
                                     int* uni, double* shape_iou, int* correct, long long* seen_class,
                                     long long* correct_class, long long batch, int n, int c, int io_dtype,
                                     void* stream) {
  if (batch < 1 || batch > 0x7fffffffll || n < 1 || c < 1 || c > kPartMaxLabels) return SIMAMBA_E_SHAPE;
  if (const int rc = check_io_dtype(io_dtype)) return rc;
  if (!scores || !target || !part_first || !part_count || !inter || !uni || !shape_iou || !correct || !seen_class ||
      !correct_class)
    return SIMAMBA_E_NULLPTR;
  hipStream_t st = static_cast<hipStream_t>(stream);
  with_io_type(io_dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(part_seg_eval_kernel<T>, dim3(static_cast<unsigned>(batch)), dim3(kPartThreads), 0, st,
                       static_cast<const T*>(scores), target, part_first, part_count, lengths, pred, inter, uni,
                       shape_iou, correct, reinterpret_cast<unsigned long long*>(seen_class),
                       reinterpret_cast<unsigned long long*>(correct_class), n, c);
  });
  return static_cast<int>(hipGetLastError());
}
