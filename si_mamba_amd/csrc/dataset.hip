// A batch out of a dataset that is resident on the device (the reference's torch DataLoader over
// datasets/ShapeNet55Dataset.py, ScanObjectNNDataset.py, ModelNetDataset.py and part_segmentation/dataset.py, without
// its workers, per-item numpy work, file reads and host-to-device copy): for every slot b of the batch
//   which cloud   s = perm(S, seed, epoch, p)  or  p,        p = (pos B + b) world + rank  the slot's global position
//   which rows    the first min(K, c) | a keyed permutation of the c candidates | K draws with replacement
//   normalise     none | subtract the mean of the selected rows, divide by their largest norm (pc_norm)
// in one launch, followed by a one-lane kernel that adds 1 to the step.
//
// One workgroup per slot, the selected rows in registers: lane t of T holds rows t, t + T, ... (at most 8 at T = 1024,
// so K <= 8192, the limit of the other point kernels here), as augment_points_kernel does.  The workgroup meets only
// for the normalisation: row 0, three sums and one maximum, through wave butterflies and one LDS row per wave, in a fixed order.
// Plain C++; no atomics, no workspace.  Every lane redoes the slot's own arithmetic (epoch, position, the shuffle's one
// permutation value) instead of sharing it.
//
// Random choices are counter based (keyed_perm.h over philox.h), so nothing is read on the host, the call can sit in a
// captured graph, and a slot depends only on (seed, epoch, p), the store and the modes: not on B, the launch geometry
// or the other slots.  The stream layout is part of the contract and stated in include/simamba.h.
//
// Rounding: built with -ffp-contract=off, and the normalisation is spelled in __fadd_rn / __fmul_rn / __fdiv_rn /
// __fsqrt_rn, one correctly rounded fp32 operation each, in an order the header states.
#include "host_common.h"
#include "keyed_perm.h"
#include "unit_sphere.h"

namespace simamba {

constexpr int kDsMaxPoints = 8192;
constexpr int kDsMaxThreads = 1024;
constexpr int kDsPerLane = kDsMaxPoints / kDsMaxThreads;
constexpr int kDsMaxWaves = kDsMaxThreads / 64;
constexpr unsigned long long kDsEpochMask = (1ull << 29) - 1;

// stream = purpose << 60 | (epoch mod 2^29) << 31 | p, p < 2^31: the layout of simamba.h
SIMAMBA_HD unsigned long long ds_stream(unsigned purpose, unsigned long long epoch, unsigned long long p) {
  return (static_cast<unsigned long long>(purpose) << 60) | ((epoch & kDsEpochMask) << 31) | p;
}

struct DsArgs {                                            // by value in the kernel arguments
  long long total, S, stride, steps_per_epoch;
  int K, first, rank, world, order, rows, norm;
};

__global__ __launch_bounds__(kDsMaxThreads) void dataset_fetch_kernel(
    const float* __restrict__ points, const long long* __restrict__ offsets, const long long* __restrict__ labels,
    const int* __restrict__ point_labels, const long long* __restrict__ state, float* __restrict__ out,
    long long* __restrict__ label_out, int* __restrict__ point_label_out, long long* __restrict__ index_out,
    int* __restrict__ lengths_out, const DsArgs a) {
  __shared__ float sRed[kDsMaxWaves];
  __shared__ float sFirst[3];
  const long long b = blockIdx.x, B = gridDim.x;
  const int T = blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = T >> 6;
  const int K = a.K;
  const unsigned long long seed = static_cast<unsigned long long>(state[0]);
  const unsigned long long step = static_cast<unsigned long long>(state[1]);
  const uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
  const unsigned long long spe = static_cast<unsigned long long>(a.steps_per_epoch);
  const unsigned long long epoch = step / spe, pos = step - epoch * spe;
  // < 2^62: the host checked steps_per_epoch * B * world
  const unsigned long long p = (pos * static_cast<unsigned long long>(B) + static_cast<unsigned long long>(b)) *
                                   static_cast<unsigned long long>(a.world) + static_cast<unsigned long long>(a.rank);

  // the slot's cloud: s < S, its rows [base, base + n) forced inside the store's T rows whatever `offsets` holds
  long long s = -1, base = 0, n = 0;
  if (p < static_cast<unsigned long long>(a.S)) {
    s = static_cast<long long>(p);
    if (a.order == SIMAMBA_DS_SHUFFLE) {
      const unsigned long long st = ds_stream(SIMAMBA_DS_STREAM_SHUFFLE, epoch, 0);
      s = keyed_perm(keyed_perm_plan(static_cast<uint32_t>(a.S)), k0, k1, static_cast<uint32_t>(st),
                     static_cast<uint32_t>(st >> 32), static_cast<uint32_t>(p));
    }
    if (offsets) {
      base = offsets[s];
      n = offsets[s + 1] - base;
    } else {
      base = s * a.stride;
      n = a.stride;
    }
    base = base < 0 ? 0 : (base > a.total ? a.total : base);
    n = n < 0 ? 0 : (n > a.total - base ? a.total - base : n);
    if (n > 0x7fffffffll) n = 0x7fffffffll;
  }
  const int c = static_cast<int>(a.first > 0 && n > a.first ? a.first : n);      // the candidates: rows [0, c)
  const int len = c == 0 ? 0 : (a.rows == SIMAMBA_DS_CHOICE ? K : (K < c ? K : c));

  const KeyedPerm plan = keyed_perm_plan(static_cast<uint32_t>(c));
  const unsigned long long rs = ds_stream(a.rows == SIMAMBA_DS_CHOICE ? SIMAMBA_DS_STREAM_CHOICE : SIMAMBA_DS_STREAM_ROWS,
                                          epoch, p);       // p < S < 2^31 wherever len > 0
  const uint32_t rs_lo = static_cast<uint32_t>(rs), rs_hi = static_cast<uint32_t>(rs >> 32);

  float x[kDsPerLane], y[kDsPerLane], z[kDsPerLane];
  int pl[kDsPerLane];
#pragma unroll
  for (int j = 0; j < kDsPerLane; ++j) {
    const int i = tid + j * T;
    x[j] = y[j] = z[j] = 0.f;
    pl[j] = -1;
    if (i < len) {
      uint32_t r = static_cast<uint32_t>(i);
      if (a.rows == SIMAMBA_DS_PERMUTE) {
        r = keyed_perm(plan, k0, k1, rs_lo, rs_hi, r);
      } else if (a.rows == SIMAMBA_DS_CHOICE) {
        const uint32_t w = philox4x32_10(k0, k1, r, kPermDomain, rs_lo, rs_hi).w[0];
        r = static_cast<uint32_t>((static_cast<uint64_t>(w) * static_cast<uint32_t>(c)) >> 32);
      }
      const long long row = base + r;                                // r < c <= n, base + n <= total
      const float* q = points + row * 3;
      x[j] = q[0];
      y[j] = q[1];
      z[j] = q[2];
      if (point_labels) pl[j] = point_labels[row];
    }
  }

  if (a.norm == SIMAMBA_DS_UNIT_SPHERE && len > 0) {                 // uniform over the workgroup
    // relative to row 0 (lane 0's first row): coinciding rows become exact zeros, and the mean loses no bits to an offset
    if (tid == 0) {
      sFirst[0] = x[0];
      sFirst[1] = y[0];
      sFirst[2] = z[0];
    }
    __syncthreads();
    unsigned valid = 0;
#pragma unroll
    for (int j = 0; j < kDsPerLane; ++j) valid |= (tid + j * T < len ? 1u : 0u) << j;
    unit_sphere_rows(x, y, z, valid, len, sFirst[0], sFirst[1], sFirst[2], sRed, lane, wave, waves);
  }

#pragma unroll
  for (int j = 0; j < kDsPerLane; ++j) {
    const int i = tid + j * T;
    if (i < K) {
      float* q = out + (b * K + i) * 3;
      const bool valid = i < len;
      q[0] = valid ? x[j] : 0.f;
      q[1] = valid ? y[j] : 0.f;
      q[2] = valid ? z[j] : 0.f;
      if (point_label_out) point_label_out[b * K + i] = valid ? pl[j] : -1;
    }
  }
  if (tid == 0) {
    index_out[b] = s;
    lengths_out[b] = len;
    if (label_out) label_out[b] = (s >= 0 && labels) ? labels[s] : -1;
  }
}

__global__ void dataset_step_kernel(long long* state) {
  state[1] = static_cast<long long>(static_cast<unsigned long long>(state[1]) + 1ull);
}

static int ds_threads(int K) {
  const int t = (K + 63) / 64 * 64;
  return t > kDsMaxThreads ? kDsMaxThreads : t;
}

}  // namespace simamba

using namespace simamba;

extern "C" int simamba_dataset_fetch(const float* points, const long long* offsets, const long long* labels,
                                     const int* point_labels, long long* state, float* out, long long* label_out,
                                     int* point_label_out, long long* index_out, int* lengths_out, long long total,
                                     long long S, long long stride, long long B, int K, int first,
                                     long long steps_per_epoch, int rank, int world, int order, int rows, int norm,
                                     void* stream) {
  if (S < 1 || S > 0x7fffffffll || B < 1 || B > 0x7fffffffll || K < 1 || K > kDsMaxPoints || world < 1 || rank < 0 ||
      rank >= world || steps_per_epoch < 1 || first < 0 || total < 0)
    return SIMAMBA_E_SHAPE;
  if (!offsets && (stride < 1 || stride > total / S)) return SIMAMBA_E_SHAPE;
  // the global position of a slot, (pos B + b) world + rank, stays below 2^62
  if (static_cast<unsigned __int128>(steps_per_epoch) * static_cast<unsigned long long>(B) *
          static_cast<unsigned>(world) > (1ull << 62))
    return SIMAMBA_E_SHAPE;
  if (!points || !state || !out || !index_out || !lengths_out) return SIMAMBA_E_NULLPTR;
  if ((order != SIMAMBA_DS_SEQUENTIAL && order != SIMAMBA_DS_SHUFFLE) ||
      (rows != SIMAMBA_DS_FIRST && rows != SIMAMBA_DS_PERMUTE && rows != SIMAMBA_DS_CHOICE) ||
      (norm != SIMAMBA_DS_NONE && norm != SIMAMBA_DS_UNIT_SPHERE))
    return SIMAMBA_E_VARIANT;
  const DsArgs a{total, S, offsets ? 0 : stride, steps_per_epoch, K, first, rank, world, order, rows, norm};
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(dataset_fetch_kernel, dim3(static_cast<unsigned>(B)), dim3(ds_threads(K)), 0, st, points, offsets,
                     labels, point_labels, state, out, label_out, point_label_out, index_out, lengths_out, a);
  if (const hipError_t e = hipGetLastError()) return static_cast<int>(e);
  hipLaunchKernelGGL(dataset_step_kernel, dim3(1), dim3(1), 0, st, state);
  return static_cast<int>(hipGetLastError());
}

extern "C" int simamba_keyed_perm(long long seed, long long tweak, long long n, long long first, long long count,
                                  long long* out) {
  if (n < 1 || n > 0x7fffffffll || first < 0 || count < 0 || first > n || count > n - first) return SIMAMBA_E_SHAPE;
  if (count > 0 && !out) return SIMAMBA_E_NULLPTR;
  const unsigned long long s = static_cast<unsigned long long>(seed), t = static_cast<unsigned long long>(tweak);
  const KeyedPerm plan = keyed_perm_plan(static_cast<uint32_t>(n));
  for (long long i = 0; i < count; ++i)
    out[i] = keyed_perm(plan, static_cast<uint32_t>(s), static_cast<uint32_t>(s >> 32), static_cast<uint32_t>(t),
                        static_cast<uint32_t>(t >> 32), static_cast<uint32_t>(first + i));
  return SIMAMBA_OK;
}
