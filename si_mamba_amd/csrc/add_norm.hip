// Fused (DropPath-scaled) residual add + LayerNorm, forward and backward, for gfx950.
//
// Replaces, inside the reference's Block.forward (models/block.py:56-60) and the final norm of MixerModel
// (models/point_mamba.py:257-258), the chain  drop_path(h) -> + residual -> LayerNorm  (4 torch launches
// reading/writing ~700 MB per block forward at the model shape, ~1 GB backward) by one streaming pass each
// way: forward reads h, residual and writes residual_out, normed (4 row-sized tensors), backward reads
// dnormed, dresidual_out, residual_out and writes dresidual (+ dhidden when DropPath rescales it).
// One wave per row; the row sits in registers as 16-byte chunks (dim <= 2048, dim % 4 == 0); mean / variance
// and the two backward projections are wave all-reduces; the LayerNorm weight/bias gradients are accumulated
// per lane across the rows a wave walks, summed over the workgroup's 4 waves in LDS and written as one
// partial row per workgroup (summed by the caller -- deterministic, no atomics).
// HBM-bound: 4*R*dim*s bytes forward, 4-5 * R*dim*s backward (R = batch * rows_per_batch).
//
// kRms (SIMAMBA_NORM_RMS): RMSNorm in place of LayerNorm -- mamba-ssm's RMSNorm, which the reference's create_block /
// MixerModel take for rms_norm=True (models/point_mamba.py:164, :227):  rstd = rsqrt(mean(x^2) + eps),
// normed = x * rstd * w, no mean, no bias; backward with x^ = x * rstd, g = dnormed * w:
// dx = rstd * (g - x^ * mean(g * x^)), dw = sum_rows dnormed * x^.  Same bytes each way; `mean` is neither read nor
// written and the partial rows' dbias half is left as it is.
//
// Slot maps (the *_slots entry points): `hidden` / `dhidden` and `normed` / `dnormed` may hold only some of the batch's
// samples, packed.  hidden_slot[b] / normed_slot[b] is sample b's index inside the compact tensor or -1.  A sample
// without hidden rows takes residual_out = residual (what hidden * 0 + residual gives) and gets no dhidden; a sample
// without normed rows gets no normed store and no statistics forward, and backward its dx is dresidual_out alone: its
// residual_out, mean, rstd and dnormed are not read and it adds nothing to the weight / bias partials (what a zero
// dnormed adds).  The row walk, the grid and with them the accumulation order of the partials are those of the full
// batch; both lookups are one wave-uniform load per row.  A slot outside [0, compact batch) counts as -1.
#include "common.h"

namespace simamba {

constexpr int kLnThreads = 256;
constexpr int kLnMaxChunks = 8;   // 16-byte chunks per lane: dim <= 64 * 4 * 8

struct LnArgs {
  const void* hidden;
  const float* residual;
  const float* rowscale;
  const float* weight;
  const float* bias;
  float* residual_out;
  void* normed;
  float* mean;
  float* rstd;
  // backward
  const void* dnormed;
  const float* dresidual_out;
  float* dresidual;
  void* dhidden;
  float* dwb_partial;   // (gridDim.x, 2, dim)
  // compact batches: (batch) sample -> index inside hidden / dhidden (normed / dnormed), -1 = none; null = identity
  const int* hidden_slot;
  const int* normed_slot;
  int hidden_batch, normed_batch;
  int batch, rows_per_batch, dim;
  float eps;
};

template <typename T>
__device__ __forceinline__ float4 ld4(const T* p) {
  const Pack<T, 4> pk = *reinterpret_cast<const Pack<T, 4>*>(p);
  return make_float4(to_f32<T>(pk.v[0]), to_f32<T>(pk.v[1]), to_f32<T>(pk.v[2]), to_f32<T>(pk.v[3]));
}
template <typename T>
__device__ __forceinline__ void st4(T* p, float4 v) {
  Pack<T, 4> pk;
  pk.v[0] = from_f32<T>(v.x); pk.v[1] = from_f32<T>(v.y); pk.v[2] = from_f32<T>(v.z); pk.v[3] = from_f32<T>(v.w);
  *reinterpret_cast<Pack<T, 4>*>(p) = pk;
}

// Sample `b`'s index inside a compact tensor of `count` samples (wave-uniform: one scalar load), -1 for none.
__device__ __forceinline__ int ln_slot(const int* __restrict__ map, int b, int count) {
  if (!map) return b;
  const int s = __builtin_amdgcn_readfirstlane(map[b]);
  return (s >= 0 && s < count) ? s : -1;
}

// Where one row's hidden / normed live.  The kernels look a row's slots up one iteration ahead: a wave has one row in
// flight, so a lookup in front of the row's loads (their addresses depend on it) would add its latency to every row.
struct LnRow {
  int b, hs, os;
};
__device__ __forceinline__ LnRow ln_row(const LnArgs& p, int row) {
  LnRow r;
  r.b = __builtin_amdgcn_readfirstlane(row / p.rows_per_batch);
  r.hs = ln_slot(p.hidden_slot, r.b, p.hidden_batch);
  r.os = ln_slot(p.normed_slot, r.b, p.normed_batch);
  return r;
}

// One body serves both forms (`slots`, uniform over the launch): a mapped row and a whole-batch row run the same
// instructions, which is what makes the two bitwise equal -- two instantiations would be free to contract their
// multiply-adds differently.
template <typename TH, typename TO, int kChunks, bool kRms>
__global__ __launch_bounds__(kLnThreads) void add_ln_fwd_kernel(LnArgs p) {
  const bool slots = p.hidden_slot || p.normed_slot;
  const int lane = threadIdx.x & 63;
  const int wave_global = (blockIdx.x * kLnThreads + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * kLnThreads) >> 6;
  const int rows = p.batch * p.rows_per_batch;
  const int nch = p.dim >> 2;
  const TH* __restrict__ hg = static_cast<const TH*>(p.hidden);
  TO* __restrict__ og = static_cast<TO*>(p.normed);
  float4 w[kChunks], bs[kChunks];
#pragma unroll
  for (int k = 0; k < kChunks; ++k) {
    const int c = lane + 64 * k;
    w[k] = c < nch ? *reinterpret_cast<const float4*>(p.weight + 4 * c) : make_float4(0, 0, 0, 0);
    bs[k] = (!kRms && c < nch && p.bias) ? *reinterpret_cast<const float4*>(p.bias + 4 * c) : make_float4(0, 0, 0, 0);
  }
  const float inv_dim = 1.f / p.dim;
  LnRow next = (slots && wave_global < rows) ? ln_row(p, wave_global) : LnRow{0, 0, 0};
  for (int row = wave_global; row < rows; row += nwaves) {
    const size_t base = static_cast<size_t>(row) * p.dim;
    const float scale = (p.rowscale && p.residual) ? p.rowscale[row / p.rows_per_batch] : 1.f;
    // where this row's hidden / normed live (compact batches); the whole-batch kernel keeps `base` for both
    size_t hbase = base, obase = base;
    bool has_h = true, has_o = true;
    if (slots) {
      const LnRow cur = next;
      const int ahead = row + nwaves;
      next = ln_row(p, ahead < rows ? ahead : row);
      const int r = __builtin_amdgcn_readfirstlane(row) - cur.b * p.rows_per_batch;
      has_h = cur.hs >= 0; has_o = cur.os >= 0;
      hbase = (static_cast<size_t>(has_h ? cur.hs : 0) * p.rows_per_batch + r) * p.dim;
      obase = (static_cast<size_t>(has_o ? cur.os : 0) * p.rows_per_batch + r) * p.dim;
    }
    float4 x[kChunks];
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < kChunks; ++k) {
      const int c = lane + 64 * k;
      if (c < nch) {
        float4 h;
        if (!has_h) {                           // no hidden rows (the host requires a residual then)
          h = *reinterpret_cast<const float4*>(p.residual + base + 4 * c);
        } else {
          h = ld4<TH>(hg + hbase + 4 * c);
          if (p.residual) {
            const float4 r = *reinterpret_cast<const float4*>(p.residual + base + 4 * c);
            h.x = fmaf(h.x, scale, r.x); h.y = fmaf(h.y, scale, r.y);
            h.z = fmaf(h.z, scale, r.z); h.w = fmaf(h.w, scale, r.w);
          }
        }
        if (p.residual_out) *reinterpret_cast<float4*>(p.residual_out + base + 4 * c) = h;
        x[k] = h;
        sum += (h.x + h.y) + (h.z + h.w);
      } else {
        x[k] = make_float4(0, 0, 0, 0);
      }
    }
    if (!has_o) continue;                                 // nobody reads this row's normed, mean or rstd
    // RMS: the constant 0 folds away (x - 0.f == x) and with it the row sum and its all-reduce
    const float mean = kRms ? 0.f : wave_allreduce_sum(sum) * inv_dim;
    float sq = 0.f;
#pragma unroll
    for (int k = 0; k < kChunks; ++k) {
      if (lane + 64 * k < nch) {
        const float a = x[k].x - mean, b = x[k].y - mean, c = x[k].z - mean, d = x[k].w - mean;
        sq += (a * a + b * b) + (c * c + d * d);
      }
    }
    const float rstd = rsqrtf(wave_allreduce_sum(sq) * inv_dim + p.eps);
#pragma unroll
    for (int k = 0; k < kChunks; ++k) {
      const int c = lane + 64 * k;
      if (c < nch) {
        float4 y;
        y.x = fmaf((x[k].x - mean) * rstd, w[k].x, bs[k].x);
        y.y = fmaf((x[k].y - mean) * rstd, w[k].y, bs[k].y);
        y.z = fmaf((x[k].z - mean) * rstd, w[k].z, bs[k].z);
        y.w = fmaf((x[k].w - mean) * rstd, w[k].w, bs[k].w);
        st4<TO>(og + obase + 4 * c, y);
      }
    }
    if (lane == 0) {
      if (!kRms) p.mean[row] = mean;
      p.rstd[row] = rstd;
    }
  }
}

template <typename TH, typename TO, int kChunks, bool kRms>
__global__ __launch_bounds__(kLnThreads) void add_ln_bwd_kernel(LnArgs p) {
  const bool slots = p.hidden_slot || p.normed_slot;
  extern __shared__ float sred[];          // [4 waves][2][dim]
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wave_global = (blockIdx.x * kLnThreads + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * kLnThreads) >> 6;
  const int rows = p.batch * p.rows_per_batch;
  const int nch = p.dim >> 2;
  const TO* __restrict__ dyg = static_cast<const TO*>(p.dnormed);
  TH* __restrict__ dhg = static_cast<TH*>(p.dhidden);
  float4 w[kChunks], dw[kChunks], db[kChunks];
#pragma unroll
  for (int k = 0; k < kChunks; ++k) {
    const int c = lane + 64 * k;
    w[k] = c < nch ? *reinterpret_cast<const float4*>(p.weight + 4 * c) : make_float4(0, 0, 0, 0);
    dw[k] = make_float4(0, 0, 0, 0);
    db[k] = make_float4(0, 0, 0, 0);
  }
  const float inv_dim = 1.f / p.dim;
  LnRow next = (slots && wave_global < rows) ? ln_row(p, wave_global) : LnRow{0, 0, 0};
  for (int row = wave_global; row < rows; row += nwaves) {
    const size_t base = static_cast<size_t>(row) * p.dim;
    // where this row's hidden / normed live (compact batches); the whole-batch kernel keeps `base` for both
    size_t hbase = base, obase = base;
    bool has_h = true, has_o = true;
    if (slots) {
      const LnRow cur = next;
      const int ahead = row + nwaves;
      next = ln_row(p, ahead < rows ? ahead : row);
      const int r = __builtin_amdgcn_readfirstlane(row) - cur.b * p.rows_per_batch;
      has_h = cur.hs >= 0; has_o = cur.os >= 0;
      hbase = (static_cast<size_t>(has_h ? cur.hs : 0) * p.rows_per_batch + r) * p.dim;
      obase = (static_cast<size_t>(has_o ? cur.os : 0) * p.rows_per_batch + r) * p.dim;
    }
    if (!has_o) {
      // no dnormed for this row: dx = dresidual_out (0 without one); residual_out, mean, rstd are not read and the
      // weight / bias partials get nothing
      const float scale = (p.rowscale && dhg) ? p.rowscale[row / p.rows_per_batch] : 1.f;
#pragma unroll
      for (int k = 0; k < kChunks; ++k) {
        const int c = lane + 64 * k;
        if (c < nch) {
          const float4 dx = p.dresidual_out ? *reinterpret_cast<const float4*>(p.dresidual_out + base + 4 * c)
                                            : make_float4(0, 0, 0, 0);
          if (p.dresidual) *reinterpret_cast<float4*>(p.dresidual + base + 4 * c) = dx;
          if (dhg && has_h)
            st4<TH>(dhg + hbase + 4 * c, make_float4(dx.x * scale, dx.y * scale, dx.z * scale, dx.w * scale));
        }
      }
      continue;
    }
    const float mean = kRms ? 0.f : p.mean[row], rstd = p.rstd[row];
    float4 xh[kChunks], g[kChunks];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < kChunks; ++k) {
      const int c = lane + 64 * k;
      if (c < nch) {
        const float4 x = *reinterpret_cast<const float4*>(p.residual_out + base + 4 * c);
        const float4 dy = ld4<TO>(dyg + obase + 4 * c);
        xh[k] = make_float4((x.x - mean) * rstd, (x.y - mean) * rstd, (x.z - mean) * rstd, (x.w - mean) * rstd);
        g[k] = make_float4(dy.x * w[k].x, dy.y * w[k].y, dy.z * w[k].z, dy.w * w[k].w);
        dw[k].x = fmaf(dy.x, xh[k].x, dw[k].x); dw[k].y = fmaf(dy.y, xh[k].y, dw[k].y);
        dw[k].z = fmaf(dy.z, xh[k].z, dw[k].z); dw[k].w = fmaf(dy.w, xh[k].w, dw[k].w);
        db[k].x += dy.x; db[k].y += dy.y; db[k].z += dy.z; db[k].w += dy.w;
        s1 += (g[k].x + g[k].y) + (g[k].z + g[k].w);
        s2 += (g[k].x * xh[k].x + g[k].y * xh[k].y) + (g[k].z * xh[k].z + g[k].w * xh[k].w);
      } else {
        xh[k] = make_float4(0, 0, 0, 0);
        g[k] = make_float4(0, 0, 0, 0);
      }
    }
    const float c1 = kRms ? 0.f : wave_allreduce_sum(s1) * inv_dim;     // RMS: no -mean(g) term
    const float c2 = wave_allreduce_sum(s2) * inv_dim;
    const float scale = (p.rowscale && dhg) ? p.rowscale[row / p.rows_per_batch] : 1.f;
#pragma unroll
    for (int k = 0; k < kChunks; ++k) {
      const int c = lane + 64 * k;
      if (c < nch) {
        float4 dx;
        dx.x = (g[k].x - c1 - xh[k].x * c2) * rstd;
        dx.y = (g[k].y - c1 - xh[k].y * c2) * rstd;
        dx.z = (g[k].z - c1 - xh[k].z * c2) * rstd;
        dx.w = (g[k].w - c1 - xh[k].w * c2) * rstd;
        if (p.dresidual_out) {
          const float4 r = *reinterpret_cast<const float4*>(p.dresidual_out + base + 4 * c);
          dx.x += r.x; dx.y += r.y; dx.z += r.z; dx.w += r.w;
        }
        if (p.dresidual) *reinterpret_cast<float4*>(p.dresidual + base + 4 * c) = dx;
        if (dhg && has_h)
          st4<TH>(dhg + hbase + 4 * c, make_float4(dx.x * scale, dx.y * scale, dx.z * scale, dx.w * scale));
      }
    }
  }
  // weight / bias gradients: lanes -> LDS per wave -> sum over the 4 waves -> one partial row per workgroup
  // (RMS: the weight half only)
  float* mine = sred + wave * 2 * p.dim;
#pragma unroll
  for (int k = 0; k < kChunks; ++k) {
    const int c = lane + 64 * k;
    if (c < nch) {
      *reinterpret_cast<float4*>(mine + 4 * c) = dw[k];
      if (!kRms) *reinterpret_cast<float4*>(mine + p.dim + 4 * c) = db[k];
    }
  }
  __syncthreads();
  float* out = p.dwb_partial + static_cast<size_t>(blockIdx.x) * 2 * p.dim;
  for (int i = threadIdx.x; i < (kRms ? 1 : 2) * p.dim; i += kLnThreads) {
    float v = 0.f;
#pragma unroll
    for (int wv = 0; wv < kLnThreads / 64; ++wv) v += sred[wv * 2 * p.dim + i];
    out[i] = v;
  }
}

static int ln_grid(int rows) {
  int g = (rows + 3) / 4;            // 4 rows (waves) per workgroup pass
  return g < 1 ? 1 : (g > 1024 ? 1024 : g);
}

template <typename TH, typename TO, bool kRms>
static int launch_ln(const LnArgs& a, bool bwd, int grid, hipStream_t s) {
  const int chunks = ((a.dim >> 2) + 63) / 64;
#define SIMAMBA_LN_CASE(K)                                                                                      \
  if (chunks <= K) {                                                                                             \
    if (bwd)                                                                                                     \
      hipLaunchKernelGGL((add_ln_bwd_kernel<TH, TO, K, kRms>), dim3(grid), dim3(kLnThreads),                     \
                         sizeof(float) * (kLnThreads / 64) * 2 * a.dim, s, a);                                   \
    else                                                                                                         \
      hipLaunchKernelGGL((add_ln_fwd_kernel<TH, TO, K, kRms>), dim3(grid), dim3(kLnThreads), 0, s, a);           \
    return static_cast<int>(hipGetLastError());                                                                  \
  }
  SIMAMBA_LN_CASE(1)
  SIMAMBA_LN_CASE(2)
  SIMAMBA_LN_CASE(4)
  SIMAMBA_LN_CASE(8)
#undef SIMAMBA_LN_CASE
  return SIMAMBA_E_SHAPE;
}

template <typename TH, typename TO>
static int launch_ln(const LnArgs& a, bool bwd, bool rms, int grid, hipStream_t s) {
  return rms ? launch_ln<TH, TO, true>(a, bwd, grid, s) : launch_ln<TH, TO, false>(a, bwd, grid, s);
}

static int dispatch_ln(const LnArgs& a, bool bwd, bool rms, int grid, int hidden_dtype, int out_dtype, hipStream_t s) {
  if (hidden_dtype == SIMAMBA_F32 && out_dtype == SIMAMBA_F32) return launch_ln<float, float>(a, bwd, rms, grid, s);
  if (hidden_dtype == SIMAMBA_BF16 && out_dtype == SIMAMBA_BF16)
    return launch_ln<bf16_t, bf16_t>(a, bwd, rms, grid, s);
  if (hidden_dtype == SIMAMBA_F32 && out_dtype == SIMAMBA_BF16) return launch_ln<float, bf16_t>(a, bwd, rms, grid, s);
  if (hidden_dtype == SIMAMBA_BF16 && out_dtype == SIMAMBA_F32) return launch_ln<bf16_t, float>(a, bwd, rms, grid, s);
  return SIMAMBA_E_DTYPE;
}

}  // namespace simamba

using namespace simamba;

static int check_ln(int batch, int rows_per_batch, int dim) {
  if (batch < 0 || rows_per_batch < 0) return SIMAMBA_E_SHAPE;
  if (dim <= 0 || (dim & 3) || dim > 64 * 4 * kLnMaxChunks) return SIMAMBA_E_SHAPE;
  return SIMAMBA_OK;
}

extern "C" int simamba_add_layer_norm_grid(int batch, int rows_per_batch) {
  const long long rows = static_cast<long long>(batch) * rows_per_batch;
  return ln_grid(rows > 2000000000ll ? 2000000000 : static_cast<int>(rows));
}

// A slot map and its compact batch: null map <=> the tensor holds the whole batch.
static int check_slots(const int* map, int compact_batch, int batch) {
  if (compact_batch < 0 || compact_batch > batch) return SIMAMBA_E_SHAPE;
  if (!map && compact_batch != batch) return SIMAMBA_E_NULLPTR;
  return SIMAMBA_OK;
}

extern "C" int simamba_add_layer_norm_check_slots(const int* slots_host, int batch, int compact_batch) {
  if (batch < 0 || compact_batch < 0 || compact_batch > batch) return SIMAMBA_E_SHAPE;
  if (batch == 0) return SIMAMBA_OK;
  if (!slots_host) return SIMAMBA_E_NULLPTR;
  for (int b = 0; b < batch; ++b) {
    const int s = slots_host[b];
    if (s < -1 || s >= compact_batch) return SIMAMBA_E_SHAPE;
    if (s < 0) continue;
    for (int c = 0; c < b; ++c)
      if (slots_host[c] == s) return SIMAMBA_E_SHAPE;      // two samples in one slot
  }
  return SIMAMBA_OK;
}

extern "C" int simamba_add_layer_norm_fwd_slots(const void* hidden, const float* residual, const float* rowscale,
                                                const float* weight, const float* bias, float* residual_out,
                                                void* normed, float* mean, float* rstd, const int* hidden_slot,
                                                int hidden_batch, const int* normed_slot, int normed_batch, int batch,
                                                int rows_per_batch, int dim, float eps, int hidden_dtype,
                                                int out_dtype, int flags, void* stream) {
  if (flags & ~SIMAMBA_NORM_RMS) return SIMAMBA_E_VARIANT;
  const bool rms = (flags & SIMAMBA_NORM_RMS) != 0;
  if (rms && bias) return SIMAMBA_E_BIAS;
  int rc = check_ln(batch, rows_per_batch, dim);
  if (rc) return rc;
  if (batch == 0 || rows_per_batch == 0) return SIMAMBA_OK;
  if ((rc = check_slots(hidden_slot, hidden_batch, batch))) return rc;
  if ((rc = check_slots(normed_slot, normed_batch, batch))) return rc;
  if ((!hidden && hidden_batch) || !weight || (!normed && normed_batch) || (!mean && !rms) || !rstd)
    return SIMAMBA_E_NULLPTR;
  // a sample without hidden rows takes the residual: there has to be one, and somewhere to put the sum
  if (hidden_slot && (!residual || !residual_out)) return SIMAMBA_E_NULLPTR;
  LnArgs a{};
  a.hidden = hidden; a.residual = residual; a.rowscale = rowscale; a.weight = weight; a.bias = bias;
  a.residual_out = residual_out; a.normed = normed; a.mean = mean; a.rstd = rstd;
  a.hidden_slot = hidden_slot; a.normed_slot = normed_slot; a.hidden_batch = hidden_batch; a.normed_batch = normed_batch;
  a.batch = batch; a.rows_per_batch = rows_per_batch; a.dim = dim; a.eps = eps;
  return dispatch_ln(a, false, rms, simamba_add_layer_norm_grid(batch, rows_per_batch), hidden_dtype, out_dtype,
                     static_cast<hipStream_t>(stream));
}

extern "C" int simamba_add_layer_norm_fwd_ex(const void* hidden, const float* residual, const float* rowscale,
                                             const float* weight, const float* bias, float* residual_out, void* normed,
                                             float* mean, float* rstd, int batch, int rows_per_batch, int dim,
                                             float eps, int hidden_dtype, int out_dtype, int flags, void* stream) {
  return simamba_add_layer_norm_fwd_slots(hidden, residual, rowscale, weight, bias, residual_out, normed, mean, rstd,
                                          nullptr, batch, nullptr, batch, batch, rows_per_batch, dim, eps, hidden_dtype,
                                          out_dtype, flags, stream);
}

extern "C" int simamba_add_layer_norm_fwd(const void* hidden, const float* residual, const float* rowscale,
                                          const float* weight, const float* bias, float* residual_out, void* normed,
                                          float* mean, float* rstd, int batch, int rows_per_batch, int dim, float eps,
                                          int hidden_dtype, int out_dtype, void* stream) {
  return simamba_add_layer_norm_fwd_ex(hidden, residual, rowscale, weight, bias, residual_out, normed, mean, rstd,
                                       batch, rows_per_batch, dim, eps, hidden_dtype, out_dtype, 0, stream);
}

extern "C" int simamba_add_layer_norm_bwd_slots(const void* dnormed, const float* dresidual_out,
                                                const float* residual_out, const float* mean, const float* rstd,
                                                const float* weight, const float* rowscale, float* dresidual,
                                                void* dhidden, float* dwb_partial, const int* hidden_slot,
                                                int hidden_batch, const int* normed_slot, int normed_batch, int batch,
                                                int rows_per_batch, int dim, int hidden_dtype, int out_dtype,
                                                int flags, void* stream) {
  if (flags & ~SIMAMBA_NORM_RMS) return SIMAMBA_E_VARIANT;
  const bool rms = (flags & SIMAMBA_NORM_RMS) != 0;
  int rc = check_ln(batch, rows_per_batch, dim);
  if (rc) return rc;
  if (batch == 0 || rows_per_batch == 0) return SIMAMBA_OK;
  if ((rc = check_slots(hidden_slot, hidden_batch, batch))) return rc;
  if ((rc = check_slots(normed_slot, normed_batch, batch))) return rc;
  // an empty compact dhidden is as good as none; an empty dnormed leaves residual_out, mean and rstd unread
  if (hidden_batch == 0) dhidden = nullptr;
  if ((!dnormed || !residual_out || (!mean && !rms) || !rstd) && normed_batch) return SIMAMBA_E_NULLPTR;
  if (!weight || !dwb_partial || (!dresidual && !dhidden)) return SIMAMBA_E_NULLPTR;
  LnArgs a{};
  a.dnormed = dnormed; a.dresidual_out = dresidual_out; a.residual_out = const_cast<float*>(residual_out);
  a.mean = const_cast<float*>(mean); a.rstd = const_cast<float*>(rstd); a.weight = weight; a.rowscale = rowscale;
  a.dresidual = dresidual; a.dhidden = dhidden; a.dwb_partial = dwb_partial;
  a.hidden_slot = hidden_slot; a.normed_slot = normed_slot; a.hidden_batch = hidden_batch; a.normed_batch = normed_batch;
  a.batch = batch; a.rows_per_batch = rows_per_batch; a.dim = dim;
  return dispatch_ln(a, true, rms, simamba_add_layer_norm_grid(batch, rows_per_batch), hidden_dtype, out_dtype,
                     static_cast<hipStream_t>(stream));
}

extern "C" int simamba_add_layer_norm_bwd_ex(const void* dnormed, const float* dresidual_out,
                                             const float* residual_out, const float* mean, const float* rstd,
                                             const float* weight, const float* rowscale, float* dresidual,
                                             void* dhidden, float* dwb_partial, int batch, int rows_per_batch, int dim,
                                             int hidden_dtype, int out_dtype, int flags, void* stream) {
  return simamba_add_layer_norm_bwd_slots(dnormed, dresidual_out, residual_out, mean, rstd, weight, rowscale, dresidual,
                                          dhidden, dwb_partial, nullptr, batch, nullptr, batch, batch, rows_per_batch,
                                          dim, hidden_dtype, out_dtype, flags, stream);
}

extern "C" int simamba_add_layer_norm_bwd(const void* dnormed, const float* dresidual_out, const float* residual_out,
                                          const float* mean, const float* rstd, const float* weight,
                                          const float* rowscale, float* dresidual, void* dhidden, float* dwb_partial,
                                          int batch, int rows_per_batch, int dim, int hidden_dtype, int out_dtype,
                                          void* stream) {
  return simamba_add_layer_norm_bwd_ex(dnormed, dresidual_out, residual_out, mean, rstd, weight, rowscale, dresidual,
                                       dhidden, dwb_partial, batch, rows_per_batch, dim, hidden_dtype, out_dtype, 0,
                                       stream);
}
