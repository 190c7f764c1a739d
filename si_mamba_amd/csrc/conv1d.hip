// Causal depthwise conv1d (+SiLU), forward and backward, for gfx950.
//
// Replaces causal_conv1d_cuda.causal_conv1d_{fwd,bwd} of causal-conv1d as used inside the mixer
// the reference calls at models/block.py:72.  Pure streaming op: every lane owns 4 consecutive
// timesteps of one (batch, channel) row (one 16-byte access for fp32), the 3-step halo comes
// from the neighbouring pack (an L1/L2 hit).  A workgroup owns a tile of channels and walks a
// slice of the batch, so the weight-gradient reduction over (batch, time) happens in registers,
// then over the 16-lane DPP row, then in LDS, and only one atomic per (channel, tap) and
// workgroup reaches HBM.
// Deterministic form (kDet, SIMAMBA_BWD_DETERMINISTIC): the 16-lane rows park their sums in LDS slots of their own, one
// thread per (channel, tap) adds a channel's slots in index order, and the workgroup STORES that partial to the
// workspace, [batch slice][dim][width] (dw) and [batch slice][dim] (dbias); det_reduce.hip sums over the slices.
// Algorithmic HBM bytes: fwd 2*B*D*L*s, bwd 3*B*D*L*s (+ (W+1)*D*4 parameters).
//
// What is stated once: the tap chain (conv_pre) and the backward of a pack (conv_bwd_pack) in conv_device.h -- the
// forward here, the conv fused into xdt_proj*.hip and the recompute of both backward kernels go through the former, both
// backward kernels through the latter; a lane's row / pack ownership (conv_lane) for all three kernels; the launch
// geometry (conv_geom) for both entry points and the workspace query.  A fusion into the backward hooks into
// conv_bwd_pack.
#include <algorithm>
#include <initializer_list>

#include "host_common.h"
#include "mfma_device.h"
#include "conv_device.h"
#include "det_reduce.h"

namespace simamba {

constexpr int kConvThreads = 256;
constexpr int kPack = 4;

struct ConvArgs {
  const void* x;
  const float* w;
  const float* bias;
  void* out;       // fwd: out ; bwd: dx
  const void* dout;
  float* dw;
  float* dbias;
  int batch, dim, seqlen, width;
  int silu;
  int vec;
  int ppr;         // padded packs per row (power of two, >= 16)
  int bchunk;      // batch samples per workgroup
  long long x_bs;  // batch stride (elements) of x
  long long o_bs;  // batch stride (elements) of out (fwd: contiguous) / dx (bwd)
};

template <typename T, int P = kPack>
__device__ __forceinline__ void load_pack(const T* row, int t0, int L, bool vec, float (&v)[P]) {
  if (t0 < 0 || t0 >= L) {
#pragma unroll
    for (int j = 0; j < P; ++j) v[j] = 0.f;
    return;
  }
  load_items<T, P>(row + t0, L - t0, vec, v);
}

__device__ __forceinline__ void load_taps(const ConvArgs& p, int d, float (&w4)[4], float& bias) {
  const int W = p.width;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int k = j - (4 - W);
    w4[j] = (k >= 0) ? p.w[d * W + k] : 0.f;
  }
  bias = p.bias ? p.bias[d] : 0.f;
}

// What a lane owns.  A row of ppr packs takes ppr lanes, so a workgroup holds rows_per_blk channels (lane -> row drow
// of the workgroup, channel d) and the lanes of a row walk its packs from pk0 in steps of pstride; a row of 256 packs
// or more takes the whole workgroup.
struct ConvLane {
  int ppr, rows_per_blk, drow, d;
  // (functions, not fields: worked out where the pack loop starts, which the forward's lanes past the last channel
  // never reach)
  __device__ __forceinline__ int pk0() const { return ppr >= kConvThreads ? threadIdx.x : threadIdx.x % ppr; }
  __device__ __forceinline__ int pstride() const { return ppr >= kConvThreads ? kConvThreads : ppr; }
};

__device__ __forceinline__ ConvLane conv_lane(const ConvArgs& p) {
  ConvLane l;
  l.ppr = p.ppr;
  l.rows_per_blk = p.ppr >= kConvThreads ? 1 : kConvThreads / p.ppr;
  l.drow = p.ppr >= kConvThreads ? 0 : threadIdx.x / p.ppr;
  l.d = blockIdx.x * l.rows_per_blk + l.drow;
  return l;
}

template <typename T>
__global__ __launch_bounds__(kConvThreads) void conv1d_fwd_kernel(ConvArgs p) {
  const int L = p.seqlen;
  const ConvLane ln = conv_lane(p);
  const int d = ln.d;
  if (d >= p.dim) return;
  float w4[4], bias;
  load_taps(p, d, w4, bias);
  const T* __restrict__ xg = static_cast<const T*>(p.x);
  T* __restrict__ og = static_cast<T*>(p.out);
  const int b0 = blockIdx.y * p.bchunk;
  const int b1 = min(b0 + p.bchunk, p.batch);
  const bool vec = p.vec != 0;
  for (int b = b0; b < b1; ++b) {
    const T* row = xg + static_cast<size_t>(b) * p.x_bs + static_cast<size_t>(d) * L;
    T* orow = og + static_cast<size_t>(b) * p.o_bs + static_cast<size_t>(d) * L;
    for (int pk = ln.pk0(); pk * kPack < L; pk += ln.pstride()) {
      const int t0 = pk * kPack;
      float xp[kPack], xc[kPack], o[kPack];
      load_pack<T>(row, t0 - kPack, L, vec, xp);
      load_pack<T>(row, t0, L, vec, xc);
      const float win[7] = {xp[1], xp[2], xp[3], xc[0], xc[1], xc[2], xc[3]};
#pragma unroll
      for (int i = 0; i < kPack; ++i) {
        const float acc = conv_pre(w4, win + i, bias);
        o[i] = p.silu ? acc * sigmoid_f(acc) : acc;
      }
      store_items<T, kPack>(orow + t0, L - t0, vec, o);
    }
  }
}

template <bool kDet = false>
__device__ __forceinline__ void conv_bwd_reduce(const ConvArgs& p, float (&sacc)[16][5], float (&gw)[4], float gb, int drow,
                                                int rows_per_blk, bool dvalid) {
  // 16-lane rows never straddle channels (ppr is a multiple of 16)
#pragma unroll
  for (int j = 0; j < 4; ++j) gw[j] = row_allreduce_sum(gw[j]);
  gb = row_allreduce_sum(gb);
  if (kDet) {
    // sacc[16-lane row][tap]: a slot per row, no atomics; channel r owns rows r * rpc .. r * rpc + rpc - 1
    const int q = threadIdx.x >> 4, rpc = 16 / rows_per_blk;
    if ((threadIdx.x & 15) == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) sacc[q][j] = gw[j];
      sacc[q][4] = gb;
    }
    __syncthreads();
    if (threadIdx.x < rows_per_blk * 5) {
      const int r = threadIdx.x / 5, j = threadIdx.x % 5;
      const int dd = blockIdx.x * rows_per_blk + r;
      if (dd < p.dim) {
        float v = 0.f;
        for (int i = 0; i < rpc; ++i) v += sacc[r * rpc + i][j];
        if (j < 4) {
          const int k = j - (4 - p.width);
          if (k >= 0) p.dw[(static_cast<size_t>(blockIdx.y) * p.dim + dd) * p.width + k] = v;
        } else if (p.dbias) {
          p.dbias[static_cast<size_t>(blockIdx.y) * p.dim + dd] = v;
        }
      }
    }
    return;
  }
  if ((threadIdx.x & 15) == 0 && dvalid) {
#pragma unroll
    for (int j = 0; j < 4; ++j) atomicAdd(&sacc[drow][j], gw[j]);
    atomicAdd(&sacc[drow][4], gb);
  }
  __syncthreads();
  if (threadIdx.x < rows_per_blk * 5) {
    const int r = threadIdx.x / 5, j = threadIdx.x % 5;
    const int dd = blockIdx.x * rows_per_blk + r;
    if (dd < p.dim) {
      const float v = sacc[r][j];
      if (j < 4) {
        const int k = j - (4 - p.width);
        if (k >= 0) atomicAdd(&p.dw[dd * p.width + k], v);
      } else if (p.dbias) {
        atomicAdd(&p.dbias[dd], v);
      }
    }
  }
}

// Backward.  The two kernels differ only in how a pack's operands reach registers; the pack's arithmetic is
// conv_bwd_pack (conv_device.h) and the reduction conv_bwd_reduce in both.
// P: timesteps per lane and step -- one 16-byte access: 4 for fp32, 8 for bf16 (with 4 the bf16 kernel issued twice the
// loads and recomputed 7 SiLU derivatives per 4 outputs instead of 11 per 8: 120 us where its bytes take 55)
template <typename T, int P, bool kDet = false>
__global__ __launch_bounds__(kConvThreads) void conv1d_bwd_kernel(ConvArgs p) {
  __shared__ float sacc[16][5];   // up to 16 channels per workgroup x (4 taps + bias)
  const int L = p.seqlen, D = p.dim;
  const ConvLane ln = conv_lane(p);
  const bool dvalid = ln.d < D;
  const int dc = dvalid ? ln.d : D - 1;
  if (threadIdx.x < 16 * 5) (&sacc[0][0])[threadIdx.x] = 0.f;
  __syncthreads();
  float w4[4], bias;
  load_taps(p, dc, w4, bias);
  const T* __restrict__ xg = static_cast<const T*>(p.x);
  const T* __restrict__ gg = static_cast<const T*>(p.dout);
  T* __restrict__ dxg = static_cast<T*>(p.out);
  const int b0 = blockIdx.y * p.bchunk;
  const int b1 = min(b0 + p.bchunk, p.batch);
  const bool vec = p.vec != 0;
  float gw[4] = {0.f, 0.f, 0.f, 0.f}, gb = 0.f;
  for (int b = b0; b < b1; ++b) {
    const size_t roff = (static_cast<size_t>(b) * D + dc) * L;                      // dout: contiguous
    const size_t xoff = static_cast<size_t>(b) * p.x_bs + static_cast<size_t>(dc) * L;
    const size_t doff = static_cast<size_t>(b) * p.o_bs + static_cast<size_t>(dc) * L;
    for (int pk = ln.pk0(); pk * P < L; pk += ln.pstride()) {
      const int t0 = pk * P;
      float xp[P], xc[P], xn[P], gc[P], gn[P];
      load_pack<T, P>(xg + xoff, t0 - P, L, vec, xp);
      load_pack<T, P>(xg + xoff, t0, L, vec, xc);
      load_pack<T, P>(xg + xoff, t0 + P, L, vec, xn);
      load_pack<T, P>(gg + roff, t0, L, vec, gc);
      load_pack<T, P>(gg + roff, t0 + P, L, vec, gn);
      // x[t0-3 .. t0+P+2], dout[t0 .. t0+P+2]
      float xw[P + 6], gv[P + 3];
#pragma unroll
      for (int i = 0; i < 3; ++i) { xw[i] = xp[P - 3 + i]; xw[P + 3 + i] = xn[i]; gv[P + i] = gn[i]; }
#pragma unroll
      for (int i = 0; i < P; ++i) { xw[3 + i] = xc[i]; gv[i] = gc[i]; }
      float dx[P];
      conv_bwd_pack<P, true>(w4, bias, p.silu, xw, gv, L - t0, dx, gw, gb);
      if (dvalid) store_items<T, P>(dxg + doff + t0, L - t0, vec, dx);
    }
  }
  conv_bwd_reduce<kDet>(p, sacc, gw, gb, ln.drow, ln.rows_per_blk, dvalid);
}

// ---- the aligned case (every pack one whole 16-byte access, L % P == 0): same arithmetic, software-pipelined ----------
// One (sample, pack) per iteration; the five raw packs of the NEXT iteration are requested before this one's arithmetic,
// so a wave has two iterations of loads in flight instead of stalling a full HBM latency per sample (the loop above:
// 103 us in bf16 where the bytes take 55).  Neighbouring packs are loaded from clamped addresses and zeroed by select:
// a load under a condition would hold the pipeline's registers live across both arms.
template <typename T, int P>
__device__ __forceinline__ void unpack16(const uint4& r, float (&v)[P]) {
  if constexpr (sizeof(T) == 4) {
    v[0] = __builtin_bit_cast(float, r.x); v[1] = __builtin_bit_cast(float, r.y);
    v[2] = __builtin_bit_cast(float, r.z); v[3] = __builtin_bit_cast(float, r.w);
  } else {
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = bf16_lo(w[i]);
      v[2 * i + 1] = bf16_hi(w[i]);
    }
  }
}

template <typename T, int P, bool kDet = false>
__global__ __launch_bounds__(kConvThreads) void conv1d_bwd_fast_kernel(ConvArgs p) {
  static_assert(sizeof(T) * P == 16, "one 16-byte access per pack");
  __shared__ float sacc[16][5];
  const int L = p.seqlen, D = p.dim;
  const ConvLane ln = conv_lane(p);
  const bool dvalid = ln.d < D;
  const int dc = dvalid ? ln.d : D - 1;
  if (threadIdx.x < 16 * 5) (&sacc[0][0])[threadIdx.x] = 0.f;
  __syncthreads();
  float w4[4], bias;
  load_taps(p, dc, w4, bias);
  const T* __restrict__ xg = static_cast<const T*>(p.x);
  const T* __restrict__ gg = static_cast<const T*>(p.dout);
  T* __restrict__ dxg = static_cast<T*>(p.out);
  const int b0 = blockIdx.y * p.bchunk;
  const int nb = min(b0 + p.bchunk, p.batch) - b0;
  const int packs = L / P;
  const int pk0 = ln.pk0(), pstride = ln.pstride();
  const int npk = pk0 < packs ? (packs - pk0 + pstride - 1) / pstride : 0;
  const int n = nb * npk;

  struct Raw { uint4 xp, xc, xn, gc, gn; };
  auto where = [&](int it, int& b, int& t0) {
    const int q = npk == 1 ? it : it / npk;
    b = b0 + q;
    t0 = (pk0 + (it - q * npk) * pstride) * P;
  };
  auto load_raw = [&](int it_) {
    const int it = it_ < n ? it_ : n - 1;                      // unconditional: the step past the end re-reads the last
    int b, t0;
    where(it, b, t0);
    const T* xr = xg + static_cast<size_t>(b) * p.x_bs + static_cast<size_t>(dc) * L;
    const T* gr = gg + (static_cast<size_t>(b) * D + dc) * L;
    const int tp = t0 >= P ? t0 - P : 0, tn = t0 + P < L ? t0 + P : t0;
    Raw r;
    r.xp = *reinterpret_cast<const uint4*>(xr + tp);
    r.xc = *reinterpret_cast<const uint4*>(xr + t0);
    r.xn = *reinterpret_cast<const uint4*>(xr + tn);
    r.gc = *reinterpret_cast<const uint4*>(gr + t0);
    r.gn = *reinterpret_cast<const uint4*>(gr + tn);
    return r;
  };

  float gw[4] = {0.f, 0.f, 0.f, 0.f}, gb = 0.f;
  if (n > 0) {
    Raw cur = load_raw(0);
    for (int it = 0; it < n; ++it) {
      const Raw nxt = load_raw(it + 1);
      int b, t0;
      where(it, b, t0);
      float xp[P], xc[P], xn[P], gc[P], gn[P];
      unpack16<T, P>(cur.xp, xp); unpack16<T, P>(cur.xc, xc); unpack16<T, P>(cur.xn, xn);
      unpack16<T, P>(cur.gc, gc); unpack16<T, P>(cur.gn, gn);
      const bool first = t0 == 0, last = t0 + P >= L;
      float xw[P + 6], gv[P + 3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        xw[i] = first ? 0.f : xp[P - 3 + i];
        xw[P + 3 + i] = last ? 0.f : xn[i];
        gv[P + i] = last ? 0.f : gn[i];                         // positions >= L carry gv = 0: no guard below
      }
#pragma unroll
      for (int i = 0; i < P; ++i) { xw[3 + i] = xc[i]; gv[i] = gc[i]; }
      float dx[P];
      conv_bwd_pack<P, false>(w4, bias, p.silu, xw, gv, 0, dx, gw, gb);
      if (dvalid)
        store_items<T, P>(dxg + static_cast<size_t>(b) * p.o_bs + static_cast<size_t>(dc) * L + t0, P, true, dx);
      cur = nxt;
    }
  }
  conv_bwd_reduce<kDet>(p, sacc, gw, gb, ln.drow, ln.rows_per_blk, dvalid);
}

// Launch geometry of a problem; `pack` = timesteps per lane and step (kPack forward, io_pack backward).  A batch stride
// of 0 means contiguous; `ptrs` are the activation pointers whose alignment the 16-byte accesses need (the workspace
// query, which only counts batch slices, passes none).
struct ConvGeom {
  int vec, ppr, bchunk;
  long long x_bs, o_bs;
  dim3 grid;       // (channel blocks, batch slices)
};

static ConvGeom conv_geom(int batch, int dim, int seqlen, int io_dtype, int pack, long long x_bs = 0, long long o_bs = 0,
                          std::initializer_list<const void*> ptrs = {}) {
  ConvGeom g;
  const int packs = (seqlen + pack - 1) / pack;
  g.ppr = 16;
  while (g.ppr < packs && g.ppr < kConvThreads) g.ppr <<= 1;
  const int rows_per_blk = g.ppr >= kConvThreads ? 1 : kConvThreads / g.ppr;
  const int dblocks = (dim + rows_per_blk - 1) / rows_per_blk;
  // enough workgroups to fill 256 CUs several times over, but long batch slices for the reduction
  g.bchunk = batch;
  while (g.bchunk > 1 && static_cast<long long>(dblocks) * ((batch + g.bchunk - 1) / g.bchunk) < 2048)
    g.bchunk = (g.bchunk + 1) / 2;
  g.grid = dim3(dblocks, (batch + g.bchunk - 1) / g.bchunk);
  g.x_bs = x_bs ? x_bs : static_cast<long long>(dim) * seqlen;
  g.o_bs = o_bs ? o_bs : static_cast<long long>(dim) * seqlen;
  const long long esz = io_esz(io_dtype);
  g.vec = (seqlen * esz) % 16 == 0 && (g.x_bs * esz) % 16 == 0 && (g.o_bs * esz) % 16 == 0;
  for (const void* q : ptrs) g.vec = g.vec && aligned16(q);
  return g;
}

template <bool kDet>
static int conv_bwd_launch(const ConvArgs& a, int io_dtype, bool fast, dim3 grid, hipStream_t s) {
  with_io_type(io_dtype, [&](auto tag) {
    using T = decltype(tag);
    constexpr int kP = 16 / sizeof(T);
    const auto kernel = fast ? conv1d_bwd_fast_kernel<T, kP, kDet> : conv1d_bwd_kernel<T, kP, kDet>;
    hipLaunchKernelGGL(kernel, grid, dim3(kConvThreads), 0, s, a);
  });
  return static_cast<int>(hipGetLastError());
}

}  // namespace simamba

using namespace simamba;

static int check_conv(const void* x, const float* w, int batch, int dim, int seqlen, int width, int io_dtype) {
  if (!x || !w) return SIMAMBA_E_NULLPTR;
  if (batch < 0 || dim <= 0 || seqlen < 0) return SIMAMBA_E_SHAPE;
  if (width < 2 || width > 4) return SIMAMBA_E_WIDTH;
  return check_io_dtype(io_dtype);
}

extern "C" int simamba_causal_conv1d_fwd(const void* x, const float* w, const float* bias, void* out,
                                         int batch, int dim, int seqlen, int width, int silu,
                                         int io_dtype, long long x_bstride, void* stream) {
  int rc = check_conv(x, w, batch, dim, seqlen, width, io_dtype);
  if (rc) return rc;
  if (!out) return SIMAMBA_E_NULLPTR;
  if (batch == 0 || seqlen == 0) return SIMAMBA_OK;
  const ConvGeom g = conv_geom(batch, dim, seqlen, io_dtype, kPack, x_bstride, 0, {x, out});
  const ConvArgs a{x, w, bias, out, nullptr, nullptr, nullptr, batch, dim, seqlen, width, silu,
                   g.vec, g.ppr, g.bchunk, g.x_bs, g.o_bs};
  hipStream_t s = static_cast<hipStream_t>(stream);
  with_io_type(io_dtype, [&](auto tag) {
    hipLaunchKernelGGL(conv1d_fwd_kernel<decltype(tag)>, g.grid, dim3(kConvThreads), 0, s, a);
  });
  return static_cast<int>(hipGetLastError());
}

// Deterministic form: workspace of the per-batch-slice partials (det_layout), in floats; the slicing depends on the
// I/O type's pack, the size asked for covers both.
static long long conv_det_dw_floats(long long slices, int dim, int width) {
  return (slices * dim * width + 63) & ~63ll;                 // dbias partials start on a 256-byte boundary
}

extern "C" long long simamba_causal_conv1d_bwd_workspace_floats(int batch, int dim, int seqlen, int width, int flags) {
  if (flags & ~SIMAMBA_BWD_DETERMINISTIC) return SIMAMBA_E_VARIANT;
  if (!flags) return 0;
  if (batch < 0 || dim <= 0 || seqlen < 0) return SIMAMBA_E_SHAPE;
  if (width < 2 || width > 4) return SIMAMBA_E_WIDTH;
  if (batch == 0 || seqlen == 0) return 0;
  long long sl = 0;
  for (int io_dtype : {SIMAMBA_F32, SIMAMBA_BF16})
    sl = std::max<long long>(sl, conv_geom(batch, dim, seqlen, io_dtype, io_pack(io_dtype)).grid.y);
  return conv_det_dw_floats(sl, dim, width) + sl * dim;
}

extern "C" int simamba_causal_conv1d_bwd_ex(const void* x, const float* w, const float* bias, const void* dout,
                                            void* dx, float* dw, float* dbias, int batch, int dim, int seqlen,
                                            int width, int silu, int io_dtype, long long x_bstride,
                                            long long dx_bstride, int flags, float* workspace,
                                            long long workspace_floats, void* stream) {
  if (flags & ~SIMAMBA_BWD_DETERMINISTIC) return SIMAMBA_E_VARIANT;
  const bool det = flags != 0;
  int rc = check_conv(x, w, batch, dim, seqlen, width, io_dtype);
  if (rc) return rc;
  if (!dout || !dx || !dw) return SIMAMBA_E_NULLPTR;
  const long long need = det ? simamba_causal_conv1d_bwd_workspace_floats(batch, dim, seqlen, width, flags) : 0;
  if (need > 0 && (!workspace || workspace_floats < need)) return SIMAMBA_E_WORKSPACE;
  if (det && !aligned16(workspace)) return SIMAMBA_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the two accumulators are zeroed here; a caller that carves dbias directly behind dw gets one memset node
  // (the deterministic form writes them whole in its sum pass: nothing to clear but for an empty problem)
  if (!det || batch == 0 || seqlen == 0) {
    const bool joined = dbias == dw + static_cast<size_t>(dim) * width;
    hipError_t e = hipMemsetAsync(dw, 0, sizeof(float) * (static_cast<size_t>(dim) * width + (joined ? dim : 0)), s);
    if (e != hipSuccess) return static_cast<int>(e);
    if (dbias && !joined) {
      e = hipMemsetAsync(dbias, 0, sizeof(float) * dim, s);
      if (e != hipSuccess) return static_cast<int>(e);
    }
  }
  if (batch == 0 || seqlen == 0) return SIMAMBA_OK;
  const ConvGeom g = conv_geom(batch, dim, seqlen, io_dtype, io_pack(io_dtype), x_bstride, dx_bstride, {x, dx, dout});
  ConvArgs a{x, w, bias, dx, dout, dw, dbias, batch, dim, seqlen, width, silu, g.vec, g.ppr, g.bchunk, g.x_bs, g.o_bs};
  const bool fast = g.vec && seqlen % io_pack(io_dtype) == 0;
  if (!det) return conv_bwd_launch<false>(a, io_dtype, fast, g.grid, s);
  const int slices = static_cast<int>(g.grid.y);
  a.dw = workspace;                                            // partials in place of the accumulators
  a.dbias = dbias ? workspace + conv_det_dw_floats(slices, dim, width) : nullptr;
  const int e = conv_bwd_launch<true>(a, io_dtype, fast, g.grid, s);
  if (e) return e;
  const long long nw = static_cast<long long>(dim) * width;
  DetSumJob jobs[2] = {{a.dw, dw, nw, nw, slices}, {a.dbias, dbias, dim, dim, slices}};
  return det_sum_launch(jobs, dbias ? 2 : 1, s);
}

extern "C" int simamba_causal_conv1d_bwd(const void* x, const float* w, const float* bias, const void* dout,
                                         void* dx, float* dw, float* dbias, int batch, int dim, int seqlen,
                                         int width, int silu, int io_dtype, long long x_bstride,
                                         long long dx_bstride, void* stream) {
  return simamba_causal_conv1d_bwd_ex(x, w, bias, dout, dx, dw, dbias, batch, dim, seqlen, width, silu, io_dtype,
                                      x_bstride, dx_bstride, 0, nullptr, 0, stream);
}
