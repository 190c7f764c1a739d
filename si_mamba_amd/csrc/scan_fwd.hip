// Selective-scan forward for gfx950.  Decomposition: see scan_common.h.
//
// Replaces selective_scan_cuda.fwd of mamba-ssm as reached from the reference's
// models/block.py:72.  Algorithmic HBM bytes: 4*B*D*L*s (u, delta, z, out) + 2*B*N*L*s (B, C)
// + small; the (B_t, C_t) tile is re-read from L2 once per 16*R channels.
#include <cstdlib>
#include "scan_host.h"

namespace simamba {

template <typename T, int kItems>
__global__ __launch_bounds__(kScanThreads) void scan_fwd_kernel(ScanArgs p) {
  constexpr int LC = 16 * kItems;
  constexpr int LDP = LC + 4;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sB = smem;                       // [kMaxState][LDP]
  float* sC = sB + kMaxState * LDP;       // [kMaxState][LDP]
  float* sCarry = sC + kMaxState * LDP;   // [16 * passes][kMaxState]
  float* sMid = sCarry + kRowsPerPass * p.passes * kMaxState;   // kItems == 16 only: state at the chunk's middle

  int tile_id, b;
  xcd_tile(tile_id, b);
  const int tile_base = tile_id * (kRowsPerPass * p.passes);
  const int lane16 = threadIdx.x & 15;
  const int rowslot = threadIdx.x >> 4;   // 0..15: wave*4 + sub-row
  const int L = p.seqlen, D = p.dim, N = p.dstate;
  const T* __restrict__ ug = static_cast<const T*>(p.u);
  const T* __restrict__ dg = static_cast<const T*>(p.delta);
  const T* __restrict__ zg = static_cast<const T*>(p.z);
  T* __restrict__ og = static_cast<T*>(p.out);
  const bool vec = p.vec != 0;
  const bool keep_state = (p.nchunks > 1) || p.x_ckpt || p.last_state;

  const int nchunks_k = (L + LC - 1) / LC;        // chunks of THIS kernel (p.nchunks counts 128-step checkpoints)
  for (int c = 0; c < nchunks_k; ++c) {
    __syncthreads();
    stage_bc<T, LC>(static_cast<const T*>(p.B), static_cast<const T*>(p.C), sB, sC, b, N, L, c, p.bc_bs, p.bc_ns,
                    p.bc_ts);
    __syncthreads();

    for (int r = 0; r < p.passes; ++r) {
      const int slot = r * kRowsPerPass + rowslot;
      const int d = tile_base + slot;
      const bool dvalid = d < D;
      const int dc = dvalid ? d : D - 1;
      const int t0 = c * LC + lane16 * kItems;
      int nvalid = L - t0;
      nvalid = nvalid < 0 ? 0 : (nvalid > kItems ? kItems : nvalid);
      const size_t off = (static_cast<size_t>(b) * D + dc) * L + t0;

      float u[kItems], dl[kItems], zz[kItems], y[kItems], du[kItems];
      load_items<T, kItems>(ug + off, nvalid, vec, u);
      load_items<T, kItems>(dg + off, nvalid, vec, dl);
      if (zg) load_items<T, kItems>(zg + static_cast<size_t>(b) * p.z_bs + static_cast<size_t>(dc) * L + t0, nvalid, vec, zz);

      const float bias = p.delta_bias ? p.delta_bias[dc] : 0.f;
      const float Dd = p.D ? p.D[dc] : 0.f;
      float sumd = 0.f;
#pragma unroll
      for (int i = 0; i < kItems; ++i) {
        float x = dl[i] + bias;
        x = p.softplus ? softplus_f(x) : x;
        x = (i < nvalid) ? x : 0.f;           // padded steps are the identity map
        dl[i] = x;
        sumd += x;
        du[i] = x * u[i];
        y[i] = Dd * u[i];
      }

      float A2[kMaxState];
      load_A_row(p.A + static_cast<size_t>(dc) * N, N, A2);
#pragma unroll
      for (int n = 0; n < kMaxState; ++n) {
        if (n < N) {
          const float A2n = A2[n];
          const float* bp = sB + n * LDP;
          const float* cp = sC + n * LDP;
          float a[kItems], bb[kItems], cc[kItems];
#pragma unroll
          for (int i = 0; i < kItems; i += 4) {
            const int qo = bc_quad<kItems>((lane16 * kItems + i) >> 2) * 4;
            float4 vb = *reinterpret_cast<const float4*>(bp + qo);
            float4 vc = *reinterpret_cast<const float4*>(cp + qo);
            bb[i] = vb.x; bb[i + 1] = vb.y; bb[i + 2] = vb.z; bb[i + 3] = vb.w;
            cc[i] = vc.x; cc[i + 1] = vc.y; cc[i + 2] = vc.z; cc[i + 3] = vc.w;
          }
          float S = 0.f;
#pragma unroll
          for (int i = 0; i < kItems; ++i) {
            a[i] = fast_exp2(dl[i] * A2n);
            bb[i] = du[i] * bb[i];
            S = fmaf(a[i], S, bb[i]);
          }
          float P = fast_exp2(A2n * sumd);
          row_scan_inclusive(P, S);
          float h = row_prev(S, 0.f);
          if (c > 0 || keep_state) {
            const float carry = (c > 0) ? sCarry[slot * kMaxState + n] : 0.f;
            if (c > 0) h = fmaf(row_prev(P, 1.f), carry, h);
            if (keep_state) {
              const float st = fmaf(P, carry, S);       // state after this lane's last step
              if (lane16 == 15) sCarry[slot * kMaxState + n] = st;
              if (kItems == 16 && lane16 == 7) sMid[slot * kMaxState + n] = st;   // 128-step boundary inside the chunk
            }
          }
#pragma unroll
          for (int i = 0; i < kItems; ++i) {
            h = fmaf(a[i], h, bb[i]);
            y[i] = fmaf(cc[i], h, y[i]);
          }
        }
      }

      if (zg) {
#pragma unroll
        for (int i = 0; i < kItems; ++i) y[i] = y[i] * zz[i] * sigmoid_f(zz[i]);
      }
      if (dvalid) store_items<T, kItems>(og + off, nvalid, vec, y);

      if (keep_state) {
        __builtin_amdgcn_wave_barrier();
        if (dvalid && lane16 < N) {
          const float st = sCarry[slot * kMaxState + lane16];
          constexpr int kPer = LC / SIMAMBA_SCAN_CHUNK > 0 ? LC / SIMAMBA_SCAN_CHUNK : 1;   // checkpoints per chunk
          float* ck = p.x_ckpt ? p.x_ckpt + (static_cast<size_t>(b) * D + d) * p.nchunks * N + lane16 : nullptr;
          if (ck) {
            if (kPer == 2) {
              ck[static_cast<size_t>(2 * c) * N] = sMid[slot * kMaxState + lane16];
              if (2 * c + 1 < p.nchunks) ck[static_cast<size_t>(2 * c + 1) * N] = st;
            } else {
              ck[static_cast<size_t>(c) * N] = st;
            }
          }
          if (p.last_state && c == nchunks_k - 1)
            p.last_state[(static_cast<size_t>(b) * D + d) * N + lane16] = st;
        }
      }
    }
  }
}

static size_t fwd_smem_bytes(int kItems, int passes) {
  const int LC = 16 * kItems;
  return sizeof(float) * (2 * kMaxState * (LC + 4) + 2 * kRowsPerPass * passes * kMaxState);
}

template <typename T>
static int launch_fwd(const ScanArgs& a, hipStream_t s) {
  dim3 grid((a.dim + kRowsPerPass * a.passes - 1) / (kRowsPerPass * a.passes), a.batch);
  if (a.seqlen <= 64) {
    hipLaunchKernelGGL((scan_fwd_kernel<T, 4>), grid, dim3(kScanThreads), fwd_smem_bytes(4, a.passes), s, a);
  } else if (a.seqlen <= 128 || !a.long_items) {
    hipLaunchKernelGGL((scan_fwd_kernel<T, 8>), grid, dim3(kScanThreads), fwd_smem_bytes(8, a.passes), s, a);
  } else {
    // 16 steps per lane: the 4 scan steps and the per-lane bookkeeping amortise over twice the work
    hipLaunchKernelGGL((scan_fwd_kernel<T, 16>), grid, dim3(kScanThreads), fwd_smem_bytes(16, a.passes), s, a);
  }
  return static_cast<int>(hipGetLastError());
}

// Kernel choice when the caller leaves it to the library (variant == SIMAMBA_SCAN_AUTO).  The lanes-per-channel
// kernel (scan_fwd_seq.hip) issues 5 VALU per (row, step, state) against ~7 for the row-scan kernel, but a wave
// covers 64 / lpc whole rows: it needs rows / (64 / lpc) waves to give every one of the 1024 SIMDs its 3 waves.
static int auto_variant(long long rows, int batch, int dim) {
  // Two lanes per channel from 49 152 rows on (1.5 waves per SIMD).  Measured kernel times, fp32, rocprofv3 medians:
  //   (64,768,1024): row-scan 329-334 us, LPC2 307-311 us, LPC4 313-320 us      (49 152 rows)
  //   (64,768, 512): row-scan 179 us,     LPC2 156 us,     LPC4 152 us
  //   (32,768,1024): row-scan 182 us,     LPC2 198 us,     LPC4 207 us          (24 576 rows: too few waves)
  //   (256,768,128): row-scan 165 us,     LPC2 115 us                           (196 608 rows, the north-star shape)
  // Where two lanes per channel leaves half a round of waves over (49 152 rows = 1536 waves) the mixed launch
  // (SIMAMBA_SCAN_MIX, scan_fwd_seq.hip) evens the SIMDs out and is 14 % faster on its own, but 15 % slower in the
  // place the mixer calls it from (right behind 400 MB of freshly written operands): not chosen here.
  (void)batch; (void)dim;
  if (rows >= 48 * 1024) return SIMAMBA_SCAN_LPC2;
  return SIMAMBA_SCAN_ROWSCAN;
}

}  // namespace simamba

using namespace simamba;

extern "C" int simamba_scan_num_chunks(int seqlen) {
  if (seqlen <= 64) return 1;
  return (seqlen + SIMAMBA_SCAN_CHUNK - 1) / SIMAMBA_SCAN_CHUNK;
}

extern "C" int simamba_scan_fwd_auto_variant(int batch, int dim) {
  if (batch <= 0 || dim <= 0) return SIMAMBA_SCAN_ROWSCAN;
  return auto_variant(static_cast<long long>(batch) * dim, batch, dim);
}

// Which checkpoints a forward / backward pair should use when the caller leaves it to the library.  The sequential
// backward (scan_bwd_seq.hip, 16-step checkpoints written by a lanes-per-channel forward) is taken from the row
// count on at which that forward is: below it neither has enough waves for the chip.
extern "C" int simamba_scan_ckpt_step(int batch, int dim, int seqlen, int dstate, int io_dtype) {
  if (batch <= 0 || dim <= 0 || seqlen <= 0) return SIMAMBA_SCAN_CKPT_ROW;
  const long long rows = static_cast<long long>(batch) * dim;
  // Long sequences keep the sequential pair down to 36 864 rows: a mixer that runs on part of a batch of 64 (the
  // samples DropPath keeps, 48 .. 60 of them) would otherwise fall back to the row-scan pair just below the line.
  // Measured inside the fp32 mixer at (B, 768, 1024), forward + backward kernel, us: B = 60 row-scan pair 340 + 971,
  // sequential pair (four lanes per channel forward) 279 + 702; B = 56 334 + 957 against 240 + 691; B = 52 305 + 961
  // against 241 + 696; B = 48 289 + 942 against 230 + 685.  Short sequences and bf16 I/O were not measured and keep
  // the line.
  const bool long_rows = io_dtype == SIMAMBA_F32 && seqlen >= 1024 && rows >= 36 * 1024;
  if (dstate == kMaxState && dim % 64 == 0 && seqlen % io_pack(io_dtype) == 0 && rows * seqlen < (1ll << 30) &&
      (auto_variant(rows, batch, dim) != SIMAMBA_SCAN_ROWSCAN || long_rows))
    return SIMAMBA_SCAN_CKPT_SEQ;
  return SIMAMBA_SCAN_CKPT_ROW;
}

extern "C" long long simamba_scan_ckpt_floats(int batch, int dim, int seqlen, int dstate, int ckpt_step) {
  if (batch <= 0 || dim <= 0 || seqlen <= 0 || dstate <= 0) return 0;
  if (ckpt_step == SIMAMBA_SCAN_CKPT_SEQ)
    return seqlen <= 16 ? 0 : static_cast<long long>(batch) * ((seqlen + 15) / 16) * dim * kMaxState;
  const int nc = simamba_scan_num_chunks(seqlen);
  return nc <= 1 ? 0 : static_cast<long long>(batch) * dim * nc * dstate;
}

// What the lanes-per-channel forward assumes beyond the argument checks of simamba_selective_scan_fwd: 16 states,
// softplus on (the only form the reference's mixer uses), pack-aligned rows (`vec`) and B / C, 32-bit byte offsets.
// One statement of it for the entry point and for simamba_scan_seq_applicable.
static bool scan_fwd_seq_ok(int batch, int dim, int seqlen, int dstate, int softplus, const ScanOperands& o,
                            const void* A, const void* B, const void* C, int io_dtype) {
  const long long rows = static_cast<long long>(batch) * dim;
  return dstate == kMaxState && softplus && o.vec && rows * seqlen < (1ll << 30) &&
         scan_fwd_seq_bc_mode(B, C, io_dtype, o.bc_bs, o.bc_ns, o.bc_ts) != 0 &&
         static_cast<long long>(batch) * o.z_bs < (1ll << 30) && aligned16(A) && o.bc_ns >= 0 && o.bc_ts >= 0 &&
         (kMaxState - 1) * o.bc_ns + (seqlen - 1) * o.bc_ts < (1ll << 30);
}

// Launch-free statement of what a CKPT_SEQ forward / backward pair accepts (include/simamba.h).  Addresses are only
// examined for alignment.  The operands go through scan_operands like those of the two entry points, then through the
// predicates those evaluate: scan_fwd_seq_ok above, and scan_fwd_seq_bc_mode + scan_bwd_seq_ok of scan_bwd_impl
// (scan_bwd.hip; its A test is the forward's, and x_ckpt is part of `act_addr_or`).
extern "C" int simamba_scan_seq_applicable(int batch, int dim, int seqlen, int dstate, int io_dtype,
                                           int delta_softplus, int has_z, size_t act_addr_or, size_t A_addr,
                                           size_t B_addr, size_t C_addr, long long z_bstride, long long dz_bstride,
                                           long long bc_bstride, long long bc_nstride, long long bc_tstride) {
  if (batch <= 0 || seqlen <= 0 || scan_check_shape(batch, dim, seqlen) || scan_check_dstate(dstate) ||
      check_io_dtype(io_dtype))
    return 0;
  const ScanOperands o = scan_operands(dim, seqlen, dstate, io_dtype, act_addr_or, has_z != 0, z_bstride, dz_bstride,
                                       bc_bstride, bc_nstride, bc_tstride);
  const void* A = reinterpret_cast<const void*>(A_addr);
  const void* B = reinterpret_cast<const void*>(B_addr);
  const void* C = reinterpret_cast<const void*>(C_addr);
  if (!scan_fwd_seq_ok(batch, dim, seqlen, dstate, delta_softplus, o, A, B, C, io_dtype)) return 0;
  const int bc_mode = scan_fwd_seq_bc_mode(B, C, io_dtype, o.bc_bs, o.bc_ns, o.bc_ts);
  return scan_bwd_seq_ok(batch, dim, seqlen, dstate, delta_softplus, o.vec, o.z_bs, o.dz_bs, has_z != 0, bc_mode,
                         o.bc_ns, o.bc_ts) ? 1 : 0;
}

// lanes per channel of a forward variant, as scan_fwd_seq_dispatch takes it
static int variant_lpc(int v) { return v == SIMAMBA_SCAN_MIX ? 6 : v == SIMAMBA_SCAN_LPC2 ? 2 : 4; }

extern "C" int simamba_selective_scan_fwd(const void* u, const void* delta, const float* A, const void* B,
                                          const void* C, const float* D, const void* z,
                                          const float* delta_bias, void* out, float* x_ckpt,
                                          float* last_state, int batch, int dim, int seqlen, int dstate,
                                          int io_dtype, int delta_softplus, long long z_bstride,
                                          long long bc_bstride, long long bc_nstride, long long bc_tstride,
                                          int ckpt_step, int variant, void* stream) {
  if (const int rc = scan_check_args(batch, dim, seqlen, dstate, io_dtype, ckpt_step)) return rc;
  if (batch == 0 || seqlen == 0) return SIMAMBA_OK;   // nothing to do (empty tensors carry NULL data)
  if (!u || !delta || !A || !B || !C || !out) return SIMAMBA_E_NULLPTR;
  const ScanOperands o = scan_operands(dim, seqlen, dstate, io_dtype, addr_or({u, delta, out, z}), z != nullptr,
                                       z_bstride, 0, bc_bstride, bc_nstride, bc_tstride);
  ScanArgs a{};
  a.u = u; a.delta = delta; a.A = A; a.B = B; a.C = C; a.D = D; a.z = z; a.delta_bias = delta_bias;
  a.out = out; a.x_ckpt = x_ckpt; a.last_state = last_state;
  a.batch = batch; a.dim = dim; a.seqlen = seqlen; a.dstate = dstate;
  a.nchunks = o.nchunks;
  a.softplus = delta_softplus;
  a.z_bs = o.z_bs; a.bc_bs = o.bc_bs; a.bc_ns = o.bc_ns; a.bc_ts = o.bc_ts;
  a.vec = o.vec;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (variant != SIMAMBA_SCAN_AUTO && variant != SIMAMBA_SCAN_ROWSCAN && variant != SIMAMBA_SCAN_LPC2 &&
      variant != SIMAMBA_SCAN_LPC4 && variant != SIMAMBA_SCAN_MIX)
    return SIMAMBA_E_VARIANT;
  const long long rows = static_cast<long long>(batch) * dim;
  const bool seq_ok = scan_fwd_seq_ok(batch, dim, seqlen, dstate, delta_softplus, o, A, B, C, io_dtype);
  int v = variant == SIMAMBA_SCAN_AUTO ? auto_variant(rows, batch, dim) : variant;
  // 16-step checkpoints are written by the lanes-per-channel kernels only (four lanes per channel where two would
  // leave the chip short of waves)
  const bool want_seq_ckpt = x_ckpt && ckpt_step == SIMAMBA_SCAN_CKPT_SEQ;
  if (want_seq_ckpt && v == SIMAMBA_SCAN_ROWSCAN) {
    if (variant != SIMAMBA_SCAN_AUTO) return SIMAMBA_E_VARIANT;
    v = SIMAMBA_SCAN_LPC4;
  }
  if (v != SIMAMBA_SCAN_ROWSCAN && !seq_ok) {
    if (variant != SIMAMBA_SCAN_AUTO || want_seq_ckpt) return SIMAMBA_E_VARIANT;   // a request the shape cannot take
    v = SIMAMBA_SCAN_ROWSCAN;
  }
  if (v != SIMAMBA_SCAN_ROWSCAN)
    return scan_fwd_seq_dispatch(u, delta, A, B, C, D, z, delta_bias, out, x_ckpt, ckpt_step, last_state, batch, dim, seqlen,
                                 io_dtype, a.z_bs, a.bc_bs, a.bc_ns, a.bc_ts, a.nchunks, variant_lpc(v), s,
                                 nullptr, nullptr, 0, 0, 0);
  // channels per workgroup: amortise the (B_t,C_t) staging, but keep >= ~3 workgroups per CU
  int passes = 4;
  while (passes > 1 && static_cast<long long>(batch) * ((dim + 16 * passes - 1) / (16 * passes)) < 768) passes >>= 1;
  a.passes = passes;
  a.long_items = seqlen >= 768;   // measured: -6 % at L = 1024, neutral at L = 512 (3 instead of 4 waves per SIMD)
  return io_dtype == SIMAMBA_F32 ? launch_fwd<float>(a, s) : launch_fwd<bf16_t>(a, s);
}

// The mixer's scan with delta formed inside the kernel (csrc/scan_fwd_seq.hip, kDt): u = the conv output, xdbl = the
// x_proj output (batch, seqlen, dt_rank + 2 * 16) token-major, wdt = dt_proj.weight (dim, dt_rank) in the I/O type.
extern "C" int simamba_selective_scan_dt_fwd(const void* u, const void* xdbl, const void* wdt, const float* A,
                                             const float* D, const void* z, const float* delta_bias, void* out,
                                             float* x_ckpt, float* last_state, int batch, int dim, int seqlen,
                                             int dstate, int dt_rank, int io_dtype, long long z_bstride,
                                             long long xdbl_bstride, long long xdbl_tstride, int ckpt_step, int variant,
                                             void* stream) {
  int rc;
  if ((rc = scan_check_shape(batch, dim, seqlen))) return rc;
  if (dstate != kMaxState) return SIMAMBA_E_DSTATE;
  if ((rc = check_io_dtype(io_dtype)) || (rc = scan_check_ckpt(ckpt_step))) return rc;
  if (variant != SIMAMBA_SCAN_AUTO && variant != SIMAMBA_SCAN_LPC2 && variant != SIMAMBA_SCAN_LPC4 &&
      variant != SIMAMBA_SCAN_MIX)
    return SIMAMBA_E_VARIANT;                               // the row-scan kernel reads a delta tensor
  if ((rc = scan_check_dt_rank(dt_rank, io_dtype))) return rc;
  if (batch == 0 || seqlen == 0) return SIMAMBA_OK;
  if (!u || !xdbl || !wdt || !A || !z || !out) return SIMAMBA_E_NULLPTR;
  const XdblOperands x = scan_xdbl_operands(xdbl, wdt, batch, seqlen, dt_rank, io_dtype, xdbl_bstride, xdbl_tstride);
  const ScanOperands o = scan_operands(dim, seqlen, dstate, io_dtype, addr_or({u, out, z}), true, z_bstride, 0, x.bs, 1,
                                       x.ts);
  const long long rows = static_cast<long long>(batch) * dim;
  const bool ok = o.vec && x.ok && aligned16(A) && rows * seqlen < (1ll << 30) &&
                  static_cast<long long>(batch) * o.z_bs < (1ll << 30) &&
                  scan_fwd_seq_bc_mode(x.B, x.C, io_dtype, x.bs, 1, x.ts) == 2;
  if (!ok) return SIMAMBA_E_VARIANT;
  int v = variant;
  if (v == SIMAMBA_SCAN_AUTO) {
    v = auto_variant(rows, batch, dim);
    if (v == SIMAMBA_SCAN_ROWSCAN) v = SIMAMBA_SCAN_LPC4;   // too few rows for two lanes per channel
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  return scan_fwd_seq_dispatch(u, nullptr, A, x.B, x.C, D, z, delta_bias, out, x_ckpt, ckpt_step, last_state, batch, dim,
                               seqlen, io_dtype, o.z_bs, x.bs, 1, x.ts, o.nchunks, variant_lpc(v), s,
                               xdbl, wdt, x.bs, x.ts, dt_rank);
}
