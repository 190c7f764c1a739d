// Selective-scan backward for gfx950.  Decomposition: see scan_common.h.
//
// Replaces selective_scan_cuda.bwd of mamba-ssm (autograd of the call at the reference's
// models/block.py:72).  Per (row, state n) the kernel re-runs the forward scan to get h_t, runs
// the adjoint scan g_t = C_t dy_t + a_{t+1} g_{t+1} right-to-left over the same 16 lanes, and
// forms all gradients in registers.  Reductions:
//   dB, dC  (sum over channels): v_permlane32_swap/v_permlane16_swap transposing reduction over
//           the wave's 4 channel rows -> ds_add_f32 into an LDS tile shared by the workgroup's
//           16*R channels -> one coalesced float-atomic flush per workgroup and chunk;
//   dA, dD, ddelta_bias (sum over time and batch): DPP row all-reduce -> one atomic per row.
// Algorithmic HBM bytes: 7*B*D*L*s + 2*B*N*L*(s+4) + small.
//
// Deterministic form (kDet, SIMAMBA_BWD_DETERMINISTIC): the same kernel with plain stores of partials instead of the
// atomics; the accumulator pointers then point into the caller's workspace (det_layout below): dB | dC per workgroup
// column into the slab [group][tensor][batch][N][L] (p.dC = p.dB + batch * N * L), dA / dD / ddelta_bias per (chunk,
// sample, row).  det_reduce.hip sums them in a fixed order.
#include "scan_host.h"
#include "scan_xlane.h"
#include "det_reduce.h"

namespace simamba {

template <typename T, int kItems, bool kDet = false>
__global__ __launch_bounds__(kScanThreads, 2) void scan_bwd_kernel(ScanArgs p) {
  constexpr int LC = 16 * kItems;
  constexpr int LDP = LC + 4;
  constexpr int KH = kItems / 2;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sB = smem;                          // [kMaxState][LDP]
  float* sC = sB + kMaxState * LDP;          // [kMaxState][LDP]
  float* sAcc = sC + kMaxState * LDP;        // [2][kMaxState][LC]   dB / dC of this chunk (cross-wave sum)
  float* sG = sAcc + 2 * kMaxState * LC;     // [16*passes][kMaxState] adjoint state entering from the right
  float* sDf = sG + kRowsPerPass * p.passes * kMaxState;  // [16*passes] delta of the next chunk's first step
  float* sCk = sDf + kRowsPerPass * p.passes;             // [16 rows][kMaxState] chunk-start states of this pass

  int tile_id, b;
  xcd_tile(tile_id, b);
  const int tile_base = tile_id * (kRowsPerPass * p.passes);
  const int lane16 = threadIdx.x & 15;
  const int rowslot = threadIdx.x >> 4;
  const int wave = threadIdx.x >> 6;
  const int sub = rowslot & 3;               // channel row inside the wave
  const int L = p.seqlen, D = p.dim, N = p.dstate;
  const T* __restrict__ ug = static_cast<const T*>(p.u);
  const T* __restrict__ dg = static_cast<const T*>(p.delta);
  const T* __restrict__ zg = static_cast<const T*>(p.z);
  const T* __restrict__ gg = static_cast<const T*>(p.dout);
  T* __restrict__ dug = static_cast<T*>(p.du);
  T* __restrict__ ddg = static_cast<T*>(p.ddelta);
  T* __restrict__ dzg = static_cast<T*>(p.dz);
  const bool vec = p.vec != 0;

  for (int c = p.nchunks - 1; c >= 0; --c) {
    __syncthreads();
    stage_bc<T, LC>(static_cast<const T*>(p.B), static_cast<const T*>(p.C), sB, sC, b, N, L, c, p.bc_bs, p.bc_ns,
                    p.bc_ts);
    __syncthreads();
    const bool last_chunk = (c == p.nchunks - 1);

    // dB / dC partial sums of this wave over its passes: after the transposing reduction, row `sub` of the
    // wave owns tensor (sub >> 1) and items [(sub & 1) * KH, +KH) of every state n.
    float acc[kMaxState][KH];
#pragma unroll
    for (int n = 0; n < kMaxState; ++n)
#pragma unroll
      for (int i = 0; i < KH; ++i) acc[n][i] = 0.f;

    for (int r = 0; r < p.passes; ++r) {
      const int slot = r * kRowsPerPass + rowslot;
      const int d = tile_base + slot;
      const bool dvalid = d < D;
      const int dc = dvalid ? d : D - 1;
      const int t0 = c * LC + lane16 * kItems;
      int nvalid = L - t0;
      nvalid = nvalid < 0 ? 0 : (nvalid > kItems ? kItems : nvalid);
      const size_t off = (static_cast<size_t>(b) * D + dc) * L + t0;

      // dy = dout * silu(z) feeds the adjoint scan; dzw = dout * silu'(z) is kept for the epilogue
      // (dz = dzw * y_pre), so neither dout nor z stays in registers through the state loop
      float u[kItems], dl[kItems], dy[kItems], dzw[kItems];
      float ypre[kItems], dxs[kItems], dda[kItems], du[kItems];
      load_items<T, kItems>(ug + off, nvalid, vec, u);
      load_items<T, kItems>(dg + off, nvalid, vec, dl);
      load_items<T, kItems>(gg + off, nvalid, vec, dy);
      const size_t zoff = static_cast<size_t>(dc) * L + t0;
      if (zg) load_items<T, kItems>(zg + static_cast<size_t>(b) * p.z_bs + zoff, nvalid, vec, dzw);
      float A2[kMaxState];
      load_A_row(p.A + static_cast<size_t>(dc) * N, N, A2);

      const float bias = p.delta_bias ? p.delta_bias[dc] : 0.f;
      const float Dd = p.D ? p.D[dc] : 0.f;
      float sumd = 0.f;
#pragma unroll
      for (int i = 0; i < kItems; ++i) {
        float x = dl[i] + bias;
        x = p.softplus ? softplus_f(x) : x;
        const bool ok = i < nvalid;
        x = ok ? x : 0.f;
        dl[i] = x;
        sumd += x;
        du[i] = x * u[i];
        const float go = (ok && dvalid) ? dy[i] : 0.f;
        if (zg) {
          const float z = dzw[i], sg = sigmoid_f(z);
          dy[i] = go * z * sg;
          dzw[i] = go * sg * (1.f + z * (1.f - sg));
        } else {
          dy[i] = go;
        }
        ypre[i] = Dd * u[i];
        dxs[i] = 0.f;
        dda[i] = 0.f;
      }
      // delta of the step right after this lane's last one (next lane, or next chunk for lane 15)
      const float dnext = row_next(dl[0], last_chunk ? 0.f : sDf[slot]);
      // chunk-start state h_{t0-1}[n] from the forward's checkpoints: lane n of the row fetches entry n (one
      // coalesced 64-byte read per row, issued with the tile loads) and parks it in LDS; the state loop then
      // reads it back row-broadcast.  (Reading x_ckpt inside the state loop cost one exposed global-load
      // round trip per state: s_waitcnt vmcnt(0) in the middle of the loop.)
      {
        const float* ck = p.x_ckpt + ((static_cast<size_t>(b) * D + dc) * p.nchunks + (c > 0 ? c - 1 : 0)) * N;
        sCk[rowslot * kMaxState + lane16] = (c > 0 && lane16 < N) ? ck[lane16] : 0.f;
      }
      float dAlane = 0.f;   // lane n of the row ends up holding dA[d][n] of this chunk

#pragma unroll
      for (int n = 0; n < kMaxState; ++n) {
        // (the runtime guard doubles as a boundary between the unrolled states: compiled away for dstate == 16,
        //  hipcc interleaves all 16 states and spills 3 KB per lane)
        if (n < N) {
          const float A2n = A2[n];
          const float* bp = sB + n * LDP;
          const float* cp = sC + n * LDP;
          float a[kItems], bw[kItems], cc[kItems], hp[kItems];
#pragma unroll
          for (int i = 0; i < kItems; i += 4) {
            const int qo = bc_quad<kItems>((lane16 * kItems + i) >> 2) * 4;
            float4 vb = *reinterpret_cast<const float4*>(bp + qo);
            float4 vc = *reinterpret_cast<const float4*>(cp + qo);
            bw[i] = vb.x; bw[i + 1] = vb.y; bw[i + 2] = vb.z; bw[i + 3] = vb.w;
            cc[i] = vc.x; cc[i + 1] = vc.y; cc[i + 2] = vc.z; cc[i + 3] = vc.w;
          }
          // ---- forward re-scan: h_t -----------------------------------------------------
          float S = 0.f;
#pragma unroll
          for (int i = 0; i < kItems; ++i) {
            a[i] = fast_exp2(dl[i] * A2n);
            S = fmaf(a[i], S, du[i] * bw[i]);
          }
          float P = fast_exp2(A2n * sumd);
          row_scan_inclusive(P, S);
          float h = row_prev(S, 0.f);
          {
            const float hin = sCk[rowslot * kMaxState + n];     // zero-filled when there is no chunk to the left
            h = fmaf(row_prev(P, 1.f), hin, h);
          }
          float red[2 * kItems];   // [0,K): dB terms, [K,2K): dC terms
#pragma unroll
          for (int i = 0; i < kItems; ++i) {
            hp[i] = h;
            h = fmaf(a[i], h, du[i] * bw[i]);
            ypre[i] = fmaf(cc[i], h, ypre[i]);
            red[kItems + i] = dy[i] * h;
            cc[i] = cc[i] * dy[i];          // c_t = C_t * dy_t, source term of the adjoint scan
          }
          // ---- adjoint scan, right to left: g_t = c_t + a_{t+1} g_{t+1} -----------------
          const float anext = fast_exp2(dnext * A2n);
          float G = 0.f;
#pragma unroll
          for (int i = kItems - 1; i >= 0; --i) {
            const float al = (i == kItems - 1) ? anext : a[i + 1];
            G = fmaf(al, G, cc[i]);
          }
          float Q = fast_exp2(A2n * (sumd - dl[0] + dnext));
          row_scan_inclusive_rev(Q, G);
          float g = row_next(G, 0.f);
          {
            // adjoint state entering from the chunk on the right (0 for the last chunk): one straight-line
            // sequence for every chunk position, the only predicated op is the LDS store of the carry
            const float gl = sG[slot * kMaxState + n];
            const float gcar = last_chunk ? 0.f : gl;
            g = fmaf(row_next(Q, 1.f), gcar, g);
            if (c > 0 && lane16 == 0) sG[slot * kMaxState + n] = fmaf(Q, gcar, G);
          }
          float dAacc = 0.f;
#pragma unroll
          for (int i = kItems - 1; i >= 0; --i) {
            const float al = (i == kItems - 1) ? anext : a[i + 1];
            g = fmaf(al, g, cc[i]);
            red[i] = g * du[i];
            dxs[i] = fmaf(g, bw[i], dxs[i]);
            const float q = g * a[i] * hp[i];
            dda[i] = fmaf(A2n, q, dda[i]);
            dAacc = fmaf(dl[i], q, dAacc);
          }
          dAacc = row_allreduce_sum(dAacc);
          dAlane = (lane16 == n) ? dAacc : dAlane;
          // ---- dB / dC: transposing reduction over the wave's 4 channel rows ---------------
          swap32_stage<kItems>(red, red + kItems);
          swap16_stage<KH>(red, red + KH);
#pragma unroll
          for (int i = 0; i < KH; ++i) acc[n][i] += red[i];
        }
      }

      // ---- per-timestep gradients ---------------------------------------------------------
      float ddl[kItems], dzv[kItems];
      float sD = 0.f, sBias = 0.f;
#pragma unroll
      for (int i = 0; i < kItems; ++i) {
        // d softplus(x)/dx = sigmoid(x), from softplus(x); padded steps carry no gradient
        const float sgm = p.softplus ? softplus_grad_from_sp(dl[i]) : 1.f;
        const float gd = fmaf(u[i], dxs[i], kLn2 * dda[i]) * sgm;
        ddl[i] = gd;
        sBias += gd;
        sD = fmaf(dy[i], u[i], sD);
        du[i] = fmaf(dl[i], dxs[i], Dd * dy[i]);
        if (zg) dzv[i] = dzw[i] * ypre[i];
      }
      if (dvalid) {
        store_items<T, kItems>(dug + off, nvalid, vec, du);
        store_items<T, kItems>(ddg + off, nvalid, vec, ddl);
        if (zg) store_items<T, kItems>(dzg + static_cast<size_t>(b) * p.dz_bs + zoff, nvalid, vec, dzv);
      }
      sD = row_allreduce_sum(sD);
      sBias = row_allreduce_sum(sBias);
      if (kDet && dvalid) {
        const size_t pr = (static_cast<size_t>(c) * p.batch + b) * D + d;
        if (lane16 < N) p.dA[pr * N + lane16] = dAlane;
        if (lane16 == 0 && p.dD) p.dD[pr] = sD;
        if (lane16 == 1 && p.ddelta_bias) p.ddelta_bias[pr] = sBias;
      } else if (dvalid) {
        if (lane16 < N) atomicAdd(&p.dA[static_cast<size_t>(d) * N + lane16], dAlane);
        if (lane16 == 0 && p.dD) atomicAdd(&p.dD[d], sD);
        if (lane16 == 1 && p.ddelta_bias) atomicAdd(&p.ddelta_bias[d], sBias);
      }
      // hand this chunk's first delta to the chunk on the left
      if (c > 0 && lane16 == 0) sDf[slot] = dl[0];
    }

    // ---- cross-wave sum of the dB / dC partials through one LDS tile, then one atomic flush -----
    float* accp = sAcc + (sub >> 1) * kMaxState * LC + lane16 * kItems + (sub & 1) * KH;
    for (int w = 0; w < kScanThreads / 64; ++w) {
      if (wave == w) {
#pragma unroll
        for (int n = 0; n < kMaxState; ++n) {
          if (n < N) {
#pragma unroll
            for (int i = 0; i < KH; ++i) {
              const float prev = (w == 0) ? 0.f : accp[n * LC + i];
              accp[n * LC + i] = prev + acc[n][i];
            }
          }
        }
      }
      __syncthreads();
    }
    for (int i = threadIdx.x; i < 2 * N * LC; i += kScanThreads) {
      const int tensor = i / (N * LC);
      const int rem = i - tensor * (N * LC);
      const int n = rem / LC, t = rem - n * LC;
      const int gt = c * LC + t;
      if (gt < L) {
        if (kDet) {
          float* dst = (tensor == 0 ? p.dB : p.dC) + static_cast<size_t>(tile_id) * 2 * p.batch * N * L +
                       (static_cast<size_t>(b) * N + n) * L + gt;
          *dst = sAcc[(tensor * kMaxState + n) * LC + t];
        } else {
          float* dst = (tensor == 0 ? p.dB : p.dC) + (static_cast<size_t>(b) * N + n) * L + gt;
          atomicAdd(dst, sAcc[(tensor * kMaxState + n) * LC + t]);
        }
      }
    }
  }
}

static size_t bwd_smem_bytes(int kItems, int passes) {
  const int LC = 16 * kItems;
  return sizeof(float) * (2 * kMaxState * (LC + 4) + 2 * kMaxState * LC + kRowsPerPass * passes * kMaxState +
                          kRowsPerPass * passes + kRowsPerPass * kMaxState);
}

template <typename T, bool kDet>
static void launch_bwd_items(const ScanArgs& a, hipStream_t s) {
  dim3 grid((a.dim + kRowsPerPass * a.passes - 1) / (kRowsPerPass * a.passes), a.batch);
  if (a.seqlen <= 64)
    hipLaunchKernelGGL((scan_bwd_kernel<T, 4, kDet>), grid, dim3(kScanThreads), bwd_smem_bytes(4, a.passes), s, a);
  else
    hipLaunchKernelGGL((scan_bwd_kernel<T, 8, kDet>), grid, dim3(kScanThreads), bwd_smem_bytes(8, a.passes), s, a);
}

template <typename T>
static int launch_bwd(const ScanArgs& a, hipStream_t s, bool det) {
  if (det) launch_bwd_items<T, true>(a, s); else launch_bwd_items<T, false>(a, s);
  return static_cast<int>(hipGetLastError());
}

// channels per workgroup of the row-scan backward = 16 * passes (the more, the fewer dB/dC atomics reach HBM; measured
// at (64,768,1024,16): 134 MB of flush traffic at passes = 3, 18 % on top of the 604 MB of gradient stores); but keep
// >= 2 workgroups per CU, the number resident at this kernel's register footprint.
static int bwd_passes(int batch, int dim) {
  static const int kCand[] = {12, 8, 6, 4, 3, 2, 1};
  for (int cand : kCand) {
    if (static_cast<long long>(batch) * ((dim + 16 * cand - 1) / (16 * cand)) >= 512) return cand;
  }
  return 1;
}

// Workspace of the deterministic backward, in floats; every region starts on a 256-byte boundary.
//   bc   dB | dC partials: [groups][2][batch][dstate][seqlen] (groups = workgroup columns of the launch)
//   a    dA partials:      [K][dim][dstate]   K = batch (sequential kernel) or nchunks * batch (row scan)
//   d    dD partials:      [K][dim]
//   bias ddelta_bias partials: [K][dim]
constexpr int kSeqBwdChannels = 64;         // channels per workgroup of scan_bwd_seq_kernel (kBsCh)
struct DetLayout { long long bc, a, d, bias, total; int groups, K; };
static long long round64(long long n) { return (n + 63) & ~63ll; }
static DetLayout det_layout(int batch, int dim, int seqlen, int dstate, int ckpt_step) {
  DetLayout l{};
  if (ckpt_step == SIMAMBA_SCAN_CKPT_SEQ) {
    l.groups = (dim + kSeqBwdChannels - 1) / kSeqBwdChannels;
    l.K = batch;
  } else {
    const int passes = bwd_passes(batch, dim);
    l.groups = (dim + kRowsPerPass * passes - 1) / (kRowsPerPass * passes);
    l.K = simamba_scan_num_chunks(seqlen) * batch;
  }
  const long long part = static_cast<long long>(l.K) * dim;
  l.bc = 0;
  l.a = round64(2ll * l.groups * batch * dstate * seqlen);
  l.d = l.a + round64(part * dstate);
  l.bias = l.d + round64(part);
  l.total = l.bias + round64(part);
  return l;
}

}  // namespace simamba

using namespace simamba;

extern "C" long long simamba_scan_bwd_workspace_floats(int batch, int dim, int seqlen, int dstate, int ckpt_step,
                                                       int flags) {
  int rc;
  if ((rc = scan_check_flags(flags))) return rc;
  if (!flags) return 0;
  if ((rc = scan_check_shape(batch, dim, seqlen)) || (rc = scan_check_dstate(dstate)) ||
      (rc = scan_check_ckpt(ckpt_step)))
    return rc;
  return det_layout(batch, dim, seqlen, dstate, ckpt_step).total;
}

// the fixed-order sum pass of the deterministic form: partials (a.dA ... in the workspace) -> the caller's spans
static int scan_det_sum(const DetLayout& wl, const ScanArgs& a, float* dA, float* dB, float* dC, float* dD,
                        float* ddelta_bias, hipStream_t s) {
  const long long bnl = static_cast<long long>(a.batch) * a.dstate * a.seqlen;
  const long long part = static_cast<long long>(a.dim);
  DetSumJob jobs[5];
  int n = 0;
  jobs[n++] = DetSumJob{a.dB, dB, 2 * bnl, bnl, wl.groups};
  jobs[n++] = DetSumJob{a.dC, dC, 2 * bnl, bnl, wl.groups};
  jobs[n++] = DetSumJob{a.dA, dA, part * a.dstate, part * a.dstate, wl.K};
  if (dD) jobs[n++] = DetSumJob{a.dD, dD, part, part, wl.K};
  if (ddelta_bias) jobs[n++] = DetSumJob{a.ddelta_bias, ddelta_bias, part, part, wl.K};
  return det_sum_launch(jobs, n, s);
}

// dt != NULL: delta is formed inside the (sequential) kernel from the x_proj output; `delta` is then NULL
static int scan_bwd_impl(const void* u, const void* delta, const float* A, const void* B,
                         const void* C, const float* D, const void* z,
                         const float* delta_bias, const void* dout, const float* x_ckpt,
                         void* du, void* ddelta, float* dA, float* dB, float* dC, float* dD,
                         void* dz, float* ddelta_bias, int batch, int dim, int seqlen,
                         int dstate, int io_dtype, int delta_softplus, long long z_bstride,
                         long long dz_bstride, long long bc_bstride, long long bc_nstride,
                         long long bc_tstride, int ckpt_step, void* stream, const void* dt, const void* wdt,
                         long long dt_bs, long long dt_ts, int dt_rank, int flags, float* workspace,
                         long long workspace_floats) {
  int rc;
  if ((rc = scan_check_flags(flags)) || (rc = scan_check_args(batch, dim, seqlen, dstate, io_dtype, ckpt_step)))
    return rc;
  const bool det = flags != 0;
  if (!A || !dA) return SIMAMBA_E_NULLPTR;
  if (batch > 0 && seqlen > 0) {
    if (!u || (!delta && !dt) || !B || !C || !dout || !du || !ddelta || !dB || !dC) return SIMAMBA_E_NULLPTR;
    if ((z != nullptr) != (dz != nullptr)) return SIMAMBA_E_NULLPTR;
  }
  const ScanOperands o = scan_operands(dim, seqlen, dstate, io_dtype, addr_or({u, delta, dout, du, ddelta, z, dz}),
                                       z != nullptr, z_bstride, dz_bstride, bc_bstride, bc_nstride, bc_tstride);
  if (ckpt_step == SIMAMBA_SCAN_CKPT_SEQ ? (seqlen > 16 && !x_ckpt) : (o.nchunks > 1 && !x_ckpt)) return SIMAMBA_E_NULLPTR;
  const DetLayout wl = det_layout(batch, dim, seqlen, dstate, ckpt_step);
  if (det && wl.total > 0 && (!workspace || workspace_floats < wl.total)) return SIMAMBA_E_WORKSPACE;
  if (det && !aligned16(workspace)) return SIMAMBA_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e;
  // The five accumulators are zeroed here (the kernel adds into them).  Never a byte outside the five spans:
  // spans that are EXACTLY adjacent in memory (the next one starts where the previous one ends; the Python
  // callers carve them that way out of one allocation) are merged into one memset node, anything else --
  // separately allocated buffers, with whatever lives between them -- gets a memset of its own.
  // The deterministic form's sum pass writes the five spans whole: nothing to clear there (but for an empty problem).
  if (!det || batch == 0 || seqlen == 0) {
    const size_t bc = sizeof(float) * static_cast<size_t>(batch) * dstate * seqlen;
    struct Span { char* p; size_t n; } sp[5] = {{reinterpret_cast<char*>(dA), sizeof(float) * dim * dstate},
                                                 {reinterpret_cast<char*>(dB), bc},
                                                 {reinterpret_cast<char*>(dC), bc},
                                                 {reinterpret_cast<char*>(dD), dD ? sizeof(float) * dim : 0},
                                                 {reinterpret_cast<char*>(ddelta_bias),
                                                  ddelta_bias ? sizeof(float) * dim : 0}};
    for (int i = 1; i < 5; ++i)                      // insertion sort by address
      for (int j = i; j > 0 && sp[j].p < sp[j - 1].p; --j) { const Span t = sp[j]; sp[j] = sp[j - 1]; sp[j - 1] = t; }
    for (int i = 0; i < 5;) {
      if (!sp[i].n) { ++i; continue; }
      char* lo = sp[i].p;
      char* hi = lo + sp[i].n;
      int j = i + 1;
      while (j < 5 && (sp[j].n == 0 || sp[j].p == hi)) { hi += sp[j].n; ++j; }
      if ((e = hipMemsetAsync(lo, 0, static_cast<size_t>(hi - lo), s)) != hipSuccess) return static_cast<int>(e);
      i = j;
    }
  }
  if (batch == 0 || seqlen == 0) return SIMAMBA_OK;
  ScanArgs a{};
  a.u = u; a.delta = delta; a.A = A; a.B = B; a.C = C; a.D = D; a.z = z; a.delta_bias = delta_bias;
  a.dout = dout; a.x_ckpt = const_cast<float*>(x_ckpt);
  a.du = du; a.ddelta = ddelta; a.dA = dA; a.dB = dB; a.dC = dC; a.dD = dD; a.dz = dz;
  a.ddelta_bias = ddelta_bias;
  if (det) {                                                 // the kernels store partials; the sum pass below adds them up
    a.dB = workspace + wl.bc;
    a.dC = a.dB + static_cast<size_t>(batch) * dstate * seqlen;
    a.dA = workspace + wl.a;
    a.dD = dD ? workspace + wl.d : nullptr;
    a.ddelta_bias = ddelta_bias ? workspace + wl.bias : nullptr;
  }
  a.batch = batch; a.dim = dim; a.seqlen = seqlen; a.dstate = dstate;
  a.nchunks = o.nchunks;
  a.softplus = delta_softplus;
  a.z_bs = o.z_bs; a.dz_bs = o.dz_bs; a.bc_bs = o.bc_bs; a.bc_ns = o.bc_ns; a.bc_ts = o.bc_ts;
  a.vec = o.vec;
  if (ckpt_step == SIMAMBA_SCAN_CKPT_SEQ) {
    const int bc_mode = scan_fwd_seq_bc_mode(B, C, io_dtype, a.bc_bs, a.bc_ns, a.bc_ts);
    if (!scan_bwd_seq_ok(batch, dim, seqlen, dstate, delta_softplus, a.vec, a.z_bs, a.dz_bs, z != nullptr, bc_mode,
                         a.bc_ns, a.bc_ts) ||
        !aligned16(A) || !aligned16(x_ckpt))
      return SIMAMBA_E_VARIANT;
    rc = scan_bwd_seq_dispatch(a, io_dtype, bc_mode, s, dt, wdt, dt_bs, dt_ts, dt_rank, det);
    return (rc || !det) ? rc : scan_det_sum(wl, a, dA, dB, dC, dD, ddelta_bias, s);
  }
  if (dt) return SIMAMBA_E_VARIANT;                          // only the sequential kernel forms delta itself
  a.passes = bwd_passes(batch, dim);
  rc = io_dtype == SIMAMBA_F32 ? launch_bwd<float>(a, s, det) : launch_bwd<bf16_t>(a, s, det);
  return (rc || !det) ? rc : scan_det_sum(wl, a, dA, dB, dC, dD, ddelta_bias, s);
}

extern "C" int simamba_selective_scan_bwd_ex(const void* u, const void* delta, const float* A, const void* B,
                                             const void* C, const float* D, const void* z,
                                             const float* delta_bias, const void* dout, const float* x_ckpt,
                                             void* du, void* ddelta, float* dA, float* dB, float* dC, float* dD,
                                             void* dz, float* ddelta_bias, int batch, int dim, int seqlen,
                                             int dstate, int io_dtype, int delta_softplus, long long z_bstride,
                                             long long dz_bstride, long long bc_bstride, long long bc_nstride,
                                             long long bc_tstride, int ckpt_step, int flags, float* workspace,
                                             long long workspace_floats, void* stream) {
  return scan_bwd_impl(u, delta, A, B, C, D, z, delta_bias, dout, x_ckpt, du, ddelta, dA, dB, dC, dD, dz, ddelta_bias,
                       batch, dim, seqlen, dstate, io_dtype, delta_softplus, z_bstride, dz_bstride, bc_bstride,
                       bc_nstride, bc_tstride, ckpt_step, stream, nullptr, nullptr, 0, 0, 0, flags, workspace,
                       workspace_floats);
}

extern "C" int simamba_selective_scan_bwd(const void* u, const void* delta, const float* A, const void* B,
                                          const void* C, const float* D, const void* z,
                                          const float* delta_bias, const void* dout, const float* x_ckpt,
                                          void* du, void* ddelta, float* dA, float* dB, float* dC, float* dD,
                                          void* dz, float* ddelta_bias, int batch, int dim, int seqlen,
                                          int dstate, int io_dtype, int delta_softplus, long long z_bstride,
                                          long long dz_bstride, long long bc_bstride, long long bc_nstride,
                                          long long bc_tstride, int ckpt_step, void* stream) {
  return simamba_selective_scan_bwd_ex(u, delta, A, B, C, D, z, delta_bias, dout, x_ckpt, du, ddelta, dA, dB, dC, dD,
                                       dz, ddelta_bias, batch, dim, seqlen, dstate, io_dtype, delta_softplus,
                                       z_bstride, dz_bstride, bc_bstride, bc_nstride, bc_tstride, ckpt_step, 0,
                                       nullptr, 0, stream);
}

// Backward of simamba_selective_scan_dt_fwd: same operands (+ dout, the forward's 16-step checkpoints); ddelta is the
// gradient with respect to the delta the kernels form (before bias and softplus), as in simamba_selective_scan_bwd.
extern "C" int simamba_selective_scan_dt_bwd_ex(const void* u, const void* xdbl, const void* wdt, const float* A,
                                                const float* D, const void* z, const float* delta_bias,
                                                const void* dout, const float* x_ckpt, void* du, void* ddelta,
                                                float* dA, float* dB, float* dC, float* dD, void* dz,
                                                float* ddelta_bias, int batch, int dim, int seqlen, int dstate,
                                                int dt_rank, int io_dtype, long long z_bstride, long long dz_bstride,
                                                long long xdbl_bstride, long long xdbl_tstride, int flags,
                                                float* workspace, long long workspace_floats, void* stream) {
  int rc;
  if ((rc = scan_check_flags(flags))) return rc;
  if (dstate != kMaxState) return SIMAMBA_E_DSTATE;
  if ((rc = check_io_dtype(io_dtype)) || (rc = scan_check_dt_rank(dt_rank, io_dtype))) return rc;
  if (batch > 0 && seqlen > 0 && (!xdbl || !wdt || !z)) return SIMAMBA_E_NULLPTR;
  const XdblOperands x = scan_xdbl_operands(xdbl, wdt, batch, seqlen, dt_rank, io_dtype, xdbl_bstride, xdbl_tstride);
  if (!x.ok) return SIMAMBA_E_VARIANT;
  return scan_bwd_impl(u, nullptr, A, x.B, x.C, D, z, delta_bias, dout, x_ckpt, du, ddelta, dA, dB, dC, dD, dz,
                       ddelta_bias, batch, dim, seqlen, dstate, io_dtype, 1, z_bstride, dz_bstride, x.bs, 1, x.ts,
                       SIMAMBA_SCAN_CKPT_SEQ, stream, xdbl, wdt, x.bs, x.ts, dt_rank, flags, workspace,
                       workspace_floats);
}

extern "C" int simamba_selective_scan_dt_bwd(const void* u, const void* xdbl, const void* wdt, const float* A,
                                             const float* D, const void* z, const float* delta_bias, const void* dout,
                                             const float* x_ckpt, void* du, void* ddelta, float* dA, float* dB,
                                             float* dC, float* dD, void* dz, float* ddelta_bias, int batch, int dim,
                                             int seqlen, int dstate, int dt_rank, int io_dtype, long long z_bstride,
                                             long long dz_bstride, long long xdbl_bstride, long long xdbl_tstride,
                                             void* stream) {
  return simamba_selective_scan_dt_bwd_ex(u, xdbl, wdt, A, D, z, delta_bias, dout, x_ckpt, du, ddelta, dA, dB, dC, dD,
                                          dz, ddelta_bias, batch, dim, seqlen, dstate, dt_rank, io_dtype, z_bstride,
                                          dz_bstride, xdbl_bstride, xdbl_tstride, 0, nullptr, 0, stream);
}
