// bf16 form of the fused conv1d + SiLU -> x_proj -> dt_proj kernel (xdt_proj.hip holds the fp32 form, xdt_walk.h the
// walk and the story of the schedule): bf16 operands and results, v_mfma_f32_32x32x16_bf16, fp32 accumulation.
//
// What the reference's mixer does under torch.autocast (tools/runner_pretrain.py:243; upstream mamba_inner_fn reached
// from models/block.py:72): the conv output, x_dbl and delta are bf16 tensors, each product accumulates in fp32 and
// rounds once.  The same roundings happen here: silu(conv(x)) is rounded to bf16 and that value is both stored as
// x_conv and fed to the matrix cores; x_dbl is rounded when it leaves the accumulator and the ROUNDED dt rows are the
// B operand of the delta product; delta is rounded when stored.
//
// Differences from the fp32 form, all forced by the operand shape of the 16-bit MFMA (a lane carries 8 consecutive k):
//   * x tile in LDS stays [d][t] (t contiguous, as loaded); the B operand -- 8 consecutive d for one t -- is gathered with
//     8 ds_read_u16 per MFMA (two lanes share every bank word: conflict-free; a transposing store would put 16 lanes
//     on one bank);
//   * Wx tile [s][d] bf16, 80-byte pitch: the A operand is one ds_read_b128 per MFMA;
//   * the dt rows of a finished tile wait in LDS as [t][r] bf16 (an accumulator lane owns 4 consecutive r of one t:
//     one 8-byte store), rows r >= R zeroed (they pad K = R = 24 to the 32 of two MFMAs), read back as ds_read_b128;
//   * delta leaves as 2-byte stores, 32 lanes on 64 contiguous bytes of a row (the other half of the line follows from
//     the unit of the neighbouring token block, two iterations later).
// A step moves half the bytes of the fp32 form and needs an eighth of its MFMAs; registers allow 3 workgroups per CU.
#include "conv_device.h"
#include "xdt_walk.h"

namespace simamba {

constexpr int kHThreads = 256;
constexpr int kHTok = 64;           // tokens per tile
constexpr int kHKS = 32;            // d per step
constexpr int kHXP = kHTok;         // x tile pitch (bf16 elements): 128-byte rows
constexpr int kHWP = kHKS + 8;      // Wx tile pitch: 80 bytes
constexpr int kHDP = 32 + 8;        // dt image pitch: 80 bytes
constexpr int kHMaxDConv = 1024;

struct XdtHArgs {
  const uint16_t* x;      // (batch, D, L) bf16; with kConv the conv INPUT
  const float* cw;        // (D, 4) fp32 taps
  const float* cb;        // (D) fp32 or NULL
  uint16_t* xconv;        // kConv: (batch, D, L) bf16
  const uint16_t* wx;     // (S, D) bf16
  const uint16_t* wdt;    // (D, R) bf16
  uint16_t* xdbl;         // (batch, L, S) bf16
  uint16_t* delta;        // (batch, D, L) bf16
  int batch, D, L, S, R;
  long long x_bs;
};

__device__ __forceinline__ unsigned hdpp_prev(unsigned v) {
  return static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), DPP_ROW_SHR + 1, 0xf, 0xf, false));
}

template <bool kConv>
__global__ __launch_bounds__(kHThreads, 3) void xdt_proj_bf16_kernel(XdtHArgs p) {
  __shared__ __attribute__((aligned(16))) uint16_t sX[2][kHKS * kHXP];      // [d][t]
  __shared__ __attribute__((aligned(16))) uint16_t sW[2][64 * kHWP];        // [s][d]
  __shared__ __attribute__((aligned(16))) uint16_t sDt[kHTok * kHDP];       // [t][r] of the tile just finished
  __shared__ __attribute__((aligned(16))) float sTap[kConv ? kHMaxDConv * 4 : 4];
  __shared__ float sBias[kConv ? kHMaxDConv : 1];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, hh = lane >> 5;
  const int sblk = wave & 1, tblk = wave >> 1;
  const int D = p.D, L = p.L, S = p.S, R = p.R;
  const XdtWalk w = xdt_walk(p.batch, (L + kHTok - 1) / kHTok, D / kHKS);   // steps per tile: even (host: D % 64 == 0)
  if (w.ntw <= 0) return;
  const int nk = w.nk, tps = w.tps, ntw = w.ntw;
  const int nwg = static_cast<int>(gridDim.x), wg = static_cast<int>(blockIdx.x);
  const int ndb = D / 32;
  const int nunits = wave < ndb ? 2 * ((ndb - wave + 3) / 4) : 0;
  const unsigned sample_bytes = static_cast<unsigned>(D) * static_cast<unsigned>(L) * 2u;

  for (int i = tid; i < kHTok * kHDP; i += kHThreads) sDt[i] = 0;
  if (kConv) {
    for (int d = tid; d < D; d += kHThreads) {
      *reinterpret_cast<float4*>(&sTap[4 * d]) = *reinterpret_cast<const float4*>(p.cw + 4 * static_cast<size_t>(d));
      sBias[d] = p.cb ? p.cb[d] : 0.f;
    }
  }
  __syncthreads();

  // ---- staging identities: x tile 32 d x 64 t = 256 packs of 8; thread -> (d = tid >> 3, t8 = 8 (tid & 7)) -----------
  const int xd = tid >> 3, xt = 8 * (tid & 7);
  const bool first = (tid & 7) == 0;
  const unsigned xoff = (static_cast<unsigned>(xd) * L + xt) * 2u;
  // Wx tile 64 s x 32 d = 256 packs of 8; thread -> (s = tid >> 2, d8 = 8 (tid & 3))
  const int ws = tid >> 2, wd = 8 * (tid & 3);
  const unsigned woff = ws < S ? (static_cast<unsigned>(ws) * D + wd) * 2u : kOob;
  const rsrc_t rs_wx = make_rsrc(p.wx, static_cast<unsigned>(S) * D * 2u);
  const rsrc_t rs_wdt = make_rsrc(p.wdt, static_cast<unsigned>(D) * R * 2u);

  struct Stage { uint4 rx, rw, rh; };
  struct Ops { uint4 a[2], b[2]; };

  auto issue = [&](Stage& st, const Cursor& c_) {
    const Cursor c = uniform(c_);
    const rsrc_t rs = make_rsrc(p.x + static_cast<size_t>(c.q) * p.x_bs, c.j < ntw ? sample_bytes : 0u);
    const int t0 = c.r * kHTok;
    const unsigned soff = (static_cast<unsigned>(c.ks) * kHKS * L + t0) * 2u;
    const bool xok = t0 + xt < L;                          // L % 8 == 0: a pack is all in or all out
    st.rx = bload16<uint4>(rs, xok ? xoff : kOob, soff);
    // the pack in front of the tile for the row's first lane (t0 > 0: soff >= 128, so soff - 16 does not wrap)
    if (kConv) st.rh = bload16<uint4>(rs, (first && t0 > 0) ? xoff : kOob, soff - 16u);
    st.rw = bload16<uint4>(rs_wx, woff, static_cast<unsigned>(c.ks) * kHKS * 2u);
  };
  auto stage = [&](const Stage& st, const Cursor& c_, int buf) {
    const Cursor c = uniform(c_);
    uint4 v = st.rx;
    if (kConv) {
      const rsrc_t rs_xc = make_rsrc(p.xconv + static_cast<size_t>(c.q) * D * L, c.j < ntw ? sample_bytes : 0u);
      const int t0 = c.r * kHTok;
      const unsigned soff = (static_cast<unsigned>(c.ks) * kHKS * L + t0) * 2u;
      const bool xok = t0 + xt < L;
      const int d = c.ks * kHKS + xd;
      // the three steps in front of the pack: elements 5, 6, 7 of the neighbouring lane's pack (DPP on every lane,
      // pinned in front of the select: xdt_proj.hip on why), the halo load for the row's first lane
      unsigned qz = hdpp_prev(v.z), qw = hdpp_prev(v.w);
      asm volatile("" : "+v"(qz), "+v"(qw));
      const unsigned pz = first ? st.rh.z : qz, pw = first ? st.rh.w : qw;
      const float win[11] = {bf16_hi(pz),  bf16_lo(pw),  bf16_hi(pw),  bf16_lo(v.x), bf16_hi(v.x), bf16_lo(v.y),
                             bf16_hi(v.y), bf16_lo(v.z), bf16_hi(v.z), bf16_lo(v.w), bf16_hi(v.w)};
      const float4 tp = *reinterpret_cast<const float4*>(&sTap[4 * d]);
      const float w4[4] = {tp.x, tp.y, tp.z, tp.w};
      const float bias = sBias[d];
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float acc = conv_pre(w4, win + e, bias);
        o[e] = acc * sigmoid_f(acc);
      }
      v = make_uint4(bf16_pack2(o[0], o[1]), bf16_pack2(o[2], o[3]), bf16_pack2(o[4], o[5]),
                     bf16_pack2(o[6], o[7]));
      bstore16(v, rs_xc, xok ? xoff : kOob, soff);
      if (!xok) v = make_uint4(0u, 0u, 0u, 0u);
    }
    *reinterpret_cast<uint4*>(&sX[buf][xd * kHXP + xt]) = v;
    *reinterpret_cast<uint4*>(&sW[buf][ws * kHWP + wd]) = st.rw;
  };
  // operands of a step: MFMA j contracts d = 16 j + 8 hh + 0..7
  auto read_ops = [&](Ops& o, int buf) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      o.a[j] = *reinterpret_cast<const uint4*>(&sW[buf][(sblk * 32 + li) * kHWP + 16 * j + 8 * hh]);
      const uint16_t* col = &sX[buf][(16 * j + 8 * hh) * kHXP + tblk * 32 + li];
      unsigned w[4];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        w[e] = static_cast<unsigned>(col[(2 * e) * kHXP]) | (static_cast<unsigned>(col[(2 * e + 1) * kHXP]) << 16);
      o.b[j] = make_uint4(w[0], w[1], w[2], w[3]);
    }
  };

  // ---- delta = Wdt @ dt of a finished tile, one (d-block, token block) unit at a time ------------------------------
  uint4 wa[2];
  // Wdt row of 2 R bytes: MFMA 0 takes r = 8 hh .. + 7, MFMA 1 r = 16 + 8 hh .. + 7 (past R: zeros)
  unsigned wdoff[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) wdoff[j] = (16 * j + 8 * hh < R) ? (static_cast<unsigned>(li) * R + 16 * j + 8 * hh) * 2u : kOob;
  const unsigned dvoff = (static_cast<unsigned>(4 * hh) * L + li) * 2u;
  auto wload = [&](int u_) {
    const int u = __builtin_amdgcn_readfirstlane(u_);
    const int db = wave + 4 * (u >> 1);
    const unsigned soff = db < ndb ? static_cast<unsigned>(db) * 32u * R * 2u : 0u;
#pragma unroll
    for (int j = 0; j < 2; ++j) wa[j] = bload16<uint4>(rs_wdt, db < ndb ? wdoff[j] : kOob, soff);
  };
  auto unit_mfma = [&](int u, f32x16& o) {
    const uint16_t* dt = &sDt[((u & 1) * 32 + li) * kHDP + 8 * hh];
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const uint4 b = *reinterpret_cast<const uint4*>(dt + 16 * j);
      o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wa[j]), __builtin_bit_cast(bf16x8, b), o,
                                                  0, 0, 0);
    }
  };
  auto unit_store = [&](int u_, const f32x16& o, int q_, int r_) {
    const int u = __builtin_amdgcn_readfirstlane(u_), q = __builtin_amdgcn_readfirstlane(q_),
              r = __builtin_amdgcn_readfirstlane(r_);
    const int db = wave + 4 * (u >> 1);
    const rsrc_t rs = make_rsrc(p.delta + static_cast<size_t>(q) * D * L, db < ndb ? sample_bytes : 0u);
    const int tb0 = r * kHTok + (u & 1) * 32;
    const unsigned voff = tb0 + li < L ? dvoff : kOob;
    const unsigned base = (static_cast<unsigned>(db) * 32u * L + tb0) * 2u;
#pragma unroll
    for (int i = 0; i < 16; ++i)
      bstore2(f32_to_bf16(o[i]), rs, voff, base + static_cast<unsigned>((i & 3) + 8 * (i >> 2)) * L * 2u);
  };

  // ---- the pipeline: the statements of xdt_pipeline (xdt_walk.h), kept here because moved into that template this form
  // compiles to one or two more VGPRs than it does below (profiles/xdt_walk.json); a change there is made here too ----
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  Stage s0, s1;
  Ops o0;
  const int q0 = __builtin_amdgcn_readfirstlane(wg / tps);
  Cursor cm{0, 0, q0, wg - q0 * tps};
  Cursor cr = cm, cs = cm, cl = cm;
  advance(cr, w);
  advance(cs, w); advance(cs, w);
  {
    issue(s0, cm);
    issue(s1, cr);
    if (kConv) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // as in xdt_pipeline (xdt_walk.h): see the note there
    stage(s0, cm, 0);
    issue(s0, cs);
    stage(s1, cr, 1);
    cl = cs; advance(cl, w);
    issue(s1, cl);
    advance(cl, w);
    __syncthreads();
    read_ops(o0, 0);
    __syncthreads();
  }
  int pq = 0, pr = 0;
  auto iteration = [&](Ops& cur, Stage& st, const int buf, auto odd_tag, auto units_tag) {
    constexpr bool kOdd = decltype(odd_tag)::value, kUnits = decltype(units_tag)::value;
    f32x16 o;
    const int u = cm.ks >> 1;
    if (kOdd && kUnits) unit_mfma(u, o);
#pragma unroll
    for (int j = 0; j < 2; ++j)
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, cur.a[j]),
                                                    __builtin_bit_cast(bf16x8, cur.b[j]), acc, 0, 0, 0);
    stage(st, cs, buf);
    if (kOdd && kUnits) {
      unit_store(u, o, pq, pr);
      wload(u + 1);
    }
    issue(st, cl);
    read_ops(cur, buf ^ 1);
    advance(cm, w); advance(cr, w); advance(cs, w); advance(cl, w);
    __syncthreads();
  };
  using T = std::true_type;
  using F = std::false_type;
  const bool want_delta = p.delta != nullptr;             // NULL: the scan forms delta itself (csrc/scan_fwd_seq.hip)
  for (int j = 0; j < ntw; ++j) {
    if (j == 0 || !want_delta) {
      for (int k = 0; k < nk; k += 2) {
        iteration(o0, s0, 0, F{}, F{});
        iteration(o0, s1, 1, T{}, F{});
      }
    } else {
      wload(0);
      for (int k = 0; k < nk; k += 2) {
        iteration(o0, s0, 0, F{}, T{});
        iteration(o0, s1, 1, T{}, T{});
      }
      for (int u = nk / 2; u < nunits; ++u) {              // ndb % 4 != 0: units past nk / 2
        f32x16 o;
        if (!(u & 1)) wload(u);
        unit_mfma(u, o);
        unit_store(u, o, pq, pr);
      }
      if (2 * ((ndb + 3) / 4) > nk / 2) __syncthreads();   // those units still read the dt image rewritten below
    }
    // ---- the tile is complete: x_dbl out (token-major, bf16), its ROUNDED dt rows into LDS, accumulator cleared ---------
    // accumulator register r holds Y[s = sblk*32 + (r & 3) + 8 (r >> 2) + 4 hh][t = tblk*32 + li]
    {
      const int tile = wg + j * nwg;
      const int b = tile / tps, t0 = (tile - b * tps) * kHTok;
      pq = b; pr = tile - b * tps;
      const int t = t0 + tblk * 32 + li;
      uint16_t* row = p.xdbl + (static_cast<size_t>(b) * L + t) * S;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int s = sblk * 32 + 8 * g + 4 * hh;
        const uint2 pk =
            make_uint2(bf16_pack2(acc[4 * g], acc[4 * g + 1]), bf16_pack2(acc[4 * g + 2], acc[4 * g + 3]));
        if (t < L && s < S) *reinterpret_cast<uint2*>(row + s) = pk;        // S % 4 == 0
        if (sblk == 0)                                                        // r = s: rows past R pad K with zeros
          *reinterpret_cast<uint2*>(&sDt[(tblk * 32 + li) * kHDP + 8 * g + 4 * hh]) = s < R ? pk : make_uint2(0u, 0u);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    }
    __syncthreads();
  }
  for (int u = 0; want_delta && u < nunits; ++u) {         // tail: delta of the last tile
    f32x16 o;
    if (!(u & 1)) wload(u);
    unit_mfma(u, o);
    unit_store(u, o, pq, pr);
  }
}

}  // namespace simamba

using namespace simamba;

// Host entry used by xdt_proj.hip's launchers for io_dtype == SIMAMBA_BF16 (same argument checks there).
int xdt_launch_bf16(const void* x, const float* cw, const float* cb, const void* wx, const void* wdt, void* xconv,
                    void* xdbl, void* delta, int batch, int D, int L, int S, int R, long long x_bs, bool conv,
                    hipStream_t stream) {
  XdtHArgs a{};
  a.x = static_cast<const uint16_t*>(x); a.cw = cw; a.cb = cb; a.xconv = static_cast<uint16_t*>(xconv);
  a.wx = static_cast<const uint16_t*>(wx); a.wdt = static_cast<const uint16_t*>(wdt);
  a.xdbl = static_cast<uint16_t*>(xdbl); a.delta = static_cast<uint16_t*>(delta);
  a.batch = batch; a.D = D; a.L = L; a.S = S; a.R = R; a.x_bs = x_bs;
  // all workgroups resident together: 3 per CU, 256 CUs
  const dim3 grid(xdt_grid(static_cast<long long>(batch) * ((L + kHTok - 1) / kHTok), 768));
  if (conv)
    hipLaunchKernelGGL(xdt_proj_bf16_kernel<true>, grid, dim3(kHThreads), 0, stream, a);
  else
    hipLaunchKernelGGL(xdt_proj_bf16_kernel<false>, grid, dim3(kHThreads), 0, stream, a);
  return static_cast<int>(hipGetLastError());
}
