// The tile walk and the software pipeline of the fused conv1d + x_proj + dt_proj kernel.  The walk (XdtWalk, Cursor,
// advance, uniform) and the host's grid rule (xdt_grid) serve its fp32 form (xdt_proj.hip) and its bf16 form
// (xdt_proj_bf16.hip) alike.  xdt_pipeline is the order in which a workgroup does its work; a form supplies what
// differs -- its staging, its MFMAs, its LDS images (the Form members listed there).  The fp32 form runs it.  The
// bf16 form keeps the same statements in its own kernel: through this template it compiled to one or two more VGPRs
// than the form it replaced (profiles/xdt_walk.json), with the same results and times -- a change to the pipeline is
// made in both places.
//
// Schedule.  The first form of this kernel ran load -> LDS -> 16 MFMAs -> barrier per step and phase 2 after phase 1:
// 51 % matrix-pipe busy, phase 1 + phase 2 = 72 + 50 us with nothing of the one under the other (a dependent chain of
// these MFMAs alone reaches 89 % of the pipe: tools/mfma_probe.hip, so the chain is not the limit -- what sits between
// the bursts is).  Now every wave overlaps its own work, four steps deep (a step = 32 d of one tile; g counts steps
// across the tiles a workgroup walks):
//     iteration g:   the MFMAs of step g (fp32: 16)              (operand registers read in iteration g - 1)
//                    one 32 x 32 block of delta of the PREVIOUS tile every other iteration (fp32: 12 MFMAs, 16 row stores)
//                    conv + LDS store of step g + 2              (global loads issued in iteration g - 2 -> buffer g & 1)
//                    issue the global loads of step g + 4
//                    ds_read the operands of step g + 1          (tile buffer (g + 1) & 1 -> the registers just used)
//                    one barrier
// so the x reads, the x_conv / delta writes and the matrix pipe run for the whole kernel instead of taking turns; only
// the last tile's delta blocks are left for a tail.  The body of an iteration is ONE basic block: every global access
// is a buffer instruction whose out-of-range lanes (tile edge, rows past S or R, steps past the last tile: the
// descriptor of such a step has zero records) load zeros / store nothing, so nothing in it branches, hipcc's scheduler
// lays the VALU and memory work between the MFMAs, and its s_waitcnt bookkeeping comes out counted (vmcnt(N), the
// loads of the two steps ahead stay in flight) where predicated loads made it drain to vmcnt(0) at every use.
// Measured on the fp32 form at (64, 768, 1024) by elimination (tools/xdt_probe.hip): with the MFMAs removed
// the kernel takes 101 us (plain) / 167 us (conv) of its 118 / 180 us -- it is bound by how many bytes 8 waves per CU
// keep in flight around a per-step barrier, not by the matrix pipe or the instruction order (sched_group_barrier /
// iglp_opt interleaves: no change).
#pragma once
#include "mfma_device.h"

namespace simamba {

// ---- the walk ------------------------------------------------------------------------------------------------------------
// Wave-uniform constants: nk steps per tile (even), tps tiles per sample, the tile stride of a workgroup (= the grid
// size) as (gq samples, gr tiles of a sample), ntw tiles of this workgroup: wg, wg + nwg, ... (the host evens the
// counts out and keeps all workgroups resident).  Kept in SGPRs (integer division runs on the VALU).
struct XdtWalk {
  int nk, tps, gq, gr, ntw;
};
__device__ __forceinline__ XdtWalk xdt_walk(int batch, int tiles_per_sample, int nk) {
  const int tps = __builtin_amdgcn_readfirstlane(tiles_per_sample);
  const int ntiles = batch * tps;
  const int nwg = static_cast<int>(gridDim.x), wg = static_cast<int>(blockIdx.x);
  const int ntw = __builtin_amdgcn_readfirstlane((ntiles - wg + nwg - 1) / nwg);
  const int gq = __builtin_amdgcn_readfirstlane(nwg / tps), gr = nwg - gq * tps;
  return XdtWalk{nk, tps, gq, gr, ntw};
}

// A step of the walk: tile `j` of this workgroup (sample q, tile r of the sample), step ks of it.  Advancing never divides.
struct Cursor {
  int j, ks, q, r;
};
__device__ __forceinline__ void advance(Cursor& c, const XdtWalk& w) {   // one step forward
  c.ks += 1;
  const bool wrap = c.ks >= w.nk;
  c.ks -= wrap ? w.nk : 0;
  c.j += wrap ? 1 : 0;
  c.r += wrap ? w.gr : 0;
  c.q += wrap ? w.gq : 0;
  const bool carry = c.r >= w.tps;
  c.r -= carry ? w.tps : 0;
  c.q += carry ? 1 : 0;
}
// Cursor fields enter descriptors and scalar offsets, and reach them only through uniform().  In the loop they live in
// SGPRs anyway; in the prologue hipcc had them in VGPRs, could not prove them uniform and wrapped those buffer loads in
// waterfall loops -- whose loads its s_waitcnt bookkeeping counts once although the counter sees every trip: the first
// conv read its neighbours' packs (DPP) before they had landed, on some workgroups, on some runs
// (tests/test_gpu_xdt_proj.py caught it on the bf16 form; the fp32 form had the same loops).  readfirstlane makes the
// uniformity explicit: no waterfall, and hipcc's vmcnt counts stay exact.
__device__ __forceinline__ Cursor uniform(const Cursor& c) {   // the same values, provably wave-uniform (SGPRs)
  return Cursor{__builtin_amdgcn_readfirstlane(c.j), __builtin_amdgcn_readfirstlane(c.ks),
                __builtin_amdgcn_readfirstlane(c.q), __builtin_amdgcn_readfirstlane(c.r)};
}

// ---- the pipeline ------------------------------------------------------------------------------------------------------
// Form: the per-form object.  What the pipeline asks of it:
//   Stage, Ops                        registers of a step in flight (global loads) / of a step's MFMA operands
//   issue(Stage&, Cursor)             global loads of a step (zeros past the tile's end and for a step past the last tile)
//   stage(const Stage&, Cursor, buf)  conv + SiLU (kConv), x_conv out, LDS tiles of the step
//   read_ops(Ops&, buf)               LDS tile buffer -> operand registers
//   step_mfma(const Ops&, acc)        the MFMAs of a step
//   wload(u)                          request the Wdt rows of delta unit u (and u + 1: same d-block)
//   unit_mfma(u, o), unit_store(u, o, q, r)   delta of one (d-block, token block) unit of tile (sample q, tile r)
//   tile_done(acc, q, r)              the tile is complete: x_dbl out, its dt rows into LDS, accumulator cleared
//   wave, ndb                         wave w owns the 32-channel blocks w, w + 4, ... of the ndb blocks of delta: a unit
//                                     past the wave's last one addresses d-block >= ndb and falls out of range
// delta == NULL (want_delta false): the scan forms delta itself (csrc/scan_fwd_seq.hip) and no unit runs.
template <typename Form>
__device__ __forceinline__ void xdt_pipeline(Form& f, const XdtWalk& w, bool want_delta) {
  const int nwg = static_cast<int>(gridDim.x), wg = static_cast<int>(blockIdx.x);
  const int nk = w.nk, ndb = f.ndb;
  const int nunits = f.wave < ndb ? 2 * ((ndb - f.wave + 3) / 4) : 0;   // units of this wave per tile
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  typename Form::Stage s0, s1;
  typename Form::Ops o0;
  const int q0 = __builtin_amdgcn_readfirstlane(wg / w.tps);
  Cursor cm{0, 0, q0, wg - q0 * w.tps};                    // step g            (MFMAs)
  Cursor cr = cm, cs = cm, cl = cm;
  advance(cr, w);                                          // step g + 1        (operand reads)
  advance(cs, w); advance(cs, w);                          // step g + 2        (conv + LDS store)
  {
    // prologue: steps 0 and 1 staged, 2 and 3 in flight, operands of step 0 in registers
    f.issue(s0, cm);
    f.issue(s1, cr);
    // What protects the first conv, which reads its neighbours' packs through DPP, is hipcc's own counted wait for
    // that pack's load, exact as long as no waterfall loop wraps a buffer load (uniform(), above).  The statement below
    // is NOT that protection: it orders memory operations only, and in the .s of both forms the DPP moves of the first
    // pack sit in front of it.  It drains the prologue's other loads once per workgroup; do not rely on it for more.
    if (Form::kHasConv) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    f.stage(s0, cm, 0);
    f.issue(s0, cs);
    f.stage(s1, cr, 1);
    cl = cs; advance(cl, w);
    f.issue(s1, cl);
    advance(cl, w);                                        // step g + 4        (global loads)
    __syncthreads();
    f.read_ops(o0, 0);
    __syncthreads();                                       // buffer 0 is restaged in iteration 0
  }
  int pq = 0, pr = 0;                                      // the previous tile (delta units)
  // One iteration; kOdd: the odd step of a pair (delta unit ks >> 1 of the previous tile when kUnits).
  auto iteration = [&](typename Form::Stage& st, const int buf, auto odd_tag, auto units_tag) {
    constexpr bool kOdd = decltype(odd_tag)::value, kUnits = decltype(units_tag)::value;
    f32x16 o;
    const int u = cm.ks >> 1;
    if (kOdd && kUnits) f.unit_mfma(u, o);
    f.step_mfma(o0, acc);
    f.stage(st, cs, buf);
    if (kOdd && kUnits) {
      f.unit_store(u, o, pq, pr);
      f.wload(u + 1);
    }
    f.issue(st, cl);
    f.read_ops(o0, buf ^ 1);                               // step g + 1, once the MFMAs above have taken step g's
    advance(cm, w); advance(cr, w); advance(cs, w); advance(cl, w);
    __syncthreads();
  };
  using T = std::true_type;
  using F = std::false_type;
  for (int j = 0; j < w.ntw; ++j) {
    if (j == 0 || !want_delta) {
      for (int k = 0; k < nk; k += 2) {                    // nk is even: a tile starts on an even step
        iteration(s0, 0, F{}, F{});
        iteration(s1, 1, T{}, F{});
      }
    } else {
      f.wload(0);
      for (int k = 0; k < nk; k += 2) {
        iteration(s0, 0, F{}, T{});
        iteration(s1, 1, T{}, T{});
      }
      for (int u = nk / 2; u < nunits; ++u) {              // ndb % 4 != 0: units past nk / 2 (none at D = 768)
        f32x16 o;
        if (!(u & 1)) f.wload(u);
        f.unit_mfma(u, o);
        f.unit_store(u, o, pq, pr);
      }
      // those units read the previous tile's dt rows, which the waves that have none are about to overwrite below
      if (2 * ((ndb + 3) / 4) > nk / 2) __syncthreads();
    }
    const int tile = wg + j * nwg;
    pq = tile / w.tps; pr = tile - pq * w.tps;
    f.tile_done(acc, pq, pr);
    __syncthreads();
  }
  // tail: delta of the last tile
  for (int u = 0; want_delta && u < nunits; ++u) {
    f32x16 o;
    if (!(u & 1)) f.wload(u);
    f.unit_mfma(u, o);
    f.unit_store(u, o, pq, pr);
  }
}

// ---- host: the grid --------------------------------------------------------------------------------------------------
// Every workgroup the same number of tiles, all workgroups resident together (`resident` = workgroups per CU x 256
// CUs).  Tiles per workgroup at full residency, evened out (per divides ntiles) when a divisor is near: a prime tile
// count must not collapse the grid to a few workgroups -- the kernel takes uneven counts (ntw), evenness is only tidier.
inline unsigned xdt_grid(long long ntiles, long long resident) {
  if (ntiles <= resident) return static_cast<unsigned>(ntiles);
  const long long per0 = (ntiles + resident - 1) / resident;
  long long per = per0;
  while (ntiles % per && per < 2 * per0) ++per;
  return static_cast<unsigned>(ntiles % per == 0 ? ntiles / per : resident);
}

}  // namespace simamba
