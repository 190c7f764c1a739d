// Host side of the selective scan, shared by its four files: ONE declaration of every function that crosses a file
// (the defining files include this too, so definitions are checked against it) and ONE statement of what the entry
// points make of their arguments -- the checks, the "0 = contiguous" strides, and `vec`.
#pragma once
#include <cstdint>
#include <initializer_list>
#include "host_common.h"
#include "scan_common.h"

namespace simamba {

// ---- scan_fwd_seq.hip -----------------------------------------------------------------------------------------------
int scan_fwd_seq_dispatch(const void* u, const void* delta, const float* A, const void* B, const void* C, const float* D,
                          const void* z, const float* delta_bias, void* out, float* x_ckpt, int ckpt_step,
                          float* last_state, int batch, int dim, int seqlen, int io_dtype, long long z_bs,
                          long long bc_bs, long long bc_ns, long long bc_ts, int nchunks128, int lpc, hipStream_t s,
                          const void* dt, const void* wdt, long long dt_bs, long long dt_ts, int dt_rank);
int scan_fwd_seq_bc_mode(const void* B, const void* C, int io_dtype, long long bc_bs, long long bc_ns, long long bc_ts);
int scan_fwd_seq_mix_c4(int batch, int dim);
// ---- scan_bwd_seq.hip -----------------------------------------------------------------------------------------------
bool scan_bwd_seq_ok(int batch, int dim, int seqlen, int dstate, int softplus, int vec, long long z_bs, long long dz_bs,
                     bool has_z, int bc_mode, long long bc_ns, long long bc_ts);
int scan_bwd_seq_dispatch(const ScanArgs& a, int io_dtype, int bc_mode, hipStream_t s, const void* dt, const void* wdt,
                          long long dt_bs, long long dt_ts, int dt_rank, bool det);

// ---- argument checks: one each, so that every entry point keeps the order it has always reported them in ------------
inline int scan_check_shape(int batch, int dim, int seqlen) {
  return (batch < 0 || dim <= 0 || seqlen < 0 || batch > 65535) ? SIMAMBA_E_SHAPE : SIMAMBA_OK;
}
inline int scan_check_ckpt(int& ckpt_step) {                   // 0 = the row-scan layout
  if (ckpt_step == 0) ckpt_step = SIMAMBA_SCAN_CKPT_ROW;
  return (ckpt_step != SIMAMBA_SCAN_CKPT_ROW && ckpt_step != SIMAMBA_SCAN_CKPT_SEQ) ? SIMAMBA_E_VARIANT : SIMAMBA_OK;
}
inline int scan_check_dstate(int dstate) { return (dstate < 1 || dstate > kMaxState) ? SIMAMBA_E_DSTATE : SIMAMBA_OK; }
inline int scan_check_flags(int flags) { return (flags & ~SIMAMBA_BWD_DETERMINISTIC) ? SIMAMBA_E_VARIANT : SIMAMBA_OK; }
// the order of simamba_selective_scan_fwd and of the backward
inline int scan_check_args(int batch, int dim, int seqlen, int dstate, int io_dtype, int& ckpt_step) {
  int rc;
  if ((rc = scan_check_shape(batch, dim, seqlen)) || (rc = scan_check_ckpt(ckpt_step)) ||
      (rc = scan_check_dstate(dstate)) || (rc = check_io_dtype(io_dtype)))
    return rc;
  return SIMAMBA_OK;
}

inline uintptr_t addr_or(std::initializer_list<const void*> ps) {
  uintptr_t o = 0;
  for (const void* p : ps) o |= reinterpret_cast<uintptr_t>(p);
  return o;
}

// What every entry point derives from checked arguments (scan_host.hip).  Strides in elements, 0 = contiguous on the
// way in; `vec` = 16-byte access is legal: every activation operand (`act_addr_or`: the OR of their addresses, NULL
// ones included) on a 16-byte boundary, rows and the batch strides of z / dz whole packs.
struct ScanOperands {
  size_t esz;
  int nchunks;                        // 128-step checkpoints (simamba_scan_num_chunks)
  int vec;
  long long z_bs, dz_bs, bc_bs, bc_ns, bc_ts;
};
ScanOperands scan_operands(int dim, int seqlen, int dstate, int io_dtype, uintptr_t act_addr_or, bool has_z,
                           long long z_bstride, long long dz_bstride, long long bc_bstride, long long bc_nstride,
                           long long bc_tstride);

// The dt entry points' B / C: columns [dt_rank, dt_rank + 16) and [dt_rank + 16, dt_rank + 32) of the token-major
// x_proj output (state stride 1).  `ok`: xdbl, wdt, both strides and the dt columns keep 16-byte packs whole and the
// batch offsets stay below 2^30 elements.
struct XdblOperands { const void* B; const void* C; long long bs, ts; bool ok; };
XdblOperands scan_xdbl_operands(const void* xdbl, const void* wdt, int batch, int seqlen, int dt_rank, int io_dtype,
                                long long xdbl_bstride, long long xdbl_tstride);
inline int scan_check_dt_rank(int dt_rank, int io_dtype) {
  const int pack = io_pack(io_dtype);
  return (dt_rank < pack || dt_rank > 24 || dt_rank % pack) ? SIMAMBA_E_SHAPE : SIMAMBA_OK;
}

}  // namespace simamba
