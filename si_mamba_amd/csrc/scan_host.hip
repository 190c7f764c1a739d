// The scan entry points' operand normaliser (scan_host.h): out of line, so that simamba_scan_seq_applicable and the
// forward / backward entry points run the same code, not copies of it.
#include "scan_host.h"

namespace simamba {

ScanOperands scan_operands(int dim, int seqlen, int dstate, int io_dtype, uintptr_t act_addr_or, bool has_z,
                           long long z_bstride, long long dz_bstride, long long bc_bstride, long long bc_nstride,
                           long long bc_tstride) {
  ScanOperands o{};
  o.esz = io_esz(io_dtype);
  o.nchunks = simamba_scan_num_chunks(seqlen);
  o.z_bs = z_bstride ? z_bstride : static_cast<long long>(dim) * seqlen;
  o.dz_bs = dz_bstride ? dz_bstride : static_cast<long long>(dim) * seqlen;
  if (!bc_bstride && !bc_nstride && !bc_tstride) {
    bc_bstride = static_cast<long long>(dstate) * seqlen; bc_nstride = seqlen; bc_tstride = 1;
  }
  o.bc_bs = bc_bstride; o.bc_ns = bc_nstride; o.bc_ts = bc_tstride;
  o.vec = ((seqlen * o.esz) % 16 == 0) && (act_addr_or & 15u) == 0 &&
          (!has_z || ((o.z_bs * o.esz) % 16 == 0 && (o.dz_bs * o.esz) % 16 == 0));
  return o;
}

XdblOperands scan_xdbl_operands(const void* xdbl, const void* wdt, int batch, int seqlen, int dt_rank, int io_dtype,
                                long long xdbl_bstride, long long xdbl_tstride) {
  const size_t esz = io_esz(io_dtype);
  const long long S = dt_rank + 2 * kMaxState;
  XdblOperands x{};
  x.bs = xdbl_bstride ? xdbl_bstride : S * seqlen;
  x.ts = xdbl_tstride ? xdbl_tstride : S;
  x.B = static_cast<const char*>(xdbl) + static_cast<size_t>(dt_rank) * esz;
  x.C = static_cast<const char*>(x.B) + kMaxState * esz;
  x.ok = aligned16(xdbl) && aligned16(wdt) && (x.bs * esz) % 16 == 0 && (x.ts * esz) % 16 == 0 &&
         (dt_rank * esz) % 16 == 0 && static_cast<long long>(batch) * x.bs < (1ll << 30);
  return x;
}

}  // namespace simamba
