// A keyed bijection of [0, n), 1 <= n <= 2^31 - 1, computable per element, host and device from one text (as philox.h):
// csrc/dataset.hip shuffles an epoch and samples rows without replacement with it inside its kernel and answers
// simamba_keyed_perm on the host.  Integer arithmetic only, so both give the same values.
//
//   perm(n, key, stream, i), 0 <= i < n:
//     n == 1: 0, without a round.
//     bits = the smallest b with 2^b >= n;  h = max(1, (bits + 1) / 2): 2h is the smallest even number >= max(2, bits),
//     so n <= 2^2h < 4 n.  mask = 2^h - 1.
//     E(x), a balanced Feistel network on the 2h bits of x:  L = x >> h, R = x & mask; four times, round r = 0 .. 3:
//       F = philox4x32_10(k0, k1, c0 = R, c1 = 0x80000000 | r, c2 = stream & 0xffffffff, c3 = stream >> 32).w[0] & mask
//       (L, R) <- (R, L ^ F)
//     E(x) = L << h | R, a bijection of [0, 2^2h) whatever F is.
//     Cycle walking: x = E(i); while x >= n: x = E(x).  It ends: E is a bijection, so the walk from i returns to i < n at
//     the latest; it visits each value >= n at most once, fewer than 3 n of them, and for a random E about 2^2h / n < 4
//     applications are expected.  Restricted to [0, n) the walk is a bijection of [0, n).
//   key (k0, k1) = the low and high word of the 64-bit seed.  `stream` separates the uses: no two may share one (the
//   layout dataset.hip uses is in include/simamba.h).  c1's top bit keeps every block drawn here apart from the
//   augmentation kernels' (their c1 is a cloud number below 2^31), so a loader and an AugmentState may share a seed.
#pragma once
#include "philox.h"

namespace simamba {

constexpr uint32_t kPermDomain = 0x80000000u;      // in c1 of every Philox block of this header and of dataset.hip
constexpr int kPermRounds = 4;

struct KeyedPerm {                                 // what depends on n alone
  uint32_t n, h, mask;
};

SIMAMBA_HD KeyedPerm keyed_perm_plan(uint32_t n) {
  uint32_t bits = 0;
  while (bits < 32 && (1ull << bits) < n) ++bits;
  const uint32_t h = bits < 2 ? 1u : (bits + 1) / 2;
  return KeyedPerm{n, h, (1u << h) - 1u};
}

SIMAMBA_HD uint32_t keyed_perm_network(const KeyedPerm& p, uint32_t k0, uint32_t k1, uint32_t s_lo, uint32_t s_hi,
                                       uint32_t x) {
  uint32_t L = x >> p.h, R = x & p.mask;
#pragma unroll
  for (int r = 0; r < kPermRounds; ++r) {
    const uint32_t F = philox4x32_10(k0, k1, R, kPermDomain | static_cast<uint32_t>(r), s_lo, s_hi).w[0] & p.mask;
    const uint32_t nr = L ^ F;
    L = R;
    R = nr;
  }
  return (L << p.h) | R;
}

// perm(p.n, (k0, k1), (s_lo, s_hi), i) for i < p.n; the result is < p.n
SIMAMBA_HD uint32_t keyed_perm(const KeyedPerm& p, uint32_t k0, uint32_t k1, uint32_t s_lo, uint32_t s_hi, uint32_t i) {
  if (p.n <= 1) return 0;
  uint32_t x = keyed_perm_network(p, k0, k1, s_lo, s_hi, i);
  while (x >= p.n) x = keyed_perm_network(p, k0, k1, s_lo, s_hi, x);
  return x;
}

}  // namespace simamba
