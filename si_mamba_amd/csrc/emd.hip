// Earth mover's distance between equal-sized point sets: the cheapest one-to-one matching under squared Euclidean
// cost, by the forward auction with Jacobi rounds and epsilon-scaling (Bertsekas).  The x points bid, the y points are
// the objects.  The value of object j to bidder i is -c_ij - price_j, c_ij = (dx*dx + dy*dy) + dz*dz formed on the fly
// from LDS (no n x n matrix anywhere).  A round:
//   bid      every unassigned bidder scans all n objects for its best and second-best value and bids
//            price_j* + (best - second) + eps on the best one: one 64-bit LDS max per bid on the object's slot,
//            (bid bits, ~bidder) -- the highest bid wins, equal bids go to the lowest bidder index;
//   resolve  lane j, as object j, takes the winner: new owner (the old one finds out below), new price
//            max(bid, nextafter(old price)) -- a bid always raises the price, also where eps is below the price's ulp;
//   refresh  every bidder looks up whether it still owns its object.
// A phase ends when no object is free (n bidders, n objects, one-to-one: then every bidder is assigned).  Phases run
// with eps = cmax/2, cmax/8, ... down to eps_final; prices carry over, the assignment restarts.  `rounds` counts over
// all phases and is capped: at the cap the unassigned bidders take the free objects in index order and converged = 0.
// Every loop is bounded by that cap and every index comes from a lane id or a loop counter, never from a float, so
// non-finite input ends like any other (with whatever matching the cap left).
//
// Two instantiations of one set of helpers: n <= 64 one wave per pair (kEmdWaves pairs per workgroup, wave-level
// synchronisation only), n <= 1024 one workgroup per pair.  Lane i is bidder i and object i.  All bidders scan the
// objects in the same order: the LDS reads of (y_j, price_j), one float4, are broadcasts.
#include <math.h>

#include "common.h"

namespace simamba {

constexpr int kEmdWaves = 4;          // pairs per workgroup of the one-wave kernel
constexpr int kEmdMaxN = 1024;
constexpr float kEmdEpsFloor = 1e-30f;  // eps_final when cmax == 0 (every point the same): any positive number does

typedef unsigned long long emd_slot_t;

struct EmdLds {          // one pair's state; N entries each
  float4* yp;            // (y_j, price_j)
  int* owner;            // bidder that holds object j, -1 = free
  emd_slot_t* slot;      // this round's highest bid on object j: bid bits << 32 | ~bidder ; 0 = none
  int* asg;              // the result, bidder -> object (written once, at the end)
  float* red;            // 16 floats: per-wave partials of the workgroup reductions
};

template <bool kWave> __device__ __forceinline__ void emd_sync() {
  if (kWave) {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
}

// how many lanes of the pair hold `p`; a barrier for the pair's LDS in both forms
template <bool kWave> __device__ __forceinline__ int emd_count(bool p) {
  if (kWave) {
    emd_sync<true>();
    return __popcll(__ballot(p));
  }
  return __syncthreads_count(p);
}

// max (kMax) or sum over the pair's lanes, the same value in every lane, the same bits every time
template <bool kWave, bool kMax> __device__ __forceinline__ float emd_reduce(float v, float* red) {
  v = kMax ? wave_xor_max(v) : wave_xor_sum(v);
  if (kWave) return v;
  const int wave = threadIdx.x >> 6, waves = (blockDim.x + 63) >> 6;
  __syncthreads();                                  // red may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  float r = red[0];
  for (int w = 1; w < waves; ++w) r = kMax ? fmaxf(r, red[w]) : r + red[w];
  return r;
}

__device__ __forceinline__ float emd_cost(float x, float y, float z, const float4& q) {
  const float dx = x - q.x, dy = y - q.y, dz = z - q.z;
  return (dx * dx + dy * dy) + dz * dz;
}

// one object of a bidder's scan: the first maximum keeps the object, `second` is the second largest with multiplicity;
// a NaN value is never taken
__device__ __forceinline__ void emd_scan_step(float x, float y, float z, const float4& q, int j, float& best,
                                              float& second, int& jb) {
  const float v = -emd_cost(x, y, z, q) - q.w;
  const bool up = v > best;
  second = fmaxf(second, up ? best : v);
  jb = up ? j : jb;
  best = up ? v : best;
}

// One pair.  `i`: this lane's bidder / object index, lanes with i >= n only keep the barriers company.
template <bool kWave>
__device__ __forceinline__ void emd_pair(const float* __restrict__ X, const float* __restrict__ Y,
                                         int* __restrict__ assign, float* __restrict__ dist,
                                         int* __restrict__ rounds_out, unsigned char* __restrict__ conv_out, int n,
                                         float eps_arg, int max_rounds, const EmdLds& s, int i) {
  const bool active = i < n;
  const int lane = threadIdx.x & 63;
  // bidders per wave up to which the shared scan is the shorter one: n steps of about 14 instructions against
  // ceil(n / 64) of them plus about 70 for the six-step merge, per bidder (5 at n = 32, 10 at 64, 48 at 1024)
  const int coop_max = (14 * n) / (14 * ((n + 63) / 64) + 70);
  float x = 0.f, y = 0.f, z = 0.f;
  if (active) {
    x = X[3 * i]; y = X[3 * i + 1]; z = X[3 * i + 2];
    s.yp[i] = make_float4(Y[3 * i], Y[3 * i + 1], Y[3 * i + 2], 0.f);
  }
  emd_sync<kWave>();

  float cm = 0.f;
  if (active)
    for (int j = 0; j < n; ++j) cm = fmaxf(cm, emd_cost(x, y, z, s.yp[j]));
  const float cmax = emd_reduce<kWave, true>(cm, s.red);
  const float eps_final = eps_arg > 0.f ? eps_arg : fmaxf(cmax * (1.f / 16384.f), kEmdEpsFloor);

  int my = (n == 1 && active) ? 0 : -1;      // the object this bidder holds
  int rounds = 0;
  bool conv = n == 1;
  float eps = 0.5f * cmax;
  while (!conv) {
    eps = fmaxf(eps, eps_final);
    const bool last = !(eps > eps_final);
    if (active) { s.owner[i] = -1; s.slot[i] = 0ull; }
    my = -1;
    bool free_ = active;
    emd_sync<kWave>();
    int nfree = n;
    do {
      // A wave with many unassigned bidders scans lane per bidder (n steps whatever their number); one with few -- most
      // rounds: the tail of a phase is a handful of bidders evicting each other -- takes them one at a time, all 64
      // lanes sharing the bidder's object scan.  Wave-uniform choice; both give the same (best, second, jb), bit for bit.
      const unsigned long long want = __ballot(active && my < 0);
      int jb = -1;
      float best = -INFINITY, second = -INFINITY;
      if (__popcll(want) > coop_max) {
        if (active && my < 0) {
          jb = 0;
          for (int j = 0; j < n; ++j) emd_scan_step(x, y, z, s.yp[j], j, best, second, jb);
        }
      } else {
        for (unsigned long long m = want; m != 0ull; m &= m - 1ull) {
          const int b = __ffsll(static_cast<long long>(m)) - 1;
          const float bx = __shfl(x, b, 64), by = __shfl(y, b, 64), bz = __shfl(z, b, 64);
          float lb = -INFINITY, ls = -INFINITY;
          int lj = 0x7fffffff;
          for (int j = lane; j < n; j += 64) emd_scan_step(bx, by, bz, s.yp[j], j, lb, ls, lj);
#pragma unroll
          for (int off = 32; off >= 1; off >>= 1) {
            const float ob = __shfl_xor(lb, off, 64), os = __shfl_xor(ls, off, 64);
            const int oj = __shfl_xor(lj, off, 64);
            const bool take = ob > lb || (ob == lb && oj < lj);          // equal values: the lower object, as above
            ls = fmaxf(fmaxf(ls, os), take ? lb : ob);
            lb = take ? ob : lb;
            lj = take ? oj : lj;
          }
          if (lane == b) { jb = lj < n ? lj : 0; best = lb; second = ls; }
        }
      }
      if (jb >= 0) {
        const float bid = s.yp[jb].w + (best - second) + eps;
        atomicMax(&s.slot[jb], (static_cast<emd_slot_t>(__float_as_uint(bid)) << 32) |
                                   static_cast<emd_slot_t>(0xffffffffu - static_cast<unsigned>(i)));
      }
      emd_sync<kWave>();
      if (active) {
        const emd_slot_t w = s.slot[i];
        if (w != 0ull) {
          s.slot[i] = 0ull;
          const float old = s.yp[i].w;
          s.yp[i].w = fmaxf(__uint_as_float(static_cast<unsigned>(w >> 32)), nextafterf(old, INFINITY));
          s.owner[i] = static_cast<int>(0xffffffffu - static_cast<unsigned>(w));
          free_ = false;
        }
      }
      ++rounds;
      nfree = emd_count<kWave>(free_);
      const int t = jb >= 0 ? jb : my;
      my = (t >= 0 && s.owner[t] == i) ? t : -1;
    } while (nfree != 0 && rounds < max_rounds);
    if (nfree != 0) break;                    // the cap, inside a phase
    if (last) conv = true;
    else if (rounds >= max_rounds) break;     // the cap, between two phases
    eps *= 0.25f;
    emd_sync<kWave>();                        // every refresh has read owner before the next phase clears it
  }

  if (active) s.asg[i] = my;
  emd_sync<kWave>();
  if (!conv && i == 0) {
    // as many bidders are unassigned as objects are free (bidder b holds j exactly when owner[j] == b)
    int b = 0;
    for (int j = 0; j < n; ++j) {
      if (s.owner[j] >= 0) continue;
      while (b < n && s.asg[b] >= 0) ++b;
      if (b >= n) break;
      s.asg[b] = j;
      ++b;
    }
  }
  emd_sync<kWave>();
  float c = 0.f;
  if (active) {
    const int a = s.asg[i];
    assign[i] = a;
    c = emd_cost(x, y, z, s.yp[a]);
  }
  const float total = emd_reduce<kWave, false>(c, s.red);
  if (i == 0) {
    *dist = total / static_cast<float>(n);
    *rounds_out = rounds;
    *conv_out = conv ? 1 : 0;
  }
}

__global__ __launch_bounds__(64 * kEmdWaves) void emd_wave_kernel(const float* __restrict__ x,
                                                                  const float* __restrict__ y,
                                                                  int* __restrict__ assign, float* __restrict__ dist,
                                                                  int* __restrict__ rounds,
                                                                  unsigned char* __restrict__ converged,
                                                                  long long pairs, int n, float eps, int max_rounds) {
  __shared__ float4 sYP[kEmdWaves][64];
  __shared__ emd_slot_t sSlot[kEmdWaves][64];
  __shared__ int sOwner[kEmdWaves][64], sAsg[kEmdWaves][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long pr = static_cast<long long>(blockIdx.x) * kEmdWaves + wave;
  if (pr >= pairs) return;                       // whole wave; no workgroup barrier below
  const EmdLds s{sYP[wave], sOwner[wave], sSlot[wave], sAsg[wave], nullptr};
  emd_pair<true>(x + pr * n * 3, y + pr * n * 3, assign + pr * n, dist + pr, rounds + pr, converged + pr, n, eps,
                 max_rounds, s, lane);
}

__global__ __launch_bounds__(kEmdMaxN) void emd_block_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                             int* __restrict__ assign, float* __restrict__ dist,
                                                             int* __restrict__ rounds,
                                                             unsigned char* __restrict__ converged, int n, float eps,
                                                             int max_rounds) {
  __shared__ float4 sYP[kEmdMaxN];
  __shared__ emd_slot_t sSlot[kEmdMaxN];
  __shared__ int sOwner[kEmdMaxN], sAsg[kEmdMaxN];
  __shared__ float sRed[16];
  const long long pr = blockIdx.x;
  const EmdLds s{sYP, sOwner, sSlot, sAsg, sRed};
  emd_pair<false>(x + pr * n * 3, y + pr * n * 3, assign + pr * n, dist + pr, rounds + pr, converged + pr, n, eps,
                  max_rounds, s, static_cast<int>(threadIdx.x));
}

}  // namespace simamba

using namespace simamba;

extern "C" int simamba_emd_fwd(const float* x, const float* y, int* assign, float* dist, int* rounds,
                               unsigned char* converged, long long pairs, int n, float eps, int max_rounds,
                               void* stream) {
  if (pairs < 1 || n < 1 || n > kEmdMaxN || max_rounds < 1 || !(eps >= 0.f)) return SIMAMBA_E_SHAPE;
  if (!x || !y || !assign || !dist || !rounds || !converged) return SIMAMBA_E_NULLPTR;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n <= 64) {
    const long long grid = (pairs + kEmdWaves - 1) / kEmdWaves;
    if (grid > 0x7fffffffll) return SIMAMBA_E_SHAPE;
    hipLaunchKernelGGL(emd_wave_kernel, dim3(static_cast<unsigned>(grid)), dim3(64 * kEmdWaves), 0, st, x, y, assign,
                       dist, rounds, converged, pairs, n, eps, max_rounds);
  } else {
    if (pairs > 0x7fffffffll) return SIMAMBA_E_SHAPE;
    hipLaunchKernelGGL(emd_block_kernel, dim3(static_cast<unsigned>(pairs)), dim3((n + 63) / 64 * 64), 0, st, x, y,
                       assign, dist, rounds, converged, n, eps, max_rounds);
  }
  return static_cast<int>(hipGetLastError());
}
