// Linear one-vs-one C-SVC (the reference's pre-training validation, tools/runner_pretrain.py:66-77: scikit-learn's
// SVC(C=0.01, kernel='linear'), i.e. libsvm) without the host.  This family is FLOAT64: the gradient's partial sums are
// of size n_SV * C * |K| against a stopping tolerance of 1e-3, which fp32 cannot resolve.
//
// svm_ovo_smo_kernel: one 256-lane workgroup per class pair p = (a, b), a < b, pairs in libsvm's order (0,1), (0,2),
// ... (nc-2, nc-1).  The pair's problem is class a's samples (y = +1) followed by class b's (y = -1), each in input
// order; it solves libsvm's dual  min 1/2 a'Qa - e'a,  0 <= a <= C,  y'a = 0,  Q = yy' o K  by SMO:
//   i = argmax over I_up of -yG;  j by libsvm's second-order rule (WSS3: over I_low with -yG_t < -yG_i, the largest
//   (yG_t - yG_i)^2 / (K_ii + K_tt - 2 K_it), curvature floor 1e-12);  libsvm's clipped two-variable update;
//   stop when m(alpha) - M(alpha) < tol;  rho as libsvm's calculate_rho.
// alpha, G, diag(K) (float64), the pair's sample indices (int32) and y (int8) live in LDS: 29 bytes per sample, 116 KiB
// at the largest pair of 4096.  Two rows of K are read per iteration, through the index list.
//
// Every lane takes part in every barrier, and the loop is left only on values all lanes read back from LDS behind a
// barrier (the reduced maxima and their positions) or on the iteration cap, so all waves leave in the same iteration.
// No index is derived from a float, positions out of a reduction are used only after the check against "none", and
// `order` is clamped into [0, N) on the way into LDS: a NaN in K ends a pair early or at the cap, never out of bounds.
// Reductions: per lane in ascending position, the xor butterfly over the wave, the four waves in order through LDS; ties
// go to the lower position.  No atomics: the same bits every call.
//
// svm_ovo_vote_kernel: libsvm's svm_predict_values on a row of decision values.  One wave per row, lane c counts the
// votes of class c (dec > 0 votes a, anything else -- 0 and NaN too -- votes b), a butterfly picks the most votes, the
// lowest class on a tie.  Matches with `labels` are counted with one 64-bit integer atomic per matching row.
#include "host_common.h"

namespace simamba {

constexpr int kSvmThreads = 256;
constexpr int kSvmWaves = kSvmThreads / 64;
constexpr int kSvmMaxClasses = 64;
constexpr int kSvmMaxPair = 4096;
constexpr int kSvmMaxN = 16384;
constexpr int kSvmMaxD = 4096;
constexpr int kSvmNone = 0x7fffffff;
constexpr double kSvmTau = 1e-12;                        // libsvm's TAU
constexpr int kSvmLdsPerSample = 3 * 8 + 4 + 1;          // alpha, G, diag(K) ; index ; y
constexpr int kSvmMaxLds = kSvmMaxPair * kSvmLdsPerSample;
constexpr int kVoteThreads = 256;
constexpr int kVoteRows = kVoteThreads / 64;

struct SvmClasses { int start[kSvmMaxClasses + 1]; };    // by value: the kernel never reads the caller's host array

// (value, position) maximum, the lower position on equal values; a NaN is never taken
__device__ __forceinline__ void svm_take_max(double& v, int& i, double ov, int oi) {
  const bool take = ov > v || (ov == v && oi < i);
  v = take ? ov : v;
  i = take ? oi : i;
}
__device__ __forceinline__ void svm_wave_argmax(double& v, int& i) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ov = __shfl_xor(v, off);
    const int oi = __shfl_xor(i, off);
    svm_take_max(v, i, ov, oi);
  }
}
__device__ __forceinline__ double svm_wave_min(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmin(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ double svm_wave_max(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  return v;
}

__global__ __launch_bounds__(kSvmThreads) void svm_ovo_smo_kernel(
    const double* __restrict__ K, const float* __restrict__ X, const int* __restrict__ order, const SvmClasses cls,
    double* __restrict__ alpha_out, double* __restrict__ w_out, double* __restrict__ rho_out,
    int* __restrict__ n_iter_out, unsigned char* __restrict__ converged_out, int N, int d, int nc, int cap, double C,
    double tol, int max_iter, int iter_per_sample) {
  extern __shared__ double svm_lds[];
  __shared__ double sV1[kSvmWaves], sV2[kSvmWaves], sV3[kSvmWaves];
  __shared__ int sI1[kSvmWaves], sI2[kSvmWaves], sI3[kSvmWaves];
  double* __restrict__ sAlpha = svm_lds;                 // cap is a multiple of 8: every array stays aligned
  double* __restrict__ sG = sAlpha + cap;
  double* __restrict__ sQD = sG + cap;
  int* __restrict__ sIdx = reinterpret_cast<int*>(sQD + cap);
  signed char* __restrict__ sY = reinterpret_cast<signed char*>(sIdx + cap);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // the pair of this workgroup and where its alpha starts: (nc - 1) N doubles in all, pairs back to back
  int a = 0, rem = blockIdx.x;
  long long off = 0;
  while (a < nc - 2 && rem >= nc - 1 - a) {
    off += static_cast<long long>(nc - 1 - a) * (cls.start[a + 1] - cls.start[a]) + (N - cls.start[a + 1]);
    rem -= nc - 1 - a;
    ++a;
  }
  const int b = a + 1 + rem;
  if (b > nc - 1) return;                                // a grid larger than the pairs: the whole workgroup leaves
  const int sa = cls.start[a], na = cls.start[a + 1] - sa, sb = cls.start[b], nb = cls.start[b + 1] - sb;
  off += static_cast<long long>(b - a - 1) * na + (sb - cls.start[a + 1]);
  const int n = na + nb;
  if (n > cap) return;                                   // refused on the host; never past the LDS arrays

  for (int t = tid; t < n; t += kSvmThreads) {
    int o = order[t < na ? sa + t : sb + (t - na)];
    o = o < 0 ? 0 : (o > N - 1 ? N - 1 : o);
    sIdx[t] = o;
    sY[t] = t < na ? 1 : -1;
    sAlpha[t] = 0.0;
    sG[t] = -1.0;
    sQD[t] = K[static_cast<long long>(o) * N + o];
  }
  __syncthreads();

  long long cap_ll = static_cast<long long>(max_iter) + static_cast<long long>(iter_per_sample) * n;
  const int cap_it = cap_ll > 0x7fffffffll ? 0x7fffffff : static_cast<int>(cap_ll);
  const double ninf = -__builtin_huge_val();
  int it = 0;
  bool conv = false;
  for (; it < cap_it; ++it) {
    // i: the largest -yG over I_up
    double bv = ninf;
    int bi = kSvmNone;
    for (int t = tid; t < n; t += kSvmThreads) {
      const int y = sY[t];
      const double al = sAlpha[t];
      const bool up = y > 0 ? al < C : al > 0.0;
      const double v = -y * sG[t];
      if (up && v > bv) { bv = v; bi = t; }
    }
    svm_wave_argmax(bv, bi);
    if (lane == 0) { sV1[wave] = bv; sI1[wave] = bi; }
    __syncthreads();
    double gmax = sV1[0];
    int i = sI1[0];
#pragma unroll
    for (int w = 1; w < kSvmWaves; ++w) svm_take_max(gmax, i, sV1[w], sI1[w]);
    if (i == kSvmNone) break;                            // no finite candidate (a NaN in K): not converged

    const double qdi = sQD[i];
    const double* __restrict__ Ki = K + static_cast<long long>(sIdx[i]) * N;
    // j: the largest second-order gain over I_low; gmax2 = max over I_low of yG = -M(alpha)
    double gv = ninf, mv = ninf;
    int gj = kSvmNone, mi = kSvmNone;
    for (int t = tid; t < n; t += kSvmThreads) {
      const double kit = Ki[sIdx[t]];
      const int y = sY[t];
      const double al = sAlpha[t];
      const bool low = y > 0 ? al > 0.0 : al < C;
      const double yg = y * sG[t];
      if (low) {
        if (yg > mv) { mv = yg; mi = t; }
        const double gd = gmax + yg;
        if (gd > 0.0) {
          const double quad = qdi + sQD[t] - 2.0 * kit;
          const double gain = gd * gd / (quad > 0.0 ? quad : kSvmTau);
          if (gain > gv) { gv = gain; gj = t; }
        }
      }
    }
    svm_wave_argmax(gv, gj);
    svm_wave_argmax(mv, mi);
    if (lane == 0) { sV2[wave] = gv; sI2[wave] = gj; sV3[wave] = mv; sI3[wave] = mi; }
    __syncthreads();
    double gain = sV2[0], gmax2 = sV3[0];
    int j = sI2[0], mj = sI3[0];
#pragma unroll
    for (int w = 1; w < kSvmWaves; ++w) {
      svm_take_max(gain, j, sV2[w], sI2[w]);
      svm_take_max(gmax2, mj, sV3[w], sI3[w]);
    }
    if (gmax + gmax2 < tol) { conv = true; break; }      // libsvm's rule: m(alpha) - M(alpha) < tol
    if (j == kSvmNone) break;

    // libsvm's two-variable update, computed by every lane from the same LDS values
    const int yi = sY[i], yj = sY[j];
    const double oai = sAlpha[i], oaj = sAlpha[j], gi = sG[i], gj_ = sG[j];
    const int oj = sIdx[j];
    double quad = qdi + sQD[j] - 2.0 * Ki[oj];
    quad = quad > 0.0 ? quad : kSvmTau;
    double ai = oai, aj = oaj;
    if (yi != yj) {
      const double delta = (-gi - gj_) / quad;
      const double diff = ai - aj;
      ai += delta;
      aj += delta;
      if (diff > 0.0) {
        if (aj < 0.0) { aj = 0.0; ai = diff; }
        if (ai > C) { ai = C; aj = C - diff; }
      } else {
        if (ai < 0.0) { ai = 0.0; aj = -diff; }
        if (aj > C) { aj = C; ai = C + diff; }
      }
    } else {
      const double delta = (gi - gj_) / quad;
      const double sum = ai + aj;
      ai -= delta;
      aj += delta;
      if (sum > C) {
        if (ai > C) { ai = C; aj = sum - C; }
        if (aj > C) { aj = C; ai = sum - C; }
      } else {
        if (aj < 0.0) { aj = 0.0; ai = sum; }
        if (ai < 0.0) { ai = 0.0; aj = sum; }
      }
    }
    ai = fmin(fmax(ai, 0.0), C);                         // the box holds exactly, whatever the rounding above did
    aj = fmin(fmax(aj, 0.0), C);
    const double ci = yi * (ai - oai), cj = yj * (aj - oaj);
    const double* __restrict__ Kj = K + static_cast<long long>(oj) * N;
    __syncthreads();                                     // every lane has read alpha and G of i and j
    if (tid == 0) { sAlpha[i] = ai; sAlpha[j] = aj; }
    for (int t = tid; t < n; t += kSvmThreads) {
      const int o = sIdx[t];
      sG[t] += sY[t] * (ci * Ki[o] + cj * Kj[o]);
    }
    __syncthreads();
  }
  __syncthreads();                                       // all waves left in the same iteration: sV1.. are free again

  // rho (libsvm's calculate_rho): the mean of yG over the free alpha, else the midpoint of the two bounds
  double ub = __builtin_huge_val(), lb = ninf, sf = 0.0;
  int nf = 0;
  for (int t = tid; t < n; t += kSvmThreads) {
    const int y = sY[t];
    const double al = sAlpha[t], yg = y * sG[t];
    if (al >= C) {
      if (y < 0) ub = fmin(ub, yg); else lb = fmax(lb, yg);
    } else if (al <= 0.0) {
      if (y > 0) ub = fmin(ub, yg); else lb = fmax(lb, yg);
    } else {
      ++nf;
      sf += yg;
    }
  }
  sf = wave_xor_sum(sf);
  nf = wave_xor_sum(nf);
  ub = svm_wave_min(ub);
  lb = svm_wave_max(lb);
  if (lane == 0) { sV1[wave] = sf; sI1[wave] = nf; sV2[wave] = ub; sV3[wave] = lb; }
  __syncthreads();
  if (tid == 0) {
    double s = sV1[0], u = sV2[0], l = sV3[0];
    int f = sI1[0];
#pragma unroll
    for (int w = 1; w < kSvmWaves; ++w) {
      s += sV1[w];
      f += sI1[w];
      u = fmin(u, sV2[w]);
      l = fmax(l, sV3[w]);
    }
    rho_out[blockIdx.x] = f > 0 ? s / f : (u + l) / 2.0;
    n_iter_out[blockIdx.x] = it;
    converged_out[blockIdx.x] = conv ? 1 : 0;
  }

  double* __restrict__ ap = alpha_out + off;
  for (int t = tid; t < n; t += kSvmThreads) ap[t] = sAlpha[t];

  // w = sum_t alpha_t y_t x_t over the support vectors, in position order; a lane per feature column
  double* __restrict__ wp = w_out + static_cast<long long>(blockIdx.x) * d;
  for (int c = tid; c < d; c += kSvmThreads) {
    double acc = 0.0;
    for (int t = 0; t < n; ++t) {
      const double al = sAlpha[t];                       // the same for every lane: no divergence
      if (al != 0.0) acc += (al * sY[t]) * static_cast<double>(X[static_cast<long long>(sIdx[t]) * d + c]);
    }
    wp[c] = acc;
  }
}

__global__ __launch_bounds__(kVoteThreads) void svm_ovo_vote_kernel(
    const double* __restrict__ dec, const long long* __restrict__ labels, int* __restrict__ pred,
    unsigned long long* __restrict__ matches, long long m, int nc) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long row = static_cast<long long>(blockIdx.x) * kVoteRows + wave;
  if (row >= m) return;                                  // a whole wave; the kernel has no barrier
  const double* __restrict__ r = dec + row * (nc * (nc - 1) / 2);
  int votes = -1, best = lane;                           // lanes beyond the classes never win: a class has >= 0 votes
  if (lane < nc) {
    votes = 0;
    for (int o = 0; o < nc; ++o) {
      if (o == lane) continue;
      const int a = o < lane ? o : lane, b = o < lane ? lane : o;
      const bool pos = r[a * (2 * nc - a - 1) / 2 + (b - a - 1)] > 0.0;     // false for 0 and NaN: the vote is b's
      votes += (lane == a) == pos;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int ov = __shfl_xor(votes, off), oi = __shfl_xor(best, off);
    const bool take = ov > votes || (ov == votes && oi < best);
    votes = take ? ov : votes;
    best = take ? oi : best;
  }
  if (lane == 0) {
    pred[row] = best;
    if (labels && labels[row] == best) atomicAdd(matches, 1ull);
  }
}

}  // namespace simamba

using namespace simamba;

extern "C" int simamba_svm_ovo_fit(const double* gram, const float* x, const int* order, const int* class_start,
                                   const double* c_tol, double* alpha, double* w, double* rho, int* n_iter,
                                   unsigned char* converged, int n, int d, int nc, int max_iter,
                                   int max_iter_per_sample, void* stream) {
  if (nc < 2 || nc > kSvmMaxClasses || n < 2 || n > kSvmMaxN || d < 1 || d > kSvmMaxD) return SIMAMBA_E_SHAPE;
  if (max_iter < 1 || max_iter_per_sample < 0) return SIMAMBA_E_SHAPE;
  double c = 0.0, tol = 0.0;
  if (c_tol) {                                           // a HOST array {C, tol}: the ABI passes no double by value
    c = c_tol[0];
    tol = c_tol[1];
    if (!(c > 0.0) || !(tol > 0.0)) return SIMAMBA_E_SHAPE;
  }
  SvmClasses cls = {};
  int max_pair = 0;
  if (class_start) {                                     // a HOST array: the class sizes are checked before any launch
    if (class_start[0] != 0 || class_start[nc] != n) return SIMAMBA_E_SHAPE;
    int big1 = 0, big2 = 0;                              // the two largest classes make the largest pair
    for (int k = 0; k < nc; ++k) {
      const long long sz = static_cast<long long>(class_start[k + 1]) - class_start[k];
      if (sz < 1 || sz > n) return SIMAMBA_E_SHAPE;
      const int s = static_cast<int>(sz);
      if (s > big1) { big2 = big1; big1 = s; } else if (s > big2) { big2 = s; }
    }
    max_pair = big1 + big2;
    if (max_pair > kSvmMaxPair) return SIMAMBA_E_SHAPE;
    for (int k = 0; k <= kSvmMaxClasses; ++k) cls.start[k] = class_start[k <= nc ? k : nc];
  }
  if (!gram || !x || !order || !class_start || !c_tol || !alpha || !w || !rho || !n_iter || !converged) return SIMAMBA_E_NULLPTR;
  const int cap = (max_pair + 7) & ~7;
  const int lds = cap * kSvmLdsPerSample;
  if (const hipError_t e = ensure_lds_cap<svm_ovo_smo_kernel>(kSvmMaxLds)) return static_cast<int>(e);
  hipLaunchKernelGGL(svm_ovo_smo_kernel, dim3(static_cast<unsigned>(nc * (nc - 1) / 2)), dim3(kSvmThreads), lds,
                     static_cast<hipStream_t>(stream), gram, x, order, cls, alpha, w, rho, n_iter, converged, n, d, nc,
                     cap, c, tol, max_iter, max_iter_per_sample);
  return static_cast<int>(hipGetLastError());
}

extern "C" int simamba_svm_ovo_vote(const double* dec, const long long* labels, int* pred, long long* matches,
                                    long long m, int nc, void* stream) {
  if (nc < 2 || nc > kSvmMaxClasses || m < 1 || m > 0x7fffffffll) return SIMAMBA_E_SHAPE;
  if (!dec || !pred || (labels && !matches)) return SIMAMBA_E_NULLPTR;
  hipLaunchKernelGGL(svm_ovo_vote_kernel, dim3(static_cast<unsigned>((m + kVoteRows - 1) / kVoteRows)),
                     dim3(kVoteThreads), 0, static_cast<hipStream_t>(stream), dec, labels, pred,
                     reinterpret_cast<unsigned long long*>(matches), m, nc);
  return static_cast<int>(hipGetLastError());
}
