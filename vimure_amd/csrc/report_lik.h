// report_lik.h -- the Poisson-mixture likelihood of one report under a tie's rho row, shared by heldout.hip (a list of entries the
// caller gives) and report_scores.hip (every element of the support): one definition of the rates, of the terms
// b_k = x log mu_k - mu_k + log rho_k, of lgamma(x + 1) and of the log-sum-exp, so that both entry points give the same bits
// for the same (rho row, theta, lambda, eta, x, xt) -- and one definition of what they reduce (LikAcc, k_lik_finish).
#ifndef VMR_REPORT_LIK_H
#define VMR_REPORT_LIK_H
#include "read_side.h"

#define HO_LGT 256      // lgamma(x + 1) tabulated below this count

// mu_k = theta lambda_k + eta xt and the mean's running sum: every product and every sum rounded on its own (rho_row.h's convention)
__device__ __forceinline__ double ho_rate(double th, double la, double exy) {
#pragma clang fp contract(off)
  const double a = th * la;
  return a + exy;
}
__device__ __forceinline__ double ho_mul(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ double ho_add(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}

// b_k = x log mu_k - mu_k + log rho_k, or -inf where the category adds nothing (rho_k not positive; a zero rate against x > 0)
__device__ __forceinline__ double ho_term(double r, double mu, double xd, bool xpos) {
  if (!(r > 0.0)) return -INFINITY;
  if (mu == 0.0) return xpos ? -INFINITY : log(r);
  return xd * log(mu) - mu + log(r);
}

// lgamma(x + 1)
__device__ __forceinline__ double ho_lgam1(unsigned x, const double* __restrict__ lgt) {
  if (x < HO_LGT) return lgt[x];
  const double z = (double)x + 1.0, r = 1.0 / z, r2 = r * r;   // z >= 257: the next term of the series is below 1e-20
  return fma(z - 0.5, log(z), -z) + 0.91893853320467274178 + r * (1.0 / 12.0 - r2 * (1.0 / 360.0 - r2 * (1.0 / 1260.0)));
}

// maximum mx and sum s of exp(b - mx), folded with another pair (either may be empty: mx = -inf, s = 0; a NaN sits in s)
__device__ __forceinline__ void ho_fold(double& mx, double& s, double mx2, double s2) {
  const double m = mx2 > mx ? mx2 : mx;
  const double e1 = mx == m ? 1.0 : exp(mx - m), e2 = mx2 == m ? 1.0 : exp(mx2 - m);
  s = s * e1 + s2 * e2;
  mx = m;
}

__device__ __forceinline__ double ho_logp(double mx, double s, double lg) {
  if (s != s) return s;
  if (mx == -INFINITY) return -INFINITY;
  return mx + log(s) - lg;
}

// logp and mean of one element, K <= KMAX, a lane per element: the row in registers (KC = 2: in one 16-byte load; KC = 0: any K),
// K rates, the K terms, their maximum and the sum of exp(b_k - max) in ascending k
template <int KC>
__device__ __forceinline__ void lik_eval_lane(int Kp, const double* __restrict__ row, double thm, const double* __restrict__ la, double eta,
                                              int x, int xt, const double* __restrict__ lgt, double& lp, double& mn) {
  const int K = KC ? KC : Kp;
  double r[KMAX], b[KMAX];
  if (KC == 2) {
    const double2 v = *reinterpret_cast<const double2*>(row);   // (rho is 256-byte aligned, a row of two doubles 16-byte)
    r[0] = v.x; r[1] = v.y;
  } else {
#pragma unroll
    for (int k = 0; k < KMAX; ++k) if (k < K) r[k] = row[k];
  }
  const double exy = eta * (double)xt, xd = (double)x;
  double mx = -INFINITY;
  bool nan_seen = false;
  mn = 0.0;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) {
      const double mu = ho_rate(thm, la[k], exy);
      mn = ho_add(mn, ho_mul(r[k], mu));
      b[k] = ho_term(r[k], mu, xd, x > 0);
      nan_seen = nan_seen || b[k] != b[k];
      if (b[k] > mx) mx = b[k];
    }
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K && b[k] > -INFINITY) s += exp(b[k] - mx);
  if (nan_seen) s = __builtin_nan("");
  lp = ho_logp(mx, s, ho_lgam1((unsigned)x, lgt));
}

// What both entry points reduce: four sums (logp where finite, squared error, x, mean) and four counts (elements, x > 0,
// logp = -inf, and one of the caller's), per thread, per workgroup, per layer -- a fixed tree, no floating-point atomic.
#define LIK_TPB 256
#define LIK_N 4
#define LIK_BAD_NAN 1   // (the walks' WALK_BAD_NAN)

struct LikAcc {
  double s[LIK_N] = {0.0, 0.0, 0.0, 0.0};
  u64 c[LIK_N] = {0ull, 0ull, 0ull, 0ull};
};

// One element into a thread's LikAcc a; lp, mn, x plain variables.  (A macro on purpose: as a function -- by value or by reference,
// member or free -- the same statements cost k_rs_walk<2, false> two registers, 129 instead of 127, and with them the fourth
// wave per SIMD.)
#define LIK_TAKE(a, lp, mn, x, fourth, bad)                                \
  do {                                                                     \
    if (lp != lp || mn != mn) atomicOr(bad, LIK_BAD_NAN);                  \
    const double xd_ = (double)(x), d_ = xd_ - mn;                         \
    if (lp == -INFINITY) (a).c[2] += 1ull; else (a).s[0] += lp;            \
    (a).s[1] += d_ * d_;                                                   \
    (a).s[2] += xd_;                                                       \
    (a).s[3] += mn;                                                        \
    (a).c[0] += 1ull;                                                      \
    (a).c[1] += (x) > 0 ? 1ull : 0ull;                                     \
    (a).c[3] += (fourth) ? 1ull : 0ull;                                    \
  } while (0)

// the workgroup's partials, row blockIdx.x of part and cpart (every thread calls it)
__device__ __forceinline__ void lik_flush(const LikAcc& a, double* __restrict__ part, u64* __restrict__ cpart, double* red, u64* redu) {
#pragma unroll
  for (int c = 0; c < LIK_N; ++c) {
    const double t = block_sum_n(a.s[c], red);
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * LIK_N + c] = t;
  }
#pragma unroll
  for (int c = 0; c < LIK_N; ++c) {
    const u64 t = block_sum_ull(a.c[c], redu);
    if (threadIdx.x == 0) cpart[(size_t)blockIdx.x * LIK_N + c] = t;
  }
}

// second stage: one workgroup adds a layer's nb partials, column by column, in index order
static __global__ __launch_bounds__(LIK_TPB) void k_lik_finish(const double* __restrict__ part, const u64* __restrict__ cpart, size_t nb,
                                                               double* __restrict__ sums, u64* __restrict__ counts) {
  __shared__ double red[16];
  __shared__ u64 redu[16];
  for (int c = 0; c < LIK_N; ++c) {
    double v = 0.0;
    for (size_t b = threadIdx.x; b < nb; b += LIK_TPB) v += part[b * LIK_N + c];
    const double t = block_sum_n(v, red);
    if (threadIdx.x == 0) sums[c] = t;
  }
  for (int c = 0; c < LIK_N; ++c) {
    u64 v = 0;
    for (size_t b = threadIdx.x; b < nb; b += LIK_TPB) v += cpart[b * LIK_N + c];
    const u64 t = block_sum_ull(v, redu);
    if (threadIdx.x == 0) counts[c] = t;
  }
}

// the host's lgamma(x + 1) for x < HO_LGT, into out [HO_LGT]: the table ho_lgam1 reads
static inline void ho_lgt_fill(double* out) {
  for (int x = 0; x < HO_LGT; ++x) {
    int sign = 0;
    out[x] = lgamma_r((double)x + 1.0, &sign);
  }
}

#endif  // VMR_REPORT_LIK_H
