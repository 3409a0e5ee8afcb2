// report_lik.h -- the Poisson-mixture likelihood of one report under a tie's rho row, shared by heldout.hip (a list of entries the
// caller gives) and report_scores.hip (every element of the support): one definition of the rates, of the terms
// b_k = x log mu_k - mu_k + log rho_k, of lgamma(x + 1) and of the log-sum-exp, so that both entry points give the same bits
// for the same (rho row, theta, lambda, eta, x, xt).
#ifndef VMR_REPORT_LIK_H
#define VMR_REPORT_LIK_H
#include "vmr_internal.h"

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

// the host's lgamma(x + 1) for x < HO_LGT, into out [HO_LGT]: the table ho_lgam1 reads
static inline void ho_lgt_fill(double* out) {
  for (int x = 0; x < HO_LGT; ++x) {
    int sign = 0;
    out[x] = lgamma_r((double)x + 1.0, &sign);
  }
}

#endif  // VMR_REPORT_LIK_H
