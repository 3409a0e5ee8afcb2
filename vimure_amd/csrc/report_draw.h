// report_draw.h -- the draw of a pair's reports, the one copy that k_gen_x (generate.hip) and the replicate kernels of the
// posterior predictive check (ppc_rep.hip) call: what vmr_generate_x writes at (l,i,j,m) and (l,j,i,m) is what
// vmr_ppc_replicates counts there.
//
// `_build_X` (synthetic.py:159-231): for an unordered pair {i, j}, i < j, and reporter m with rates a (of i -> j) and b (of j -> i)
//     a fair coin picks which direction is drawn first:   first  ~ Poisson((own + eta mirror) / (1 - eta^2))
//                                                         second ~ Poisson(own + eta first)
// in float64, from a counter-based stream: Philox4x32-10 keyed by the seed, counter = (pair t = i N + j, reporter ^ layer << 20,
// call) -- a draw depends on (seed, l, i, j, m) only.
#ifndef VMR_REPORT_DRAW_H
#define VMR_REPORT_DRAW_H
#include "vmr_internal.h"

struct Rng {   // a stream of uniforms for one (layer, pair, reporter): Philox calls as needed
  unsigned k0, k1, c0, c1, c2, n, have;
  unsigned w[4];
  __device__ Rng(unsigned long long seed, unsigned l, unsigned long long pair, unsigned m)
      : k0((unsigned)seed), k1((unsigned)(seed >> 32)), c0((unsigned)pair), c1((unsigned)(pair >> 32)), c2(m ^ (l << 20)), n(0), have(0) {}
  // [2^-54, 1]: 53 bits + 0.5, never 0.  A call's words are consumed 3, 2 then 1, 0.  The + 0.5 is exact below 2^52 and rounds to even
  // from there on, so all-ones words (the integer 2^53 - 1) give exactly 1.0 -- at probability 2^-53, left as it is.
  __device__ double uniform() {
    if (have < 2) {
      unsigned c[4] = {c0, c1, c2, n++};
      philox4x32_10(c, k0, k1);
      w[0] = c[0]; w[1] = c[1]; w[2] = c[2]; w[3] = c[3];
      have = 4;
    }
    const unsigned a = w[have - 1], b = w[have - 2];
    have -= 2;
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6) + 0.5) * (1.0 / 9007199254740992.0);
  }
};

// Poisson(rate): inversion by sequential search below 30 (one uniform, about `rate` steps), Hoermann's transformed rejection (PTRS,
// 1993) above -- the algorithm NumPy's legacy generator uses for rate >= 10 -- both exact.
static __device__ unsigned poisson_draw(double rate, Rng& g) {
  if (!(rate > 0.0)) return 0u;
  if (rate < 30.0) {
    const double u = g.uniform();
    double p = exp(-rate), cdf = p;
    unsigned k = 0;
    while (u > cdf && k < 1000u) { ++k; p *= rate / (double)k; cdf += p; }
    return k;
  }
  const double slam = sqrt(rate), loglam = log(rate), b = 0.931 + 2.53 * slam, a = -0.059 + 0.02483 * b;
  const double invalpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2.0);
  for (int it = 0; it < 64; ++it) {
    const double U = g.uniform() - 0.5, V = g.uniform(), us = 0.5 - fabs(U);
    const double kf = floor((2.0 * a / us + b) * U + rate + 0.43);
    if (us >= 0.07 && V <= vr) return (unsigned)kf;
    if (kf < 0.0 || (us < 0.013 && V > us)) continue;
    if (log(V) + log(invalpha) - log(a / (us * us) + b) <= -rate + kf * loglam - lgamma(kf + 1.0)) return (unsigned)kf;
  }
  return (unsigned)(rate + 0.5);   // (not reached in practice: acceptance is > 0.9 per trial)
}

// 1 / (1 - eta^2) of the first draw's rate
__device__ __forceinline__ double pair_inv(double eta) { return 1.0 / (1.0 - eta * eta); }

// The reports of reporter m on the pair t = i N + j (i < j) of layer l: la, lb the lambda of i -> j and of j -> i, th the reporter's
// theta, inv = pair_inv(eta).  Counts are returned as drawn (no clamp).
__device__ __forceinline__ void pair_draw(unsigned long long seed, unsigned l, unsigned long long t, unsigned m, double la, double lb, double th,
                                          double eta, double inv, unsigned& xij, unsigned& xji) {
  const double a = la * th, b = lb * th;
  Rng g(seed, l, t, m);
  const bool ij_first = g.uniform() < 0.5;
  if (ij_first) {
    xij = poisson_draw((a + eta * b) * inv, g);
    xji = poisson_draw(b + eta * (double)xij, g);
  } else {
    xji = poisson_draw((b + eta * a) * inv, g);
    xij = poisson_draw(a + eta * (double)xji, g);
  }
}

#endif  // VMR_REPORT_DRAW_H
