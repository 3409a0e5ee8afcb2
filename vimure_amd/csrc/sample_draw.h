// sample_draw.h -- the per-tie draw of the device sampler, the one copy that k_sample (vimure_hip.hip), k_sample_gen (sweep_gen.hip)
// and the network-statistics kernels (netstats.hip) call: what vmr_sample writes for (seed, tie) is what vmr_sample_stats counts.
//
// `sample_inferred_model` (model.py:1062-1096): n_trials categorical trials from the tie's rho, the most frequent category (first
// maximum) -- Generator.multinomial(n, rho).argmax(-1).  The uniforms come from Philox4x32-10 with key = seed and counter = (tie
// index in [L,N,N] order, trial pair): a call gives the 53-bit uniforms of two trials.  A trial selects the first k with
// u < rho_0 + .. + rho_k (running sum, k ascending; the last category catches the rest).
#ifndef VMR_SAMPLE_DRAW_H
#define VMR_SAMPLE_DRAW_H
#include "vmr_internal.h"

// r: the tie's K probabilities; t: the tie's index in [L,N,N] order.  LDS_CNT = false: K <= KMAX, the trial counts live in registers
// (cnt_lds unused); true: any K, they live in cnt_lds[k * 64] (a column of a [K][64] LDS array per thread).
template <bool LDS_CNT>
__device__ __forceinline__ int draw_tie(const double* __restrict__ r, int K, int n_trials, unsigned long long seed, size_t t, unsigned* cnt_lds) {
  unsigned cnt[KMAX];
  if (LDS_CNT) {
    for (int k = 0; k < K; ++k) cnt_lds[k * 64] = 0u;
  } else {
#pragma unroll
    for (int k = 0; k < KMAX; ++k) cnt[k] = 0u;
  }
  for (int n = 0; n < n_trials; n += 2) {
    unsigned c[4] = {(unsigned)t, (unsigned)((unsigned long long)t >> 32), (unsigned)(n >> 1), 0u};
    philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (n + i < n_trials) {
        const double u = ((double)(c[2 * i] >> 5) * 67108864.0 + (double)(c[2 * i + 1] >> 6)) * (1.0 / 9007199254740992.0);
        int sel = 0;
        double acc = r[0];
        for (int k = 1; k < K; ++k) { if (u >= acc) sel = k; acc += r[k]; }   // first k with u < cumulative sum; the last one catches the rest
        if (LDS_CNT) {
          cnt_lds[sel * 64] += 1u;
        } else {
#pragma unroll
          for (int k = 0; k < KMAX; ++k) cnt[k] += (sel == k) ? 1u : 0u;
        }
      }
    }
  }
  int best = 0;
  if (LDS_CNT) {
    for (int k = 1; k < K; ++k) if (cnt_lds[k * 64] > cnt_lds[best * 64]) best = k;
  } else {
#pragma unroll
    for (int k = 1; k < KMAX; ++k) if (k < K && cnt[k] > cnt[best]) best = k;
  }
  return best;
}

#endif  // VMR_SAMPLE_DRAW_H
