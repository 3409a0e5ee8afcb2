// rho_row.h -- what the read-side kernels take from one tie's row of rho: the first maximum, the readout byte and the two
// ascending sums, written once so that every caller rounds alike.
#ifndef VMR_RHO_ROW_H
#define VMR_RHO_ROW_H
#include "vmr_internal.h"

// the category vmr_readout(VMR_READ_RHO_MAX) writes for a tie (k_readout, vimure_hip.hip): the first maximum, as np.argmax
__device__ __forceinline__ unsigned rho_row_argmax(const double* __restrict__ r, int K) {
  int best = 0;
  double bv = r[0];
  for (int k = 1; k < K; ++k) if (r[k] > bv) { bv = r[k]; best = k; }
  return (unsigned)best;
}

// the byte vmr_readout writes for a tie under a readout of categories: the threshold on rho_1, else the first maximum
__device__ __forceinline__ unsigned rho_row_readout(const double* __restrict__ r, int K, int method, double threshold) {
  if (method == VMR_READ_THRESHOLD) return r[1] >= threshold ? 1u : 0u;
  return rho_row_argmax(r, K);
}

// prob = sum_{k>=1} rho_k and mean = sum_k k rho_k, k ascending, every product and every sum rounded on its own: the compiler may
// not contract k * rho_k + mean to a fused multiply-add here (__dmul_rn / __dadd_rn are inlined header code and do not stop it)
__device__ __forceinline__ void rho_row_prob_mean(const double* __restrict__ q, int K, double& prob, double& mean) {
#pragma clang fp contract(off)
  double pr = 0.0, mn = 0.0;
  for (int k = 1; k < K; ++k) {
    const double v = q[k];
    const double kv = (double)k * v;
    pr = pr + v;
    mn = mn + kv;
  }
  prob = pr; mean = mn;
}

#endif  // VMR_RHO_ROW_H
