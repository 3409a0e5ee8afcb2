// node_fold.h -- what the units that return a per-node value of every posterior sample share (centrality.hip, betweenness.hip, cores.hip), on
// top of sampled_side.h: the wave's maximum and the fold of a chunk's values and ranks into the call's per-node accumulators.
// Everything here is static or inline.
#ifndef VMR_NODE_FOLD_H
#define VMR_NODE_FOLD_H
#include "sampled_side.h"

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// One thread per (l, v): the chunk's samples in ascending s into the call's accumulators.  The square is rounded before it is
// added (no contraction), as a host restatement rounds it.
static __global__ __launch_bounds__(256) void k_node_fold(const double* __restrict__ cval, const unsigned* __restrict__ crank, int c, size_t LN,
                                                          unsigned top_k, double* __restrict__ sum, double* __restrict__ sumsq,
                                                          u64* __restrict__ rank_sum, unsigned* __restrict__ top) {
#pragma clang fp contract(off)
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= LN) return;
  double a = sum[e], b = sumsq[e];
  u64 r = rank_sum[e];
  unsigned tp = top[e];
  for (int s = 0; s < c; ++s) {
    const double v = cval[(size_t)s * LN + e];
    const unsigned k = crank[(size_t)s * LN + e];
    const double v2 = v * v;
    a += v;
    b += v2;
    r += k;
    tp += k < top_k ? 1u : 0u;
  }
  sum[e] = a; sumsq[e] = b; rank_sum[e] = r; top[e] = tp;
}

#endif  // VMR_NODE_FOLD_H
