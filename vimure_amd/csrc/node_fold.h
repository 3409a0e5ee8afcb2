// node_fold.h -- what the units that return a per-node value of every posterior sample share (centrality.hip, betweenness.hip, cores.hip), on
// top of sampled_side.h: the fold of a chunk's values and ranks into the call's per-node accumulators -- the kernel, and the
// host struct that owns the accumulators from the entry checks to the copy-out.  Everything here is static or inline.
#ifndef VMR_NODE_FOLD_H
#define VMR_NODE_FOLD_H
#include "sampled_side.h"

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

// what every call that folds refuses of top_k and node_sum, after its own arguments and before the state is looked at
static inline int node_fold_args(vmr_ctx* h, const char* fn, int top_k, const void* node_sum) {
  if (top_k < 1 || top_k > h->g.N) {
    char msg[256];
    snprintf(msg, sizeof msg, "%s: top_k must be in [1, N = %d], got %d", fn, h->g.N, top_k);
    return fail(h, VMR_EINVAL, msg);
  }
  if (!node_sum) return fail(h, VMR_EINVAL, (std::string(fn) + ": node_sum is NULL").c_str());
  return VMR_OK;
}

// The per-node accumulators of a call, which span its chunks: sum_s v, sum_s v^2, sum_s rank and #{s : rank < top_k}, [L][N] each.
struct NodeFold {
  size_t LN = 0;
  unsigned top_k = 0;
  double *sum = nullptr, *sumsq = nullptr;
  u64* rank_sum = nullptr;
  unsigned* top = nullptr;
  static size_t bytes(size_t LN) { return LN * 28; }   // device bytes per call
  // allocates them from tm and zeroes them on the handle's stream
  int begin(vmr_ctx* h, Tmp& tm, const char* fn, size_t LN_, int top_k_) {
    LN = LN_;
    top_k = (unsigned)top_k_;
    const std::string f = std::string(fn) + ": the node ";
    int rc;
    if ((rc = tm.get(&sum, LN * 8, (f + "sums").c_str())) || (rc = tm.get(&sumsq, LN * 8, (f + "sums of squares").c_str())) ||
        (rc = tm.get(&rank_sum, LN * 8, (f + "rank sums").c_str())) || (rc = tm.get(&top, LN * 4, (f + "top counts").c_str())))
      return rc;
    HIPCHK(h, hipMemsetAsync(sum, 0, LN * 8, h->stream));
    HIPCHK(h, hipMemsetAsync(sumsq, 0, LN * 8, h->stream));
    HIPCHK(h, hipMemsetAsync(rank_sum, 0, LN * 8, h->stream));
    HIPCHK(h, hipMemsetAsync(top, 0, LN * 4, h->stream));
    return VMR_OK;
  }
  // a chunk of c samples: cval[c][L][N], crank[c][L][N]
  int add(vmr_ctx* h, const double* cval, const unsigned* crank, int c) {
    hipLaunchKernelGGL(k_node_fold, dim3(grid_for(LN, 256, 0xffffffffu)), dim3(256), 0, h->stream, cval, crank, c, LN, top_k, sum, sumsq, rank_sum, top);
    HIPCHK(h, hipGetLastError());
    return VMR_OK;
  }
  // the outputs that are asked for to the host (node_sum always is), then waits for the stream
  int finish(vmr_ctx* h, double* node_sum, double* node_sumsq, uint64_t* node_rank_sum, uint32_t* node_top) {
    HIPCHK(h, hipMemcpyAsync(node_sum, sum, LN * 8, hipMemcpyDeviceToHost, h->stream));
    if (node_sumsq) HIPCHK(h, hipMemcpyAsync(node_sumsq, sumsq, LN * 8, hipMemcpyDeviceToHost, h->stream));
    if (node_rank_sum) HIPCHK(h, hipMemcpyAsync(node_rank_sum, rank_sum, LN * 8, hipMemcpyDeviceToHost, h->stream));
    if (node_top) HIPCHK(h, hipMemcpyAsync(node_top, top, LN * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return VMR_OK;
  }
};

#endif  // VMR_NODE_FOLD_H
