// conn_expand.h -- the expansion step of the 64-source breadth-first search over bit rows, what connectivity.hip (every level of
// its closures) and cascades.hip (every period of a cascade) share, on top of sampled_side.h.  Node v carries a 64-bit word in LDS
// whose bit q belongs to source (or seed set) q; a level ORs the word of every frontier node into the words of its neighbours.
#ifndef VMR_CONN_EXPAND_H
#define VMR_CONN_EXPAND_H
#include "sampled_side.h"

#define CONN_TPB 256
#define CONN_FLY 8                            // rows whose words a lane group has in flight: the expansion waits on L2, not on bytes

// The expansion of one level: every node u of the frontier ORs fr[u] into nx[v] for every set bit v of its row of A (| B with
// UNION).  A wave takes 64 consecutive nodes, one per lane, and ballots the non-empty frontier words; G = 1 << lG lanes stride the
// W words of a row, 64 / G rows side by side, and the words of CONN_FLY rows are loaded before the first is used.
template <bool UNION>
__device__ __forceinline__ void conn_expand(const u64* __restrict__ A, const u64* __restrict__ B, int N, int W, int lG, const u64* fr, u64* nx) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int G = 1 << lG, nps = 64 >> lG, sub = lane >> lG, wl = lane & (G - 1);
  for (int base = wv * 64; base < N; base += CONN_TPB) {
    const int u1 = base + lane;
    const u64 mask = __ballot(u1 < N && fr[u1] != 0ull);
    if (!mask) continue;   // (the same in every lane of the wave)
    for (int ww = wl; ww < W; ww += G) {   // (one trip when W is a power of two)
      for (int j0 = sub; j0 < 64; j0 += CONN_FLY * nps) {
        u64 wa[CONN_FLY], wb[CONN_FLY], f[CONN_FLY];
#pragma unroll
        for (int t = 0; t < CONN_FLY; ++t) {
          const int j = j0 + t * nps;
          wa[t] = 0ull; wb[t] = 0ull; f[t] = 0ull;
          if (j < 64 && ((mask >> j) & 1ull)) {   // (then base + j < N)
            const size_t o = (size_t)(base + j) * W + ww;
            f[t] = fr[base + j];
            wa[t] = A[o];
            if (UNION) wb[t] = B[o];
          }
        }
#pragma unroll
        for (int t = 0; t < CONN_FLY; ++t) {
          u64 wd = wa[t] | wb[t];
          while (wd) {
            const int bit = __ffsll((long long)wd) - 1;
            atomicOr(&nx[ww * 64 + bit], f[t]);   // (< 64 W: inside the array whatever the pad bits hold)
            wd &= wd - 1ull;
          }
        }
      }
    }
  }
}

#endif  // VMR_CONN_EXPAND_H
