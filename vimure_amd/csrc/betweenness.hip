// betweenness.hip -- betweenness centrality of the posterior on the device: vmr_sample_betweenness, vmr_network_betweenness.
//
// Who brokers: b(v) = sum over the ordered pairs s != v != t, t reachable from s, of the share sigma_st(v) / sigma_st of the
// shortest s -> t paths that pass through v, on G = A (DIRECTED) or A | A^T (UNION, every unordered pair counted once), A =
// (Y > 0) with the diagonal cleared; unnormalised, endpoints excluded (include/vimure_hip.h has the contract).  It is Brandes'
// algorithm (2001), by levels: from every source s the levels d[v] of a breadth-first search, the path counts sigma[v] =
// sum of sigma[u] over the in-neighbours u one level up, and from the deepest level back delta[w] = sum over the out-neighbours v
// one level down of sigma[w] / sigma[v] (1 + delta[v]); b(v) = sum_s delta_s[v].
//
// vmr_sample_betweenness draws S posterior samples of Y in chunks (sampled_side.h: sample s is what vmr_sample(h, seed + s,
// n_trials) writes) and packs them into bit rows (sampled_side.h has the layout); vmr_network_betweenness uploads the caller's
// networks in chunks and packs them the same way.
// k_btw_brandes: one workgroup (4 waves) per (block of BTW_SB = 16 consecutive sources, layer, sample): the block depends on N
// only, never on the device or the chunk.  Per source, in LDS: sigma and delta (FP64, N each), d (16-bit, over the 64 W padded
// nodes) and one bit row `nx`, and 64 slots of 16 bits per node a thread owns for the waves' node lists: 16 N + 136 W + 512 KPT
// bytes and 256 of the barrier's OR -- 40,704 at N = 2000, four workgroups to a CU; 41,472 at N = VMR_BTW_NMAX = 2048, three.  Thread t owns nodes t,
// t + 256, .. : it keeps their share of b over the block's sources in registers, and a wave therefore owns whole 64-node words
// (KPT of them).  Every step that walks rows has one shape (btw_level): a wave lists its own
// nodes at one level (ballots; a level's nodes lie scattered over the words, the list packs them so that no lane group idles on
// an absent node), G lanes (the largest power of two <= min(W, 64)) stride the W words of a row, 64 / G rows side by side, the
// words of BTW_FLY rows are loaded before the first is used, and a fixed xor tree runs over the G lanes.  Per level l = 1, 2, ..:
//   expand   the nodes at level l - 1 OR their out-rows into nx (integer LDS atomics); barrier;
//   update   a wave's nodes whose nx bit is set and that have no level yet get d = l; the wave clears its words of nx; barrier
//            (and the search ends when no thread added a node, or at l = N - 1: the loop is bounded by N by construction);
//   sigma    the nodes at level l read their in-row once and add sigma[u] of the set bits u with d[u] = l - 1, each lane its
//            words in ascending u -- no barrier: the next expand touches nx and d only.
// Then from the deepest level up: sigma[v] of a finished node v is replaced by its coefficient c[v] = (1 + delta[v]) / sigma[v],
// and a node w at level l reads its out-row once, adds c[v] over the set bits v with d[v] = l + 1 and stores delta[w] =
// sigma[w] * sum.  That is the recommended (sigma[w] / sigma[v]) (1 + delta[v]) with sigma[w] taken out of the sum: one division
// per node and source, not one per tie of the shortest-path graph -- an IEEE FP64 division is some thirty instructions, and a
// source's ties outnumber its nodes by the mean degree -- and the gather of the two pulls is the same code.  Roundings per term:
// 1 + delta, the quotient, the add, and the product once per node: no more than the form it replaces.  So each row is read three
// times per source (expand, sigma, delta), never once per level.  sigma is FP64 throughout: exact up to 2^53 and for every
// power of two; beyond 1.8e308 (a chain of ~680 three-way joins) it overflows and b is not defined.
// The workgroups of one (sample, layer) share its bit rows (16 N W bytes: 1 MB at N = 2000): the linear workgroup index is
// mapped so that those of equal index mod 8 -- which share an XCD's L2 as the dispatcher is observed to place them -- take the
// blocks of one graph after another.  The map changes where a block runs, not what it computes.
// k_btw_fold_blocks: one workgroup per (layer, sample) adds the blocks' shares in ascending block order, halves the sum for
// UNION, ranks the nodes (strictly larger entries, as k_cent_walk) and stores the sample's total (a fixed tree) and maximum.
// k_node_fold (node_fold.h) adds the chunk's samples in ascending s into the per-node accumulators of the call.
// No floating-point atomics, every sum in a fixed order, no contraction where a product feeds a sum: every output is the same
// from run to run and for any chunking.
// Bytes per source: 3 N W 8 from L2 (6 N W 8 with UNION) -- at N = 2000: 1.5 MB, 3.1 GB per (sample, layer) -- against 2 N 8
// written once per block of 16 sources; d, sigma and delta never leave the compute unit.  The kernel waits on the latency of the
// row gathers from L2 and, per level, on two barriers.
#include "node_fold.h"

namespace {

#define BTW_TPB 256
#define BTW_SB 16                            // sources per workgroup: a function of nothing, so that results are the same everywhere
#define BTW_FLY 4                            // rows whose words a lane group has in flight
#define BTW_KPT (VMR_BTW_NMAX / BTW_TPB)     // nodes a thread owns at most
#define BTW_UNSEEN 0xffffu                   // the level of a node the search has not reached (levels are < N <= 2048)

enum { BTW_EXPAND = 0, BTW_SIGMA = 1, BTW_DELTA = 2 };

// One walk over the rows R (| R2 with UNION) of this wave's nodes at level `lvl`, every lane of the workgroup calls it:
//   BTW_EXPAND  nx |= row
//   BTW_SIGMA   sig[row] = sum of sig[x] over the set bits x with d[x] == want
//   BTW_DELTA   the same sum a, then del[row] = sig[row] * a and sig[row] = (1 + del[row]) / sig[row], the node's coefficient
// each lane its own words in ascending order, then the xor tree over the G = 1 << lG lanes of the row.  list: the wave's 64 KPT
// node slots.
template <bool UNION, int MODE, int KPT>
__device__ __forceinline__ void btw_level(const u64* __restrict__ R, const u64* __restrict__ R2, int N, int W, int lG, int lvl, int want,
                                          const unsigned short* d, double* sig, double* del, u64* nx, unsigned short* list) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int G = 1 << lG, nps = 64 >> lG, sub = lane >> lG, wl = lane & (G - 1);
  const u64 lt = (1ull << lane) - 1ull;
  int n = 0;   // (the same in every lane of the wave)
#pragma unroll
  for (int k = 0; k < KPT; ++k) {
    const int u = k * BTW_TPB + wv * 64 + lane;
    const bool in = u < N && d[u] == lvl;
    const u64 m = __ballot(in);
    if (in) list[n + __popcll(m & lt)] = (unsigned short)u;
    n += __popcll(m);
  }
  wave_sync();
  for (int t0 = 0; t0 < n; t0 += BTW_FLY * nps) {
    int row[BTW_FLY];
    double acc[BTW_FLY];
#pragma unroll
    for (int f = 0; f < BTW_FLY; ++f) {
      const int idx = t0 + f * nps + sub;
      row[f] = idx < n ? (int)list[idx] : -1;   // (< N)
      acc[f] = 0.0;
    }
    for (int ww = wl; ww < W; ww += G) {   // (one trip when W is a power of two)
      u64 wd[BTW_FLY];
#pragma unroll
      for (int f = 0; f < BTW_FLY; ++f) {
        wd[f] = 0ull;
        if (row[f] >= 0) {
          const size_t o = (size_t)row[f] * W + ww;
          wd[f] = R[o];
          if (UNION) wd[f] |= R2[o];
        }
      }
#pragma unroll
      for (int f = 0; f < BTW_FLY; ++f) {
        u64 w = wd[f];
        if (MODE == BTW_EXPAND) {
          if (w) atomicOr(&nx[ww], w);
        } else {
          while (w) {
            const int x = ww * 64 + __ffsll((long long)w) - 1;   // (< 64 W: inside the arrays whatever the pad bits hold)
            if (d[x] == want) acc[f] += sig[x];
            w &= w - 1ull;
          }
        }
      }
    }
    if (MODE != BTW_EXPAND) {
#pragma unroll
      for (int f = 0; f < BTW_FLY; ++f) {
        double a = acc[f];
        for (int o = G >> 1; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);   // (every lane of the wave is here)
        if (wl == 0 && row[f] >= 0) {
          if (MODE == BTW_SIGMA) {
            sig[row[f]] = a;
          } else {   // (nobody reads sig of this level any more: the levels above read it as the coefficient)
            const double s = sig[row[f]], dl = s * a;
            del[row[f]] = dl;
            sig[row[f]] = (1.0 + dl) / s;
          }
        }
      }
    }
  }
  wave_sync();   // (the list is free for the next walk)
}

// Grid: 8 nblk ceil(nsl / 8) workgroups in one dimension, nblk = ceil(N / BTW_SB) source blocks, nsl = the chunk's (sample, layer)
// pairs; index id takes block (id / 8) % nblk of graph 8 ((id / 8) / nblk) + id % 8.  Dynamic LDS: N doubles sigma, N doubles
// delta, W words nx, 64 W 16-bit levels.  part[nsl][nblk][N]: the block's share of b, every element stored.
template <bool UNION, int KPT>
__global__ __launch_bounds__(BTW_TPB) void k_btw_brandes(const u64* __restrict__ Aout, const u64* __restrict__ Ain, int N, int W, int lG, int nblk,
                                                         int nsl, double* __restrict__ part) {
  extern __shared__ double btw_lds[];
  __shared__ unsigned short lists[BTW_TPB / 64][KPT * 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r = (int)(blockIdx.x >> 3), blk = r % nblk;
  const int g = 8 * (r / nblk) + (int)(blockIdx.x & 7u);
  if (g >= nsl) return;   // (the whole workgroup)
  const int Np = W * 64;
  double *sig = btw_lds, *del = btw_lds + N;   // (a pad node has no level: its sigma is never read)
  u64* nx = reinterpret_cast<u64*>(btw_lds + 2 * N);
  unsigned short* d = reinterpret_cast<unsigned short*>(nx + W);
  unsigned short* list = lists[wv];
  const u64* Ao = Aout + (size_t)g * N * W;
  const u64* Ai = Ain + (size_t)g * N * W;
  double b[KPT];
#pragma unroll
  for (int k = 0; k < KPT; ++k) b[k] = 0.0;
  const int s_end = (blk + 1) * BTW_SB < N ? (blk + 1) * BTW_SB : N;
  for (int s = blk * BTW_SB; s < s_end; ++s) {
    __syncthreads();   // (the last source's delta has been read)
    for (int v = tid; v < Np; v += BTW_TPB) {
      d[v] = (unsigned short)(v == s ? 0u : BTW_UNSEEN);
      if (v < N) { sig[v] = v == s ? 1.0 : 0.0; del[v] = 0.0; }
    }
    for (int w = tid; w < W; w += BTW_TPB) nx[w] = 0ull;
    __syncthreads();
    int last = 0;
    for (int lvl = 1; lvl < N; ++lvl) {   // (a shortest path has at most N - 1 ties)
      btw_level<UNION, BTW_EXPAND, KPT>(Ao, Ai, N, W, lG, lvl - 1, 0, d, sig, del, nx, list);
      __syncthreads();
      bool any = false;
#pragma unroll
      for (int k = 0; k < KPT; ++k) {
        const int wi = k * (BTW_TPB / 64) + wv, v = wi * 64 + lane;   // (this wave's word, this thread's node of it)
        if (wi < W) {
          const bool nw = v < N && ((nx[wi] >> lane) & 1ull) && d[v] == BTW_UNSEEN;
          if (nw) d[v] = (unsigned short)lvl;
          any |= nw;
          wave_sync();   // (every lane has read the word)
          if (lane == 0) nx[wi] = 0ull;
        }
      }
      if (!__syncthreads_or(any)) break;
      last = lvl;
      btw_level<UNION, BTW_SIGMA, KPT>(Ai, Ao, N, W, lG, lvl, lvl - 1, d, sig, del, nx, list);
    }
    __syncthreads();   // (sigma is complete)
    // the deepest level has delta = 0 and the coefficient 1 / sigma; then level by level up to the source's neighbours
#pragma unroll
    for (int k = 0; k < KPT; ++k) {
      const int v = tid + k * BTW_TPB;
      if (last > 0 && v < N && d[v] == last) sig[v] = 1.0 / sig[v];
    }
    __syncthreads();
    for (int lvl = last - 1; lvl >= 1; --lvl) {
      btw_level<UNION, BTW_DELTA, KPT>(Ao, Ai, N, W, lG, lvl, lvl + 1, d, sig, del, nx, list);
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < KPT; ++k) {
      const int v = tid + k * BTW_TPB;
      if (v < N) b[k] += del[v];   // (0 for the source and for what it does not reach)
    }
  }
  double* out = part + ((size_t)g * nblk + blk) * N;
#pragma unroll
  for (int k = 0; k < KPT; ++k) {
    const int v = tid + k * BTW_TPB;
    if (v < N) out[v] = b[k];
  }
}

// Grid (nsl): b[v] = the blocks' shares in ascending block order (times 1/2 with `half`, exact), into cval[sl][N]; crank[sl][N]
// = #{u : b[u] > b[v]} and summary[sl][2] = (sum_v b[v] by a fixed tree, max_v b[v]) unless null.
__global__ __launch_bounds__(BTW_TPB) void k_btw_fold_blocks(const double* __restrict__ part, int N, int nblk, int half, double* __restrict__ cval,
                                                             unsigned* __restrict__ crank, double* __restrict__ summary) {
  __shared__ double bs[VMR_BTW_NMAX];
  __shared__ double red[16];
  const int tid = threadIdx.x;
  const size_t sl = blockIdx.x;
  const double* p = part + sl * nblk * N;
  double c[BTW_KPT];
  double tsum = 0.0, tmax = 0.0;
#pragma unroll
  for (int k = 0; k < BTW_KPT; ++k) {
    const int v = tid + k * BTW_TPB;
    c[k] = 0.0;
    if (v < N) {
      double a = 0.0;
      for (int q = 0; q < nblk; ++q) a += p[(size_t)q * N + v];
      if (half) a *= 0.5;
      c[k] = a; bs[v] = a;
      cval[sl * N + v] = a;
      tsum += a; tmax = fmax(tmax, a);
    }
  }
  __syncthreads();
  if (crank) {
    unsigned rk[BTW_KPT];
#pragma unroll
    for (int k = 0; k < BTW_KPT; ++k) rk[k] = 0u;
    for (int u = 0; u < N; ++u) {
      const double bu = bs[u];   // (the same address in every lane)
#pragma unroll
      for (int k = 0; k < BTW_KPT; ++k) rk[k] += bu > c[k] ? 1u : 0u;
    }
#pragma unroll
    for (int k = 0; k < BTW_KPT; ++k) {
      const int v = tid + k * BTW_TPB;
      if (v < N) crank[sl * N + v] = rk[k];
    }
  }
  if (summary) {   // (the same in every thread)
    const double sum = block_sum_n(tsum, red);
    tmax = wave_max(tmax);
    __syncthreads();
    if ((tid & 63) == 0) red[8 + (tid >> 6)] = tmax;
    __syncthreads();
    if (tid == 0) {
      double m = red[8];
      for (int w = 1; w < BTW_TPB / 64; ++w) m = fmax(m, red[8 + w]);
      summary[sl * 2] = sum;
      summary[sl * 2 + 1] = m;
    }
  }
}

// what both calls refuse of N and direction, or VMR_OK
int btw_args(vmr_ctx* h, const char* fn, int direction) {
  char msg[256];
  if (h->g.N > VMR_BTW_NMAX) {
    snprintf(msg, sizeof msg, "%s: a source keeps 18 N bytes in LDS: N <= %d, the handle has N = %d", fn, VMR_BTW_NMAX, h->g.N);
    return fail(h, VMR_EINVAL, msg);
  }
  if (direction < VMR_BTW_DIRECTED || direction > VMR_BTW_UNION) {
    snprintf(msg, sizeof msg, "%s: direction must be 0 (directed) or 1 (union), got %d", fn, direction);
    return fail(h, VMR_EINVAL, msg);
  }
  return VMR_OK;
}

// the shape of both calls' kernels on a handle: the bit rows' and what is this unit's
struct BtwShape : BitRows {
  int nblk, kpt;
  size_t smem, part_b;   // part_b: bytes per sample of the blocks' shares
};
BtwShape btw_shape(const Geo& g) {
  BtwShape b;
  static_cast<BitRows&>(b) = bit_rows(g);
  b.nblk = (g.N + BTW_SB - 1) / BTW_SB;
  b.kpt = (g.N + BTW_TPB - 1) / BTW_TPB;   // nodes a thread owns: 1 .. BTW_KPT
  b.smem = (size_t)g.N * 16 + (size_t)b.W * (8 + 64 * 2);
  b.part_b = b.LN * b.nblk * 8;
  return b;
}

// the packed chunk of c samples (or networks) -> cval[c][L][N], and crank, summary unless null
int btw_chunk(vmr_ctx* h, const BtwShape& b, int c, int direction, const u64* Ao, const u64* Ai, double* part, double* cval, unsigned* crank,
              double* summary) {
  const int nsl = c * h->g.L;
  const unsigned grid = 8u * (unsigned)b.nblk * (unsigned)((nsl + 7) / 8);
  auto launch = [&](auto U, auto K) {
    hipLaunchKernelGGL((k_btw_brandes<decltype(U)::value, decltype(K)::value>), dim3(grid), dim3(BTW_TPB), b.smem, h->stream, Ao, Ai, h->g.N, b.W, b.lG,
                       b.nblk, nsl, part);
  };
  with_kpt(b.kpt, [&](auto K) {
    if (direction == VMR_BTW_UNION) launch(std::true_type{}, K);
    else launch(std::false_type{}, K);
  });
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(k_btw_fold_blocks, dim3((unsigned)nsl), dim3(BTW_TPB), 0, h->stream, part, h->g.N, b.nblk, direction == VMR_BTW_UNION, cval, crank,
                     summary);
  HIPCHK(h, hipGetLastError());
  return VMR_OK;
}

}  // namespace

extern "C" int vmr_sample_betweenness(vmr_handle h, uint64_t seed, int n_samples, int n_trials, int direction, int top_k, double* node_sum,
                                      double* node_sumsq, uint64_t* node_rank_sum, uint32_t* node_top, double* summary, double* values) {
  if (!h) return VMR_EINVAL;
  const char* fn = "vmr_sample_betweenness";
  int rc;
  if ((rc = sampled_counts(h, fn, n_samples, n_trials))) return rc;
  if ((rc = btw_args(h, fn, direction))) return rc;
  if ((rc = node_fold_args(h, fn, top_k, node_sum))) return rc;
  if ((rc = expected_begin(h, fn))) return rc;
  const Geo& g = h->g;
  const BtwShape b = btw_shape(g);
  const size_t LN = b.LN;
  SampledOut out[1] = {{summary, (size_t)g.L * 16, false, "vmr_sample_betweenness: the summary", nullptr}};
  // device bytes per sample of a chunk: the bit-row chunk, the blocks' shares, b and the ranks, the summary; per call: the accumulators
  const size_t per = b.per() + b.part_b + LN * 12 + (summary ? out[0].bytes : 0);
  size_t C;
  if ((rc = chunk_samples(h, fn, (size_t)n_samples, per, NodeFold::bytes(LN), &C))) return rc;
  Tmp tm(h);
  uint8_t* Y = nullptr;
  u64 *Ao = nullptr, *Ai = nullptr;
  double *part = nullptr, *cval = nullptr;
  unsigned* crank = nullptr;
  NodeFold fold;
  if ((rc = bit_rows_get(tm, b, C, fn, "samples", &Y, &Ao, &Ai)) ||
      (rc = tm.get(&part, C * b.part_b, "vmr_sample_betweenness: the source blocks' shares")) ||
      (rc = tm.get(&cval, C * LN * 8, "vmr_sample_betweenness: the values")) ||
      (rc = tm.get(&crank, C * LN * 4, "vmr_sample_betweenness: the ranks")) || (rc = fold.begin(h, tm, fn, LN, top_k)))
    return rc;
  rc = sampled_chunks(h, tm, (size_t)n_samples, C, seed, n_trials, Y, out, [&](size_t s0, int c) -> int {
    int rc2;
    if ((rc2 = tri_pack_chunk(h, Y, c, Ao, Ai))) return rc2;
    if ((rc2 = btw_chunk(h, b, c, direction, Ao, Ai, part, cval, crank, out[0].as<double>()))) return rc2;
    if ((rc2 = fold.add(h, cval, crank, c))) return rc2;
    if (values) HIPCHK(h, hipMemcpyAsync(values + s0 * LN, cval, (size_t)c * LN * 8, hipMemcpyDeviceToHost, h->stream));
    return VMR_OK;
  });
  return rc ? rc : fold.finish(h, node_sum, node_sumsq, node_rank_sum, node_top);
}

extern "C" int vmr_network_betweenness(vmr_handle h, const uint8_t* Y, int n, int direction, double* values) {
  if (!h) return VMR_EINVAL;
  const char* fn = "vmr_network_betweenness";
  int rc;
  if (n < 1) return fail(h, VMR_EINVAL, "vmr_network_betweenness: n must be positive");
  if ((rc = btw_args(h, fn, direction))) return rc;
  if (!Y) return fail(h, VMR_EINVAL, "vmr_network_betweenness: Y is NULL");
  if (!values) return fail(h, VMR_EINVAL, "vmr_network_betweenness: values is NULL");
  HIPCHK(h, hipSetDevice(h->device));
  const BtwShape b = btw_shape(h->g);
  const size_t per = b.per() + b.part_b + b.LN * 8;
  size_t C;
  if ((rc = chunk_samples(h, fn, (size_t)n, per, 0, &C, "network"))) return rc;
  Tmp tm(h);
  uint8_t* Yd = nullptr;
  u64 *Ao = nullptr, *Ai = nullptr;
  double *part = nullptr, *cval = nullptr;
  if ((rc = bit_rows_get(tm, b, C, fn, "networks", &Yd, &Ao, &Ai)) ||
      (rc = tm.get(&part, C * b.part_b, "vmr_network_betweenness: the source blocks' shares")) ||
      (rc = tm.get(&cval, C * b.LN * 8, "vmr_network_betweenness: the values")))
    return rc;
  return uploaded_chunks(h, b, (size_t)n, C, Y, Yd, Ao, Ai, [&](size_t s0, int c) -> int {
    int rc2;
    if ((rc2 = btw_chunk(h, b, c, direction, Ao, Ai, part, cval, nullptr, nullptr))) return rc2;
    HIPCHK(h, hipMemcpyAsync(values + s0 * b.LN, cval, (size_t)c * b.LN * 8, hipMemcpyDeviceToHost, h->stream));
    return VMR_OK;
  });
}
