// cores.hip -- the k-core decomposition of the posterior on the device: vmr_sample_cores, vmr_network_cores.
//
// Where the dense core is: with A = (Y > 0), the diagonal cleared, the k-core is the largest node set in which every node has
// degree >= k counted inside the set, core(v) the largest k whose core holds v, the degeneracy max_v core(v) and the main core the
// nodes that attain it.  The degree is chosen by mode (include/vimure_hip.h has the contract): UNION the distinct neighbours in
// A | A^T, TOTAL in-degree plus out-degree, IN, OUT.
//
// vmr_sample_cores draws S posterior samples of Y in chunks (sampled_side.h: sample s is what vmr_sample(h, seed + s, n_trials)
// writes) and packs them into bit rows (sampled_side.h has the layout); vmr_network_cores uploads the caller's networks in chunks
// and packs them the same way.
// k_core_peel: one workgroup (4 waves) per (sample or network, layer).  In LDS: deg (32 bits for each of the 64 W padded nodes),
// the bit row `alive` (W words), 64 slots of 16 bits per node a thread owns for the waves' node lists and 28 words of the rounds'
// tallies and the summary's sums: 8192 + 256 + 4096 + 112 = 12,656 bytes whatever N, twelve workgroups' worth to a CU.  Thread t owns nodes t, t + 256,
// ..; a wave therefore owns whole 64-node words of `alive`.  The degrees are popcounts of the rows (of Aout | Ain for UNION), G
// lanes (the largest power of two <= min(W, 64)) to a row and a fixed xor tree over them.  Then rounds, k from 0:
//   select   every thread looks at its nodes that are alive with deg <= k: the wave lists them (ballots), stores core = k in their
//            deg slot -- a dead node's deg is never read or decremented again, so the slot is free -- and clears them from its own
//            words of `alive`.  Nothing is decremented here: the degrees are a snapshot.  Each wave leaves its count and the
//            smallest deg of the nodes it keeps alive; barrier.
//   jump     no wave listed a node: k = the smallest deg over the alive nodes and the round ends (one barrier).  Never k + 1: a
//            clique beside isolated nodes would take N empty rounds.
//   remove   otherwise the listed nodes' rows are walked as btw_level of betweenness.hip walks them -- G lanes stride the W words
//            of a row, 64 / G rows side by side, the words of CORE_FLY rows loaded before the first is used -- each word ANDed
//            with `alive` and one integer LDS atomicSub per set bit: UNION the bits of Aout[v] | Ain[v], TOTAL the bits of Aout[v]
//            and those of Ain[v] (a mutual neighbour loses 2), IN the bits of Aout[v] (its out-neighbours lose an in-tie), OUT
//            those of Ain[v].  Dead nodes are never decremented, so deg cannot wrap.  Barrier.
// The nodes listed in one round are already out of `alive` when the rows are walked: adjacent nodes removed together do not
// decrement each other, and need not -- both have their coreness.  The loop ends when no node is alive; it is a `for` over at most
// 2 N rounds: at most N rounds remove a node, and every jump is followed by one that does.  Integer atomics commute: every output
// is the same from run to run.  The same launch then stores the coreness (16-bit for the caller, FP64 for k_node_fold), the rank
// #{u : core[u] > core[v]} (a whole shell shares a rank) and per (sample, layer) the degeneracy, the size of the main core,
// sum_v core(v) and #{v : core(v) >= k_min}.
// k_node_fold (node_fold.h) adds the chunk's samples in ascending s into the per-node accumulators of the call (core <= 4094 and
// S < 2^31: every sum is an integer below 2^53, exact in FP64); k_core_fold_counts adds the two counters of this unit: the
// samples in which the node is in the main core and those in which its coreness is >= k_min.
// Bytes per network: a row is read when the degrees are taken and once more when its node leaves -- 2 N W 8 from L2 for IN and
// OUT, 4 N W 8 for UNION and TOTAL: 1 MB at N = 2000 -- against L N^2 written by the draw and read by the pack.
#include "node_fold.h"

namespace {

#define CORE_TPB 256
#define CORE_FLY 4                             // rows whose words a lane group has in flight
#define CORE_KPT (VMR_CORE_NMAX / CORE_TPB)    // nodes a thread owns at most
#define CORE_NONE 0xffffffffu                  // the smallest deg of no node

// one LDS atomicSub per set bit of w, the bits of word ww (x < 64 W: inside deg whatever the pad bits hold)
__device__ __forceinline__ void core_drop(u64 w, int ww, unsigned* deg) {
  while (w) {
    atomicSub(&deg[ww * 64 + __ffsll((long long)w) - 1], 1u);
    w &= w - 1ull;
  }
}

// The rows of the n nodes this wave listed, every lane of the wave calls it: the alive neighbours of each lose what the mode says.
template <int MODE>
__device__ __forceinline__ void core_walk(const u64* __restrict__ Ao, const u64* __restrict__ Ai, int W, int lG, int n, const unsigned short* list,
                                          const u64* alive, unsigned* deg) {
  const int lane = threadIdx.x & 63;
  const int G = 1 << lG, nps = 64 >> lG, sub = lane >> lG, wl = lane & (G - 1);
  for (int t0 = 0; t0 < n; t0 += CORE_FLY * nps) {
    int row[CORE_FLY];
#pragma unroll
    for (int f = 0; f < CORE_FLY; ++f) {
      const int idx = t0 + f * nps + sub;
      row[f] = idx < n ? (int)list[idx] : -1;   // (< N)
    }
    for (int ww = wl; ww < W; ww += G) {   // (one trip when W is a power of two)
      u64 a[CORE_FLY], b[CORE_FLY];
#pragma unroll
      for (int f = 0; f < CORE_FLY; ++f) {
        a[f] = b[f] = 0ull;
        if (row[f] >= 0) {
          const size_t o = (size_t)row[f] * W + ww;
          if (MODE != VMR_CORE_OUT) a[f] = Ao[o];
          if (MODE != VMR_CORE_IN) b[f] = Ai[o];
        }
      }
      const u64 al = alive[ww];
#pragma unroll
      for (int f = 0; f < CORE_FLY; ++f) {
        if (MODE == VMR_CORE_UNION) {
          core_drop((a[f] | b[f]) & al, ww, deg);
        } else {   // (TOTAL: both walks)
          core_drop(a[f] & al, ww, deg);
          core_drop(b[f] & al, ww, deg);
        }
      }
    }
  }
}

// Grid (nsl), nsl = the chunk's (sample, layer) pairs.  values[nsl][N] the coreness; cval[nsl][N] the same as doubles, crank[nsl][N]
// = #{u : core[u] > core[v]} and summary[nsl][4] = (degeneracy, nodes that attain it, sum_v core(v), #{v : core(v) >= k_min})
// unless null.
template <int MODE>
__global__ __launch_bounds__(CORE_TPB) void k_core_peel(const u64* __restrict__ Aout, const u64* __restrict__ Ain, int N, int W, int lG, unsigned k_min,
                                                        unsigned short* __restrict__ values, double* __restrict__ cval, unsigned* __restrict__ crank,
                                                        unsigned* __restrict__ summary) {
  __shared__ unsigned deg[VMR_CORE_NMAX];
  __shared__ u64 alive[VMR_CORE_NMAX / 64];
  __shared__ unsigned short lists[CORE_TPB / 64][CORE_KPT * 64];
  __shared__ unsigned tally[2][8];   // per round parity: the waves' listed nodes, the waves' smallest kept deg
  __shared__ unsigned red[12];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const size_t sl = blockIdx.x;
  const u64* Ao = Aout + sl * N * W;
  const u64* Ai = Ain + sl * N * W;
  unsigned short* list = lists[wv];
  const int kpt = (N + CORE_TPB - 1) / CORE_TPB;   // (<= CORE_KPT: the host refuses a larger N)
  const u64 lt = (1ull << lane) - 1ull;
  {   // the degrees: nps rows per wave side by side, G lanes to a row
    const int G = 1 << lG, nps = 64 >> lG, sub = lane >> lG, wl = lane & (G - 1);
    for (int r0 = wv * nps; r0 < N; r0 += (CORE_TPB / 64) * nps) {   // (the same trips in every lane of the wave)
      const int r = r0 + sub;
      unsigned d = 0u;
      if (r < N)
        for (int ww = wl; ww < W; ww += G) {
          const size_t o = (size_t)r * W + ww;
          if (MODE == VMR_CORE_UNION) d += (unsigned)__popcll(Ao[o] | Ai[o]);
          if (MODE == VMR_CORE_TOTAL) d += (unsigned)(__popcll(Ao[o]) + __popcll(Ai[o]));
          if (MODE == VMR_CORE_IN) d += (unsigned)__popcll(Ai[o]);
          if (MODE == VMR_CORE_OUT) d += (unsigned)__popcll(Ao[o]);
        }
      for (int o = G >> 1; o > 0; o >>= 1) d += (unsigned)__shfl_xor((int)d, o, 64);   // (every lane of the wave is here)
      if (wl == 0 && r < N) deg[r] = d;
    }
    for (int w = tid; w < W; w += CORE_TPB) alive[w] = (w + 1) * 64 <= N ? ~0ull : (1ull << (N - w * 64)) - 1ull;   // (N - 64 w in [1, 63])
  }
  __syncthreads();
  unsigned k = 0u;
  int left = N;
  for (int r = 0; r < 2 * N && left > 0; ++r) {   // (at most N rounds remove a node, and a jump is followed by one that does)
    unsigned* tl = tally[r & 1];
    int n = 0;   // (the same in every lane of the wave)
    unsigned mn = CORE_NONE;
    for (int q = 0; q < kpt; ++q) {
      const int wi = q * (CORE_TPB / 64) + wv, v = wi * 64 + lane;   // (this wave's word, this thread's node of it)
      if (wi < W) {
        const bool al = (alive[wi] >> lane) & 1ull;   // (no pad bit is set: v < N)
        const unsigned d = al ? deg[v] : CORE_NONE;
        const bool in = al && d <= k;
        const u64 m = __ballot(in);
        if (in) {
          list[n + __popcll(m & lt)] = (unsigned short)v;
          deg[v] = k;   // its coreness
        } else {
          mn = min(mn, d);
        }
        n += __popcll(m);
        wave_sync();   // (every lane has read the word)
        if (lane == 0 && m) alive[wi] &= ~m;
      }
    }
    mn = wave_min_u(mn);
    if (lane == 0) { tl[wv] = (unsigned)n; tl[4 + wv] = mn; }
    __syncthreads();   // (the lists, `alive` and the tallies are complete; two rounds on, when tl is written again, every wave has read it)
    const int tot = (int)(tl[0] + tl[1] + tl[2] + tl[3]);
    if (tot == 0) {   // (the whole workgroup; left > 0: some node is alive and the minimum is a degree)
      k = min(min(tl[4], tl[5]), min(tl[6], tl[7]));
      continue;
    }
    left -= tot;
    if (left > 0) core_walk<MODE>(Ao, Ai, W, lG, n, list, alive, deg);
    __syncthreads();   // (the degrees the next select reads)
  }
  __syncthreads();   // deg[v] = core(v) for every v < N
  unsigned c[CORE_KPT];
  unsigned tmax = 0u, tsum = 0u, tat = 0u;
#pragma unroll
  for (int q = 0; q < CORE_KPT; ++q) {
    const int v = tid + q * CORE_TPB;
    c[q] = 0u;
    if (v < N) {
      c[q] = deg[v];
      values[sl * N + v] = (unsigned short)c[q];   // (<= 2 (N - 1) <= 4094)
      if (cval) cval[sl * N + v] = (double)c[q];
      tmax = max(tmax, c[q]);
      tsum += c[q];
      tat += c[q] >= k_min ? 1u : 0u;
    }
  }
  if (crank) {
    unsigned rk[CORE_KPT];
#pragma unroll
    for (int q = 0; q < CORE_KPT; ++q) rk[q] = 0u;
    for (int u = 0; u < N; ++u) {
      const unsigned cu = deg[u];   // (the same address in every lane)
#pragma unroll
      for (int q = 0; q < CORE_KPT; ++q) rk[q] += cu > c[q] ? 1u : 0u;
    }
#pragma unroll
    for (int q = 0; q < CORE_KPT; ++q) {
      const int v = tid + q * CORE_TPB;
      if (v < N) crank[sl * N + v] = rk[q];
    }
  }
  if (summary) {   // (the same in every thread)
    tmax = wave_max_u(tmax); tsum = wave_sum_u(tsum); tat = wave_sum_u(tat);
    if (lane == 0) { red[wv] = tmax; red[4 + wv] = tsum; red[8 + wv] = tat; }
    __syncthreads();
    const unsigned dgn = max(max(red[0], red[1]), max(red[2], red[3]));
    const unsigned sum = red[4] + red[5] + red[6] + red[7], at = red[8] + red[9] + red[10] + red[11];
    unsigned tm = 0u;
#pragma unroll
    for (int q = 0; q < CORE_KPT; ++q) tm += (tid + q * CORE_TPB < N && c[q] == dgn) ? 1u : 0u;
    tm = wave_sum_u(tm);
    __syncthreads();   // (red has been read)
    if (lane == 0) red[wv] = tm;
    __syncthreads();
    if (tid == 0) {
      unsigned* o = summary + sl * 4;
      o[0] = dgn; o[1] = red[0] + red[1] + red[2] + red[3]; o[2] = sum; o[3] = at;
    }
  }
}

// One thread per (l, v): the chunk's samples in ascending s into the two counters of this unit -- the samples in which the node
// attains its layer's degeneracy (summary[s][l][0]) and those in which its coreness is >= k_min.
__global__ __launch_bounds__(256) void k_core_fold_counts(const unsigned short* __restrict__ values, const unsigned* __restrict__ summary, int c, int L,
                                                          int N, unsigned k_min, unsigned* __restrict__ in_main, unsigned* __restrict__ atleast) {
  const size_t LN = (size_t)L * N;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= LN) return;
  const size_t l = e / N;
  unsigned a = in_main[e], b = atleast[e];
  for (int s = 0; s < c; ++s) {
    const unsigned v = values[(size_t)s * LN + e];
    a += v == summary[((size_t)s * L + l) * 4] ? 1u : 0u;
    b += v >= k_min ? 1u : 0u;
  }
  in_main[e] = a; atleast[e] = b;
}

// what both calls refuse of N, mode and k_min, or VMR_OK
int core_args(vmr_ctx* h, const char* fn, int mode, int k_min) {
  char msg[256];
  if (h->g.N > VMR_CORE_NMAX) {
    snprintf(msg, sizeof msg, "%s: the peel keeps every node's degree in LDS: N <= %d, the handle has N = %d", fn, VMR_CORE_NMAX, h->g.N);
    return fail(h, VMR_EINVAL, msg);
  }
  if (mode < VMR_CORE_UNION || mode > VMR_CORE_OUT) {
    snprintf(msg, sizeof msg, "%s: mode must be 0 (union), 1 (total), 2 (in) or 3 (out), got %d", fn, mode);
    return fail(h, VMR_EINVAL, msg);
  }
  if (k_min < 0 || k_min > 2 * (h->g.N - 1)) {
    snprintf(msg, sizeof msg, "%s: k_min must be in [0, 2 (N - 1) = %d], got %d", fn, 2 * (h->g.N - 1), k_min);
    return fail(h, VMR_EINVAL, msg);
  }
  return VMR_OK;
}

// the packed chunk of c samples (or networks) -> values[c][L][N], summary[c][L][4], and cval, crank unless null
int core_chunk(vmr_ctx* h, const BitRows& b, int c, int mode, int k_min, const u64* Ao, const u64* Ai, unsigned short* values, double* cval,
               unsigned* crank, unsigned* summary) {
  auto launch = [&](auto M) {
    hipLaunchKernelGGL(k_core_peel<decltype(M)::value>, dim3((unsigned)(c * h->g.L)), dim3(CORE_TPB), 0, h->stream, Ao, Ai, h->g.N, b.W, b.lG,
                       (unsigned)k_min, values, cval, crank, summary);
  };
  switch (mode) {
    case VMR_CORE_UNION: launch(std::integral_constant<int, VMR_CORE_UNION>{}); break;
    case VMR_CORE_TOTAL: launch(std::integral_constant<int, VMR_CORE_TOTAL>{}); break;
    case VMR_CORE_IN: launch(std::integral_constant<int, VMR_CORE_IN>{}); break;
    default: launch(std::integral_constant<int, VMR_CORE_OUT>{}); break;
  }
  HIPCHK(h, hipGetLastError());
  return VMR_OK;
}

}  // namespace

extern "C" int vmr_sample_cores(vmr_handle h, uint64_t seed, int n_samples, int n_trials, int mode, int k_min, int top_k, double* node_sum,
                                double* node_sumsq, uint64_t* node_rank_sum, uint32_t* node_top, uint32_t* node_main, uint32_t* node_atleast,
                                uint32_t* summary, uint16_t* values) {
  if (!h) return VMR_EINVAL;
  const char* fn = "vmr_sample_cores";
  int rc;
  if ((rc = sampled_counts(h, fn, n_samples, n_trials))) return rc;
  if ((rc = core_args(h, fn, mode, k_min))) return rc;
  if ((rc = node_fold_args(h, fn, top_k, node_sum))) return rc;
  if ((rc = expected_begin(h, fn))) return rc;
  const Geo& g = h->g;
  const BitRows b = bit_rows(g);
  const size_t LN = b.LN;
  // the summary is kept on the device whether or not it is asked for: k_core_fold_counts reads the degeneracy from it
  SampledOut out[2] = {{summary, (size_t)g.L * 16, false, "vmr_sample_cores: the summary", nullptr},
                       {values, LN * 2, false, "vmr_sample_cores: the values", nullptr}};
  uint32_t* no_summary = nullptr;
  uint16_t* no_values = nullptr;
  // device bytes per sample of a chunk: the bit-row chunk, the coreness as doubles and as 16-bit words, the ranks, the summary;
  // per call: the accumulators and this unit's two counters
  const size_t per = b.per() + LN * 14 + (size_t)g.L * 16;
  size_t C;
  if ((rc = chunk_samples(h, fn, (size_t)n_samples, per, NodeFold::bytes(LN) + LN * 8, &C))) return rc;
  Tmp tm(h);
  uint8_t* Y = nullptr;
  u64 *Ao = nullptr, *Ai = nullptr;
  double* cval = nullptr;
  unsigned *crank = nullptr, *amain = nullptr, *aleast = nullptr;
  NodeFold fold;
  if (!summary && (rc = tm.get(&no_summary, C * g.L * 16, "vmr_sample_cores: the summary"))) return rc;
  if (!values && (rc = tm.get(&no_values, C * LN * 2, "vmr_sample_cores: the values"))) return rc;
  if ((rc = bit_rows_get(tm, b, C, fn, "samples", &Y, &Ao, &Ai)) ||
      (rc = tm.get(&cval, C * LN * 8, "vmr_sample_cores: the values as doubles")) ||
      (rc = tm.get(&crank, C * LN * 4, "vmr_sample_cores: the ranks")) || (rc = fold.begin(h, tm, fn, LN, top_k)) ||
      (rc = tm.get(&amain, LN * 4, "vmr_sample_cores: the node main-core counts")) ||
      (rc = tm.get(&aleast, LN * 4, "vmr_sample_cores: the node k-core counts")))
    return rc;
  HIPCHK(h, hipMemsetAsync(amain, 0, LN * 4, h->stream));
  HIPCHK(h, hipMemsetAsync(aleast, 0, LN * 4, h->stream));
  rc = sampled_chunks(h, tm, (size_t)n_samples, C, seed, n_trials, Y, out, [&](size_t, int c) -> int {
    int rc2;
    unsigned* csum = summary ? out[0].as<unsigned>() : no_summary;
    unsigned short* cv = values ? out[1].as<unsigned short>() : no_values;
    if ((rc2 = tri_pack_chunk(h, Y, c, Ao, Ai))) return rc2;
    if ((rc2 = core_chunk(h, b, c, mode, k_min, Ao, Ai, cv, cval, crank, csum))) return rc2;
    if ((rc2 = fold.add(h, cval, crank, c))) return rc2;
    hipLaunchKernelGGL(k_core_fold_counts, dim3(grid_for(LN, 256, 0xffffffffu)), dim3(256), 0, h->stream, cv, csum, c, g.L, g.N, (unsigned)k_min,
                       amain, aleast);
    HIPCHK(h, hipGetLastError());
    return VMR_OK;
  });
  if (rc) return rc;
  if (node_main) HIPCHK(h, hipMemcpyAsync(node_main, amain, LN * 4, hipMemcpyDeviceToHost, h->stream));
  if (node_atleast) HIPCHK(h, hipMemcpyAsync(node_atleast, aleast, LN * 4, hipMemcpyDeviceToHost, h->stream));
  return fold.finish(h, node_sum, node_sumsq, node_rank_sum, node_top);
}

extern "C" int vmr_network_cores(vmr_handle h, const uint8_t* Y, int n, int mode, int k_min, uint16_t* values, uint32_t* summary) {
  if (!h) return VMR_EINVAL;
  const char* fn = "vmr_network_cores";
  int rc;
  if (n < 1) return fail(h, VMR_EINVAL, "vmr_network_cores: n must be positive");
  if ((rc = core_args(h, fn, mode, k_min))) return rc;
  if (!Y) return fail(h, VMR_EINVAL, "vmr_network_cores: Y is NULL");
  if (!values) return fail(h, VMR_EINVAL, "vmr_network_cores: values is NULL");
  HIPCHK(h, hipSetDevice(h->device));
  const Geo& g = h->g;
  const BitRows b = bit_rows(g);
  const size_t per = b.per() + b.LN * 2 + (size_t)g.L * 16;
  size_t C;
  if ((rc = chunk_samples(h, fn, (size_t)n, per, 0, &C, "network"))) return rc;
  Tmp tm(h);
  uint8_t* Yd = nullptr;
  u64 *Ao = nullptr, *Ai = nullptr;
  unsigned short* cv = nullptr;
  unsigned* csum = nullptr;
  if ((rc = bit_rows_get(tm, b, C, fn, "networks", &Yd, &Ao, &Ai)) || (rc = tm.get(&cv, C * b.LN * 2, "vmr_network_cores: the values")) ||
      (summary && (rc = tm.get(&csum, C * g.L * 16, "vmr_network_cores: the summary"))))
    return rc;
  return uploaded_chunks(h, b, (size_t)n, C, Y, Yd, Ao, Ai, [&](size_t s0, int c) -> int {
    int rc2;
    if ((rc2 = core_chunk(h, b, c, mode, k_min, Ao, Ai, cv, nullptr, nullptr, csum))) return rc2;
    HIPCHK(h, hipMemcpyAsync(values + s0 * b.LN, cv, (size_t)c * b.LN * 2, hipMemcpyDeviceToHost, h->stream));
    if (summary) HIPCHK(h, hipMemcpyAsync(summary + s0 * g.L * 4, csum, (size_t)c * g.L * 16, hipMemcpyDeviceToHost, h->stream));
    return VMR_OK;
  });
}
