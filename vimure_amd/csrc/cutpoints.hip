// cutpoints.hip -- who holds the posterior network together, on the device: vmr_sample_cutpoints, vmr_network_cutpoints.
//
// connectivity.hip reports that a sample is split; this unit says where it is fragile.  With A = (Y > 0), the diagonal cleared, G
// is the undirected graph A | A^T (UNION) or A & A^T (MUTUAL).  The branches of node v are the components of v's component once v
// is taken out, of sizes s_1..s_b: branches[v] = b (v is a cut point iff b >= 2), pairs_cut[v] = sum_{i<j} s_i s_j = ((sum s)^2 -
// sum s^2) / 2 the pairs of other nodes that lose every path, bridges[v] the branches that hold exactly one neighbour of v -- the
// tie to that neighbour is a bridge of G (include/vimure_hip.h has the contract).  Everything is an integer.
//
// vmr_sample_cutpoints draws S posterior samples of Y in chunks (sampled_side.h: sample s is what vmr_sample(h, seed + s, n_trials)
// writes) and packs them into bit rows (sampled_side.h has the layout); vmr_network_cutpoints uploads the caller's networks in
// chunks and packs them the same way.
// k_cut_graph: U = Aout | Ain or Aout & Ain, word by word, once per chunk: conn_expand only ORs, and forming U once spares the
// second gather of every expansion.  U is symmetric: bit q of word b of row u says that u is a neighbour of node 64 b + q.
// k_cut_block: one workgroup (4 waves) per (block b of 64 nodes, layer, sample): the layout of k_conn_closure, used for 64 removal
// experiments in place of 64 sources.  Node u carries a 64-bit word in LDS whose bit q belongs to the experiment "node 64 b + q
// has been removed".  seen, the frontier and the next frontier are 64 W words each (24 N bytes: N <= VMR_CUT_NMAX = 2048 is 48
// KiB), beside them three arrays of 64 integers (768 bytes): three workgroups to a CU.  Thread t owns nodes t, t + 256, .. and
// keeps word b of their rows in registers.  Removal costs nothing: the removed node starts with its own bit set in seen and is
// never put on a frontier, so no search passes through it.  The branches are found in rounds:
//   seed     every experiment that still has an unvisited neighbour of its removed node takes the lowest-numbered one: node u ANDs
//            word b of its row with ~seen[u], which lists every experiment for which u is such a neighbour, and one integer LDS
//            atomicMin per set bit picks the seed.  The round ends the loop when no experiment seeds;
//   close    conn_expand and the update step of connectivity.hip until a level adds nothing, for all 64 experiments at once;
//   count    new = seen[u] & ~(seen[u] before the round) are the experiments whose branch of this round holds u: per experiment the
//            branch size, and -- ANDed with word b of u's row -- how many neighbours of the removed node it holds.  A wave owns 64
//            consecutive nodes: where a lane has more than CUT_SPARSE bits the wave counts by two ballots per experiment, else
//            by one integer LDS atomicAdd per set bit (the late rounds: a few small branches);
//   tally    every experiment that seeded adds 1 to its branches, s to sum s, s^2 to sum s^2 and, with exactly one neighbour in
//            the branch, 1 to its bridges (the first 64 threads, in registers).
// At most max-degree-of-the-block's-nodes rounds.  Steps per block: one closure's worth of expansions in all where the graph is
// one component (every node is reached once per experiment) plus, per round, 5 barriers and the levels of the deepest branch.
// k_cut_finish: one workgroup per (layer, sample) ranks pairs_cut in LDS, rank[v] = #{u : pairs_cut[u] > pairs_cut[v]}, as
// k_core_peel ranks, and stores the summary: cut points, bridges = sum_v bridges[v] / 2, max_v pairs_cut, connected pairs =
// sum_v (sum_i s_i(v)) / 2.
// k_node_fold (node_fold.h) adds the chunk's samples in ascending s into the per-node accumulators of the call (pairs_cut <
// 2^21 and S < 2^31: every sum is an integer below 2^53, exact in FP64); k_cut_fold_counts adds the three counters of this unit.
// No floating point but that fold; integer adds, minima and ORs only: every output is the same from run to run and for any
// chunking.
// Bytes per network: the pre-pass reads 2 and writes 1 set of bit rows (24 N W); every block reads column word b of every row
// once (8 N, strided) and, per experiment-block, each row once per closure from L2 as connectivity.hip does: N W 8 per block, W
// blocks: 8 N W^2 = 8 MB at N = 2000, all of it L2 hits -- against L N^2 written by the draw and read by the pack.
#include "conn_expand.h"
#include "node_fold.h"

namespace {

#define CUT_KPT (VMR_CUT_NMAX / CONN_TPB)   // nodes a thread owns at most
#define CUT_SPARSE 4                        // bits of a lane's word up to which a wave counts by atomics
#define CUT_NONE 0x7fffffff                 // the seed of an experiment that has none

// Grid-stride: U[i] = A[i] | B[i], or A[i] & B[i] with `mutual`, n words.
__global__ __launch_bounds__(256) void k_cut_graph(const u64* __restrict__ A, const u64* __restrict__ B, size_t n, int mutual, u64* __restrict__ U) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) U[i] = mutual ? A[i] & B[i] : A[i] | B[i];
}

// Grid (W blocks of 64 nodes, L, samples of the chunk); dynamic LDS: 3 x 64 W words.  Stores for every node v of the block
// pairs_cut, branches, bridges and reach = sum_i s_i(v) = |C(v)| - 1, [nsl][N] each.
__global__ __launch_bounds__(CONN_TPB) void k_cut_block(const u64* __restrict__ Ug, int N, int L, int W, int lG, unsigned* __restrict__ pairs_cut,
                                                        unsigned short* __restrict__ branches, unsigned short* __restrict__ bridges,
                                                        unsigned short* __restrict__ reach) {
  extern __shared__ u64 cut_lds[];
  __shared__ int seedv[64];
  __shared__ unsigned cnt_s[64], cnt_n[64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int b = blockIdx.x, l = blockIdx.y, s = blockIdx.z;
  const size_t sl = (size_t)s * L + l;
  const u64* U = Ug + sl * N * W;
  u64 *seen = cut_lds, *fr = cut_lds + (size_t)W * 64, *nx = cut_lds + (size_t)W * 128;
  u64 nbw[CUT_KPT], before[CUT_KPT];
#pragma unroll
  for (int k = 0; k < CUT_KPT; ++k) {
    const int v = tid + k * CONN_TPB;
    nbw[k] = v < N ? U[(size_t)v * W + b] : 0ull;   // (the bits of the nodes at and above N are zero: such an experiment never seeds)
    before[k] = 0ull;
    if (v < W * 64) {
      seen[v] = (v >> 6) == b && v < N ? 1ull << (v & 63) : 0ull;
      fr[v] = 0ull; nx[v] = 0ull;
    }
  }
  unsigned br = 0u, ssum = 0u, ssq = 0u, bdg = 0u;   // of experiment tid, in the first 64 threads
  __syncthreads();
  for (int round = 0; round < N; ++round) {   // (a round that seeds visits a neighbour of every seeding experiment: fewer than N do)
    if (tid < 64) { seedv[tid] = CUT_NONE; cnt_s[tid] = 0u; cnt_n[tid] = 0u; }
#pragma unroll
    for (int k = 0; k < CUT_KPT; ++k) {
      const int v = tid + k * CONN_TPB;
      if (v < W * 64) before[k] = seen[v];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CUT_KPT; ++k) {
      u64 m = nbw[k] & ~before[k];   // (0 for v >= N)
      while (m) {
        atomicMin(&seedv[__ffsll((long long)m) - 1], tid + k * CONN_TPB);
        m &= m - 1ull;
      }
    }
    __syncthreads();
    bool act = false;
    if (tid < 64) {
      const int sv = seedv[tid];   // (< N)
      act = sv != CUT_NONE;
      if (act) {   // (several experiments may seed the same node)
        atomicOr(&fr[sv], 1ull << tid);
        atomicOr(&seen[sv], 1ull << tid);
      }
    }
    if (!__syncthreads_or(act)) break;
    for (;;) {   // the closure of connectivity.hip
      conn_expand<false>(U, U, N, W, lG, fr, nx);
      __syncthreads();
      bool any = false;
#pragma unroll
      for (int k = 0; k < CUT_KPT; ++k) {
        const int v = tid + k * CONN_TPB;
        if (v < W * 64) {
          const u64 nw = nx[v] & ~seen[v];
          if (nw) seen[v] |= nw;
          nx[v] = nw;
          fr[v] = 0ull;
          any |= nw != 0ull;
        }
      }
      { u64* t = fr; fr = nx; nx = t; }
      if (!__syncthreads_or(any)) break;
    }   // (both frontiers are zero again)
#pragma unroll
    for (int k = 0; k < CUT_KPT; ++k) {
      const int v = tid + k * CONN_TPB;
      if (k * CONN_TPB < W * 64) {   // (the same in every lane of the wave: W * 64 is a multiple of 64)
        const u64 d = v < W * 64 ? seen[v] & ~before[k] : 0ull;
        const u64 dn = d & nbw[k];
        const unsigned mx = wave_max_u((unsigned)__popcll(d));
        if (mx > CUT_SPARSE) {
          unsigned cs = 0u, cn = 0u;
          for (int q = 0; q < 64; ++q) {
            const u64 m1 = __ballot((d >> q) & 1ull), m2 = __ballot((dn >> q) & 1ull);
            if (lane == q) { cs = (unsigned)__popcll(m1); cn = (unsigned)__popcll(m2); }
          }
          if (cs) atomicAdd(&cnt_s[lane], cs);
          if (cn) atomicAdd(&cnt_n[lane], cn);
        } else if (mx) {
          u64 m = d;
          while (m) {
            const int q = __ffsll((long long)m) - 1;
            atomicAdd(&cnt_s[q], 1u);
            if ((dn >> q) & 1ull) atomicAdd(&cnt_n[q], 1u);
            m &= m - 1ull;
          }
        }
      }
    }
    __syncthreads();
    if (act) {   // (tid < 64; s >= 1: the seed itself, which is a neighbour)
      const unsigned sz = cnt_s[tid];
      br += 1u; ssum += sz; ssq += sz * sz;   // (sum s <= N - 1 <= 2047: the squares fit 32 bits)
      bdg += cnt_n[tid] == 1u ? 1u : 0u;
    }
  }
  const int r = b * 64 + tid;
  if (tid < 64 && r < N) {
    pairs_cut[sl * N + r] = (ssum * ssum - ssq) >> 1;
    branches[sl * N + r] = (unsigned short)br;
    bridges[sl * N + r] = (unsigned short)bdg;
    reach[sl * N + r] = (unsigned short)ssum;
  }
}

// Grid (nsl), nsl = the chunk's (sample, layer) pairs.  cval[nsl][N] pairs_cut as doubles, crank[nsl][N] = #{u : pairs_cut[u] >
// pairs_cut[v]} and summary[nsl][4] = (cut points, bridges, max_v pairs_cut, connected pairs) unless null.
__global__ __launch_bounds__(CONN_TPB) void k_cut_finish(const unsigned* __restrict__ pairs_cut, const unsigned short* __restrict__ branches,
                                                         const unsigned short* __restrict__ bridges, const unsigned short* __restrict__ reach, int N,
                                                         double* __restrict__ cval, unsigned* __restrict__ crank, unsigned* __restrict__ summary) {
  __shared__ unsigned pc[VMR_CUT_NMAX];
  __shared__ unsigned red[16];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const size_t sl = blockIdx.x;
  unsigned c[CUT_KPT];
  unsigned ncut = 0u, nbr = 0u, mx = 0u, rs = 0u;
#pragma unroll
  for (int q = 0; q < CUT_KPT; ++q) {
    const int v = tid + q * CONN_TPB;
    c[q] = 0u;
    if (v < N) {
      c[q] = pairs_cut[sl * N + v];
      pc[v] = c[q];
      if (cval) cval[sl * N + v] = (double)c[q];
      ncut += branches[sl * N + v] >= 2 ? 1u : 0u;
      nbr += bridges[sl * N + v];
      rs += reach[sl * N + v];
      mx = max(mx, c[q]);
    }
  }
  __syncthreads();
  if (crank) {
    unsigned rk[CUT_KPT];
#pragma unroll
    for (int q = 0; q < CUT_KPT; ++q) rk[q] = 0u;
    for (int u = 0; u < N; ++u) {
      const unsigned cu = pc[u];   // (the same address in every lane)
#pragma unroll
      for (int q = 0; q < CUT_KPT; ++q) rk[q] += cu > c[q] ? 1u : 0u;
    }
#pragma unroll
    for (int q = 0; q < CUT_KPT; ++q) {
      const int v = tid + q * CONN_TPB;
      if (v < N) crank[sl * N + v] = rk[q];
    }
  }
  if (summary) {
    ncut = wave_sum_u(ncut); nbr = wave_sum_u(nbr); rs = wave_sum_u(rs); mx = wave_max_u(mx);
    if (lane == 0) { red[wv] = ncut; red[4 + wv] = nbr; red[8 + wv] = mx; red[12 + wv] = rs; }
    __syncthreads();
    if (tid == 0) {
      unsigned* o = summary + sl * 4;
      o[0] = red[0] + red[1] + red[2] + red[3];
      o[1] = (red[4] + red[5] + red[6] + red[7]) >> 1;      // (every bridge is counted at both of its ends)
      o[2] = max(max(red[8], red[9]), max(red[10], red[11]));
      o[3] = (red[12] + red[13] + red[14] + red[15]) >> 1;  // (sum_v (|C(v)| - 1) = 2 sum_C C(|C|, 2) < 2^22)
    }
  }
}

// One thread per (l, v): the chunk's samples in ascending s into the three counters of this unit -- the samples in which the node
// is a cut point, and the sums of its branches and of its bridges.
__global__ __launch_bounds__(256) void k_cut_fold_counts(const unsigned short* __restrict__ branches, const unsigned short* __restrict__ bridges,
                                                         int c, size_t LN, unsigned* __restrict__ node_cut, u64* __restrict__ branch_sum,
                                                         u64* __restrict__ bridge_sum) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= LN) return;
  unsigned a = node_cut[e];
  u64 bs = branch_sum[e], gs = bridge_sum[e];
  for (int s = 0; s < c; ++s) {
    const unsigned br = branches[(size_t)s * LN + e];
    a += br >= 2u ? 1u : 0u;
    bs += br;
    gs += bridges[(size_t)s * LN + e];
  }
  node_cut[e] = a; branch_sum[e] = bs; bridge_sum[e] = gs;
}

// what both calls refuse of N and mode, or VMR_OK
int cut_args(vmr_ctx* h, const char* fn, int mode) {
  char msg[256];
  if (h->g.N > VMR_CUT_NMAX) {
    snprintf(msg, sizeof msg, "%s: the removal experiments keep 24 N bytes in LDS: N <= %d, the handle has N = %d", fn, VMR_CUT_NMAX, h->g.N);
    return fail(h, VMR_EINVAL, msg);
  }
  if (mode < VMR_CUT_UNION || mode > VMR_CUT_MUTUAL) {
    snprintf(msg, sizeof msg, "%s: mode must be 0 (union) or 1 (mutual), got %d", fn, mode);
    return fail(h, VMR_EINVAL, msg);
  }
  return VMR_OK;
}

// The device buffers of a chunk beside the bit rows: U and the four per-node arrays every chunk computes.
struct CutChunk {
  u64* U = nullptr;
  unsigned* pairs = nullptr;
  unsigned short *branches = nullptr, *bridges = nullptr, *reach = nullptr;
  static size_t per(const BitRows& b) { return b.bits_b + b.LN * 10; }   // device bytes per sample of a chunk
  int get(Tmp& tm, const BitRows& b, size_t C, const char* fn) {
    const std::string f = std::string(fn) + ": the ";
    int rc;
    if ((rc = tm.get(&U, C * b.bits_b, (f + "graph's bits").c_str())) || (rc = tm.get(&pairs, C * b.LN * 4, (f + "pairs cut").c_str())) ||
        (rc = tm.get(&branches, C * b.LN * 2, (f + "branches").c_str())) || (rc = tm.get(&bridges, C * b.LN * 2, (f + "bridges").c_str())) ||
        (rc = tm.get(&reach, C * b.LN * 2, (f + "component sizes").c_str())))
      return rc;
    return VMR_OK;
  }
};

// the packed chunk of c samples (or networks) -> pairs, branches, bridges [c][L][N], and cval, crank, summary[c][L][4] unless null
int cut_chunk(vmr_ctx* h, const BitRows& b, int c, int mode, const u64* Ao, const u64* Ai, const CutChunk& k, double* cval, unsigned* crank,
              unsigned* summary) {
  const Geo& g = h->g;
  const size_t words = (size_t)c * b.LN * b.W;
  hipLaunchKernelGGL(k_cut_graph, dim3(grid_for(words, 256, 16384)), dim3(256), 0, h->stream, Ao, Ai, words, mode == VMR_CUT_MUTUAL ? 1 : 0, k.U);
  HIPCHK(h, hipGetLastError());
  const size_t smem = (size_t)b.W * 64 * 3 * 8;
  hipLaunchKernelGGL(k_cut_block, dim3((unsigned)b.W, (unsigned)g.L, (unsigned)c), dim3(CONN_TPB), smem, h->stream, k.U, g.N, g.L, b.W, b.lG, k.pairs,
                     k.branches, k.bridges, k.reach);
  HIPCHK(h, hipGetLastError());
  if (cval || crank || summary) {
    hipLaunchKernelGGL(k_cut_finish, dim3((unsigned)(c * g.L)), dim3(CONN_TPB), 0, h->stream, k.pairs, k.branches, k.bridges, k.reach, g.N, cval, crank,
                       summary);
    HIPCHK(h, hipGetLastError());
  }
  return VMR_OK;
}

}  // namespace

extern "C" int vmr_sample_cutpoints(vmr_handle h, uint64_t seed, int n_samples, int n_trials, int mode, int top_k, double* node_sum,
                                    double* node_sumsq, uint64_t* node_rank_sum, uint32_t* node_top, uint32_t* node_cut, uint64_t* node_branch_sum,
                                    uint64_t* node_bridge_sum, uint32_t* summary, uint32_t* pairs_cut, uint16_t* branches, uint16_t* bridges) {
  if (!h) return VMR_EINVAL;
  const char* fn = "vmr_sample_cutpoints";
  int rc;
  if ((rc = sampled_counts(h, fn, n_samples, n_trials))) return rc;
  if ((rc = cut_args(h, fn, mode))) return rc;
  if ((rc = node_fold_args(h, fn, top_k, node_sum))) return rc;
  if ((rc = expected_begin(h, fn))) return rc;
  const Geo& g = h->g;
  const BitRows b = bit_rows(g);
  const size_t LN = b.LN;
  SampledOut out[1] = {{summary, (size_t)g.L * 16, false, "vmr_sample_cutpoints: the summary", nullptr}};
  // device bytes per sample of a chunk: the bit-row chunk, U and the four node arrays, pairs_cut as doubles, the ranks, the
  // summary; per call: the accumulators and this unit's three counters
  const size_t per = b.per() + CutChunk::per(b) + LN * 12 + (size_t)g.L * 16;
  size_t C;
  if ((rc = chunk_samples(h, fn, (size_t)n_samples, per, NodeFold::bytes(LN) + LN * 20, &C))) return rc;
  Tmp tm(h);
  uint8_t* Y = nullptr;
  u64 *Ao = nullptr, *Ai = nullptr, *abr = nullptr, *abg = nullptr;
  double* cval = nullptr;
  unsigned *crank = nullptr, *acut = nullptr;
  CutChunk k;
  NodeFold fold;
  if ((rc = bit_rows_get(tm, b, C, fn, "samples", &Y, &Ao, &Ai)) || (rc = k.get(tm, b, C, fn)) ||
      (rc = tm.get(&cval, C * LN * 8, "vmr_sample_cutpoints: the values as doubles")) ||
      (rc = tm.get(&crank, C * LN * 4, "vmr_sample_cutpoints: the ranks")) || (rc = fold.begin(h, tm, fn, LN, top_k)) ||
      (rc = tm.get(&acut, LN * 4, "vmr_sample_cutpoints: the node cut-point counts")) ||
      (rc = tm.get(&abr, LN * 8, "vmr_sample_cutpoints: the node branch sums")) ||
      (rc = tm.get(&abg, LN * 8, "vmr_sample_cutpoints: the node bridge sums")))
    return rc;
  HIPCHK(h, hipMemsetAsync(acut, 0, LN * 4, h->stream));
  HIPCHK(h, hipMemsetAsync(abr, 0, LN * 8, h->stream));
  HIPCHK(h, hipMemsetAsync(abg, 0, LN * 8, h->stream));
  rc = sampled_chunks(h, tm, (size_t)n_samples, C, seed, n_trials, Y, out, [&](size_t s0, int c) -> int {
    int rc2;
    if ((rc2 = tri_pack_chunk(h, Y, c, Ao, Ai))) return rc2;
    if ((rc2 = cut_chunk(h, b, c, mode, Ao, Ai, k, cval, crank, out[0].as<unsigned>()))) return rc2;
    if ((rc2 = fold.add(h, cval, crank, c))) return rc2;
    hipLaunchKernelGGL(k_cut_fold_counts, dim3(grid_for(LN, 256, 0xffffffffu)), dim3(256), 0, h->stream, k.branches, k.bridges, c, LN, acut, abr, abg);
    HIPCHK(h, hipGetLastError());
    if (pairs_cut) HIPCHK(h, hipMemcpyAsync(pairs_cut + s0 * LN, k.pairs, (size_t)c * LN * 4, hipMemcpyDeviceToHost, h->stream));
    if (branches) HIPCHK(h, hipMemcpyAsync(branches + s0 * LN, k.branches, (size_t)c * LN * 2, hipMemcpyDeviceToHost, h->stream));
    if (bridges) HIPCHK(h, hipMemcpyAsync(bridges + s0 * LN, k.bridges, (size_t)c * LN * 2, hipMemcpyDeviceToHost, h->stream));
    return VMR_OK;
  });
  if (rc) return rc;
  if (node_cut) HIPCHK(h, hipMemcpyAsync(node_cut, acut, LN * 4, hipMemcpyDeviceToHost, h->stream));
  if (node_branch_sum) HIPCHK(h, hipMemcpyAsync(node_branch_sum, abr, LN * 8, hipMemcpyDeviceToHost, h->stream));
  if (node_bridge_sum) HIPCHK(h, hipMemcpyAsync(node_bridge_sum, abg, LN * 8, hipMemcpyDeviceToHost, h->stream));
  return fold.finish(h, node_sum, node_sumsq, node_rank_sum, node_top);
}

extern "C" int vmr_network_cutpoints(vmr_handle h, const uint8_t* Y, int n, int mode, uint32_t* pairs_cut, uint16_t* branches, uint16_t* bridges,
                                     uint32_t* summary) {
  if (!h) return VMR_EINVAL;
  const char* fn = "vmr_network_cutpoints";
  int rc;
  if (n < 1) return fail(h, VMR_EINVAL, "vmr_network_cutpoints: n must be positive");
  if ((rc = cut_args(h, fn, mode))) return rc;
  if (!Y) return fail(h, VMR_EINVAL, "vmr_network_cutpoints: Y is NULL");
  if (!pairs_cut) return fail(h, VMR_EINVAL, "vmr_network_cutpoints: pairs_cut is NULL");
  HIPCHK(h, hipSetDevice(h->device));
  const Geo& g = h->g;
  const BitRows b = bit_rows(g);
  const size_t per = b.per() + CutChunk::per(b) + (size_t)g.L * 16;
  size_t C;
  if ((rc = chunk_samples(h, fn, (size_t)n, per, 0, &C, "network"))) return rc;
  Tmp tm(h);
  uint8_t* Yd = nullptr;
  u64 *Ao = nullptr, *Ai = nullptr;
  unsigned* csum = nullptr;
  CutChunk k;
  if ((rc = bit_rows_get(tm, b, C, fn, "networks", &Yd, &Ao, &Ai)) || (rc = k.get(tm, b, C, fn)) ||
      (summary && (rc = tm.get(&csum, C * g.L * 16, "vmr_network_cutpoints: the summary"))))
    return rc;
  return uploaded_chunks(h, b, (size_t)n, C, Y, Yd, Ao, Ai, [&](size_t s0, int c) -> int {
    int rc2;
    if ((rc2 = cut_chunk(h, b, c, mode, Ao, Ai, k, nullptr, nullptr, csum))) return rc2;
    HIPCHK(h, hipMemcpyAsync(pairs_cut + s0 * b.LN, k.pairs, (size_t)c * b.LN * 4, hipMemcpyDeviceToHost, h->stream));
    if (branches) HIPCHK(h, hipMemcpyAsync(branches + s0 * b.LN, k.branches, (size_t)c * b.LN * 2, hipMemcpyDeviceToHost, h->stream));
    if (bridges) HIPCHK(h, hipMemcpyAsync(bridges + s0 * b.LN, k.bridges, (size_t)c * b.LN * 2, hipMemcpyDeviceToHost, h->stream));
    if (summary) HIPCHK(h, hipMemcpyAsync(summary + s0 * g.L * 4, csum, (size_t)c * g.L * 16, hipMemcpyDeviceToHost, h->stream));
    return VMR_OK;
  });
}
