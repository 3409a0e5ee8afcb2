// holes.hip -- Burt's structural holes of the posterior on the device: vmr_sample_structural_holes, vmr_network_structural_holes.
//
// The other node read-outs say who is central, who lies on shortest paths and who sits in the dense core; this one says whose own
// contacts are disconnected from one another.  include/vimure_hip.h has the contract: with A = (Y > 0), the diagonal cleared, U =
// A | A^T and Mu = A & A^T, z_ij = U_ij (VMR_SH_UNION) or U_ij + Mu_ij (VMR_SH_WEIGHTED), d_i = sum_j U_ij, s_i = sum_j z_ij,
//   R_i  = sum_{j in U_i} f_j sum_q z_iq z_jq, f_j = 1 where j has a mutual tie in weighted mode (s_j > d_j), else 2   (an integer)
//   ES_i = d_i - R_i / (2 s_i), evaluated as (2 s_i d_i - R_i) / (2 s_i): one division of two exact integers
//   c_i  = sum_{j in U_i} ((z_ij + sum_{q in U_i & U_j} z_iq z_qj / s_q) / s_i)^2
// and 0.0 for both where d_i = 0.
//
// k_sh_strength: G lanes per (node, layer, sample) popcount the row's words of U (and of Mu): deg and str, 32-bit.
// k_sh_node: one wave per (node i, layer, sample), the neighbour-list walk of k_sp_count (partners.hip) in its ordered form: the
// neighbours j of i in U are listed a block of SH_BLK words of row i at a time and walked 64 / G neighbours per step, G lanes
// striding the W words of row j, row i's words in registers when W <= G.  Per word u = U_i & U_j: the integer sum_q z_iq z_jq is one
// popcount (four in weighted mode: U.U, Mu_i.U_j, U_i.Mu_j, Mu_i.Mu_j), the FP64 sum walks the set bits of u in ascending order and
// adds w_q / s_q, w_q = (1 + Mu_i bit)(1 + Mu_j bit) in {1, 2, 4}.  Both are summed over the group by a fixed xor tree; the group's
// first lane forms the local constraint, its square and f_j times the count, and keeps them in registers; the wave sums them by a
// fixed xor tree and lane 0 stores the node's values.  No atomics: a node is owned by one wave, and the order of every sum depends
// on N only (through G): every output is bit-identical from run to run and for any chunking.  No contraction in this file: the
// square and the divisions are rounded as written.  LDS: the four waves' lists, 4 x 2048 x 2 = 16,384 bytes.
// k_sh_rank: grid (ceil(N / 256), layers, samples), a thread per node.  The (sample, layer)'s values stream through LDS in tiles of
// 256 nodes -- an undefined node enters as (-inf, +inf), which no comparison counts -- and every thread counts the defined u with
// ES_u > ES_v and those with c_u < c_v; an undefined v gets #defined.  Thread t loads nodes t, t + 256, .. of the tiles, in
// ascending order: its partial sums are those of the summary (#defined, sum ES, sum c), which workgroup x = 0 reduces with
// block_sum_n and stores.  LDS: 2 x 256 x 8 for the tile, 16 x 8 for block_sum_n, 4 x 4 for the count: 4,240 bytes whatever N.
// k_node_fold (node_fold.h), once per measure, adds the chunk's samples in ascending s; k_sh_fold_defined adds the samples in
// which the node is not isolated.
// Bytes per network: row j is read once per tie (i, j) of U, 2 ties x 2 W 8 from L2, against L N^2 written by the draw and read
// by the pack; the ranks are N^2 comparisons out of LDS.
#include "node_fold.h"

#pragma clang fp contract(off)

namespace {

#define SH_BLK 32       // words of row i whose neighbours are listed at a time
#define SH_LIST (SH_BLK * 64)
#define SH_TILE 256     // nodes of a tile of k_sh_rank: its workgroup

// word w of U and of Mu (0 in union mode, where it is not read) of the row (ao, ai)
template <int MODE>
__device__ __forceinline__ void sh_words(const u64* __restrict__ ao, const u64* __restrict__ ai, int w, u64& u, u64& m) {
  const u64 o = ao[w], n = ai[w];
  u = o | n;
  m = MODE == VMR_SH_WEIGHTED ? (o & n) : 0ull;
}

// word ww of the rows i (ui, mi) and j: cnt += sum_q z_iq z_jq, acc += sum_q z_iq z_jq / s_q over the bits q of the word
template <int MODE>
__device__ __forceinline__ void sh_pair(u64 ui, u64 mi, const u64* __restrict__ ao_j, const u64* __restrict__ ai_j, int ww, const int* __restrict__ st,
                                        unsigned& cnt, double& acc) {
  u64 uj, mj;
  sh_words<MODE>(ao_j, ai_j, ww, uj, mj);
  u64 u = ui & uj;
  cnt += (unsigned)__popcll(u);
  if (MODE == VMR_SH_WEIGHTED) cnt += (unsigned)(__popcll(mi & uj) + __popcll(ui & mj) + __popcll(mi & mj));   // (Mu is inside U)
  while (u) {
    const int bit = __ffsll((long long)u) - 1;
    double t = 1.0 / (double)st[ww * 64 + bit];   // (q < N: the pad bits are zero; s_q >= 1: q has a tie)
    if (MODE == VMR_SH_WEIGHTED) t *= (double)((1 + (int)((mi >> bit) & 1ull)) * (1 + (int)((mj >> bit) & 1ull)));   // (by 1, 2 or 4: exact)
    acc += t;
    u &= u - 1ull;
  }
}

// G = 1 << lG lanes per (node i, layer = blockIdx.y, sample = blockIdx.z), 256 >> lG nodes per workgroup.  deg, str [c][L][N].
__global__ __launch_bounds__(256) void k_sh_strength(const u64* __restrict__ Aout, const u64* __restrict__ Ain, int N, int L, int W, int lG, int weighted,
                                                     int* __restrict__ deg, int* __restrict__ str) {
  const int G = 1 << lG, wl = threadIdx.x & (G - 1);
  const int i = blockIdx.x * (256 >> lG) + (threadIdx.x >> lG);
  const size_t sl = (size_t)blockIdx.z * L + blockIdx.y;
  unsigned d = 0u, m = 0u;
  if (i < N) {
    const u64* ao = Aout + (sl * N + i) * W;
    const u64* ai = Ain + (sl * N + i) * W;
    for (int ww = wl; ww < W; ww += G) {
      const u64 o = ao[ww], n = ai[ww];
      d += (unsigned)__popcll(o | n);
      if (weighted) m += (unsigned)__popcll(o & n);
    }
  }
  d = group_sum_u(d, G);   // (every lane of the wave is here)
  m = group_sum_u(m, G);
  if (i < N && wl == 0) {
    deg[sl * N + i] = (int)d;
    str[sl * N + i] = (int)(d + m);
  }
}

// One wave per (node i = 4 blockIdx.x + wave, layer, sample); G = 1 << lG lanes per neighbour, 64 / G neighbours per step.
// es, con [c][L][N]; red [c][L][N] or null.
template <int MODE>
__global__ __launch_bounds__(256) void k_sh_node(const u64* __restrict__ Aout, const u64* __restrict__ Ain, const int* __restrict__ deg,
                                                 const int* __restrict__ str, int N, int L, int W, int lG, u64* __restrict__ red,
                                                 double* __restrict__ es, double* __restrict__ con) {
  __shared__ unsigned short list_s[4][SH_LIST];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wv, l = blockIdx.y, s = blockIdx.z;
  if (i >= N) return;   // (the same in every lane of the wave; the workgroup has no barrier)
  const size_t sl = (size_t)s * L + l;
  const int G = 1 << lG, nps = 64 >> lG, sub = lane >> lG, wl = lane & (G - 1);
  unsigned short* list = list_s[wv];
  const u64* Ao = Aout + sl * N * W;
  const u64* Ai = Ain + sl * N * W;
  const u64* ao_i = Ao + (size_t)i * W;
  const u64* ai_i = Ai + (size_t)i * W;
  const int* dg = deg + sl * N;
  const int* st = str + sl * N;
  const int d_i = dg[i], s_i = st[i];
  if (d_i == 0) {   // an isolate: undefined
    if (lane == 0) {
      es[sl * N + i] = 0.0;
      con[sl * N + i] = 0.0;
      if (red) red[sl * N + i] = 0ull;
    }
    return;
  }
  const double si = (double)s_i;
  const bool one = W <= G;   // (W a power of two up to 64) a lane meets one word of a row only: row i's stays in registers
  u64 ui1 = 0ull, mi1 = 0ull;
  if (one && wl < W) sh_words<MODE>(ao_i, ai_i, wl, ui1, mi1);
  double r_con = 0.0;   // of the neighbours whose group this lane leads
  u64 r_red = 0ull;
  for (int wb = 0; wb < W; wb += SH_BLK) {
    const int w = wb + lane;
    u64 u = 0ull;
    if (lane < SH_BLK && w < W) u = ao_i[w] | ai_i[w];
    const unsigned c = (unsigned)__popcll(u);
    unsigned inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
    const int n = __builtin_amdgcn_readfirstlane((int)__shfl(inc, 63, 64));   // neighbours in this block of words, <= SH_LIST
    unsigned off = inc - c;
    wave_sync();   // (the walk of the last block is done with the list)
    while (u) {
      const int bit = __ffsll((long long)u) - 1;
      list[off++] = (unsigned short)(lane * 64 + bit);
      u &= u - 1ull;
    }
    wave_sync();
    for (int t = 0; t < n; t += nps) {
      const int idx = t + sub;
      const bool live = idx < n;
      const int j = live ? wb * 64 + (int)list[idx] : 0;   // < N: the pad bits are zero
      unsigned cnt = 0u;
      double acc = 0.0;
      if (live) {
        const u64* ao_j = Ao + (size_t)j * W;
        const u64* ai_j = Ai + (size_t)j * W;
        if (one) {
          if (wl < W) sh_pair<MODE>(ui1, mi1, ao_j, ai_j, wl, st, cnt, acc);
        } else {
          for (int ww = wl; ww < W; ww += G) {
            u64 ui, mi;
            sh_words<MODE>(ao_i, ai_i, ww, ui, mi);
            sh_pair<MODE>(ui, mi, ao_j, ai_j, ww, st, cnt, acc);
          }
        }
      }
      cnt = group_sum_u(cnt, G);   // (every lane of the wave is here)
      acc = group_sum(acc, G);
      if (live && wl == 0) {
        int zij = 1, fj = 2;
        if (MODE == VMR_SH_WEIGHTED) {
          zij += (int)(((ao_i[j >> 6] & ai_i[j >> 6]) >> (j & 63)) & 1ull);
          if (st[j] > dg[j]) fj = 1;   // j has a mutual tie: its largest weight is 2
        }
        const double local = ((double)zij + acc) / si;
        const double sq = local * local;
        r_con += sq;
        r_red += (u64)fj * cnt;
      }
    }
  }
  r_con = wave_sum(r_con);
  r_red = wave_sum_ull(r_red);
  if (lane == 0) {
    const u64 den = 2ull * (u64)s_i;
    es[sl * N + i] = (double)(den * (u64)d_i - r_red) / (double)den;   // (R <= 2 s (d - 1): the numerator is positive, below 2^53)
    con[sl * N + i] = r_con;
    if (red) red[sl * N + i] = r_red;
  }
}

// Grid (ceil(N / SH_TILE), L, c), a thread per node v.  rank_es, rank_con [c][L][N] or null (both or neither); summary [c][L][3]
// or null.
__global__ __launch_bounds__(SH_TILE) void k_sh_rank(const int* __restrict__ deg, const double* __restrict__ es, const double* __restrict__ con, int N,
                                                     int L, unsigned* __restrict__ rank_es, unsigned* __restrict__ rank_con,
                                                     double* __restrict__ summary) {
  __shared__ double es_t[SH_TILE], con_t[SH_TILE];
  __shared__ double redd[16];
  __shared__ unsigned redu[4];
  const int tid = threadIdx.x;
  const size_t sl = (size_t)blockIdx.z * L + blockIdx.y;
  const int* dg = deg + sl * N;
  const double* e = es + sl * N;
  const double* cn = con + sl * N;
  const int v = blockIdx.x * SH_TILE + tid;
  const bool mine = v < N, def = mine && dg[v] > 0;
  const double ev = def ? e[v] : 0.0, cv = def ? cn[v] : 0.0;
  unsigned re = 0u, rc = 0u, nd = 0u;
  double a_es = 0.0, a_con = 0.0;
  for (int u0 = 0; u0 < N; u0 += SH_TILE) {
    const int u = u0 + tid;
    double eu = -INFINITY, cu = INFINITY;   // what no comparison counts
    if (u < N && dg[u] > 0) {
      eu = e[u]; cu = cn[u];
      nd += 1u; a_es += eu; a_con += cu;
    }
    __syncthreads();   // (the last tile's reads are done)
    es_t[tid] = eu; con_t[tid] = cu;
    __syncthreads();
    if (def) {
#pragma unroll 8
      for (int q = 0; q < SH_TILE; ++q) {   // (the same address in every lane)
        re += es_t[q] > ev ? 1u : 0u;
        rc += con_t[q] < cv ? 1u : 0u;
      }
    }
  }
  nd = wave_sum_u(nd);
  if ((tid & 63) == 0) redu[tid >> 6] = nd;
  __syncthreads();
  nd = redu[0] + redu[1] + redu[2] + redu[3];
  if (mine && rank_es) {
    rank_es[sl * N + v] = def ? re : nd;
    rank_con[sl * N + v] = def ? rc : nd;
  }
  if (summary && blockIdx.x == 0) {   // (the same in every thread)
    const double t_es = block_sum_n(a_es, redd);
    const double t_con = block_sum_n(a_con, redd);
    if (tid == 0) {
      double* o = summary + sl * VMR_SH_NSUMMARY;
      o[0] = (double)nd; o[1] = t_es; o[2] = t_con;
    }
  }
}

// One thread per (l, v): the samples of the chunk in which the node has a tie, added to the call's counter.
__global__ __launch_bounds__(256) void k_sh_fold_defined(const int* __restrict__ deg, int c, size_t LN, unsigned* __restrict__ defined) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= LN) return;
  unsigned a = defined[e];
  for (int s = 0; s < c; ++s) a += deg[(size_t)s * LN + e] > 0 ? 1u : 0u;
  defined[e] = a;
}

struct ShOut {   // the device buffers of one chunk: red, the ranks and summary may be null
  int *deg, *str;
  u64* red;
  double *es, *con;
  unsigned *rank_es, *rank_con;
  double* summary;
};

// the packed chunk of c samples (or networks) -> deg, str, es, con [c][L][N] and what else of o is not null
int sh_chunk(vmr_ctx* h, const BitRows& b, int c, int mode, const u64* Ao, const u64* Ai, const ShOut& o) {
  const Geo& g = h->g;
  const int npb = 256 >> b.lG;   // nodes per workgroup of k_sh_strength
  hipLaunchKernelGGL(k_sh_strength, dim3((unsigned)((g.N + npb - 1) / npb), (unsigned)g.L, (unsigned)c), dim3(256), 0, h->stream, Ao, Ai, g.N, g.L, b.W,
                     b.lG, mode == VMR_SH_WEIGHTED ? 1 : 0, o.deg, o.str);
  const dim3 grid((unsigned)((g.N + 3) / 4), (unsigned)g.L, (unsigned)c);
  if (mode == VMR_SH_WEIGHTED)
    hipLaunchKernelGGL(k_sh_node<VMR_SH_WEIGHTED>, grid, dim3(256), 0, h->stream, Ao, Ai, o.deg, o.str, g.N, g.L, b.W, b.lG, o.red, o.es, o.con);
  else
    hipLaunchKernelGGL(k_sh_node<VMR_SH_UNION>, grid, dim3(256), 0, h->stream, Ao, Ai, o.deg, o.str, g.N, g.L, b.W, b.lG, o.red, o.es, o.con);
  if (o.rank_es || o.summary)
    hipLaunchKernelGGL(k_sh_rank, dim3((unsigned)((g.N + SH_TILE - 1) / SH_TILE), (unsigned)g.L, (unsigned)c), dim3(SH_TILE), 0, h->stream, o.deg, o.es,
                       o.con, g.N, g.L, o.rank_es, o.rank_con, o.summary);
  HIPCHK(h, hipGetLastError());
  return VMR_OK;
}

// what both calls refuse of mode, or VMR_OK
int sh_args(vmr_ctx* h, const char* fn, int mode) {
  if (mode < VMR_SH_UNION || mode > VMR_SH_WEIGHTED) {
    char msg[256];
    snprintf(msg, sizeof msg, "%s: mode must be 0 (union) or 1 (weighted), got %d", fn, mode);
    return fail(h, VMR_EINVAL, msg);
  }
  return VMR_OK;
}

}  // namespace

extern "C" int vmr_sample_structural_holes(vmr_handle h, uint64_t seed, int n_samples, int n_trials, int mode, int top_k, double* node_sum,
                                           double* node_sumsq, uint64_t* node_rank_sum, uint32_t* node_top, uint32_t* node_defined, double* summary,
                                           int32_t* degree, int32_t* strength, uint64_t* redundancy, double* effective_size, double* constraint) {
  if (!h) return VMR_EINVAL;
  const char* fn = "vmr_sample_structural_holes";
  int rc;
  if ((rc = sampled_counts(h, fn, n_samples, n_trials))) return rc;
  if ((rc = sh_args(h, fn, mode))) return rc;
  if ((rc = node_fold_args(h, fn, top_k, node_sum))) return rc;
  if ((rc = expected_begin(h, fn))) return rc;
  const Geo& g = h->g;
  const BitRows b = bit_rows(g);
  const size_t LN = b.LN;
  SampledOut out[6] = {{summary, (size_t)g.L * VMR_SH_NSUMMARY * 8, false, "vmr_sample_structural_holes: the summary", nullptr},
                       {degree, LN * 4, false, "vmr_sample_structural_holes: the degrees", nullptr},
                       {strength, LN * 4, false, "vmr_sample_structural_holes: the strengths", nullptr},
                       {redundancy, LN * 8, false, "vmr_sample_structural_holes: the redundancy numerators", nullptr},
                       {effective_size, LN * 8, false, "vmr_sample_structural_holes: the effective sizes", nullptr},
                       {constraint, LN * 8, false, "vmr_sample_structural_holes: the constraints", nullptr}};
  // device bytes per sample of a chunk: the bit-row chunk, the degrees and strengths, the redundancy numerators, the two measures,
  // their ranks and the summary, whichever outputs are asked for; per call: two sets of accumulators and this unit's counter
  const size_t per = b.per() + LN * (4 + 4 + 8 + 8 + 8 + 4 + 4) + (size_t)g.L * VMR_SH_NSUMMARY * 8;
  size_t C;
  if ((rc = chunk_samples(h, fn, (size_t)n_samples, per, 2 * NodeFold::bytes(LN) + LN * 4, &C))) return rc;
  Tmp tm(h);
  uint8_t* Y = nullptr;
  u64 *Ao = nullptr, *Ai = nullptr;
  int *no_deg = nullptr, *no_str = nullptr;
  double *no_es = nullptr, *no_con = nullptr;
  unsigned *rank_es = nullptr, *rank_con = nullptr, *adef = nullptr;
  NodeFold fold_es, fold_con;
  // the kernels read the degrees, the strengths and the two measures whether or not they are asked for
  if (!degree && (rc = tm.get(&no_deg, C * LN * 4, "vmr_sample_structural_holes: the degrees"))) return rc;
  if (!strength && (rc = tm.get(&no_str, C * LN * 4, "vmr_sample_structural_holes: the strengths"))) return rc;
  if (!effective_size && (rc = tm.get(&no_es, C * LN * 8, "vmr_sample_structural_holes: the effective sizes"))) return rc;
  if (!constraint && (rc = tm.get(&no_con, C * LN * 8, "vmr_sample_structural_holes: the constraints"))) return rc;
  if ((rc = bit_rows_get(tm, b, C, fn, "samples", &Y, &Ao, &Ai)) ||
      (rc = tm.get(&rank_es, C * LN * 4, "vmr_sample_structural_holes: the ranks by effective size")) ||
      (rc = tm.get(&rank_con, C * LN * 4, "vmr_sample_structural_holes: the ranks by constraint")) || (rc = fold_es.begin(h, tm, fn, LN, top_k)) ||
      (rc = fold_con.begin(h, tm, fn, LN, top_k)) || (rc = tm.get(&adef, LN * 4, "vmr_sample_structural_holes: the node defined counts")))
    return rc;
  HIPCHK(h, hipMemsetAsync(adef, 0, LN * 4, h->stream));
  rc = sampled_chunks(h, tm, (size_t)n_samples, C, seed, n_trials, Y, out, [&](size_t, int c) -> int {
    int rc2;
    const ShOut o = {degree ? out[1].as<int>() : no_deg, strength ? out[2].as<int>() : no_str, out[3].as<u64>(),
                     effective_size ? out[4].as<double>() : no_es, constraint ? out[5].as<double>() : no_con, rank_es, rank_con,
                     out[0].as<double>()};
    if ((rc2 = tri_pack_chunk(h, Y, c, Ao, Ai))) return rc2;
    if ((rc2 = sh_chunk(h, b, c, mode, Ao, Ai, o))) return rc2;
    if ((rc2 = fold_es.add(h, o.es, rank_es, c)) || (rc2 = fold_con.add(h, o.con, rank_con, c))) return rc2;
    hipLaunchKernelGGL(k_sh_fold_defined, dim3(grid_for(LN, 256, 0xffffffffu)), dim3(256), 0, h->stream, o.deg, c, LN, adef);
    HIPCHK(h, hipGetLastError());
    return VMR_OK;
  });
  if (rc) return rc;
  if (node_defined) HIPCHK(h, hipMemcpyAsync(node_defined, adef, LN * 4, hipMemcpyDeviceToHost, h->stream));
  if ((rc = fold_es.finish(h, node_sum, node_sumsq, node_rank_sum, node_top))) return rc;
  return fold_con.finish(h, node_sum + LN, node_sumsq ? node_sumsq + LN : nullptr, node_rank_sum ? node_rank_sum + LN : nullptr,
                         node_top ? node_top + LN : nullptr);
}

extern "C" int vmr_network_structural_holes(vmr_handle h, const uint8_t* Y, int n, int mode, double* effective_size, double* constraint,
                                            int32_t* degree, int32_t* strength, uint64_t* redundancy, double* summary) {
  if (!h) return VMR_EINVAL;
  const char* fn = "vmr_network_structural_holes";
  int rc;
  if (n < 1) return fail(h, VMR_EINVAL, "vmr_network_structural_holes: n must be positive");
  if ((rc = sh_args(h, fn, mode))) return rc;
  if (!Y) return fail(h, VMR_EINVAL, "vmr_network_structural_holes: Y is NULL");
  if (!effective_size) return fail(h, VMR_EINVAL, "vmr_network_structural_holes: effective_size is NULL");
  if (!constraint) return fail(h, VMR_EINVAL, "vmr_network_structural_holes: constraint is NULL");
  HIPCHK(h, hipSetDevice(h->device));
  const Geo& g = h->g;
  const BitRows b = bit_rows(g);
  const size_t LN = b.LN, sb = (size_t)g.L * VMR_SH_NSUMMARY * 8;
  const size_t per = b.per() + LN * (4 + 4 + 8 + 8) + (redundancy ? LN * 8 : 0) + (summary ? sb : 0);
  size_t C;
  if ((rc = chunk_samples(h, fn, (size_t)n, per, 0, &C, "network"))) return rc;
  Tmp tm(h);
  uint8_t* Yd = nullptr;
  u64 *Ao = nullptr, *Ai = nullptr;
  ShOut o = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if ((rc = bit_rows_get(tm, b, C, fn, "networks", &Yd, &Ao, &Ai)) || (rc = tm.get(&o.deg, C * LN * 4, "vmr_network_structural_holes: the degrees")) ||
      (rc = tm.get(&o.str, C * LN * 4, "vmr_network_structural_holes: the strengths")) ||
      (rc = tm.get(&o.es, C * LN * 8, "vmr_network_structural_holes: the effective sizes")) ||
      (rc = tm.get(&o.con, C * LN * 8, "vmr_network_structural_holes: the constraints")) ||
      (redundancy && (rc = tm.get(&o.red, C * LN * 8, "vmr_network_structural_holes: the redundancy numerators"))) ||
      (summary && (rc = tm.get(&o.summary, C * sb, "vmr_network_structural_holes: the summary"))))
    return rc;
  return uploaded_chunks(h, b, (size_t)n, C, Y, Yd, Ao, Ai, [&](size_t s0, int c) -> int {
    int rc2;
    if ((rc2 = sh_chunk(h, b, c, mode, Ao, Ai, o))) return rc2;
    HIPCHK(h, hipMemcpyAsync(effective_size + s0 * LN, o.es, (size_t)c * LN * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(constraint + s0 * LN, o.con, (size_t)c * LN * 8, hipMemcpyDeviceToHost, h->stream));
    if (degree) HIPCHK(h, hipMemcpyAsync(degree + s0 * LN, o.deg, (size_t)c * LN * 4, hipMemcpyDeviceToHost, h->stream));
    if (strength) HIPCHK(h, hipMemcpyAsync(strength + s0 * LN, o.str, (size_t)c * LN * 4, hipMemcpyDeviceToHost, h->stream));
    if (redundancy) HIPCHK(h, hipMemcpyAsync(redundancy + s0 * LN, o.red, (size_t)c * LN * 8, hipMemcpyDeviceToHost, h->stream));
    if (summary) HIPCHK(h, hipMemcpyAsync(summary + s0 * g.L * VMR_SH_NSUMMARY, o.summary, (size_t)c * sb, hipMemcpyDeviceToHost, h->stream));
    return VMR_OK;
  });
}
