// cascades.hip -- cascades on the posterior on the device: vmr_sample_outreach, vmr_sample_seed_outreach, vmr_network_outreach,
// vmr_network_seed_outreach.
//
// If information enters the network at a node, or at a set of nodes, and every tie passes it on with probability q_l, how many
// nodes has it reached after T periods -- the independent-cascade model in its live-edge form on posterior samples of Y.
// vmr_sample_centrality counts walks (a node heard twice counts twice), vmr_sample_connectivity is the case q = 1, T = infinity;
// this is the cascade itself.  include/vimure_hip.h has the model: the live ties of cascade k of network s are a pure function
// of (cascade_seed + s, k, the tie's index), one Philox4x32-10 call per tie, and everything after the one comparison u < q_l is
// an integer.
//
// The sampled calls draw S posterior samples of Y in chunks (sampled_side.h: sample s is what vmr_sample(h, seed + s, n_trials)
// writes) and pack them into bit rows (sampled_side.h has the layout); the network calls upload the caller's networks in chunks
// and pack them the same way.  Per chunk and cascade k, two launches:
// k_casc_thin: a thread per 64-bit word of the ONE row set the closure walks (Aout, Ain, or their OR for UNION); every set bit
//   costs one Philox call, and the bit stays when u < q_l.  The draw is indexed by the tie, not by the row set: bit u of row v of
//   Ain is tie (l, u, v), and under UNION the pair {i, j} draws at (l, min, max), so its rows come out symmetric.  Work is
//   proportional to the ties; the live rows are one row set per sample, N ceil(N / 64) 8 bytes per layer, written once and
//   read by the closure from L2.
// k_casc_nodes: every node as a seed.  One workgroup (4 waves) per (block b of 64 sources, layer, sample) runs the breadth-first
//   search of connectivity.hip from the block's 64 sources at once (seen, frontier, next frontier: 24 N bytes of LDS, conn_expand
//   for a level) over the live rows of the direction OPPOSITE to the spread, for at most T levels: bit q of seen[v] then says
//   that v reaches source 64 b + q within T periods, and popc(seen[v]) - [v in block b] is v's own outreach towards the block's
//   nodes.  One integer atomicAdd per node at the end of the closure, into values[s][l][v], which sums over the blocks and, launch
//   after launch, over the cascades.
// k_casc_sets: up to 64 seed sets.  One workgroup per (layer, sample), initial words = seed_words (bit b of word v: v is in set
//   b), walking ALONG the spread.  The update of a period counts the new bits per set into an LDS table of 64 counters (integer
//   atomics); thread b adds counter b to the set's total and to the curve's bin min(t, 64) - 1 (a 64-bit integer atomic), and
//   node_hits takes the bits of the final seen words.
// The cascades are launched one after the other rather than looped over inside a workgroup or spread over the grid: the thinning
// scratch is then ONE live row set per sample of the chunk (8 L N ceil(N / 64) bytes, 0.5 MB per sample at N = 2048, L = 1) whatever
// n_cascades is, and a launch already holds ceil(N / 64) L c workgroups.
// k_casc_finish: one workgroup per (sample, layer): c = values / n_cascades (one FP64 division), the ranks #{u : values[u] >
//   values[v]} -- c is monotone in values and distinct values give distinct c, so the integers are compared -- and the summary.
// k_node_fold (node_fold.h) adds the chunk's samples in ascending s into the per-node accumulators of the call.
// All sums are sums of integers: the same from run to run in any order, and for any chunking.
#include "conn_expand.h"
#include "node_fold.h"

namespace {

#define CASC_KPT (VMR_CASC_NMAX / CONN_TPB)   // nodes a thread owns at most

// which tie a bit of the walked row set is: bit u of row r is tie (r, u) of Aout, (u, r) of Ain, (min, max) of their OR
enum { CASC_ROWS_OUT = 0, CASC_ROWS_IN = 1, CASC_ROWS_UNION = 2 };

// One thread per word e of the chunk's row set, [c][L][N][W] (grid-stride).  live is zero on the chunk's first cascade and only
// the words with ties are ever written.  live[e] = the bits of A[e] (| B[e] with
// CASC_ROWS_UNION) whose tie is live in cascade k: u < q_l with u from words 0 and 1 of Philox4x32-10, key = key0 + s (s the
// sample of the chunk; key0 = cascade_seed + the chunk's first sample, mod 2^64), counter = (t low, t high, k, 1).
__global__ __launch_bounds__(256) void k_casc_thin(const u64* __restrict__ A, const u64* __restrict__ B, int rows, int N, int L, int W, size_t nwords,
                                                   u64 key0, unsigned k, const double* __restrict__ qv, u64* __restrict__ live) {
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < nwords; e += (size_t)gridDim.x * 256) {
    u64 w = A[e];
    if (rows == CASC_ROWS_UNION) w |= B[e];
    if (w) {   // (a word without ties stays the zero the chunk's memset wrote: the pass reads the rows and writes little)
      u64 keep = 0ull;
      const int ww = (int)(e % (size_t)W);
      const size_t rr = e / (size_t)W;
      const int r = (int)(rr % (size_t)N);
      const size_t sl = rr / (size_t)N;
      const int l = (int)(sl % (size_t)L);
      const u64 key = key0 + (u64)(sl / (size_t)L);
      const double q = qv[l];
      do {
        const int bit = __ffsll((long long)w) - 1;
        const int col = ww * 64 + bit;   // (< N: the pad bits of a row are zero)
        int i = r, j = col;
        if (rows == CASC_ROWS_IN || (rows == CASC_ROWS_UNION && col < r)) { i = col; j = r; }
        const u64 t = ((u64)l * (u64)N + (u64)i) * (u64)N + (u64)j;
        unsigned c[4] = {(unsigned)t, (unsigned)(t >> 32), k, 1u};
        philox4x32_10(c, (unsigned)key, (unsigned)(key >> 32));
        const double u = ((double)(c[0] >> 5) * 67108864.0 + (double)(c[1] >> 6)) * (1.0 / 9007199254740992.0);
        if (u < q) keep |= 1ull << bit;
        w &= w - 1ull;
      } while (w);
      live[e] = keep;
    }
  }
}

// Grid (W source blocks, L, samples of the chunk); dynamic LDS: 3 x 64 W words.  rows: the chunk's live rows of the direction
// opposite to the spread.  values[s][l][v] += the nodes of block b that v reaches within T periods, v itself not counted.
__global__ __launch_bounds__(CONN_TPB) void k_casc_nodes(const u64* __restrict__ rows, int N, int L, int W, int lG, int T, unsigned* __restrict__ values) {
  extern __shared__ u64 casc_lds[];
  const int tid = threadIdx.x;
  const int b = blockIdx.x, l = blockIdx.y, s = blockIdx.z;
  const size_t sl = (size_t)s * L + l;
  const u64* R = rows + sl * N * W;
  u64 *seen = casc_lds, *fr = casc_lds + (size_t)W * 64, *nx = casc_lds + (size_t)W * 128;
  for (int v = tid; v < W * 64; v += CONN_TPB) {
    const u64 bit = (v >> 6) == b && v < N ? 1ull << (v & 63) : 0ull;
    seen[v] = bit; fr[v] = bit; nx[v] = 0ull;
  }
  __syncthreads();
  for (int d = 1; d <= T; ++d) {
    conn_expand<false>(R, R, N, W, lG, fr, nx);
    __syncthreads();
    int any = 0;
    for (int v = tid; v < W * 64; v += CONN_TPB) {   // (thread t owns nodes t, t + 256, ..)
      const u64 nw = nx[v] & ~seen[v];
      if (nw) { seen[v] |= nw; any = 1; }
      nx[v] = nw;
      fr[v] = 0ull;
    }
    { u64* t = fr; fr = nx; nx = t; }
    if (!__syncthreads_or(any)) break;   // (a period that reaches nobody new ends the cascade)
  }
  for (int v = tid; v < N; v += CONN_TPB) {   // (the words this thread wrote)
    const unsigned c = (unsigned)__popcll(seen[v]) - ((v >> 6) == b ? 1u : 0u);
    if (c) atomicAdd(values + sl * N + v, c);
  }
}

// Grid (L, samples of the chunk); dynamic LDS: 3 x 64 W words.  rows: the chunk's live rows along the spread; seeds[N]: bit q of
// word v says that v is in set q (no bit at or above n_sets).  values[s][l][q] += the outreach of set q; curve[l][q][.] (the
// call's, 64-bit) and hits[l][q][v] (the call's) unless null.
__global__ __launch_bounds__(CONN_TPB) void k_casc_sets(const u64* __restrict__ rows, const u64* __restrict__ seeds, int N, int L, int W, int lG, int T,
                                                        int n_sets, unsigned* __restrict__ values, u64* __restrict__ curve,
                                                        unsigned* __restrict__ hits) {
  extern __shared__ u64 casc_lds[];
  __shared__ unsigned cnt_s[VMR_CASC_SETS];
  const int tid = threadIdx.x;
  const int l = blockIdx.x, s = blockIdx.y;
  const size_t sl = (size_t)s * L + l;
  const u64* R = rows + sl * N * W;
  u64 *seen = casc_lds, *fr = casc_lds + (size_t)W * 64, *nx = casc_lds + (size_t)W * 128;
  for (int v = tid; v < W * 64; v += CONN_TPB) {
    const u64 w = v < N ? seeds[v] : 0ull;
    seen[v] = w; fr[v] = w; nx[v] = 0ull;
  }
  if (tid < VMR_CASC_SETS) cnt_s[tid] = 0u;
  __syncthreads();
  unsigned tot = 0u;   // thread q < n_sets: the outreach of set q
  for (int d = 1; d <= T; ++d) {
    conn_expand<false>(R, R, N, W, lG, fr, nx);
    __syncthreads();
    int any = 0;
    for (int v = tid; v < W * 64; v += CONN_TPB) {
      u64 nw = nx[v] & ~seen[v];
      if (nw) { seen[v] |= nw; any = 1; }
      nx[v] = nw;
      fr[v] = 0ull;
      while (nw) {   // (bits below n_sets only: a word is an OR of seed words)
        atomicAdd(&cnt_s[__ffsll((long long)nw) - 1], 1u);
        nw &= nw - 1ull;
      }
    }
    { u64* t = fr; fr = nx; nx = t; }
    const int more = __syncthreads_or(any);   // (the period's counters are complete; they are next added to after the next barrier)
    if (tid < n_sets) {
      const unsigned c = cnt_s[tid];
      if (c) {
        cnt_s[tid] = 0u;
        tot += c;
        if (curve) atomicAdd(curve + ((size_t)l * n_sets + tid) * VMR_CASC_NPER + (d < VMR_CASC_NPER ? d : VMR_CASC_NPER) - 1, (u64)c);
      }
    }
    if (!more) break;
  }
  if (tid < n_sets && tot) atomicAdd(values + sl * n_sets + tid, tot);
  if (hits)
    for (int v = tid; v < N; v += CONN_TPB) {   // (the words this thread wrote)
      u64 w = seen[v];
      while (w) {
        atomicAdd(hits + ((size_t)l * n_sets + (__ffsll((long long)w) - 1)) * N + v, 1u);
        w &= w - 1ull;
      }
    }
}

// Grid (nsl), nsl = the chunk's (sample, layer) pairs.  values[nsl][N] -> cval[nsl][N] = values / kc, crank[nsl][N] = #{u :
// values[u] > values[v]} and summary[nsl][2] = (sum_v values mod 2^32, max_v values), each unless null.
__global__ __launch_bounds__(CONN_TPB) void k_casc_finish(const unsigned* __restrict__ values, int N, double kc, double* __restrict__ cval,
                                                          unsigned* __restrict__ crank, unsigned* __restrict__ summary) {
  __shared__ unsigned val[VMR_CASC_NMAX];
  __shared__ unsigned red[8];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const size_t sl = blockIdx.x;
  for (int v = tid; v < N; v += CONN_TPB) val[v] = values[sl * N + v];
  __syncthreads();
  unsigned c[CASC_KPT];
  unsigned tsum = 0u, tmax = 0u;
#pragma unroll
  for (int q = 0; q < CASC_KPT; ++q) {
    const int v = tid + q * CONN_TPB;
    c[q] = 0u;
    if (v < N) {
      c[q] = val[v];
      if (cval) cval[sl * N + v] = (double)c[q] / kc;
      tsum += c[q];
      tmax = max(tmax, c[q]);
    }
  }
  if (crank) {
    unsigned rk[CASC_KPT];
#pragma unroll
    for (int q = 0; q < CASC_KPT; ++q) rk[q] = 0u;
    for (int u = 0; u < N; ++u) {
      const unsigned cu = val[u];   // (the same address in every lane)
#pragma unroll
      for (int q = 0; q < CASC_KPT; ++q) rk[q] += cu > c[q] ? 1u : 0u;
    }
#pragma unroll
    for (int q = 0; q < CASC_KPT; ++q) {
      const int v = tid + q * CONN_TPB;
      if (v < N) crank[sl * N + v] = rk[q];
    }
  }
  if (summary) {   // (the same in every thread)
    tsum = wave_sum_u(tsum); tmax = wave_max_u(tmax);
    if (lane == 0) { red[wv] = tsum; red[4 + wv] = tmax; }
    __syncthreads();
    if (tid == 0) {
      summary[sl * 2] = red[0] + red[1] + red[2] + red[3];
      summary[sl * 2 + 1] = max(max(red[4], red[5]), max(red[6], red[7]));
    }
  }
}

// what the four calls refuse of N, direction, T, n_cascades and q, or VMR_OK
int casc_args(vmr_ctx* h, const char* fn, int n_cascades, const double* q, int T, int direction) {
  char msg[256];
  if (h->g.N > VMR_CASC_NMAX) {
    snprintf(msg, sizeof msg, "%s: the closure keeps 24 N bytes in LDS: N <= %d, the handle has N = %d", fn, VMR_CASC_NMAX, h->g.N);
    return fail(h, VMR_EINVAL, msg);
  }
  if (direction < VMR_CASC_OUT || direction > VMR_CASC_UNION) {
    snprintf(msg, sizeof msg, "%s: direction must be 0 (out), 1 (in) or 2 (union), got %d", fn, direction);
    return fail(h, VMR_EINVAL, msg);
  }
  if (T < 1 || T > VMR_CASC_TMAX) {
    snprintf(msg, sizeof msg, "%s: T must be in [1, %d], got %d", fn, VMR_CASC_TMAX, T);
    return fail(h, VMR_EINVAL, msg);
  }
  if (n_cascades < 1 || n_cascades > VMR_CASC_KMAX) {
    snprintf(msg, sizeof msg, "%s: n_cascades must be in [1, %d], got %d", fn, VMR_CASC_KMAX, n_cascades);
    return fail(h, VMR_EINVAL, msg);
  }
  if (!q) return fail(h, VMR_EINVAL, (std::string(fn) + ": q is NULL").c_str());
  for (int l = 0; l < h->g.L; ++l)
    if (!(q[l] >= 0.0 && q[l] <= 1.0)) {   // (a NaN fails both)
      snprintf(msg, sizeof msg, "%s: q[%d] must be finite and in [0, 1], got %g", fn, l, q[l]);
      return fail(h, VMR_EINVAL, msg);
    }
  return VMR_OK;
}

// what the two seed-set calls refuse of seed_words, n_sets and values, or VMR_OK
int casc_set_args(vmr_ctx* h, const char* fn, const uint64_t* seed_words, int n_sets, const void* values) {
  char msg[256];
  if (n_sets < 1 || n_sets > VMR_CASC_SETS) {
    snprintf(msg, sizeof msg, "%s: n_sets must be in [1, %d], got %d", fn, VMR_CASC_SETS, n_sets);
    return fail(h, VMR_EINVAL, msg);
  }
  if (!seed_words) return fail(h, VMR_EINVAL, (std::string(fn) + ": seed_words is NULL").c_str());
  if (n_sets < 64)
    for (int v = 0; v < h->g.N; ++v)
      if (seed_words[v] >> n_sets) {
        snprintf(msg, sizeof msg, "%s: seed_words[%d] has a bit at or above n_sets = %d", fn, v, n_sets);
        return fail(h, VMR_EINVAL, msg);
      }
  if (!values) return fail(h, VMR_EINVAL, (std::string(fn) + ": values is NULL").c_str());
  return VMR_OK;
}

// The cascades of a packed chunk of c samples (or networks), the first of which has key key0.  sets == false: every node as a
// seed, vals[c][L][N] (zeroed here); else the seed sets, vals[c][L][n_sets] (zeroed here), curve and hits the call's or null.
struct CascRun {
  int n_cascades, T, direction;
  const double* qd;
  u64* live;
  bool sets;
  const u64* seeds;
  int n_sets;
  u64* curve;
  unsigned* hits;
};
int casc_chunk(vmr_ctx* h, const BitRows& b, int c, u64 key0, const CascRun& r, const u64* Ao, const u64* Ai, unsigned* vals) {
  const Geo& g = h->g;
  // the row set the closure walks: along the spread for the sets, against it for the nodes
  int rows = CASC_ROWS_UNION;
  if (r.direction != VMR_CASC_UNION) rows = (r.direction == VMR_CASC_OUT) == r.sets ? CASC_ROWS_OUT : CASC_ROWS_IN;
  const u64* A = rows == CASC_ROWS_IN ? Ai : Ao;
  const size_t nwords = (size_t)c * b.LN * b.W;
  const size_t smem = (size_t)b.W * 64 * 3 * 8;
  HIPCHK(h, hipMemsetAsync(vals, 0, (size_t)c * g.L * (r.sets ? (size_t)r.n_sets : (size_t)g.N) * 4, h->stream));
  HIPCHK(h, hipMemsetAsync(r.live, 0, nwords * 8, h->stream));
  for (int k = 0; k < r.n_cascades; ++k) {
    hipLaunchKernelGGL(k_casc_thin, dim3(grid_for(nwords, 256, 65536)), dim3(256), 0, h->stream, A, Ai, rows, g.N, g.L, b.W, nwords, key0, (unsigned)k,
                       r.qd, r.live);
    if (r.sets)
      hipLaunchKernelGGL(k_casc_sets, dim3((unsigned)g.L, (unsigned)c), dim3(CONN_TPB), smem, h->stream, r.live, r.seeds, g.N, g.L, b.W, b.lG, r.T,
                         r.n_sets, vals, r.curve, r.hits);
    else
      hipLaunchKernelGGL(k_casc_nodes, dim3((unsigned)b.W, (unsigned)g.L, (unsigned)c), dim3(CONN_TPB), smem, h->stream, r.live, g.N, g.L, b.W, b.lG,
                         r.T, vals);
    HIPCHK(h, hipGetLastError());
  }
  return VMR_OK;
}

// q, and for the seed-set calls the seed words, the curve and the hits (zeroed), on the device, from tm
int casc_upload(vmr_ctx* h, Tmp& tm, const std::string& fn, const double* q, const uint64_t* seed_words, int n_sets, bool want_curve, bool want_hits,
                CascRun& r, double** qd) {
  const Geo& g = h->g;
  int rc;
  if ((rc = tm.get(qd, (size_t)g.L * 8, (fn + ": q").c_str()))) return rc;
  HIPCHK(h, hipMemcpyAsync(*qd, q, (size_t)g.L * 8, hipMemcpyHostToDevice, h->stream));
  r.qd = *qd;
  r.sets = seed_words != nullptr;
  r.seeds = nullptr; r.n_sets = n_sets; r.curve = nullptr; r.hits = nullptr;
  if (!r.sets) return VMR_OK;
  u64* sd = nullptr;
  if ((rc = tm.get(&sd, (size_t)g.N * 8, (fn + ": the seed words").c_str()))) return rc;
  HIPCHK(h, hipMemcpyAsync(sd, seed_words, (size_t)g.N * 8, hipMemcpyHostToDevice, h->stream));
  r.seeds = sd;
  if (want_curve) {
    const size_t nb = (size_t)g.L * n_sets * VMR_CASC_NPER * 8;
    if ((rc = tm.get(&r.curve, nb, (fn + ": the curve").c_str()))) return rc;
    HIPCHK(h, hipMemsetAsync(r.curve, 0, nb, h->stream));
  }
  if (want_hits) {
    const size_t nb = (size_t)g.L * n_sets * g.N * 4;
    if ((rc = tm.get(&r.hits, nb, (fn + ": the node hits").c_str()))) return rc;
    HIPCHK(h, hipMemsetAsync(r.hits, 0, nb, h->stream));
  }
  return VMR_OK;
}

// device bytes per call of the seed-set calls beside the chunk: the seed words, q, the curve and the hits
size_t casc_set_fixed(const Geo& g, int n_sets, bool want_curve, bool want_hits) {
  return (size_t)g.N * 8 + (size_t)g.L * 8 + (want_curve ? (size_t)g.L * n_sets * VMR_CASC_NPER * 8 : 0) +
         (want_hits ? (size_t)g.L * n_sets * g.N * 4 : 0);
}

// the curve and the hits of a seed-set call to the host, then waits for the stream
int casc_set_finish(vmr_ctx* h, const CascRun& r, uint64_t* curve, uint32_t* node_hits) {
  const Geo& g = h->g;
  if (curve) HIPCHK(h, hipMemcpyAsync(curve, r.curve, (size_t)g.L * r.n_sets * VMR_CASC_NPER * 8, hipMemcpyDeviceToHost, h->stream));
  if (node_hits) HIPCHK(h, hipMemcpyAsync(node_hits, r.hits, (size_t)g.L * r.n_sets * g.N * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return VMR_OK;
}

}  // namespace

extern "C" int vmr_sample_outreach(vmr_handle h, uint64_t seed, int n_samples, int n_trials, uint64_t cascade_seed, int n_cascades, const double* q,
                                   int T, int direction, int top_k, double* node_sum, double* node_sumsq, uint64_t* node_rank_sum,
                                   uint32_t* node_top, uint32_t* summary, uint32_t* values) {
  if (!h) return VMR_EINVAL;
  const char* fn = "vmr_sample_outreach";
  int rc;
  if ((rc = sampled_counts(h, fn, n_samples, n_trials))) return rc;
  if ((rc = casc_args(h, fn, n_cascades, q, T, direction))) return rc;
  if ((rc = node_fold_args(h, fn, top_k, node_sum))) return rc;
  if ((rc = expected_begin(h, fn))) return rc;
  const Geo& g = h->g;
  const BitRows b = bit_rows(g);
  const size_t LN = b.LN;
  SampledOut out[1] = {{summary, (size_t)g.L * 8, false, "vmr_sample_outreach: the summary", nullptr}};
  // device bytes per sample of a chunk: the bit-row chunk, the live rows, the values, c and the ranks, the summary; per call: the
  // accumulators and q
  const size_t per = b.per() + b.bits_b + LN * 16 + (size_t)g.L * 8;
  size_t C;
  if ((rc = chunk_samples(h, fn, (size_t)n_samples, per, NodeFold::bytes(LN) + (size_t)g.L * 8, &C))) return rc;
  Tmp tm(h);
  uint8_t* Y = nullptr;
  u64 *Ao = nullptr, *Ai = nullptr;
  double *cval = nullptr, *qd = nullptr;
  unsigned *crank = nullptr, *vals = nullptr;
  CascRun r{n_cascades, T, direction, nullptr, nullptr, false, nullptr, 0, nullptr, nullptr};
  NodeFold fold;
  if ((rc = bit_rows_get(tm, b, C, fn, "samples", &Y, &Ao, &Ai)) ||
      (rc = tm.get(&r.live, C * b.bits_b, "vmr_sample_outreach: the live rows")) ||
      (rc = tm.get(&vals, C * LN * 4, "vmr_sample_outreach: the values")) ||
      (rc = tm.get(&cval, C * LN * 8, "vmr_sample_outreach: the values as doubles")) ||
      (rc = tm.get(&crank, C * LN * 4, "vmr_sample_outreach: the ranks")) ||
      (rc = casc_upload(h, tm, fn, q, nullptr, 0, false, false, r, &qd)) || (rc = fold.begin(h, tm, fn, LN, top_k)))
    return rc;
  rc = sampled_chunks(h, tm, (size_t)n_samples, C, seed, n_trials, Y, out, [&](size_t s0, int c) -> int {
    int rc2;
    if ((rc2 = tri_pack_chunk(h, Y, c, Ao, Ai))) return rc2;
    if ((rc2 = casc_chunk(h, b, c, cascade_seed + (u64)s0, r, Ao, Ai, vals))) return rc2;   // (mod 2^64)
    hipLaunchKernelGGL(k_casc_finish, dim3((unsigned)(c * g.L)), dim3(CONN_TPB), 0, h->stream, vals, g.N, (double)n_cascades, cval, crank,
                       out[0].as<unsigned>());
    HIPCHK(h, hipGetLastError());
    if ((rc2 = fold.add(h, cval, crank, c))) return rc2;
    if (values) HIPCHK(h, hipMemcpyAsync(values + s0 * LN, vals, (size_t)c * LN * 4, hipMemcpyDeviceToHost, h->stream));
    return VMR_OK;
  });
  return rc ? rc : fold.finish(h, node_sum, node_sumsq, node_rank_sum, node_top);
}

extern "C" int vmr_sample_seed_outreach(vmr_handle h, uint64_t seed, int n_samples, int n_trials, uint64_t cascade_seed, int n_cascades,
                                        const double* q, int T, int direction, const uint64_t* seed_words, int n_sets, uint32_t* values,
                                        uint64_t* curve, uint32_t* node_hits) {
  if (!h) return VMR_EINVAL;
  const char* fn = "vmr_sample_seed_outreach";
  int rc;
  if ((rc = sampled_counts(h, fn, n_samples, n_trials))) return rc;
  if ((rc = casc_args(h, fn, n_cascades, q, T, direction))) return rc;
  if ((rc = casc_set_args(h, fn, seed_words, n_sets, values))) return rc;
  if ((rc = expected_begin(h, fn))) return rc;
  const Geo& g = h->g;
  const BitRows b = bit_rows(g);
  SampledOut out[1] = {{values, (size_t)g.L * n_sets * 4, false, "vmr_sample_seed_outreach: the values", nullptr}};
  // device bytes per sample of a chunk: the bit-row chunk, the live rows, the values
  const size_t per = b.per() + b.bits_b + out[0].bytes;
  size_t C;
  if ((rc = chunk_samples(h, fn, (size_t)n_samples, per, casc_set_fixed(g, n_sets, curve, node_hits), &C))) return rc;
  Tmp tm(h);
  uint8_t* Y = nullptr;
  u64 *Ao = nullptr, *Ai = nullptr;
  double* qd = nullptr;
  CascRun r{n_cascades, T, direction, nullptr, nullptr, true, nullptr, n_sets, nullptr, nullptr};
  if ((rc = bit_rows_get(tm, b, C, fn, "samples", &Y, &Ao, &Ai)) ||
      (rc = tm.get(&r.live, C * b.bits_b, "vmr_sample_seed_outreach: the live rows")) ||
      (rc = casc_upload(h, tm, fn, q, seed_words, n_sets, curve, node_hits, r, &qd)))
    return rc;
  rc = sampled_chunks(h, tm, (size_t)n_samples, C, seed, n_trials, Y, out, [&](size_t s0, int c) -> int {
    int rc2;
    if ((rc2 = tri_pack_chunk(h, Y, c, Ao, Ai))) return rc2;
    return casc_chunk(h, b, c, cascade_seed + (u64)s0, r, Ao, Ai, out[0].as<unsigned>());   // (mod 2^64)
  });
  return rc ? rc : casc_set_finish(h, r, curve, node_hits);
}

extern "C" int vmr_network_outreach(vmr_handle h, const uint8_t* Y, int n, uint64_t cascade_seed, int n_cascades, const double* q, int T,
                                    int direction, uint32_t* values, uint32_t* summary) {
  if (!h) return VMR_EINVAL;
  const char* fn = "vmr_network_outreach";
  int rc;
  if (n < 1) return fail(h, VMR_EINVAL, "vmr_network_outreach: n must be positive");
  if ((rc = casc_args(h, fn, n_cascades, q, T, direction))) return rc;
  if (!Y) return fail(h, VMR_EINVAL, "vmr_network_outreach: Y is NULL");
  if (!values) return fail(h, VMR_EINVAL, "vmr_network_outreach: values is NULL");
  HIPCHK(h, hipSetDevice(h->device));
  const Geo& g = h->g;
  const BitRows b = bit_rows(g);
  const size_t per = b.per() + b.bits_b + b.LN * 4 + (size_t)g.L * 8;
  size_t C;
  if ((rc = chunk_samples(h, fn, (size_t)n, per, (size_t)g.L * 8, &C, "network"))) return rc;
  Tmp tm(h);
  uint8_t* Yd = nullptr;
  u64 *Ao = nullptr, *Ai = nullptr;
  double* qd = nullptr;
  unsigned *vals = nullptr, *csum = nullptr;
  CascRun r{n_cascades, T, direction, nullptr, nullptr, false, nullptr, 0, nullptr, nullptr};
  if ((rc = bit_rows_get(tm, b, C, fn, "networks", &Yd, &Ao, &Ai)) ||
      (rc = tm.get(&r.live, C * b.bits_b, "vmr_network_outreach: the live rows")) ||
      (rc = tm.get(&vals, C * b.LN * 4, "vmr_network_outreach: the values")) ||
      (summary && (rc = tm.get(&csum, C * g.L * 8, "vmr_network_outreach: the summary"))) ||
      (rc = casc_upload(h, tm, fn, q, nullptr, 0, false, false, r, &qd)))
    return rc;
  return uploaded_chunks(h, b, (size_t)n, C, Y, Yd, Ao, Ai, [&](size_t s0, int c) -> int {
    int rc2;
    if ((rc2 = casc_chunk(h, b, c, cascade_seed + (u64)s0, r, Ao, Ai, vals))) return rc2;   // (mod 2^64)
    HIPCHK(h, hipMemcpyAsync(values + s0 * b.LN, vals, (size_t)c * b.LN * 4, hipMemcpyDeviceToHost, h->stream));
    if (summary) {
      hipLaunchKernelGGL(k_casc_finish, dim3((unsigned)(c * g.L)), dim3(CONN_TPB), 0, h->stream, vals, g.N, (double)n_cascades, (double*)nullptr,
                         (unsigned*)nullptr, csum);
      HIPCHK(h, hipGetLastError());
      HIPCHK(h, hipMemcpyAsync(summary + s0 * g.L * 2, csum, (size_t)c * g.L * 8, hipMemcpyDeviceToHost, h->stream));
    }
    return VMR_OK;
  });
}

extern "C" int vmr_network_seed_outreach(vmr_handle h, const uint8_t* Y, int n, uint64_t cascade_seed, int n_cascades, const double* q, int T,
                                         int direction, const uint64_t* seed_words, int n_sets, uint32_t* values, uint64_t* curve,
                                         uint32_t* node_hits) {
  if (!h) return VMR_EINVAL;
  const char* fn = "vmr_network_seed_outreach";
  int rc;
  if (n < 1) return fail(h, VMR_EINVAL, "vmr_network_seed_outreach: n must be positive");
  if ((rc = casc_args(h, fn, n_cascades, q, T, direction))) return rc;
  if ((rc = casc_set_args(h, fn, seed_words, n_sets, values))) return rc;
  if (!Y) return fail(h, VMR_EINVAL, "vmr_network_seed_outreach: Y is NULL");
  HIPCHK(h, hipSetDevice(h->device));
  const Geo& g = h->g;
  const BitRows b = bit_rows(g);
  const size_t vb = (size_t)g.L * n_sets * 4;
  const size_t per = b.per() + b.bits_b + vb;
  size_t C;
  if ((rc = chunk_samples(h, fn, (size_t)n, per, casc_set_fixed(g, n_sets, curve, node_hits), &C, "network"))) return rc;
  Tmp tm(h);
  uint8_t* Yd = nullptr;
  u64 *Ao = nullptr, *Ai = nullptr;
  double* qd = nullptr;
  unsigned* vals = nullptr;
  CascRun r{n_cascades, T, direction, nullptr, nullptr, true, nullptr, n_sets, nullptr, nullptr};
  if ((rc = bit_rows_get(tm, b, C, fn, "networks", &Yd, &Ao, &Ai)) ||
      (rc = tm.get(&r.live, C * b.bits_b, "vmr_network_seed_outreach: the live rows")) ||
      (rc = tm.get(&vals, C * vb, "vmr_network_seed_outreach: the values")) ||
      (rc = casc_upload(h, tm, fn, q, seed_words, n_sets, curve, node_hits, r, &qd)))
    return rc;
  rc = uploaded_chunks(h, b, (size_t)n, C, Y, Yd, Ao, Ai, [&](size_t s0, int c) -> int {
    int rc2;
    if ((rc2 = casc_chunk(h, b, c, cascade_seed + (u64)s0, r, Ao, Ai, vals))) return rc2;   // (mod 2^64)
    HIPCHK(h, hipMemcpyAsync(values + s0 * g.L * n_sets, vals, (size_t)c * vb, hipMemcpyDeviceToHost, h->stream));
    return VMR_OK;
  });
  return rc ? rc : casc_set_finish(h, r, curve, node_hits);
}
