// centrality.hip -- diffusion centrality of the posterior on the device: vmr_sample_centrality, vmr_mean_centrality.
//
// The read-side stops at dyads (netstats.hip), triads (triads.hip), groups (mixing.hip) and reach (connectivity.hip); who is
// central, and how sure the posterior is of it, is a statement about nodes.  Diffusion centrality (Banerjee, Chandrasekhar, Duflo
// and Jackson 2013) of a node is the expected number of times a piece of news that starts there is heard within T rounds when
// every tie passes it on with probability q:  c = sum_{t=1..T} (q M)^t 1.  It is a finite sum of non-negative terms, defined on
// any graph; T = 1 is the degree, large T with q below 1 / lambda_1 Katz centrality.
//
// vmr_sample_centrality draws S posterior samples of Y in chunks (sampled_side.h: sample s is what vmr_sample(h, seed + s,
// n_trials) writes), packs them into bit rows (sampled_side.h has the layout) and runs, per sample and layer, x_0 = 1, x_t = q_l
// (M x_{t-1}), c = x_1 + .. + x_T with M = A (the rows of Aout), A^T (the rows of Ain) or A | A^T (the OR of the two words).
// k_cent_walk: one workgroup (4 waves) per (layer, sample).  x_{t-1} and x_t ping-pong in LDS (16 N bytes: N <= VMR_CENT_NMAX =
// 2048 is 32 KiB); thread t keeps the c of nodes t, t + 256, .. in registers (KPT of them).  A step: a wave takes 64 consecutive
// rows at a time; G lanes (the largest power of two <= min(W, 64)) stride the W words of a row, 64 / G rows side by side, the
// words of CENT_FLY rows are loaded before the first is used; a lane walks its words' set bits in ascending order and adds
// x[bit] from LDS, a fixed xor tree runs over the G lanes and the group's first lane stores q times the sum.  One barrier per
// step.  After step T, c goes to LDS and every thread counts, for its nodes, the strictly larger entries (all lanes read the same
// address: a broadcast); c, the rank and the sample's (sum by a fixed tree, maximum) go to the chunk's buffers.
// k_node_fold (node_fold.h): one thread per (layer, node) adds the chunk's samples in ascending s into the per-node accumulators,
// which span the chunks of a call.
// Every sum has a fixed order and there is no floating-point atomic: every output is the same from run to run and for any
// chunking.
// Bytes of the walk per (sample, layer): the rows are read on each of the T steps, 8 N W T bytes from L2 (16 N W T with UNION)
// -- at N = 2000, T = 8: 4.1 MB -- and 12 N + 16 bytes are written once; x and c never leave the compute unit.
//
// vmr_mean_centrality: the same recursion on the posterior mean network, no sampling.  P (ns_exp_p) is formed once, its diagonal
// zeroed; IN and UNION keep a second matrix (P^T, or U with u_ij = 1 - (1 - p_ij)(1 - p_ji)) written through a transposed tile in
// LDS, so that every one of the T steps reads along rows: a wave per row, a fixed shuffle tree, no atomics, x in global memory.
#include <cmath>
#include "node_fold.h"

namespace {

#define CENT_TPB 256
#define CENT_FLY 4   // rows whose words a lane group has in flight

// One step: xn[i] = q * sum over the set bits j of row i of A (| B with UNION) of x[j], i in [0, N).  Every lane of the
// workgroup calls it; the lane's own words in ascending order, then the xor tree over the G = 1 << lG lanes of the row.
template <bool UNION>
__device__ __forceinline__ void cent_step(const u64* __restrict__ A, const u64* __restrict__ B, int N, int W, int lG, double q, const double* x,
                                          double* xn) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int G = 1 << lG, nps = 64 >> lG, sub = lane >> lG, wl = lane & (G - 1);
  for (int base = wv * 64; base < N; base += CENT_TPB) {
    for (int j0 = sub; j0 < 64; j0 += CENT_FLY * nps) {
      double acc[CENT_FLY];
#pragma unroll
      for (int t = 0; t < CENT_FLY; ++t) acc[t] = 0.0;
      for (int ww = wl; ww < W; ww += G) {   // (one trip when W is a power of two)
        u64 wd[CENT_FLY];
#pragma unroll
        for (int t = 0; t < CENT_FLY; ++t) {
          const int j = j0 + t * nps, row = base + j;
          wd[t] = 0ull;
          if (j < 64 && row < N) {
            const size_t o = (size_t)row * W + ww;
            wd[t] = A[o];
            if (UNION) wd[t] |= B[o];
          }
        }
#pragma unroll
        for (int t = 0; t < CENT_FLY; ++t) {
          u64 w = wd[t];
          while (w) {
            const int bit = __ffsll((long long)w) - 1;
            acc[t] += x[ww * 64 + bit];   // (< 64 W: inside the array whatever the pad bits hold)
            w &= w - 1ull;
          }
        }
      }
#pragma unroll
      for (int t = 0; t < CENT_FLY; ++t) {
        double a = acc[t];
        for (int o = G >> 1; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);   // (every lane of the wave is here)
        const int j = j0 + t * nps, row = base + j;
        if (wl == 0 && j < 64 && row < N) xn[row] = q * a;
      }
    }
  }
}

// Grid (L, samples of the chunk); dynamic LDS: 2 x 64 W doubles.  dir: 0 the rows of Aout, 1 those of Ain, 2 their OR.
// cval[s][l][N] and crank[s][l][N] are stored for every node; summary[s][l][2] may be null.  KPT >= ceil(N / 256).
template <int KPT>
__global__ __launch_bounds__(CENT_TPB) void k_cent_walk(const u64* __restrict__ Aout, const u64* __restrict__ Ain, int N, int L, int W, int lG,
                                                         int dir, int T, const double* __restrict__ qv, double* __restrict__ cval,
                                                         unsigned* __restrict__ crank, double* __restrict__ summary) {
  extern __shared__ double cent_lds[];
  __shared__ double red[16];
  const int tid = threadIdx.x;
  const int l = blockIdx.x, s = blockIdx.y;
  const size_t sl = (size_t)s * L + l;
  const u64* A = (dir == 1 ? Ain : Aout) + sl * N * W;
  const u64* B = (dir == 1 ? Aout : Ain) + sl * N * W;
  const int Np = W * 64;
  const double q = qv[l];
  double *x = cent_lds, *xn = cent_lds + Np;
  double c[KPT];
#pragma unroll
  for (int k = 0; k < KPT; ++k) c[k] = 0.0;
  for (int v = tid; v < Np; v += CENT_TPB) { x[v] = v < N ? 1.0 : 0.0; xn[v] = 0.0; }
  __syncthreads();
  for (int t = 1; t <= T; ++t) {
    if (dir == 2) cent_step<true>(A, B, N, W, lG, q, x, xn);
    else cent_step<false>(A, B, N, W, lG, q, x, xn);
    __syncthreads();   // (x has been read by every wave, xn is complete: the next step writes x and reads xn only)
#pragma unroll
    for (int k = 0; k < KPT; ++k) {
      const int v = tid + k * CENT_TPB;
      if (v < N) c[k] += xn[v];
    }
    { double* sw = x; x = xn; xn = sw; }
  }
  // c into the buffer the last step read (nobody reads it any more), then the ranks
  double tsum = 0.0, tmax = 0.0;
#pragma unroll
  for (int k = 0; k < KPT; ++k) {
    const int v = tid + k * CENT_TPB;
    if (v < N) { xn[v] = c[k]; tsum += c[k]; tmax = fmax(tmax, c[k]); }
  }
  __syncthreads();
  unsigned rk[KPT];
#pragma unroll
  for (int k = 0; k < KPT; ++k) rk[k] = 0u;
  for (int u = 0; u < N; ++u) {
    const double cu = xn[u];   // (the same address in every lane)
#pragma unroll
    for (int k = 0; k < KPT; ++k) rk[k] += cu > c[k] ? 1u : 0u;
  }
#pragma unroll
  for (int k = 0; k < KPT; ++k) {
    const int v = tid + k * CENT_TPB;
    if (v < N) { cval[sl * N + v] = c[k]; crank[sl * N + v] = rk[k]; }
  }
  if (summary) {   // (the same in every thread)
    const double sum = block_sum_n(tsum, red);
    tmax = wave_max(tmax);
    __syncthreads();
    if ((tid & 63) == 0) red[8 + (tid >> 6)] = tmax;
    __syncthreads();
    if (tid == 0) {
      double m = red[8];
      for (int w = 1; w < CENT_TPB / 64; ++w) m = fmax(m, red[8 + w]);
      summary[sl * 2] = sum;
      summary[sl * 2 + 1] = m;
    }
  }
}

// ------------------------------------------------------------------------------------------
// the mean network
// ------------------------------------------------------------------------------------------
#define CM_T 32   // tile edge of the transposed read

__global__ __launch_bounds__(256) void k_cent_zero_diag(double* __restrict__ P, int N, size_t LN) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= LN) return;
  const size_t l = e / N, i = e - l * N;
  P[(l * N + i) * N + i] = 0.0;
}

// M[l][i][j] = p_ji (dir 1) or 1 - (1 - p_ij)(1 - p_ji) (dir 2) off the diagonal, 0 on it.  Grid (nt^2 tiles, L), tile (bi, bj) =
// (blockIdx.x / nt, blockIdx.x % nt); the tile (bj, bi) of P is read along rows and turned in LDS.  u_ij is the formula as it
// reads, every operation rounded (no contraction): where both p are tiny it is a difference of numbers near 1, and a fused
// product would give another u than a host that follows the definition -- and u_ij = u_ji bit for bit: the product commutes.
__global__ __launch_bounds__(256) void k_cent_mean_m(const double* __restrict__ P, double* __restrict__ M, int N, int nt, int dir) {
#pragma clang fp contract(off)
  __shared__ double Ts[CM_T][CM_T + 1];
  const int tx = threadIdx.x & (CM_T - 1), ty = threadIdx.x / CM_T;
  const int i0 = (blockIdx.x / nt) * CM_T, j0 = (blockIdx.x % nt) * CM_T;
  const size_t T = (size_t)N * N;
  const double* Pl = P + (size_t)blockIdx.y * T;
  double* Ml = M + (size_t)blockIdx.y * T;
  for (int r = ty; r < CM_T; r += 256 / CM_T) {
    const int jj = j0 + r, ii = i0 + tx;
    Ts[r][tx] = (jj < N && ii < N) ? Pl[(size_t)jj * N + ii] : 0.0;
  }
  __syncthreads();
  for (int r = ty; r < CM_T; r += 256 / CM_T) {
    const int i = i0 + r, j = j0 + tx;
    if (i < N && j < N) {
      const double pt = Ts[tx][r];   // p_ji
      double m = pt;
      if (dir == 2) m = 1.0 - (1.0 - Pl[(size_t)i * N + j]) * (1.0 - pt);
      Ml[(size_t)i * N + j] = i == j ? 0.0 : m;
    }
  }
}

// One wave per row i = 4 blockIdx.x + wave of layer blockIdx.y: xn[i] = q_l sum_j M_ij x_j (x = 1 when `first`), lane j, j + 64,
// .. in ascending order, then the xor tree; c[i] = xn[i] (first) or c[i] + xn[i].
__global__ __launch_bounds__(256) void k_cent_mean_step(const double* __restrict__ M, const double* __restrict__ x, double* __restrict__ xn,
                                                        double* __restrict__ c, const double* __restrict__ qv, int N, int first) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6), l = blockIdx.y;
  if (i >= N) return;   // (the same in every lane of the wave)
  const double* row = M + ((size_t)l * N + i) * N;
  const double* xl = x + (size_t)l * N;
  double a = 0.0;
  if (first) for (int j = lane; j < N; j += 64) a += row[j];
  else for (int j = lane; j < N; j += 64) a += row[j] * xl[j];
  a = wave_sum(a);
  if (lane == 0) {
    const size_t e = (size_t)l * N + i;
    const double v = qv[l] * a;
    xn[e] = v;
    c[e] = first ? v : c[e] + v;
  }
}

// what both calls refuse of q, T and direction, or VMR_OK
int cent_args(vmr_ctx* h, const char* fn, const double* q, int T, int direction) {
  char msg[256];
  if (direction < VMR_CENT_OUT || direction > VMR_CENT_UNION) {
    snprintf(msg, sizeof msg, "%s: direction must be 0 (out), 1 (in) or 2 (union), got %d", fn, direction);
    return fail(h, VMR_EINVAL, msg);
  }
  if (T < 1 || T > VMR_CENT_TMAX) {
    snprintf(msg, sizeof msg, "%s: T must be in [1, %d], got %d", fn, VMR_CENT_TMAX, T);
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

}  // namespace

extern "C" int vmr_sample_centrality(vmr_handle h, uint64_t seed, int n_samples, int n_trials, const double* q, int T, int direction, int top_k,
                                     double* node_sum, double* node_sumsq, uint64_t* node_rank_sum, uint32_t* node_top, double* summary,
                                     double* values) {
  if (!h) return VMR_EINVAL;
  const char* fn = "vmr_sample_centrality";
  int rc;
  if ((rc = sampled_counts(h, fn, n_samples, n_trials))) return rc;
  const Geo& g = h->g;
  char msg[256];
  if (g.N > VMR_CENT_NMAX) {
    snprintf(msg, sizeof msg, "%s: the walk keeps 16 N bytes in LDS: N <= %d, the handle has N = %d", fn, VMR_CENT_NMAX, g.N);
    return fail(h, VMR_EINVAL, msg);
  }
  if ((rc = cent_args(h, fn, q, T, direction))) return rc;
  if ((rc = node_fold_args(h, fn, top_k, node_sum))) return rc;
  if ((rc = expected_begin(h, fn))) return rc;
  const BitRows b = bit_rows(g);
  const size_t LN = b.LN;
  SampledOut out[1] = {{summary, (size_t)g.L * 16, false, "vmr_sample_centrality: the summary", nullptr}};
  // device bytes per sample of a chunk: the bit-row chunk, c and the ranks, the summary; per call: the accumulators and q
  const size_t per = b.per() + LN * 12 + (summary ? out[0].bytes : 0);
  const size_t fixed = NodeFold::bytes(LN) + (size_t)g.L * 8;
  size_t C;
  if ((rc = chunk_samples(h, fn, (size_t)n_samples, per, fixed, &C))) return rc;
  Tmp tm(h);
  uint8_t* Y = nullptr;
  u64 *Ao = nullptr, *Ai = nullptr;
  double *cval = nullptr, *qd = nullptr;
  unsigned* crank = nullptr;
  NodeFold fold;
  if ((rc = bit_rows_get(tm, b, C, fn, "samples", &Y, &Ao, &Ai)) ||
      (rc = tm.get(&cval, C * LN * 8, "vmr_sample_centrality: the values")) ||
      (rc = tm.get(&crank, C * LN * 4, "vmr_sample_centrality: the ranks")) ||
      (rc = tm.get(&qd, (size_t)g.L * 8, "vmr_sample_centrality: q")))
    return rc;
  HIPCHK(h, hipMemcpyAsync(qd, q, (size_t)g.L * 8, hipMemcpyHostToDevice, h->stream));
  if ((rc = fold.begin(h, tm, fn, LN, top_k))) return rc;
  const size_t smem = (size_t)b.W * 64 * 2 * 8;
  const int kpt = (g.N + CENT_TPB - 1) / CENT_TPB;   // nodes a thread owns: 1 .. VMR_CENT_NMAX / 256 = 8
  rc = sampled_chunks(h, tm, (size_t)n_samples, C, seed, n_trials, Y, out, [&](size_t s0, int c) -> int {
    int rc2;
    if ((rc2 = tri_pack_chunk(h, Y, c, Ao, Ai))) return rc2;
    with_kpt(kpt, [&](auto K) {
      hipLaunchKernelGGL(k_cent_walk<decltype(K)::value>, dim3((unsigned)g.L, (unsigned)c), dim3(CENT_TPB), smem, h->stream, Ao, Ai, g.N, g.L, b.W,
                         b.lG, direction, T, qd, cval, crank, out[0].as<double>());
    });
    HIPCHK(h, hipGetLastError());
    if ((rc2 = fold.add(h, cval, crank, c))) return rc2;
    if (values) HIPCHK(h, hipMemcpyAsync(values + s0 * LN, cval, (size_t)c * LN * 8, hipMemcpyDeviceToHost, h->stream));
    return VMR_OK;
  });
  return rc ? rc : fold.finish(h, node_sum, node_sumsq, node_rank_sum, node_top);
}

extern "C" int vmr_mean_centrality(vmr_handle h, const double* q, int T, int direction, double* out) {
  if (!h) return VMR_EINVAL;
  const char* fn = "vmr_mean_centrality";
  int rc;
  if ((rc = cent_args(h, fn, q, T, direction))) return rc;
  if (!out) return fail(h, VMR_EINVAL, "vmr_mean_centrality: out is NULL");
  if ((rc = expected_begin(h, fn))) return rc;
  const Geo& g = h->g;
  const size_t NN = (size_t)g.N * g.N, ties = (size_t)g.L * NN, LN = (size_t)g.L * g.N;
  const int nbp = exp_p_blocks(NN);
  const int nt = (g.N + CM_T - 1) / CM_T;
  if ((size_t)nt * nt > 0x7fffffffu) return fail(h, VMR_EINVAL, "vmr_mean_centrality: N is too large");
  Tmp tm(h);
  double *P = nullptr, *M = nullptr, *wpart = nullptr, *xa = nullptr, *xb = nullptr, *cd = nullptr, *qd = nullptr;
  if ((rc = tm.get(&P, ties * 8, "vmr_mean_centrality: the edge probabilities")) ||
      (direction != VMR_CENT_OUT && (rc = tm.get(&M, ties * 8, "vmr_mean_centrality: the transposed probabilities"))) ||
      (rc = tm.get(&wpart, (size_t)g.L * nbp * 32, "vmr_mean_centrality: partial sums")) ||
      (rc = tm.get(&xa, LN * 8, "vmr_mean_centrality: the walk")) || (rc = tm.get(&xb, LN * 8, "vmr_mean_centrality: the walk")) ||
      (rc = tm.get(&cd, LN * 8, "vmr_mean_centrality: the result")) || (rc = tm.get(&qd, (size_t)g.L * 8, "vmr_mean_centrality: q")))
    return rc;
  HIPCHK(h, hipMemcpyAsync(qd, q, (size_t)g.L * 8, hipMemcpyHostToDevice, h->stream));
  if ((rc = ns_exp_p(h, P, wpart, nbp))) return rc;
  if (direction == VMR_CENT_OUT) {
    hipLaunchKernelGGL(k_cent_zero_diag, dim3(grid_for(LN, 256, 0xffffffffu)), dim3(256), 0, h->stream, P, g.N, LN);
    M = P;
  } else {
    hipLaunchKernelGGL(k_cent_mean_m, dim3((unsigned)(nt * nt), (unsigned)g.L), dim3(256), 0, h->stream, P, M, g.N, nt, direction);
  }
  HIPCHK(h, hipGetLastError());
  for (int t = 1; t <= T; ++t) {   // (the grid depends on N and L only)
    hipLaunchKernelGGL(k_cent_mean_step, dim3((unsigned)((g.N + 3) / 4), (unsigned)g.L), dim3(256), 0, h->stream, M, xa, xb, cd, qd, g.N, t == 1);
    HIPCHK(h, hipGetLastError());
    std::swap(xa, xb);
  }
  HIPCHK(h, hipMemcpyAsync(out, cd, LN * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return VMR_OK;
}
