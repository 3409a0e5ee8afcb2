// netstats.hip -- network statistics of the posterior on the device: vmr_sample_stats, vmr_expected_stats.
//
// What people compute from a fit's rho (the reference's utils.calculate_overall_reciprocity, utils.py:69-70; the expected
// reciprocity and the F1 of its notebooks) are a few integers per network.  vmr_sample_stats draws S posterior samples of Y -- sample
// s is exactly what vmr_sample(h, seed + s, n_trials) writes: the same draw_tie (sample_draw.h) -- and returns, per sample and
// layer, over ALL (i, j), the diagonal included:
//     edges #{Y > 0}, weight sum Y, mutual #{(i,j) : Y_ij > 0 and Y_ji > 0}, tp #{Y > 0 and y_ref > 0}, out- and in-degrees.
//
// Layout (sampled_side.h has the chunking and the transposed tile).  rho is stored by tie (dense tiles) or by sorted position
// (report lists: only perm, position -> tie, exists), and `mutual` needs tie (j,i) next to tie (i,j).  So the samples are DRAWN by
// position -- k_ns_draw: one thread per position reads its rho row once and draws a whole chunk of C samples from it, writing
// Y[s][l][i][j] through perm -- and REDUCED in natural order: k_ns_reduce, one workgroup per (strip of 64 rows, layer, sample),
// walks the strip's tiles.  The workgroup of strip bi thereby sees all of rows i and all of columns i of its 64 nodes: both degree
// arrays are plain stores, no atomics.  The chunk's Y is read twice.  No inverse permutation is built.
//
// Every count is an integer: ballots and popcounts inside the wave, a wave sum for the weight, LDS atomics, then one 64-bit
// global atomic per workgroup, sample and column -- sums of integers, the same from run to run in any order.
//
// vmr_expected_stats: the same quantities in expectation under q(Y) = prod rho, p_ij = sum_{k>=1} rho_ijk:
//     (sum p, sum_ij sum_k k rho_ijk, sum_ij p_ij p_ji, sum p (1 - p)) per layer,
// p written in natural order by position (k_ns_exp_p), then read with its transpose (k_ns_exp_pairs); sums of doubles by a fixed
// two-stage tree -- per-workgroup partials on a grid that depends on N only, one workgroup per layer to finish -- no atomics.
#include "sampled_side.h"
#include "sample_draw.h"

namespace {

// A chunk of C samples drawn from one read of rho: Y[s][q's tie] = the draw of (seed0 + s, tie), s in [0, C).
// LDS_CNT: K > KMAX, the trial counts in LDS (64 threads, [K][64] words); KC > 0: K = KC, the row is held in registers.
template <bool LDS_CNT, int KC>
__global__ __launch_bounds__(LDS_CNT ? 64 : 256) void k_ns_draw(const double* __restrict__ rho, uint8_t* __restrict__ Y, size_t ties, int K, int n_trials,
                                                                unsigned long long seed0, int C, const unsigned* __restrict__ perm, size_t T, size_t NS) {
  extern __shared__ unsigned cnt_s[];   // LDS_CNT: [K][64]
  unsigned* cnt = LDS_CNT ? cnt_s + threadIdx.x : nullptr;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < ties; q += (size_t)gridDim.x * blockDim.x) {
    const double* r = rho + q * K;
    size_t t = q;
    if (perm) { const size_t l = q / T, pos = q - l * T; t = l * T + perm[l * NS * 64 + pos]; }   // rho by sorted position, Y by tie
    if (KC > 0) {
      double rl[KC > 0 ? KC : 1];
#pragma unroll
      for (int k = 0; k < KC; ++k) rl[k] = r[k];
      for (int s = 0; s < C; ++s) Y[(size_t)s * ties + t] = (uint8_t)draw_tie<LDS_CNT>(rl, KC, n_trials, seed0 + (unsigned long long)s, t, cnt);
    } else {
      for (int s = 0; s < C; ++s) Y[(size_t)s * ties + t] = (uint8_t)draw_tie<LDS_CNT>(r, K, n_trials, seed0 + (unsigned long long)s, t, cnt);
    }
  }
}

// One workgroup (4 waves) per (strip bi of 64 rows, layer l, sample s).  For every column tile bj: wave w takes rows r = 4 it + w
// of tile (bi, bj) with lane = column c, and reads B[c][r] = Y[j0 + c][i0 + r] of the transposed tile from LDS.  Per row r:
//   ballot(A > 0)          the row's edges: out-degree of node i0 + r within the tile
//   ballot(B > 0)          the edges INTO node i0 + r from the tile's 64 sources: its in-degree within the tile
//   ballot(A > 0 & B > 0)  mutual pairs
// Lane `it` of wave w keeps the degrees of row 4 it + w.
__global__ __launch_bounds__(256) void k_ns_reduce(const uint8_t* __restrict__ Y, const uint8_t* __restrict__ yref, int N, int L,
                                                   unsigned long long* __restrict__ counts, int32_t* __restrict__ deg_out, int32_t* __restrict__ deg_in) {
  __shared__ uint8_t Bs[SS_TILE * SS_BSTRIDE];
  __shared__ unsigned long long tot[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int bi = blockIdx.x, l = blockIdx.y, s = blockIdx.z;
  const size_t T = (size_t)N * N;
  const uint8_t* Ys = Y + ((size_t)s * L + l) * T;
  const uint8_t* Yr = yref ? yref + (size_t)l * T : nullptr;
  const int i0 = bi * SS_TILE, nb = (N + SS_TILE - 1) / SS_TILE;
  if (threadIdx.x < 4) tot[threadIdx.x] = 0ull;
  unsigned long long edges = 0, mutual = 0, tp = 0, wsum = 0;   // edges, mutual, tp: uniform over the wave; wsum: per lane
  unsigned dout = 0, din = 0;
  for (int bj = 0; bj < nb; ++bj) {
    const int j0 = bj * SS_TILE;
    __syncthreads();   // (the last tile's reads of Bs are done)
    tile_transposed(Bs, Ys, i0, j0, N);
    __syncthreads();
    const int j = j0 + lane;
    for (int it = 0; it < SS_TILE / 4; ++it) {
      const int r = it * 4 + w, i = i0 + r;
      const bool in = i < N && j < N;
      const unsigned a = in ? Ys[(size_t)i * N + j] : 0u;
      const unsigned b = Bs[lane * SS_BSTRIDE + r];
      const unsigned long long ba = __ballot(a > 0u), bb = __ballot(b > 0u);
      const unsigned ne = (unsigned)__popcll(ba);
      edges += ne;
      mutual += (unsigned)__popcll(ba & bb);
      if (Yr) {
        const bool hit = a > 0u && Yr[(size_t)i * N + j] > 0;   // (a > 0 only in range)
        tp += (unsigned)__popcll(__ballot(hit));
      }
      wsum += a;
      if (lane == it) { dout += ne; din += (unsigned)__popcll(bb); }
    }
  }
  wsum = wave_sum_ull(wsum);
  if (lane == 0) {
    if (edges) atomicAdd(&tot[0], edges);
    if (wsum) atomicAdd(&tot[1], wsum);
    if (mutual) atomicAdd(&tot[2], mutual);
    if (tp) atomicAdd(&tot[3], tp);
  }
  if (lane < SS_TILE / 4) {
    const int i = i0 + lane * 4 + w;
    if (i < N) {
      const size_t o = ((size_t)s * L + l) * N + i;
      if (deg_out) deg_out[o] = (int32_t)dout;
      if (deg_in) deg_in[o] = (int32_t)din;
    }
  }
  __syncthreads();
  if (threadIdx.x < 4 && tot[threadIdx.x]) atomicAdd(counts + ((size_t)s * L + l) * 4 + threadIdx.x, tot[threadIdx.x]);
}

// p = sum_{k>=1} rho_k (k ascending) of every tie of layer blockIdx.y, written in natural order; the workgroup's sum of
// sum_k k rho_k goes to part[l][blockIdx.x][1]
__global__ __launch_bounds__(256) void k_ns_exp_p(const double* __restrict__ rho, double* __restrict__ P, double* __restrict__ part, int K,
                                                  const unsigned* __restrict__ perm, size_t T, size_t NS) {
  __shared__ double red[16];
  const int l = blockIdx.y;
  double aw = 0.0;
  for (size_t pos = (size_t)blockIdx.x * 256 + threadIdx.x; pos < T; pos += (size_t)gridDim.x * 256) {
    const double* r = rho + ((size_t)l * T + pos) * K;
    const size_t t = perm ? (size_t)perm[(size_t)l * NS * 64 + pos] : pos;
    double p = 0.0, wt = 0.0;
    for (int k = 1; k < K; ++k) { p += r[k]; wt += (double)k * r[k]; }
    P[(size_t)l * T + t] = p;
    aw += wt;
  }
  const double sw = block_sum_n(aw, red);
  if (threadIdx.x == 0) part[((size_t)l * gridDim.x + blockIdx.x) * 4 + 1] = sw;
}

// the workgroup's sums of p, p_ij p_ji and p (1 - p) over its ties: part[l][blockIdx.x][0, 2, 3]
__global__ __launch_bounds__(256) void k_ns_exp_pairs(const double* __restrict__ P, double* __restrict__ part, int N) {
  __shared__ double red[16];
  const int l = blockIdx.y;
  const size_t T = (size_t)N * N;
  const double* Pl = P + (size_t)l * T;
  double ae = 0.0, am = 0.0, av = 0.0;
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < T; t += (size_t)gridDim.x * 256) {
    const size_t i = t / N, j = t - i * N;
    const double p = Pl[t], q = Pl[j * N + i];
    ae += p; am += p * q; av += p * (1.0 - p);
  }
  const double se = block_sum_n(ae, red), sm = block_sum_n(am, red), sv = block_sum_n(av, red);
  if (threadIdx.x == 0) {
    double* o = part + ((size_t)l * gridDim.x + blockIdx.x) * 4;
    o[0] = se; o[2] = sm; o[3] = sv;
  }
}

// second stage: one workgroup per layer sums the nb partials of each column in a fixed order
__global__ __launch_bounds__(256) void k_ns_exp_finish(const double* __restrict__ part, int nb, double* __restrict__ out) {
  __shared__ double red[16];
  const int l = blockIdx.x;
  for (int c = 0; c < 4; ++c) {
    const double sum = partials_col_sum(part + (size_t)l * nb * 4, nb, 4, c, red);
    if (threadIdx.x == 0) out[l * 4 + c] = sum;
  }
}

}  // namespace

// declared in vmr_internal.h: the replicates of the posterior predictive check (ppc_rep.hip) draw their Y with it too
int ns_draw_chunk(vmr_ctx* h, uint8_t* Y, unsigned long long seed0, int C, int n_trials) {
  const Geo& g = h->g;
  const size_t T = (size_t)g.N * g.N, ties = (size_t)g.L * T, NS = (T + 63) / 64;
  if (g.K > KMAX) {
    const size_t smem = (size_t)g.K * 64 * 4;
    if (smem > 48 * 1024) HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(k_ns_draw<true, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL((k_ns_draw<true, 0>), dim3((unsigned)std::min<size_t>(65536, (ties + 63) / 64)), dim3(64), smem, h->stream, h->rho, Y, ties, g.K,
                       n_trials, seed0, C, h->perm, T, NS);
  } else {
    const dim3 grid((unsigned)std::min<size_t>(65536, (ties + 255) / 256));
    if (g.K == 2) hipLaunchKernelGGL((k_ns_draw<false, 2>), grid, dim3(256), 0, h->stream, h->rho, Y, ties, g.K, n_trials, seed0, C, h->perm, T, NS);
    else hipLaunchKernelGGL((k_ns_draw<false, 0>), grid, dim3(256), 0, h->stream, h->rho, Y, ties, g.K, n_trials, seed0, C, h->perm, T, NS);
  }
  HIPCHK(h, hipGetLastError());
  return VMR_OK;
}

// declared in vmr_internal.h: the expected triads (triads.hip) start from the same edge probabilities
int ns_exp_p(vmr_ctx* h, double* P, double* part, int nb) {
  const Geo& g = h->g;
  const size_t T = (size_t)g.N * g.N;
  hipLaunchKernelGGL(k_ns_exp_p, dim3((unsigned)nb, (unsigned)g.L), dim3(256), 0, h->stream, h->rho, P, part, g.K, h->perm, T, (T + 63) / 64);
  HIPCHK(h, hipGetLastError());
  return VMR_OK;
}

extern "C" int vmr_sample_stats(vmr_handle h, uint64_t seed, int n_samples, int n_trials, const uint8_t* y_ref, int y_ref_on_device,
                                uint64_t* counts, int32_t* deg_out, int32_t* deg_in) {
  if (!h) return VMR_EINVAL;
  if (!counts) return fail(h, VMR_EINVAL, "vmr_sample_stats: counts is NULL");
  int rc;
  if ((rc = sampled_begin(h, "vmr_sample_stats", n_samples, n_trials))) return rc;
  const Geo& g = h->g;
  const size_t ties = (size_t)g.L * g.N * g.N, deg_b = (size_t)g.L * g.N * 4;
  SampledOut out[3] = {{counts, (size_t)g.L * 4 * 8, true, "vmr_sample_stats: the counts"},
                       {deg_out, deg_b, false, "vmr_sample_stats: the out-degrees"},
                       {deg_in, deg_b, false, "vmr_sample_stats: the in-degrees"}};
  const size_t per = ties + out[0].bytes + (deg_out ? deg_b : 0) + (deg_in ? deg_b : 0);   // device bytes per sample of a chunk
  const bool upload = y_ref && !y_ref_on_device;
  size_t C;
  if ((rc = chunk_samples(h, "vmr_sample_stats", (size_t)n_samples, per, upload ? ties : 0, &C))) return rc;
  Tmp tm(h);
  uint8_t *Y = nullptr, *yr = nullptr;
  if ((rc = tm.get(&Y, C * ties, "vmr_sample_stats: the samples"))) return rc;
  const uint8_t* yref_dev = y_ref;
  if (upload) {
    if ((rc = tm.get(&yr, ties, "vmr_sample_stats: the reference network"))) return rc;
    HIPCHK(h, hipMemcpyAsync(yr, y_ref, ties, hipMemcpyHostToDevice, h->stream));
    yref_dev = yr;
  }
  const unsigned nstrip = (unsigned)((g.N + SS_TILE - 1) / SS_TILE);
  return sampled_chunks(h, tm, (size_t)n_samples, C, seed, n_trials, Y, out, [&](size_t, int c) -> int {
    hipLaunchKernelGGL(k_ns_reduce, dim3(nstrip, (unsigned)g.L, (unsigned)c), dim3(256), 0, h->stream, Y, yref_dev, g.N, g.L,
                       out[0].as<unsigned long long>(), out[1].as<int32_t>(), out[2].as<int32_t>());
    HIPCHK(h, hipGetLastError());
    return VMR_OK;
  });
}

extern "C" int vmr_expected_stats(vmr_handle h, double* out) {
  if (!h) return VMR_EINVAL;
  if (!out) return fail(h, VMR_EINVAL, "vmr_expected_stats: out is NULL");
  int rc;
  if ((rc = expected_begin(h, "vmr_expected_stats"))) return rc;
  const Geo& g = h->g;
  const size_t T = (size_t)g.N * g.N, ties = (size_t)g.L * T;
  const int nb = exp_p_blocks(T);
  const size_t need = ties * 8 + (size_t)g.L * nb * 32 + (size_t)g.L * 32;
  size_t fr = 0, tot = 0;
  HIPCHK(h, hipMemGetInfo(&fr, &tot));
  if (need + (64u << 20) > fr) {
    char msg[256];
    snprintf(msg, sizeof msg, "vmr_expected_stats: the edge probabilities need %.3f GB of device memory, %.3f GB are free", need / 1e9, fr / 1e9);
    return fail(h, VMR_EINVAL, msg);
  }
  Tmp tm(h);
  double *P = nullptr, *part = nullptr, *od = nullptr;
  if ((rc = tm.get(&P, ties * 8, "vmr_expected_stats: the edge probabilities")) ||
      (rc = tm.get(&part, (size_t)g.L * nb * 32, "vmr_expected_stats: partial sums")) ||
      (rc = tm.get(&od, (size_t)g.L * 32, "vmr_expected_stats: the result")))
    return rc;
  if ((rc = ns_exp_p(h, P, part, nb))) return rc;
  hipLaunchKernelGGL(k_ns_exp_pairs, dim3((unsigned)nb, (unsigned)g.L), dim3(256), 0, h->stream, P, part, g.N);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(k_ns_exp_finish, dim3((unsigned)g.L), dim3(256), 0, h->stream, part, nb, od);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(out, od, (size_t)g.L * 32, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return VMR_OK;
}
