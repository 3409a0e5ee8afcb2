// ppc_rep.hip -- posterior predictive checks on the device: vmr_ppc_replicates, vmr_ppc_observed.
//
// A replicate is data drawn from the fitted model over the support of the handle's own mask: Y_r from rho (the draw of
// vmr_sample, in chunks: sampled_side.h), lambda of a tie from the replicate's table at Y_r, and for every unordered pair
// i < j and every reporter m that R keeps in either direction the pair draw of the generator (report_draw.h: what
// vmr_generate_x would write at (l,i,j,m) and (l,j,i,m), unclamped).  The reports are never written: they are reduced where
// they are drawn to VMR_PPC_NSTAT integers per replicate and layer (include/vimure_hip.h has the table), and the observed data is
// reduced by the same definitions (k_obs).
//
// k_rep: a group of G lanes (a wave when the rows are long) per unordered pair, its lanes over the pair's support -- the range
// [0, M) tested against both rows when either is all ones or held as mask words, else the merge of the two reporter lists (the
// second list's lanes drop what the first list holds).  A draw depends on (seed, l, i, j, m) only; a direction that R does not
// keep is zeroed after the draw.  Tie-level statistics (ties_reported, ties_agreed) come from ballots inside the group.  Every
// lane keeps integer partials; they leave the workgroup as one 64-bit atomic per statistic.  by_reporter: an LDS histogram
// [M][2] where it fits (M <= PR_HIST_M), flushed once per workgroup, else global atomics (wide reporter sets: a few reporters
// per row).  Integer sums in any order: bit-identical from run to run.
//
// k_obs: a group per ORDERED tie over the tie's own reports -- the dense row, or the tie's entries of the tie-major index of
// ppc.hip (value x << 1 | R) -- `mutual` looks the mirror report up (dense: the mirror row; lists: binary search in the mirror
// tie's entries).  A support element without a report adds nothing to any statistic, so the report lists are walked, not S.
#include "sampled_side.h"
#include "report_draw.h"

namespace {

#define PR_SLOTS 256     // tie slots a group walks per workgroup

struct RepArgs {
  int L, N, M, K, W, G;
  const uint8_t* cls;                  // [L][T]
  const uint64_t* Rb;                  // [L][T][W] or null
  const unsigned* rq;                  // [L][T + 1] or null
  const unsigned short* Rm;
  const unsigned long long* rbase;     // device [L]
  const uint8_t* Y;                    // [C][L][T] the chunk's samples
  const double *theta, *lambda, *eta;  // [C][L][M], [C][L][K], [C]
  unsigned long long seed_x;           // of the chunk's first replicate
  unsigned long long* counts;          // [C][L][VMR_PPC_NSTAT]
  unsigned long long* byrep;           // [C][L][M][2] or null
};

// the lanes' partials -> one atomic per statistic and workgroup; the LDS histogram -> global
template <bool HIST>
__device__ __forceinline__ void flush_stats(unsigned long long (&v)[VMR_PPC_NSTAT], unsigned long long* tot, unsigned long long* hist, int M,
                                            unsigned long long* __restrict__ counts, unsigned long long* __restrict__ byrep) {
#pragma unroll
  for (int k = 0; k < VMR_PPC_NSTAT; ++k) {
    v[k] = wave_sum_ull(v[k]);
    if ((threadIdx.x & 63) == 0 && v[k]) atomicAdd(&tot[k], v[k]);
  }
  __syncthreads();
  if (threadIdx.x < VMR_PPC_NSTAT && tot[threadIdx.x]) atomicAdd(counts + threadIdx.x, tot[threadIdx.x]);
  if (HIST && byrep) flush_bins(hist, byrep, 2 * M, 256);
}

template <bool HIST>
__device__ __forceinline__ void add_reporter(unsigned long long* hist, unsigned long long* __restrict__ byrep, unsigned m, unsigned np, unsigned long long tt) {
  unsigned long long* o = (HIST ? hist : byrep) + 2 * (size_t)m;
  atomicAdd(o, (unsigned long long)np);
  atomicAdd(o + 1, tt);
}

// (two workgroups per CU: the draw's registers fit 256 with two spilled; without the bound it takes 258 and one workgroup)
template <bool HIST>
__global__ __launch_bounds__(256, 2) void k_rep(RepArgs a) {
  extern __shared__ unsigned long long hist[];   // HIST: [M][2]
  __shared__ unsigned long long tot[VMR_PPC_NSTAT];
  const int l = blockIdx.y, r = blockIdx.z, G = a.G;
  const WalkGroup g = walk_group(G);
  const size_t T = (size_t)a.N * a.N, gpb = 256 / G, rl = (size_t)r * a.L + l;
  if (threadIdx.x < VMR_PPC_NSTAT) tot[threadIdx.x] = 0ull;
  if (HIST && a.byrep) for (int q = threadIdx.x; q < 2 * a.M; q += 256) hist[q] = 0ull;
  __syncthreads();
  const uint8_t* cls = a.cls + (size_t)l * T;
  const uint64_t* Rb = a.Rb ? a.Rb + (size_t)l * T * a.W : nullptr;
  const unsigned* rq = a.rq ? a.rq + (size_t)l * (T + 1) : nullptr;
  const unsigned short* Rm = a.rq ? a.Rm + a.rbase[l] : nullptr;
  const uint8_t* Y = a.Y + rl * T;
  const double* th = a.theta + rl * a.M;
  const double* lam = a.lambda + rl * a.K;
  const double eta = a.eta[r], inv = pair_inv(eta);
  const unsigned long long seed = a.seed_x + (unsigned long long)r;   // (mod 2^64)
  unsigned long long* byrep = a.byrep ? a.byrep + rl * a.M * 2 : nullptr;
  unsigned long long v[VMR_PPC_NSTAT] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
  const size_t t_lim = ((size_t)blockIdx.x + 1) * gpb * PR_SLOTS, t_end = t_lim < T ? t_lim : T;
  for (size_t t = (size_t)blockIdx.x * gpb * PR_SLOTS + threadIdx.x / G; t < t_end; t += gpb) {   // (uniform over the group)
    const size_t i = t / a.N, j = t - i * a.N;
    if (j <= i) continue;   // every unordered pair once; a diagonal tie holds no replicated report
    const size_t tm = j * a.N + i;
    const MaskRow A = mask_row(cls, Rb, rq, Rm, a.W, t), B = mask_row(cls, Rb, rq, Rm, a.W, tm);
    if (A.c == 0 && B.c == 0) continue;
    const unsigned ya = Y[t], yb = Y[tm];
    const double la = lam[ya < (unsigned)a.K ? ya : (unsigned)a.K - 1u], lb = lam[yb < (unsigned)a.K ? yb : (unsigned)a.K - 1u];
    const bool range = A.c == 1 || B.c == 1 || (A.c == 2 && !A.lst) || (B.c == 2 && !B.lst);
    const unsigned nc = range ? (unsigned)a.M : A.n + B.n;
    unsigned ca = 0, cb = 0;   // positives of tie (i,j) and of tie (j,i)
    for (unsigned c0 = 0; c0 < nc; c0 += (unsigned)G) {
      const unsigned q = c0 + (unsigned)g.gl;
      bool inA = false, inB = false;
      unsigned m = 0;
      if (q < nc) {
        if (range) { m = q; inA = row_has(A, m); inB = row_has(B, m); }
        else if (q < A.n) { m = A.lst[q]; inA = true; inB = row_has(B, m); }
        else { m = B.lst[q - A.n]; inB = !row_has(A, m); }   // (what both lists hold is the first list's)
      }
      unsigned xij = 0, xji = 0;
      if (inA || inB) {
        pair_draw(seed, (unsigned)l, (unsigned long long)t, m, la, lb, th[m], eta, inv, xij, xji);
        if (!inA) xij = 0;   // a direction outside the support is dropped
        if (!inB) xji = 0;
      }
      const bool pa = xij > 0u, pb = xji > 0u;
      const unsigned np = (pa ? 1u : 0u) + (pb ? 1u : 0u);
      if (np) {
        const unsigned long long tt = (unsigned long long)xij + xji;
        v[0] += np;
        v[1] += tt;
        v[2] += (unsigned long long)xij * xij + (unsigned long long)xji * xji;
        if (np == 2u) v[3] += 2ull;
        if (byrep) add_reporter<HIST>(hist, byrep, m, np, tt);
      }
      ca += (unsigned)__popcll(__ballot(pa) & g.gmask);
      cb += (unsigned)__popcll(__ballot(pb) & g.gmask);
    }
    if (g.gl == 0) {
      v[4] += (ca > 0u) + (cb > 0u);
      v[5] += (ca > 1u) + (cb > 1u);
    }
  }
  flush_stats<HIST>(v, tot, hist, a.M, a.counts + rl * VMR_PPC_NSTAT, byrep);
}

// one layer's observed data: a group per ordered tie
template <bool HIST>
__global__ __launch_bounds__(256) void k_obs(PpcLayer p, int G, unsigned long long* __restrict__ counts, unsigned long long* __restrict__ byrep) {
  extern __shared__ unsigned long long hist[];
  __shared__ unsigned long long tot[VMR_PPC_NSTAT];
  const WalkGroup g = walk_group(G);
  const size_t gpb = 256 / G;
  if (threadIdx.x < VMR_PPC_NSTAT) tot[threadIdx.x] = 0ull;
  if (HIST && byrep) for (int q = threadIdx.x; q < 2 * p.M; q += 256) hist[q] = 0ull;
  __syncthreads();
  unsigned long long v[VMR_PPC_NSTAT] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
  const size_t t_lim = ((size_t)blockIdx.x + 1) * gpb * PR_SLOTS, t_end = t_lim < p.T ? t_lim : p.T;
  for (size_t t = (size_t)blockIdx.x * gpb * PR_SLOTS + threadIdx.x / G; t < t_end; t += gpb) {
    const MaskRow A = mask_row(p.cls, p.Rb, p.rq, p.Rm, p.W, t);
    if (A.c == 0) continue;
    const size_t i = t / p.N, j = t - i * p.N, tm = j * p.N + i;
    const unsigned e0 = p.X ? 0u : p.ip[t], nc = p.X ? (unsigned)p.M : p.ip[t + 1] - e0;
    if (nc == 0u) continue;
    MaskRow B;
    B.c = 0; B.n = 0; B.w = nullptr; B.lst = nullptr;
    if (i != j) B = mask_row(p.cls, p.Rb, p.rq, p.Rm, p.W, tm);
    unsigned ca = 0;
    for (unsigned c0 = 0; c0 < nc; c0 += (unsigned)G) {
      const TieReport rp = tie_report(p, A, t, e0, nc, c0 + (unsigned)g.gl);
      const unsigned x = rp.in ? rp.x : 0u, m = rp.m;   // a count outside the mask is no report
      const bool mut = x && B.c != 0 && mirror_reported(p, B, tm, m);
      const bool pos = x > 0u;
      if (pos) {
        v[0] += 1ull;
        v[1] += x;
        v[2] += (unsigned long long)x * x;
        if (mut) v[3] += 1ull;
        if (byrep) add_reporter<HIST>(hist, byrep, m, 1u, (unsigned long long)x);
      }
      ca += (unsigned)__popcll(__ballot(pos) & g.gmask);
    }
    if (g.gl == 0) {
      v[4] += ca > 0u;
      v[5] += ca > 1u;
    }
  }
  flush_stats<HIST>(v, tot, hist, p.M, counts, byrep);
}

}  // namespace

extern "C" int vmr_ppc_replicates(vmr_handle h, int n_rep, uint64_t seed_y, uint64_t seed_x, int n_trials, const double* theta,
                                  const double* lambda, const double* eta, uint64_t* counts, uint64_t* by_reporter) {
  int rc;
  if ((rc = sampled_counts(h, "vmr_ppc_replicates", n_rep, n_trials, "n_rep"))) return rc;
  if (!theta || !lambda || !eta || !counts) return fail(h, VMR_EINVAL, "vmr_ppc_replicates: theta, lambda, eta or counts is NULL");
  const Geo& g = h->g;
  const size_t T = (size_t)g.N * g.N, ties = (size_t)g.L * T, LM = (size_t)g.L * g.M, LK = (size_t)g.L * g.K;
  for (int r = 0; r < n_rep; ++r)
    if (!(eta[r] >= 0.0 && eta[r] < 1.0)) return fail(h, VMR_EINVAL, "The mutuality parameter has to be in [0, 1)!");
  if (!table_nonneg(theta, (size_t)n_rep * LM)) return fail(h, VMR_EINVAL, "vmr_ppc_replicates: theta must be finite and non-negative");
  if (!table_nonneg(lambda, (size_t)n_rep * LK)) return fail(h, VMR_EINVAL, "vmr_ppc_replicates: lambda must be finite and non-negative");
  if ((rc = expected_begin(h, "vmr_ppc_replicates"))) return rc;
  // a chunk of replicates: Y (L N^2 bytes each), the parameters, the outputs
  SampledOut out[2] = {{counts, (size_t)g.L * VMR_PPC_NSTAT * 8, true, "the replicates' statistics"},
                       {by_reporter, LM * 16, true, "the replicates' statistics by reporter"}};
  const size_t per = ties + out[0].bytes + (by_reporter ? out[1].bytes : 0) + (LM + LK + 1) * 8;
  size_t C;
  if ((rc = chunk_samples(h, "vmr_ppc_replicates", (size_t)n_rep, per, 0, &C, "replicate"))) return rc;
  Tmp tm(h);
  uint8_t* Y = nullptr;
  double *thd = nullptr, *lad = nullptr, *etd = nullptr;
  if ((rc = tm.get(&Y, C * ties, "the replicates' Y")) || (rc = tm.get(&thd, C * LM * 8, "the replicates' theta")) ||
      (rc = tm.get(&lad, C * LK * 8, "the replicates' lambda")) || (rc = tm.get(&etd, C * 8, "the replicates' eta")))
    return rc;
  RepArgs a;
  a.L = g.L; a.N = g.N; a.M = g.M; a.K = g.K; a.W = g.W;
  a.cls = h->rcls; a.Rb = h->Rb; a.rq = h->rq; a.Rm = h->Rm; a.rbase = h->rbase;
  a.Y = Y; a.theta = thd; a.lambda = lad; a.eta = etd;
  // rows of a handle with mask lists are all ones, empty or listed: a pair's support is two lists at most, unless a row is all ones
  a.G = pow2_lanes((h->rq && !h->all_full && 2u * h->rm_maxrow < (unsigned)g.M) ? 2u * h->rm_maxrow : (unsigned)g.M);
  const bool hist = by_reporter && g.M <= PR_HIST_M;
  const size_t smem = hist ? (size_t)g.M * 16 : 0;
  const dim3 grid(walk_blocks(T, 256, a.G, PR_SLOTS), (unsigned)g.L);
  // per chunk: its replicates' parameters go up before the draw, and the reports' seed moves with the first replicate
  const auto upload = [&](size_t s0, int c) -> int {
    HIPCHK(h, hipMemcpyAsync(thd, theta + s0 * LM, (size_t)c * LM * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(lad, lambda + s0 * LK, (size_t)c * LK * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(etd, eta + s0, (size_t)c * 8, hipMemcpyHostToDevice, h->stream));
    return VMR_OK;
  };
  return sampled_chunks(h, tm, (size_t)n_rep, C, seed_y, n_trials, Y, out, upload, [&](size_t s0, int c) -> int {
    a.counts = out[0].as<unsigned long long>(); a.byrep = out[1].as<unsigned long long>();
    a.seed_x = (unsigned long long)seed_x + (unsigned long long)s0;   // (mod 2^64)
    const dim3 gr(grid.x, grid.y, (unsigned)c);
    if (hist) hipLaunchKernelGGL(k_rep<true>, gr, dim3(256), smem, h->stream, a);
    else hipLaunchKernelGGL(k_rep<false>, gr, dim3(256), 0, h->stream, a);
    HIPCHK(h, hipGetLastError());
    return VMR_OK;
  });
}

extern "C" int vmr_ppc_observed(vmr_handle h, uint64_t* counts, uint64_t* by_reporter) {
  if (!h) return VMR_EINVAL;
  if (!counts) return fail(h, VMR_EINVAL, "vmr_ppc_observed: counts is NULL");
  if (!h->have_state) return fail(h, VMR_ESTATE, "vmr_set_state must be called before vmr_ppc_observed");
  HIPCHK(h, hipSetDevice(h->device));
  const Geo& g = h->g;
  const size_t T = (size_t)g.N * g.N, LM = (size_t)g.L * g.M;
  Tmp tm(h);
  int rc;
  unsigned long long *cd = nullptr, *bd = nullptr;
  if ((rc = tm.get(&cd, (size_t)g.L * VMR_PPC_NSTAT * 8, "the observed statistics"))) return rc;
  if (by_reporter && (rc = tm.get(&bd, LM * 16, "the observed statistics by reporter"))) return rc;
  HIPCHK(h, hipMemsetAsync(cd, 0, (size_t)g.L * VMR_PPC_NSTAT * 8, h->stream));
  if (bd) HIPCHK(h, hipMemsetAsync(bd, 0, LM * 16, h->stream));
  const int G = pow2_lanes((unsigned)g.M);
  const bool hist = by_reporter && g.M <= PR_HIST_M;
  const size_t smem = hist ? (size_t)g.M * 16 : 0;
  for (int l = 0; l < g.L; ++l) {
    LayerPrep lp;
    if ((rc = ppc_prep_layer(h, tm, l, false, false, lp, true))) return rc;
    unsigned long long* bl = bd ? bd + (size_t)l * g.M * 2 : nullptr;
    if (hist) hipLaunchKernelGGL(k_obs<true>, dim3(walk_blocks(T, 256, G, PR_SLOTS)), dim3(256), smem, h->stream, lp.p, G, cd + (size_t)l * VMR_PPC_NSTAT, bl);
    else hipLaunchKernelGGL(k_obs<false>, dim3(walk_blocks(T, 256, G, PR_SLOTS)), dim3(256), 0, h->stream, lp.p, G, cd + (size_t)l * VMR_PPC_NSTAT, bl);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    ppc_release_layer(tm, lp);
  }
  HIPCHK(h, hipMemcpyAsync(counts, cd, (size_t)g.L * VMR_PPC_NSTAT * 8, hipMemcpyDeviceToHost, h->stream));
  if (bd) HIPCHK(h, hipMemcpyAsync(by_reporter, bd, LM * 16, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return VMR_OK;
}
