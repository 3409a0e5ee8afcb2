// report_scores.hip -- every report of the support scored under the posterior, where rho lives: vmr_report_scores_size,
// vmr_report_scores (include/vimure_hip.h states the values, the order, the outputs and every refusal).
//
// The per-report counterpart of vmr_reporter_table: which (l,i,j,m) hold a count, or a zero, that the fitted model finds
// improbable.  The likelihood is vmr_heldout_loglik's (report_lik.h: the same device functions), evaluated not over a list the
// caller writes down (24 B per entry) but over the support itself, walked as k_ppc_walk (ppc.hip) walks it; only integer
// histograms, a few sums and the rows worth reading leave the pass.
//   k_rs_walk<.., FILL = false>   the count pass.  A group of G lanes per tie takes the tie's support reporters in ascending m, G at
//                 a time: x from the dense row or the tie-major index, xt from the mirror tie's, the tie's rho row, logp and mean.
//                 Every element goes into the histogram of s = -logp (LDS bins, flushed once per workgroup by integer atomics;
//                 global integer atomics where they do not fit), into the lane's four sums and four counts; a flagged element
//                 into its reporter's bin and into the tie's flagged count cnt[t].
//   (scan)        exclusive 64-bit sum of cnt: a tie's first row.
//   k_rs_walk<.., FILL = true>    the fill pass, only when rows are asked for and only over ties that hold one: the same walk, a
//                 flagged element written at its tie's offset plus its ballot rank inside the group -- lexicographic order, no atomics.
//   k_rs_finish   adds a layer's per-workgroup partial sums and counts in index order.
// Determinism: a workgroup owns a fixed contiguous range of RS_SLOTS ties per group; a lane adds its elements in walk order, the
// waves fold by shuffles, the workgroup in LDS, k_rs_finish in index order: the tree depends on T and G alone.  Everything else
// is an integer.  No floating-point atomic, no ticket: all outputs are bit-identical from run to run.
// K <= KMAX: the statements of k_ho_lane (heldout.hip).  K > KMAX: a lane plays the HO_G lanes of k_ho_group one after another --
// category k into pair k mod HO_G in ascending k, then the pairs folded by the butterfly as lane 0 of the group sees it -- the
// same operations on the same operands, so the same bits.
#include "vmr_internal.h"
#include "ppc_layer.h"
#include "rho_row.h"
#include "report_lik.h"

namespace {

#define RS_TPB 256
#define RS_SLOTS 64          // ties a group walks per workgroup
#define RS_G 16              // HO_G of heldout.hip: the pairs a row of K > KMAX categories is folded through
#define RS_LDS_MAX (128u << 10)   // dynamic LDS of the count pass at most (gfx950: 160 KB per workgroup)

// flag bits
#define RS_BAD_NAN 1
#define RS_BAD_WALK 2

typedef unsigned long long u64;
static_assert(VMR_RS_NSUM == 4 && VMR_RS_NCOUNT == 4, "RsAcc, k_rs_finish");

struct RsArgs {
  const double *th, *la, *lgt;   // theta [M] and lambda [K] of the layer, lgamma(x + 1) [HO_LGT]
  double eta, threshold;
  int select, n_edges;
  const double* edges;           // [n_edges], or null: no histogram
  u64* hist;                     // [n_edges + 1][2] of the layer, or null
  u64* byrep;                    // [M][2] of the layer, or null
  int hist_lds, byrep_lds;       // bins in LDS first
  u64* cnt;                      // count pass: [T] flagged elements of a tie; fill pass: [T + 1] its exclusive sum
  double* part;                  // [workgroups][VMR_RS_NSUM]
  u64* cpart;                    // [workgroups][VMR_RS_NCOUNT]
  // fill pass
  u64 lim;                       // rows of the layer
  int32_t *sl, *si, *sj, *sm, *x, *xt;
  double *logp, *mean;
  int* bad;
};

struct RsAcc {
  double s[VMR_RS_NSUM];
  u64 c[VMR_RS_NCOUNT];
};

// logp and mean of one element: K <= KMAX, the row in registers (k_ho_lane's statements)
template <int KC>
__device__ __forceinline__ void rs_eval_lane(int Kp, const double* __restrict__ row, double thm, const double* __restrict__ la, double eta,
                                             int x, int xt, const double* __restrict__ lgt, double& lp, double& mn) {
  const int K = KC ? KC : Kp;
  double r[KMAX], b[KMAX];
  if (KC == 2) {
    const double2 v = *reinterpret_cast<const double2*>(row);   // (rho is 256-byte aligned, a row of two doubles 16-byte)
    r[0] = v.x; r[1] = v.y;
  } else {
#pragma unroll
    for (int k = 0; k < KMAX; ++k) if (k < K) r[k] = row[k];
  }
  const double exy = eta * (double)xt, xd = (double)x;
  double mx = -INFINITY;
  bool nan_seen = false;
  mn = 0.0;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) {
      const double mu = ho_rate(thm, la[k], exy);
      mn = ho_add(mn, ho_mul(r[k], mu));
      b[k] = ho_term(r[k], mu, xd, x > 0);
      nan_seen = nan_seen || b[k] != b[k];
      if (b[k] > mx) mx = b[k];
    }
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K && b[k] > -INFINITY) s += exp(b[k] - mx);
  if (nan_seen) s = __builtin_nan("");
  lp = ho_logp(mx, s, ho_lgam1((unsigned)x, lgt));
}

// K > KMAX: the RS_G running pairs of k_ho_group, kept by one lane, folded as its lane 0 folds them
__device__ __forceinline__ void rs_eval_wide(int K, const double* __restrict__ row, double thm, const double* __restrict__ la, double eta,
                                             int x, int xt, const double* __restrict__ lgt, double& lp, double& mn) {
  const double exy = eta * (double)xt, xd = (double)x;
  double mx[RS_G], s[RS_G];
#pragma unroll
  for (int g = 0; g < RS_G; ++g) { mx[g] = -INFINITY; s[g] = 0.0; }
  mn = 0.0;
  for (int k0 = 0; k0 < K; k0 += RS_G) {
#pragma unroll
    for (int g = 0; g < RS_G; ++g) {
      const int k = k0 + g;
      if (k < K) {
        const double r = row[k], mu = ho_rate(thm, la[k], exy);
        mn = ho_add(mn, ho_mul(r, mu));
        const double b = ho_term(r, mu, xd, x > 0);
        if (b != b) s[g] = b;
        else if (b > -INFINITY) ho_fold(mx[g], s[g], b, 1.0);
      }
    }
  }
#pragma unroll
  for (int w = RS_G >> 1; w > 0; w >>= 1) {
#pragma unroll
    for (int g = 0; g < RS_G; ++g)
      if (g < w) ho_fold(mx[g], s[g], mx[g + w], s[g + w]);
  }
  lp = ho_logp(mx[0], s[0], ho_lgam1((unsigned)x, lgt));
}

__device__ __forceinline__ u64 rs_block_sum_u(u64 v, u64* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (u64)__shfl_xor((long long)v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  u64 r = 0;
  if (threadIdx.x == 0)
    for (unsigned w = 0; w < (blockDim.x >> 6); ++w) r += red[w];
  return r;
}

// c = #{tau : edges[tau] <= s}; a NaN lands in bin 0 (the call then ends in VMR_ENAN)
__device__ __forceinline__ int rs_bin(const double* __restrict__ edges, int n, double s) {
  int a = 0, b = n;
  while (a < b) { const int c = a + ((b - a) >> 1); if (edges[c] <= s) a = c + 1; else b = c; }
  return a;
}

// The walk over the ties [blockIdx.x * gpb * RS_SLOTS, ..) of one layer; KC: 2, 0 (any K <= KMAX) or -1 (K > KMAX).
template <int KC, bool FILL>
__global__ __launch_bounds__(RS_TPB) void k_rs_walk(PpcLayer p, int G, RsArgs a) {
  extern __shared__ u64 rs_lds[];   // count pass: [M][2] reporters' bins (byrep_lds), then [n_edges + 1][2] histogram (hist_lds)
  __shared__ double red[16];
  __shared__ u64 redu[16];
  u64* const lds_rep = rs_lds;
  u64* const lds_hist = rs_lds + (a.byrep_lds ? 2 * (size_t)p.M : 0);
  const int n_hist = 2 * (a.n_edges + 1);
  if (!FILL) {
    const int n_lds = (a.byrep_lds ? 2 * p.M : 0) + (a.hist_lds ? n_hist : 0);
    for (int q = threadIdx.x; q < n_lds; q += RS_TPB) rs_lds[q] = 0ull;
    __syncthreads();
  }
  u64* const o_rep = a.byrep_lds ? lds_rep : a.byrep;
  u64* const o_hist = a.hist_lds ? lds_hist : a.hist;
  const int lane = threadIdx.x & 63, gl = lane & (G - 1), g0 = lane - gl;
  const u64 gmask = (G == 64 ? ~0ull : ((1ull << G) - 1ull)) << g0, lt = (1ull << lane) - 1ull;
  const size_t gpb = RS_TPB / G;
  const bool words = p.rq == nullptr;
  RsAcc acc;
#pragma unroll
  for (int c = 0; c < VMR_RS_NSUM; ++c) { acc.s[c] = 0.0; acc.c[c] = 0ull; }
  const size_t t_lim = ((size_t)blockIdx.x + 1) * gpb * RS_SLOTS, t_end = t_lim < p.T ? t_lim : p.T;
  for (size_t t = (size_t)blockIdx.x * gpb * RS_SLOTS + threadIdx.x / G; t < t_end; t += gpb) {   // (uniform over the group)
    const int c = p.cls[t];
    u64 o_t = 0;
    if (FILL) {
      o_t = a.cnt[t];
      if (c == 0 || a.cnt[t + 1] == o_t) continue;   // no row of this tie
    } else if (c == 0) {
      continue;                                      // (cnt comes zeroed)
    }
    const bool listed = c == 2 && !words, bits = c == 2 && words;
    const unsigned nc = listed ? p.rq[t + 1] - p.rq[t] : (unsigned)p.M;
    const unsigned short* lst = listed ? p.Rm + p.rq[t] : nullptr;
    const size_t i = t / p.N, j = t - i * p.N, tm = j * p.N + i;
    const double* row = p.rho + (p.inv ? (size_t)p.inv[t] : t) * p.K;
    u64 jf = 0;
    for (unsigned c0 = 0; c0 < nc; c0 += (unsigned)G) {
      const unsigned q = c0 + (unsigned)gl;
      const unsigned m = listed ? (q < nc ? (unsigned)lst[q] : 0u) : q;
      const bool in = q < nc && m < (unsigned)p.M && (!bits || ((p.Rb[t * p.W + (m >> 6)] >> (m & 63)) & 1ull));
      bool flag = false;
      int x = 0, xt = 0;
      double lp = 0.0, mn = 0.0;
      if (in) {
        x = (int)ppc_x(p, t, m);
        if (p.mut) xt = (int)ppc_x(p, tm, m);
        if (KC >= 0) rs_eval_lane<(KC > 0 ? KC : 0)>(p.K, row, a.th[m], a.la, a.eta, x, xt, a.lgt, lp, mn);
        else rs_eval_wide(p.K, row, a.th[m], a.la, a.eta, x, xt, a.lgt, lp, mn);
        const double s = -lp;
        const int cl = x > 0 ? 0 : 1;   // a report, an omission
        flag = (a.select & (cl == 0 ? VMR_RS_REPORTS : VMR_RS_OMISSIONS)) != 0 && s >= a.threshold;
        if (!FILL) {
          if (lp != lp || mn != mn) atomicOr(a.bad, RS_BAD_NAN);
          const double xd = (double)x, d = xd - mn;
          if (lp == -INFINITY) acc.c[2] += 1ull; else acc.s[0] += lp;
          acc.s[1] += d * d;
          acc.s[2] += xd;
          acc.s[3] += mn;
          acc.c[0] += 1ull;
          acc.c[1] += x > 0 ? 1ull : 0ull;
          acc.c[3] += flag ? 1ull : 0ull;
          if (o_hist) atomicAdd(o_hist + 2 * (size_t)rs_bin(a.edges, a.n_edges, s) + cl, 1ull);
          if (flag && o_rep) atomicAdd(o_rep + 2 * (size_t)m + cl, 1ull);
        }
      }
      const u64 bf = __ballot(flag) & gmask;
      if (FILL && flag) {
        const u64 at = o_t + jf + (u64)__popcll(bf & lt);
        if (at >= a.lim) {
          atomicOr(a.bad, RS_BAD_WALK);   // (the count pass and the fill pass disagree: never written out of bounds)
        } else {
          if (a.sl) a.sl[at] = p.l;
          if (a.si) a.si[at] = (int32_t)i;
          if (a.sj) a.sj[at] = (int32_t)j;
          if (a.sm) a.sm[at] = (int32_t)m;
          if (a.x) a.x[at] = x;
          if (a.xt) a.xt[at] = xt;
          if (a.logp) a.logp[at] = lp;
          if (a.mean) a.mean[at] = mn;
        }
      }
      jf += (u64)__popcll(bf);
    }
    if (!FILL && gl == 0) a.cnt[t] = jf;
  }
  if (FILL) return;
#pragma unroll
  for (int c = 0; c < VMR_RS_NSUM; ++c) {
    const double v = block_sum_n(acc.s[c], red);
    if (threadIdx.x == 0) a.part[(size_t)blockIdx.x * VMR_RS_NSUM + c] = v;
  }
#pragma unroll
  for (int c = 0; c < VMR_RS_NCOUNT; ++c) {
    const u64 v = rs_block_sum_u(acc.c[c], redu);
    if (threadIdx.x == 0) a.cpart[(size_t)blockIdx.x * VMR_RS_NCOUNT + c] = v;
  }
  __syncthreads();
  if (a.byrep_lds)
    for (int q = threadIdx.x; q < 2 * p.M; q += RS_TPB) { const u64 u = lds_rep[q]; if (u) atomicAdd(a.byrep + q, u); }
  if (a.hist_lds)
    for (int q = threadIdx.x; q < n_hist; q += RS_TPB) { const u64 u = lds_hist[q]; if (u) atomicAdd(a.hist + q, u); }
}

// one workgroup adds a layer's nb partials, column by column, in index order
__global__ __launch_bounds__(RS_TPB) void k_rs_finish(const double* __restrict__ part, const u64* __restrict__ cpart, size_t nb,
                                                      double* __restrict__ sums, u64* __restrict__ counts) {
  __shared__ double red[16];
  __shared__ u64 redu[16];
  for (int c = 0; c < VMR_RS_NSUM; ++c) {
    double v = 0.0;
    for (size_t b = threadIdx.x; b < nb; b += RS_TPB) v += part[b * VMR_RS_NSUM + c];
    const double t = block_sum_n(v, red);
    if (threadIdx.x == 0) sums[c] = t;
  }
  for (int c = 0; c < VMR_RS_NCOUNT; ++c) {
    u64 v = 0;
    for (size_t b = threadIdx.x; b < nb; b += RS_TPB) v += cpart[b * VMR_RS_NCOUNT + c];
    const u64 t = rs_block_sum_u(v, redu);
    if (threadIdx.x == 0) counts[c] = t;
  }
}

static bool rs_table_ok(const double* v, size_t n) {
  for (size_t q = 0; q < n; ++q)
    if (!(v[q] >= 0.0 && v[q] <= 1.79769313486231570815e308)) return false;
  return true;
}

// lanes per tie: a support row holds up to M reporters (group_lanes of ppc.hip)
static int rs_lanes(const vmr_ctx* h) {
  int G = 1;
  while (G < 64 && G < h->g.M) G <<= 1;
  return G;
}

template <bool FILL>
static int rs_launch(vmr_ctx* h, const PpcLayer& p, int G, const RsArgs& a, unsigned nb, size_t smem) {
  const int K = p.K;
  auto go = [&](auto kern) -> int {
    if (smem > 48 * 1024) HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL(kern, dim3(nb), dim3(RS_TPB), smem, h->stream, p, G, a);
    HIPCHK(h, hipGetLastError());
    return VMR_OK;
  };
  if (K == 2) return go(k_rs_walk<2, FILL>);
  if (K <= KMAX) return go(k_rs_walk<0, FILL>);
  return go(k_rs_walk<-1, FILL>);
}

// What both entry points share.  rows: the table is asked for (n its capacity); n_out: the row count, or null.
static int rs_run(vmr_ctx* h, const char* fn, int layer, const double* theta, const double* lambda, double eta, int select, double threshold,
                  int n_edges, const double* edges, uint64_t* hist, double* sums, uint64_t* counts, uint64_t* by_reporter, bool rows,
                  uint64_t n, int32_t* const* sub /* sl si sj sm x xt */, double* logp, double* mean, int out_on_device, uint64_t* n_out) {
  auto bad_arg = [&](const char* what) { return fail(h, VMR_EINVAL, (std::string(fn) + ": " + what).c_str()); };
  if (!theta || !lambda) return bad_arg("theta or lambda is NULL");
  const Geo& g = h->g;
  const int L = g.L, M = g.M, K = g.K;
  if (!rs_table_ok(theta, (size_t)L * M)) return bad_arg("theta must be finite and non-negative");
  if (!rs_table_ok(lambda, (size_t)L * K)) return bad_arg("lambda must be finite and non-negative");
  if (!rs_table_ok(&eta, 1)) return bad_arg("eta must be finite and non-negative");
  if (select < 1 || select > 3) return bad_arg("select must be VMR_RS_REPORTS, VMR_RS_OMISSIONS or both (1, 2 or 3)");
  if (threshold != threshold || threshold == -INFINITY) return bad_arg("the threshold must be finite or +inf");
  if (layer >= L) return bad_arg("layer out of range");
  if (n_edges < 0 || n_edges > VMR_RS_MAX_EDGES) return bad_arg("n_edges must lie in [0, VMR_RS_MAX_EDGES]");
  if (hist && n_edges > 0 && !edges) return bad_arg("hist is asked for and edges is NULL");
  if (hist)
    for (int q = 0; q < n_edges; ++q)
      if (!(edges[q] >= -1.79769313486231570815e308 && edges[q] <= 1.79769313486231570815e308) || (q && edges[q] < edges[q - 1]))
        return bad_arg("the edges must be finite and non-decreasing");
  if (!h->have_state) return fail(h, VMR_ESTATE, (std::string("vmr_set_state must be called before ") + fn).c_str());
  const size_t T = (size_t)g.N * g.N;
  if (T >= 0x7fffffffull) return bad_arg("2^31 ties or more in one layer");
  HIPCHK(h, hipSetDevice(h->device));
  { const int rce = ensure_rho_ext(h); if (rce) return rce; }
  const int l0 = layer < 0 ? 0 : layer, l1 = layer < 0 ? L : layer + 1, Lq = l1 - l0;
  if (!hist) n_edges = 0;

  // the caller's tables, the lgamma table and the edges, one upload: theta [L][M], lambda [L][K], lgamma(x + 1) [HO_LGT], edges
  const size_t o_la = (size_t)L * M, o_lg = o_la + (size_t)L * K, o_ed = o_lg + HO_LGT, n_par = o_ed + (size_t)n_edges;
  std::vector<double> par_h(n_par);
  memcpy(par_h.data(), theta, (size_t)L * M * 8);
  memcpy(par_h.data() + o_la, lambda, (size_t)L * K * 8);
  ho_lgt_fill(par_h.data() + o_lg);
  if (n_edges) memcpy(par_h.data() + o_ed, edges, (size_t)n_edges * 8);

  const int G = rs_lanes(h);
  const size_t per = (size_t)(RS_TPB / G) * RS_SLOTS;
  const unsigned nb = (unsigned)((T + per - 1) / per);
  const size_t n_hist = hist ? 2 * ((size_t)n_edges + 1) : 0, n_rep = by_reporter ? 2 * (size_t)M : 0;
  const bool rep_lds = by_reporter && M <= PR_HIST_M;
  const bool hist_lds = hist && ((rep_lds ? n_rep : 0) + n_hist) * 8 <= RS_LDS_MAX;
  const size_t smem = ((rep_lds ? n_rep : 0) + (hist_lds ? n_hist : 0)) * 8;

  Tmp tm(h);
  int rc;
  int* bad = nullptr;
  double *par_d = nullptr, *part = nullptr, *sums_d = nullptr;
  u64 *cpart = nullptr, *counts_d = nullptr, *hist_d = nullptr, *rep_d = nullptr, *cnt = nullptr, *off = nullptr;
  void* ts = nullptr;
  size_t tb = 0;
  if ((rc = tm.get(&bad, 4, "a flag")) || (rc = tm.get(&par_d, n_par * 8, "the parameter tables")) ||
      (rc = tm.get(&part, (size_t)nb * VMR_RS_NSUM * 8, "the partial sums")) || (rc = tm.get(&cpart, (size_t)nb * VMR_RS_NCOUNT * 8, "the partial counts")) ||
      (rc = tm.get(&sums_d, (size_t)Lq * VMR_RS_NSUM * 8, "the sums")) || (rc = tm.get(&counts_d, (size_t)Lq * VMR_RS_NCOUNT * 8, "the counts")) ||
      (rc = tm.get(&hist_d, (size_t)Lq * n_hist * 8, "the histogram")) || (rc = tm.get(&rep_d, (size_t)Lq * n_rep * 8, "the reporters' bins")) ||
      (rc = tm.get(&cnt, (T + 1) * 8, "the ties' flagged counts")))
    return rc;
  if (rows) {   // a tie's first row, every layer's: kept until the capacity is checked against all of them
    if ((rc = tm.get(&off, (size_t)Lq * (T + 1) * 8, "the ties' row offsets"))) return rc;
    HIPCHK(h, hipcub::DeviceScan::ExclusiveSum(nullptr, tb, cnt, off, (int)(T + 1), h->stream));
    if ((rc = tm.get(&ts, tb, "the scan of the flagged counts"))) return rc;
  }
  HIPCHK(h, hipMemcpyAsync(par_d, par_h.data(), n_par * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemsetAsync(bad, 0, 4, h->stream));
  if (n_hist) HIPCHK(h, hipMemsetAsync(hist_d, 0, (size_t)Lq * n_hist * 8, h->stream));
  if (n_rep) HIPCHK(h, hipMemsetAsync(rep_d, 0, (size_t)Lq * n_rep * 8, h->stream));

  RsArgs a;
  memset(&a, 0, sizeof a);
  a.lgt = par_d + o_lg;
  a.eta = eta; a.threshold = threshold; a.select = select; a.n_edges = n_edges;
  a.edges = hist ? par_d + o_ed : nullptr;
  a.hist_lds = hist_lds; a.byrep_lds = rep_lds;
  a.part = part; a.cpart = cpart; a.bad = bad;

  // the count pass, layer by layer
  for (int l = l0; l < l1; ++l) {
    LayerPrep lp;
    if ((rc = ppc_prep_layer(h, tm, l, false, true, lp, true, false))) return rc;
    a.th = par_d + (size_t)l * M;
    a.la = par_d + o_la + (size_t)l * K;
    a.hist = hist ? hist_d + (size_t)(l - l0) * n_hist : nullptr;
    a.byrep = by_reporter ? rep_d + (size_t)(l - l0) * n_rep : nullptr;
    a.cnt = cnt;
    HIPCHK(h, hipMemsetAsync(cnt, 0, (T + 1) * 8, h->stream));
    if ((rc = rs_launch<false>(h, lp.p, G, a, nb, smem))) return rc;
    hipLaunchKernelGGL(k_rs_finish, dim3(1), dim3(RS_TPB), 0, h->stream, (const double*)part, (const u64*)cpart, (size_t)nb,
                       sums_d + (size_t)(l - l0) * VMR_RS_NSUM, counts_d + (size_t)(l - l0) * VMR_RS_NCOUNT);
    HIPCHK(h, hipGetLastError());
    if (rows) HIPCHK(h, hipcub::DeviceScan::ExclusiveSum(ts, tb, cnt, off + (size_t)(l - l0) * (T + 1), (int)(T + 1), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    ppc_release_layer(tm, lp);
  }
  std::vector<u64> counts_h((size_t)Lq * VMR_RS_NCOUNT);
  int b = 0;
  HIPCHK(h, hipMemcpyAsync(counts_h.data(), counts_d, counts_h.size() * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(&b, bad, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  u64 total = 0;
  for (int q = 0; q < Lq; ++q) total += counts_h[(size_t)q * VMR_RS_NCOUNT + 3];
  if (n_out) *n_out = total;
  if (rows && n < total) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: the table holds %llu rows, %llu elements are flagged", fn, (unsigned long long)n, (unsigned long long)total);
    return fail(h, VMR_EINVAL, msg);
  }

  // the fill pass: the layers that hold a row
  if (rows && total && !(b & RS_BAD_NAN)) {
    u64 base = 0;
    for (int l = l0; l < l1; ++l) {
      const u64 nl = counts_h[(size_t)(l - l0) * VMR_RS_NCOUNT + 3];
      if (!nl) continue;
      LayerPrep lp;
      if ((rc = ppc_prep_layer(h, tm, l, false, true, lp, true, false))) return rc;
      a.th = par_d + (size_t)l * M;
      a.la = par_d + o_la + (size_t)l * K;
      a.hist = nullptr; a.byrep = nullptr; a.edges = nullptr; a.n_edges = 0; a.hist_lds = 0; a.byrep_lds = 0;
      a.cnt = off + (size_t)(l - l0) * (T + 1);
      a.lim = nl;
      int32_t* d32[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
      double* d64[2] = {nullptr, nullptr};
      double* h64[2] = {logp, mean};
      int32_t* st32 = nullptr;
      double* st64 = nullptr;
      if (out_on_device) {
        for (int q = 0; q < 6; ++q) d32[q] = sub[q] ? sub[q] + base : nullptr;
        for (int q = 0; q < 2; ++q) d64[q] = h64[q] ? h64[q] + base : nullptr;
      } else {   // host outputs: the layer's rows through device staging
        int n32 = 0, n64 = 0;
        for (int q = 0; q < 6; ++q) n32 += sub[q] != nullptr;
        for (int q = 0; q < 2; ++q) n64 += h64[q] != nullptr;
        if ((n32 && (rc = tm.get(&st32, (size_t)n32 * nl * 4, "the staging of the rows"))) ||
            (n64 && (rc = tm.get(&st64, (size_t)n64 * nl * 8, "the staging of the rows"))))
          return rc;
        for (int q = 0, u = 0; q < 6; ++q) if (sub[q]) d32[q] = st32 + (size_t)(u++) * nl;
        for (int q = 0, u = 0; q < 2; ++q) if (h64[q]) d64[q] = st64 + (size_t)(u++) * nl;
      }
      a.sl = d32[0]; a.si = d32[1]; a.sj = d32[2]; a.sm = d32[3]; a.x = d32[4]; a.xt = d32[5];
      a.logp = d64[0]; a.mean = d64[1];
      if ((rc = rs_launch<true>(h, lp.p, G, a, nb, 0))) return rc;
      if (!out_on_device) {
        for (int q = 0; q < 6; ++q)
          if (sub[q]) HIPCHK(h, hipMemcpyAsync(sub[q] + base, d32[q], (size_t)nl * 4, hipMemcpyDeviceToHost, h->stream));
        for (int q = 0; q < 2; ++q)
          if (h64[q]) HIPCHK(h, hipMemcpyAsync(h64[q] + base, d64[q], (size_t)nl * 8, hipMemcpyDeviceToHost, h->stream));
      }
      HIPCHK(h, hipStreamSynchronize(h->stream));
      if (st32) tm.release(st32);
      if (st64) tm.release(st64);
      ppc_release_layer(tm, lp);
      base += nl;
    }
    HIPCHK(h, hipMemcpyAsync(&b, bad, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (b & RS_BAD_WALK) return fail(h, VMR_EHIP, (std::string(fn) + ": the count pass and the fill pass disagree").c_str());
  }
  if (hist) HIPCHK(h, hipMemcpyAsync(hist, hist_d, (size_t)Lq * n_hist * 8, hipMemcpyDeviceToHost, h->stream));
  if (by_reporter) HIPCHK(h, hipMemcpyAsync(by_reporter, rep_d, (size_t)Lq * n_rep * 8, hipMemcpyDeviceToHost, h->stream));
  if (sums) HIPCHK(h, hipMemcpyAsync(sums, sums_d, (size_t)Lq * VMR_RS_NSUM * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (counts) memcpy(counts, counts_h.data(), counts_h.size() * 8);
  if (b & RS_BAD_NAN) return fail(h, VMR_ENAN, (std::string(fn) + ": a logp or a mean is NaN").c_str());
  return VMR_OK;
}

}  // namespace

extern "C" int vmr_report_scores_size(vmr_handle h, int layer, const double* theta, const double* lambda, double eta, int select,
                                      double threshold, uint64_t* n) {
  if (!h) return VMR_EINVAL;
  if (!n) return fail(h, VMR_EINVAL, "vmr_report_scores_size: n is NULL");
  int32_t* none[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  return rs_run(h, "vmr_report_scores_size", layer, theta, lambda, eta, select, threshold, 0, nullptr, nullptr, nullptr, nullptr, nullptr, false, 0,
                none, nullptr, nullptr, 0, n);
}

extern "C" int vmr_report_scores(vmr_handle h, int layer, const double* theta, const double* lambda, double eta, int select, double threshold,
                                 int n_edges, const double* edges, uint64_t* hist, double* sums, uint64_t* counts, uint64_t* by_reporter,
                                 uint64_t n, int32_t* sl, int32_t* si, int32_t* sj, int32_t* sm, int32_t* x, int32_t* xt, double* logp,
                                 double* mean, int out_on_device) {
  if (!h) return VMR_EINVAL;
  int32_t* sub[6] = {sl, si, sj, sm, x, xt};
  const bool any_row = sl || si || sj || sm || x || xt || logp || mean;
  if (!any_row && !hist && !sums && !counts && !by_reporter) return fail(h, VMR_EINVAL, "vmr_report_scores: every output is NULL");
  const bool rows = any_row || n != 0;   // (n = 0 and every row pointer NULL: no table pass)
  return rs_run(h, "vmr_report_scores", layer, theta, lambda, eta, select, threshold, n_edges, edges, hist, sums, counts, by_reporter, rows, n,
                sub, logp, mean, out_on_device, nullptr);
}
