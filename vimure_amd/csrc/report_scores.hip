// report_scores.hip -- every report of the support scored under the posterior, where rho lives: vmr_report_scores_size,
// vmr_report_scores (include/vimure_hip.h states the values, the order, the outputs and every refusal).
//
// The per-report counterpart of vmr_reporter_table: which (l,i,j,m) hold a count, or a zero, that the fitted model finds
// improbable.  The likelihood is vmr_heldout_loglik's (report_lik.h: the same device functions), evaluated not over a list the
// caller writes down (24 B per entry) but over the support itself, by the support walk and its count-and-fill driver
// (read_side.h: support_walk, walk_count_fill); only integer histograms, a few sums and the rows worth reading leave the pass.
//   k_rs_walk<.., FILL = false>   the count pass.  Per support element: logp and mean; every element goes into the histogram of
//                 s = -logp (LDS bins, flushed once per workgroup by integer atomics; global integer atomics where they do not
//                 fit), into the lane's four sums and four counts (LikAcc); a flagged element into its reporter's bin.
//   k_rs_walk<.., FILL = true>    the fill pass: logp and mean of the flagged elements beside the walk's six integer columns.
//   k_lik_finish  adds a layer's per-workgroup partial sums and counts in index order.
// Determinism: a workgroup owns a fixed contiguous range of RS_SLOTS ties per group; a lane adds its elements in walk order, the
// waves fold by shuffles, the workgroup in LDS, k_lik_finish in index order: the tree depends on T and G alone.  Everything else
// is an integer.  No floating-point atomic, no ticket: all outputs are bit-identical from run to run.
// K <= KMAX: lik_eval_lane, as k_ho_lane (heldout.hip).  K > KMAX: a lane plays the HO_G lanes of k_ho_group one after another --
// category k into pair k mod HO_G in ascending k, then the pairs folded by the butterfly as lane 0 of the group sees it -- the
// same operations on the same operands, so the same bits.
#include "report_lik.h"

namespace {

#define RS_TPB 256
#define RS_SLOTS 64          // ties a group walks per workgroup
#define RS_G 16              // HO_G of heldout.hip: the pairs a row of K > KMAX categories is folded through
#define RS_LDS_MAX (128u << 10)   // dynamic LDS of the count pass at most (gfx950: 160 KB per workgroup)

static_assert(VMR_RS_NSUM == LIK_N && VMR_RS_NCOUNT == LIK_N && RS_TPB == LIK_TPB, "LikAcc, k_lik_finish");

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

// The walk over the ties [blockIdx.x * gpb * RS_SLOTS, ..) of one layer; KC: 2, 0 (any K <= KMAX) or -1 (K > KMAX).
template <int KC, bool FILL>
__global__ __launch_bounds__(RS_TPB) void k_rs_walk(PpcLayer p, int G, RsArgs a) {
  extern __shared__ u64 rs_lds[];   // count pass: [M][2] reporters' bins (byrep_lds), then [n_edges + 1][2] histogram (hist_lds)
  __shared__ double red[16];
  __shared__ u64 redu[16];
  const int n_hist = 2 * (a.n_edges + 1), n_rep = 2 * p.M;
  const WalkBins o = walk_bins<FILL>(rs_lds, n_rep, n_hist, a.byrep_lds, a.hist_lds, a.byrep, a.hist, RS_TPB);
  LikAcc acc;
  double lp = 0.0, mn = 0.0;
  support_walk<FILL, RS_TPB, RS_SLOTS>(
      p, G, a, [](const double*) {},
      [&](const double* row, unsigned m, int x, int xt) {
        if (KC >= 0) lik_eval_lane<(KC > 0 ? KC : 0)>(p.K, row, a.th[m], a.la, a.eta, x, xt, a.lgt, lp, mn);
        else rs_eval_wide(p.K, row, a.th[m], a.la, a.eta, x, xt, a.lgt, lp, mn);
        const double s = -lp;
        const int cl = x > 0 ? 0 : 1;   // a report, an omission
        const bool flag = (a.select & (cl == 0 ? VMR_RS_REPORTS : VMR_RS_OMISSIONS)) != 0 && s >= a.threshold;
        if (!FILL) {
          LIK_TAKE(acc, lp, mn, x, flag, a.bad);
          if (o.hist) atomicAdd(o.hist + 2 * (size_t)edge_bin(a.edges, a.n_edges, s) + cl, 1ull);
          if (flag && o.rep) atomicAdd(o.rep + 2 * (size_t)m + cl, 1ull);
        }
        return flag;
      },
      [&](u64 at) {
        if (a.logp) a.logp[at] = lp;
        if (a.mean) a.mean[at] = mn;
      });
  if (FILL) return;
  lik_flush(acc, a.part, a.cpart, red, redu);
  walk_bins_flush(rs_lds, n_rep, n_hist, a.byrep_lds, a.hist_lds, a.byrep, a.hist, RS_TPB);
}

template <bool FILL>
static int rs_launch(vmr_ctx* h, const PpcLayer& p, int G, const RsArgs& a, unsigned nb, size_t smem) {
  return launch_by_k(h, p.K, nb, RS_TPB, smem, [](auto kc) { return k_rs_walk<decltype(kc)::value, FILL>; }, p, G, a);
}

// What both entry points share.  rows: the table is asked for (n its capacity); n_out: the row count, or null.
static int rs_run(vmr_ctx* h, const char* fn, int layer, const double* theta, const double* lambda, double eta, int select, double threshold,
                  int n_edges, const double* edges, uint64_t* hist, double* sums, uint64_t* counts, uint64_t* by_reporter, bool rows,
                  uint64_t n, int32_t* const* sub /* sl si sj sm x xt */, double* logp, double* mean, int out_on_device, uint64_t* n_out) {
  auto bad_arg = [&](const char* what) { return fail(h, VMR_EINVAL, (std::string(fn) + ": " + what).c_str()); };
  if (!theta || !lambda) return bad_arg("theta or lambda is NULL");
  const Geo& g = h->g;
  const int L = g.L, M = g.M, K = g.K;
  if (!table_nonneg(theta, (size_t)L * M)) return bad_arg("theta must be finite and non-negative");
  if (!table_nonneg(lambda, (size_t)L * K)) return bad_arg("lambda must be finite and non-negative");
  if (!table_nonneg(&eta, 1)) return bad_arg("eta must be finite and non-negative");
  if (select < 1 || select > 3) return bad_arg("select must be VMR_RS_REPORTS, VMR_RS_OMISSIONS or both (1, 2 or 3)");
  if (threshold != threshold || threshold == -INFINITY) return bad_arg("the threshold must be finite or +inf");
  if (layer >= L) return bad_arg("layer out of range");
  if (const char* why = hist_refusal(hist, n_edges, VMR_RS_MAX_EDGES, "n_edges must lie in [0, VMR_RS_MAX_EDGES]", edges)) return bad_arg(why);
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

  const size_t n_rep = by_reporter ? 2 * (size_t)M : 0;
  const WalkShape ws = walk_shape(h, RS_TPB, RS_SLOTS, hist != nullptr, n_edges, n_rep, RS_LDS_MAX);
  const int G = ws.G;
  const unsigned nb = ws.nb;
  const size_t n_hist = ws.n_hist, smem = ws.smem;

  Tmp tm(h);
  int rc, b = 0;
  double *par_d = nullptr, *part = nullptr, *sums_d = nullptr;
  u64 *cpart = nullptr, *counts_d = nullptr, *hist_d = nullptr, *rep_d = nullptr;
  std::vector<u64> counts_h((size_t)Lq * VMR_RS_NCOUNT);
  RsArgs a;
  memset(&a, 0, sizeof a);
  if ((rc = tm.get(&a.bad, 4, "a flag")) || (rc = tm.get(&par_d, n_par * 8, "the parameter tables")) ||
      (rc = tm.get(&part, (size_t)nb * VMR_RS_NSUM * 8, "the partial sums")) || (rc = tm.get(&cpart, (size_t)nb * VMR_RS_NCOUNT * 8, "the partial counts")) ||
      (rc = tm.get(&sums_d, (size_t)Lq * VMR_RS_NSUM * 8, "the sums")) || (rc = tm.get(&counts_d, (size_t)Lq * VMR_RS_NCOUNT * 8, "the counts")) ||
      (rc = tm.get(&hist_d, (size_t)Lq * n_hist * 8, "the histogram")) || (rc = tm.get(&rep_d, (size_t)Lq * n_rep * 8, "the reporters' bins")))
    return rc;
  HIPCHK(h, hipMemcpyAsync(par_d, par_h.data(), n_par * 8, hipMemcpyHostToDevice, h->stream));
  if (n_hist) HIPCHK(h, hipMemsetAsync(hist_d, 0, (size_t)Lq * n_hist * 8, h->stream));
  if (n_rep) HIPCHK(h, hipMemsetAsync(rep_d, 0, (size_t)Lq * n_rep * 8, h->stream));
  a.lgt = par_d + o_lg;
  a.edges = hist ? par_d + o_ed : nullptr;
  a.part = part; a.cpart = cpart;
  a.eta = eta; a.threshold = threshold; a.select = select; a.n_edges = n_edges;
  a.hist_lds = ws.hist_lds; a.byrep_lds = ws.rep_lds;
  auto tables = [&](int l) {
    a.th = par_d + (size_t)l * M;
    a.la = par_d + o_la + (size_t)l * K;
  };
  double* const dbl[2] = {logp, mean};
  const WalkTable w = {rows, n, sub, dbl, 2, out_on_device, n_out};
  rc = walk_count_fill(
      h, fn, tm, l0, l1, w, a, b,
      [&](int l, const PpcLayer& p) -> int {
        tables(l);
        a.hist = hist ? hist_d + (size_t)(l - l0) * n_hist : nullptr;
        a.byrep = by_reporter ? rep_d + (size_t)(l - l0) * n_rep : nullptr;
        const int rc = rs_launch<false>(h, p, G, a, nb, smem);
        if (rc) return rc;
        hipLaunchKernelGGL(k_lik_finish, dim3(1), dim3(RS_TPB), 0, h->stream, (const double*)part, (const u64*)cpart, (size_t)nb,
                           sums_d + (size_t)(l - l0) * VMR_RS_NSUM, counts_d + (size_t)(l - l0) * VMR_RS_NCOUNT);
        HIPCHK(h, hipGetLastError());
        return VMR_OK;
      },
      [&](u64* flagged) -> int {
        HIPCHK(h, hipMemcpy(counts_h.data(), counts_d, counts_h.size() * 8, hipMemcpyDeviceToHost));
        for (int q = 0; q < Lq; ++q) flagged[q] = counts_h[(size_t)q * VMR_RS_NCOUNT + 3];
        return VMR_OK;
      },
      [&](int l, const PpcLayer& p, double* const* d64) -> int {
        tables(l);
        a.hist = nullptr; a.byrep = nullptr; a.edges = nullptr; a.n_edges = 0; a.hist_lds = 0; a.byrep_lds = 0;
        a.logp = d64[0]; a.mean = d64[1];
        return rs_launch<true>(h, p, G, a, nb, 0);
      });
  if (rc) return rc;
  if (hist) HIPCHK(h, hipMemcpyAsync(hist, hist_d, (size_t)Lq * n_hist * 8, hipMemcpyDeviceToHost, h->stream));
  if (by_reporter) HIPCHK(h, hipMemcpyAsync(by_reporter, rep_d, (size_t)Lq * n_rep * 8, hipMemcpyDeviceToHost, h->stream));
  if (sums) HIPCHK(h, hipMemcpyAsync(sums, sums_d, (size_t)Lq * VMR_RS_NSUM * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (counts) memcpy(counts, counts_h.data(), counts_h.size() * 8);
  if (b & WALK_BAD_NAN) return fail(h, VMR_ENAN, (std::string(fn) + ": a logp or a mean is NaN").c_str());
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
