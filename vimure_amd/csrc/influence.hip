// influence.hip -- whose word does an inferred tie rest on: the leave-one-reporter-out row of every element of the support, where
// rho lives: vmr_reporter_influence_size, vmr_reporter_influence (include/vimure_hip.h states the values, the order of every
// operation, the outputs and every refusal).
//
// The CAVI update of a tie's row is additive over the reporters of its mask: log rho_k = logpr_k + sum_m c_mk + const.  Dividing
// reporter m's factor exp(c_mk) out of the current row and normalising again gives the row the update would have produced without
// that reporter's word -- closed form, no refit.  The walk and its count-and-fill driver are the shared ones (read_side.h:
// support_walk, walk_count_fill); the arithmetic per element and what is reduced are this unit's:
//   k_inf_walk<.., FILL = false>  the count pass.  Per tie prob and the readout of its row; per support element the leave-one-out
//                 row q, and from it prob_loo, tv and the readout of q.  Every element goes into its reporter's six integer bins
//                 (n_scope, lost, gained, flagged, and tv and the shift prob_loo - prob in fixed point) and into the histogram of
//                 tv -- LDS bins, flushed once per workgroup by integer atomics; global integer atomics where they do not fit.
//   k_inf_walk<.., FILL = true>   the fill pass: prob, prob_loo and tv of the flagged elements beside the walk's six integer columns.
// Determinism: every accumulator is a 64-bit integer; the two sums are signed fixed point in 2^-(61 - b), b = ceil(log2 N^2) (the
// route of reporter_table.hip).  Integer adds commute; there is no floating-point atomic and no ticket.
// K = 2 and K <= KMAX keep the row and the exponents in registers; K > KMAX streams the row three times (maximum, sum, values)
// and forms every exponent again each time by the same operations, so the three variants give the same bits.
#include "read_side.h"

namespace {

#define INF_TPB 256
#define INF_SLOTS 64          // ties a group walks per workgroup
#define INF_NB 6              // bins per reporter: n_scope, lost, gained, flagged, sum tv, sum shift (fixed point)
#define INF_LDS_MAX (128u << 10)   // dynamic LDS of the count pass at most (gfx950: 160 KB per workgroup)

#define INF_BAD_RANGE 4       // flag bit, beside the walk's

static_assert(VMR_INF_NCOUNT == 4 && VMR_INF_NSUM == 2, "the bins of k_inf_walk");

struct InfArgs {
  const double *gth, *elt, *eth;   // exp(elog_theta), elog_theta, e_theta [M] of the layer
  const double *gla, *ell, *ela;   // exp(elog_lambda), elog_lambda, e_lambda [K] of the layer
  double gnu, threshold, min_tv;
  int method, select, n_edges, sh;
  const double* edges;           // [n_edges], or null: no histogram
  u64* hist;                     // [n_edges + 1][2] of the layer, or null
  u64* bins;                     // [M][INF_NB] of the layer
  int hist_lds, bins_lds;        // bins in LDS first
  u64* cnt;                      // count pass: [T] flagged elements of a tie; fill pass: [T + 1] its exclusive sum
  // fill pass
  u64 lim;                       // rows of the layer
  int32_t *sl, *si, *sj, *sm, *x, *xt;
  double *prob, *prob_loo, *tv;
  int* bad;
};

struct InfVal {
  double prob_loo, tv;
  unsigned y;   // the readout of q
};

// d_k = -c_k, the exponent that divides reporter m's factor out of category k: every product and every sum rounded on its own
__device__ __forceinline__ double inf_d(double gth, double gla, double gx, double elt, double ell, double eth, double ela, double xd) {
#pragma clang fp contract(off)
  const double z1 = gth * gla;
  double den = z1 + gx;
  if (den == 0.0) den = 1.0;
  const double w1 = z1 / den;
  const double xw = xd * w1;
  const double a = elt + ell;
  const double p1 = a * xw;
  const double p2 = eth * ela;
  const double c = p1 - p2;
  return -c;
}

// K <= KMAX: the row, the exponents and q in registers
template <int KC>
__device__ __forceinline__ InfVal inf_eval_lane(int Kp, const double* __restrict__ row, const InfArgs& a, unsigned m, int x, int xt) {
#pragma clang fp contract(off)
  const int K = KC ? KC : Kp;
  double r[KMAX], d[KMAX], q[KMAX];
  if (KC == 2) {
    const double2 v = *reinterpret_cast<const double2*>(row);   // (rho is 256-byte aligned, a row of two doubles 16-byte)
    r[0] = v.x; r[1] = v.y;
  } else {
#pragma unroll
    for (int k = 0; k < KMAX; ++k) if (k < K) r[k] = row[k];
  }
  const double gth = a.gth[m], elt = a.elt[m], eth = a.eth[m], xd = (double)x;
  const double gx = a.gnu * (double)xt;
  double mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K && r[k] > 0.0) {
      d[k] = inf_d(gth, a.gla[k], gx, elt, a.ell[k], eth, a.ela[k], xd);
      if (d[k] > mx) mx = d[k];
    }
  double S = 0.0;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) {
      q[k] = 0.0;
      if (r[k] > 0.0) { q[k] = r[k] * exp(d[k] - mx); S = S + q[k]; }
    }
  InfVal o;
  double pl = 0.0, t = 0.0, bv = 0.0;
  unsigned best = 0;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) {
      if (r[k] > 0.0) q[k] = q[k] / S;
      if (k == 0) bv = q[0];
      else { pl = pl + q[k]; if (q[k] > bv) { bv = q[k]; best = (unsigned)k; } }
      t = t + fabs(q[k] - r[k]);
    }
  o.prob_loo = pl;
  o.tv = 0.5 * t;
  o.y = a.method == VMR_READ_THRESHOLD ? (q[1] >= a.threshold ? 1u : 0u) : best;
  return o;
}

// K > KMAX: the row streamed -- the maximum, the sum, the values -- every exponent formed again by the same operations
__device__ __forceinline__ InfVal inf_eval_wide(int K, const double* __restrict__ row, const InfArgs& a, unsigned m, int x, int xt) {
#pragma clang fp contract(off)
  const double gth = a.gth[m], elt = a.elt[m], eth = a.eth[m], xd = (double)x;
  const double gx = a.gnu * (double)xt;
  double mx = -INFINITY;
  for (int k = 0; k < K; ++k)
    if (row[k] > 0.0) {
      const double d = inf_d(gth, a.gla[k], gx, elt, a.ell[k], eth, a.ela[k], xd);
      if (d > mx) mx = d;
    }
  double S = 0.0;
  for (int k = 0; k < K; ++k) {
    const double r = row[k];
    if (r > 0.0) {
      const double u = r * exp(inf_d(gth, a.gla[k], gx, elt, a.ell[k], eth, a.ela[k], xd) - mx);
      S = S + u;
    }
  }
  InfVal o;
  double pl = 0.0, t = 0.0, bv = 0.0, q1 = 0.0;
  unsigned best = 0;
  for (int k = 0; k < K; ++k) {
    const double r = row[k];
    double q = 0.0;
    if (r > 0.0) {
      const double u = r * exp(inf_d(gth, a.gla[k], gx, elt, a.ell[k], eth, a.ela[k], xd) - mx);
      q = u / S;
    }
    if (k == 0) bv = q;
    else { pl = pl + q; if (q > bv) { bv = q; best = (unsigned)k; } }
    if (k == 1) q1 = q;
    t = t + fabs(q - r);
  }
  o.prob_loo = pl;
  o.tv = 0.5 * t;
  o.y = a.method == VMR_READ_THRESHOLD ? (q1 >= a.threshold ? 1u : 0u) : best;
  return o;
}

// v, |v| <= 2, as a signed multiple of 2^-sh; NaN and values out of range are flagged and add nothing
__device__ __forceinline__ u64 inf_fx(double v, int sh, int* __restrict__ bad) {
  if (!(fabs(v) <= 2.0)) { atomicOr(bad, v != v ? WALK_BAD_NAN : INF_BAD_RANGE); return 0ull; }
  return det_fx(v, sh);
}

// The walk over the ties [blockIdx.x * gpb * INF_SLOTS, ..) of one layer; KC: 2, 0 (any K <= KMAX) or -1 (K > KMAX).
template <int KC, bool FILL>
__global__ __launch_bounds__(INF_TPB) void k_inf_walk(PpcLayer p, int G, InfArgs a) {
  extern __shared__ u64 inf_lds[];   // count pass: [M][INF_NB] reporters' bins (bins_lds), then [n_edges + 1][2] histogram (hist_lds)
  const int n_hist = a.hist ? 2 * (a.n_edges + 1) : 0, n_rep = INF_NB * p.M;
  const WalkBins o = walk_bins<FILL>(inf_lds, n_rep, n_hist, a.bins_lds, a.hist_lds, a.bins, a.hist, INF_TPB);
  double prob = 0.0;
  unsigned y = 0u;
  InfVal v;
  support_walk<FILL, INF_TPB, INF_SLOTS>(
      p, G, a,
      [&](const double* row) {   // what the tie's own row gives, once per tie: prob and the byte of vmr_readout
        double mean_unused;
        rho_row_prob_mean(row, p.K, prob, mean_unused);
        y = rho_row_readout(row, p.K, a.method, a.threshold);
      },
      [&](const double* row, unsigned m, int x, int xt) {
        if (KC >= 0) v = inf_eval_lane<(KC > 0 ? KC : 0)>(p.K, row, a, m, x, xt);
        else v = inf_eval_wide(p.K, row, a, m, x, xt);
        const bool lost = y > 0u && v.y == 0u, gained = y == 0u && v.y > 0u;
        const bool flag = (lost && (a.select & VMR_INF_LOST)) || (gained && (a.select & VMR_INF_GAINED)) || v.tv >= a.min_tv;
        if (!FILL) {
          double shift;
          {
#pragma clang fp contract(off)
            shift = v.prob_loo - prob;
          }
          if (prob != prob || v.prob_loo != v.prob_loo || v.tv != v.tv) atomicOr(a.bad, WALK_BAD_NAN);
          u64* b = o.rep + (size_t)m * INF_NB;
          atomicAdd(b, 1ull);
          if (lost) atomicAdd(b + 1, 1ull);
          if (gained) atomicAdd(b + 2, 1ull);
          if (flag) atomicAdd(b + 3, 1ull);
          const u64 ft = inf_fx(v.tv, a.sh, a.bad), fs = inf_fx(shift, a.sh, a.bad);
          if (ft) atomicAdd(b + 4, ft);
          if (fs) atomicAdd(b + 5, fs);
          if (o.hist) atomicAdd(o.hist + 2 * (size_t)edge_bin(a.edges, a.n_edges, v.tv) + (x > 0 ? 0 : 1), 1ull);
        }
        return flag;
      },
      [&](u64 at) {
        if (a.prob) a.prob[at] = prob;
        if (a.prob_loo) a.prob_loo[at] = v.prob_loo;
        if (a.tv) a.tv[at] = v.tv;
      });
  if (FILL) return;
  walk_bins_flush(inf_lds, n_rep, n_hist, a.bins_lds, a.hist_lds, a.bins, a.hist, INF_TPB);
}

template <bool FILL>
static int inf_launch(vmr_ctx* h, const PpcLayer& p, int G, const InfArgs& a, unsigned nb, size_t smem) {
  return launch_by_k(h, p.K, nb, INF_TPB, smem, [](auto kc) { return k_inf_walk<decltype(kc)::value, FILL>; }, p, G, a);
}

struct InfTables {
  const double *e_theta, *elog_theta, *e_lambda, *elog_lambda;
  double g_nu;
};

// What both entry points share.  rows: the table is asked for (n its capacity); n_out: the row count, or null.
static int inf_run(vmr_ctx* h, const char* fn, int layer, const InfTables& tb, int method, double threshold, int select, double min_tv,
                   int n_edges, const double* edges, uint64_t* hist, uint64_t* counts, double* sums, bool rows, uint64_t n,
                   int32_t* const* sub /* sl si sj sm x xt */, double* const* dbl /* prob prob_loo tv */, int out_on_device,
                   uint64_t* n_out) {
  auto bad_arg = [&](const char* what) { return fail(h, VMR_EINVAL, (std::string(fn) + ": " + what).c_str()); };
  if (!tb.e_theta || !tb.elog_theta || !tb.e_lambda || !tb.elog_lambda) return bad_arg("e_theta, elog_theta, e_lambda or elog_lambda is NULL");
  const Geo& g = h->g;
  const int L = g.L, M = g.M, K = g.K;
  if (!table_nonneg(tb.e_theta, (size_t)L * M)) return bad_arg("e_theta must be finite and non-negative");
  if (!table_nonneg(tb.e_lambda, (size_t)L * K)) return bad_arg("e_lambda must be finite and non-negative");
  if (!table_finite(tb.elog_theta, (size_t)L * M)) return bad_arg("elog_theta must be finite");
  if (!table_finite(tb.elog_lambda, (size_t)L * K)) return bad_arg("elog_lambda must be finite");
  if (!table_nonneg(&tb.g_nu, 1)) return bad_arg("g_nu must be finite and non-negative");
  if (method != VMR_READ_RHO_MAX && method != VMR_READ_THRESHOLD)
    return bad_arg("the method must be VMR_READ_RHO_MAX or VMR_READ_THRESHOLD (a readout of categories)");
  if (select < 0 || select > 3) return bad_arg("select must be a combination of VMR_INF_LOST and VMR_INF_GAINED (0..3)");
  if (!(min_tv >= 0.0)) return bad_arg("min_tv must lie in [0, +inf]");
  if (layer >= L) return bad_arg("layer out of range");
  if (const char* why = hist_refusal(hist, n_edges, VMR_INF_MAX_EDGES, "n_edges must lie in [0, VMR_INF_MAX_EDGES]", edges)) return bad_arg(why);
  if (!h->have_state) return fail(h, VMR_ESTATE, (std::string("vmr_set_state must be called before ") + fn).c_str());
  const size_t T = (size_t)g.N * g.N;
  if (T >= 0x7fffffffull) return bad_arg("2^31 ties or more in one layer");
  HIPCHK(h, hipSetDevice(h->device));
  { const int rce = ensure_rho_ext(h); if (rce) return rce; }
  const int l0 = layer < 0 ? 0 : layer, l1 = layer < 0 ? L : layer + 1, Lq = l1 - l0;
  if (!hist) n_edges = 0;

  // the caller's tables and the edges, one upload: per layer (g_theta, elog_theta, e_theta) [3][M] and (g_lambda, elog_lambda,
  // e_lambda) [3][K]; then the edges
  const size_t o_la = (size_t)L * 3 * M, o_ed = o_la + (size_t)L * 3 * K, n_par = o_ed + (size_t)n_edges;
  std::vector<double> par_h(n_par);
  for (int l = 0; l < L; ++l) {
    double* pt = par_h.data() + (size_t)l * 3 * M;
    for (int m = 0; m < M; ++m) {
      const double el = tb.elog_theta[(size_t)l * M + m];
      pt[m] = exp(el); pt[M + m] = el; pt[2 * (size_t)M + m] = tb.e_theta[(size_t)l * M + m];
    }
    double* pl = par_h.data() + o_la + (size_t)l * 3 * K;
    for (int k = 0; k < K; ++k) {
      const double el = tb.elog_lambda[(size_t)l * K + k];
      pl[k] = exp(el); pl[K + k] = el; pl[2 * (size_t)K + k] = tb.e_lambda[(size_t)l * K + k];
    }
  }
  if (!table_finite(par_h.data(), o_ed)) return bad_arg("exp(elog_theta) or exp(elog_lambda) overflows");
  if (n_edges) memcpy(par_h.data() + o_ed, edges, (size_t)n_edges * 8);

  const size_t n_rep = (size_t)INF_NB * M;
  const WalkShape ws = walk_shape(h, INF_TPB, INF_SLOTS, hist != nullptr, n_edges, n_rep, INF_LDS_MAX);
  const int G = ws.G;
  const unsigned nb = ws.nb;
  const size_t n_hist = ws.n_hist, smem = ws.smem;
  const int sh = 61 - ceil_log2((u64)T);   // |term| <= 2, at most N^2 of them per reporter: below 2^62

  Tmp tm(h);
  int rc, b = 0;
  double* par_d = nullptr;
  u64 *hist_d = nullptr, *rep_d = nullptr;
  std::vector<u64> rep_h((size_t)Lq * n_rep);
  InfArgs a;
  memset(&a, 0, sizeof a);
  if ((rc = tm.get(&a.bad, 4, "a flag")) || (rc = tm.get(&par_d, n_par * 8, "the parameter tables")) ||
      (rc = tm.get(&hist_d, (size_t)Lq * n_hist * 8, "the histogram")) || (rc = tm.get(&rep_d, (size_t)Lq * n_rep * 8, "the reporters' bins")))
    return rc;
  HIPCHK(h, hipMemcpyAsync(par_d, par_h.data(), n_par * 8, hipMemcpyHostToDevice, h->stream));
  if (n_hist) HIPCHK(h, hipMemsetAsync(hist_d, 0, (size_t)Lq * n_hist * 8, h->stream));
  HIPCHK(h, hipMemsetAsync(rep_d, 0, (size_t)Lq * n_rep * 8, h->stream));
  a.edges = hist ? par_d + o_ed : nullptr;
  a.gnu = g.mut ? tb.g_nu : 0.0;
  a.threshold = threshold; a.min_tv = min_tv; a.method = method; a.select = select; a.n_edges = n_edges; a.sh = sh;
  a.hist_lds = ws.hist_lds; a.bins_lds = ws.rep_lds;
  auto tables = [&](int l) {
    a.gth = par_d + (size_t)l * 3 * M; a.elt = a.gth + M; a.eth = a.elt + M;
    a.gla = par_d + o_la + (size_t)l * 3 * K; a.ell = a.gla + K; a.ela = a.ell + K;
  };
  const WalkTable w = {rows, n, sub, dbl, 3, out_on_device, n_out};
  rc = walk_count_fill(
      h, fn, tm, l0, l1, w, a, b,
      [&](int l, const PpcLayer& p) -> int {
        tables(l);
        a.hist = hist ? hist_d + (size_t)(l - l0) * n_hist : nullptr;
        a.bins = rep_d + (size_t)(l - l0) * n_rep;
        return inf_launch<false>(h, p, G, a, nb, smem);
      },
      [&](u64* flagged) -> int {
        HIPCHK(h, hipMemcpy(rep_h.data(), rep_d, rep_h.size() * 8, hipMemcpyDeviceToHost));
        for (int q = 0; q < Lq; ++q)
          for (int m = 0; m < M; ++m) flagged[q] += rep_h[((size_t)q * M + m) * INF_NB + 3];
        if (b & WALK_BAD_NAN) return fail(h, VMR_ENAN, (std::string(fn) + ": a leave-one-out value is NaN").c_str());
        if (b & INF_BAD_RANGE)
          return fail(h, VMR_EINVAL, (std::string(fn) + ": a row of rho sums to more than 2 (the fixed point of the sums is sized for normalised rows)").c_str());
        return VMR_OK;
      },
      [&](int l, const PpcLayer& p, double* const* d64) -> int {
        tables(l);
        a.hist = nullptr; a.bins = nullptr; a.edges = nullptr; a.n_edges = 0; a.hist_lds = 0; a.bins_lds = 0;
        a.prob = d64[0]; a.prob_loo = d64[1]; a.tv = d64[2];
        return inf_launch<true>(h, p, G, a, nb, 0);
      });
  if (rc) return rc;
  if (hist) HIPCHK(h, hipMemcpyAsync(hist, hist_d, (size_t)Lq * n_hist * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (size_t r = 0; r < (size_t)Lq * M; ++r) {
    const u64* s = &rep_h[r * INF_NB];
    if (counts)
      for (int c = 0; c < VMR_INF_NCOUNT; ++c) counts[r * VMR_INF_NCOUNT + c] = s[c];
    if (sums)
      for (int c = 0; c < VMR_INF_NSUM; ++c) sums[r * VMR_INF_NSUM + c] = ldexp((double)(long long)s[VMR_INF_NCOUNT + c], -sh);
  }
  return VMR_OK;
}

}  // namespace

extern "C" int vmr_reporter_influence_size(vmr_handle h, int layer, const double* e_theta, const double* elog_theta, const double* e_lambda,
                                           const double* elog_lambda, double g_nu, int method, double threshold, int select, double min_tv,
                                           uint64_t* n) {
  if (!h) return VMR_EINVAL;
  if (!n) return fail(h, VMR_EINVAL, "vmr_reporter_influence_size: n is NULL");
  int32_t* none[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  double* noned[3] = {nullptr, nullptr, nullptr};
  const InfTables tb = {e_theta, elog_theta, e_lambda, elog_lambda, g_nu};
  return inf_run(h, "vmr_reporter_influence_size", layer, tb, method, threshold, select, min_tv, 0, nullptr, nullptr, nullptr, nullptr, false, 0,
                 none, noned, 0, n);
}

extern "C" int vmr_reporter_influence(vmr_handle h, int layer, const double* e_theta, const double* elog_theta, const double* e_lambda,
                                      const double* elog_lambda, double g_nu, int method, double threshold, int select, double min_tv,
                                      int n_edges, const double* edges, uint64_t* hist, uint64_t* counts, double* sums, uint64_t n,
                                      int32_t* sl, int32_t* si, int32_t* sj, int32_t* sm, int32_t* x, int32_t* xt, double* prob,
                                      double* prob_loo, double* tv, int out_on_device) {
  if (!h) return VMR_EINVAL;
  int32_t* sub[6] = {sl, si, sj, sm, x, xt};
  double* dbl[3] = {prob, prob_loo, tv};
  const bool any_row = sl || si || sj || sm || x || xt || prob || prob_loo || tv;
  if (!any_row && !hist && !counts && !sums) return fail(h, VMR_EINVAL, "vmr_reporter_influence: every output is NULL");
  const bool rows = any_row || n != 0;   // (n = 0 and every row pointer NULL: no table pass)
  const InfTables tb = {e_theta, elog_theta, e_lambda, elog_lambda, g_nu};
  return inf_run(h, "vmr_reporter_influence", layer, tb, method, threshold, select, min_tv, n_edges, edges, hist, counts, sums, rows, n, sub,
                 dbl, out_on_device, nullptr);
}
