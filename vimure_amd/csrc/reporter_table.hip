// reporter_table.hip -- each reporter's reports against the posterior, where rho lives: vmr_reporter_table (include/vimure_hip.h has
// the table of the seven counts and three sums per layer and reporter).
//
// A sum over the support S_m of reporter m is, for every tie whose mask row is all ones, the same number for all M reporters.  So
// the pass over the ties adds such a row ONCE, into four scalars of its layer, and only partial rows are walked reporter by
// reporter; everything else a reporter's row needs sits at its own reports.  O(ties + mask entries of partial rows + reports)
// instead of the O(|S|) of the support walk (k_ppc_walk):
//   k_rt_ties     a thread per tie in storage order (rho read once, 8 K bytes, coalesced): y (vmr_readout's byte), prob (rho_row.h),
//                 rs = sum_k rho_k and q = sum_k rho_k G_lambda_k.  All-ones row: (1, [y > 0], prob, q) into the thread's partials,
//                 which leave the workgroup as four integer atomics.  Partial row: its mask words' set bits, or its reporter list,
//                 into the bins (n_scope, n_inferred, E, Q) of every reporter it holds.
//   k_rt_reports  a group of G lanes per ordered tie over the tie's reports (the dense row, or the tie's row of the tie-major
//                 index of ppc.hip), fetched by tie_report (read_side.h) as in k_obs.  A report x > 0 of reporter m inside the mask adds to
//                 (n_rep, total, hits, H, mutual), outside it to n_out; and, with mutuality, it IS the X^T of the mirror tie: where
//                 the mirror tie's mask row holds m it adds rs_mirror x to U.  The rho rows of ties with reports are read again here.
// The host then puts a row together:  n_scope = all-ones n + bin, n_inferred likewise, exp_ties = E, exp_hits = H,
//   exp_total = G_theta[l,m] (Q_all + Q_m) + G_nu U_m      (sum_{S_m} sum_k rho_k (G_theta G_lambda_k + G_nu X^T), regrouped).
//
// Determinism: every accumulator is a 64-bit INTEGER -- the counts, and the four double sums in fixed point (the route of
// VMR_DETERMINISTIC's sweeps): E and H in 2^-sh_p, Q in 2^-sh_q, U in 2^-sh_u, sized on the host so that no sum can leave 62 bits
// (rt_fixed_point below; a row of rho summing to more than 2 is refused).  Integer adds commute: LDS and global integer atomics
// in any order give the same bits, and there is no floating-point atomic anywhere.  Bins live in LDS up to PR_HIST_M reporters
// (flushed once per workgroup), in global memory beyond.
#include "read_side.h"

namespace {

#define RT_TPB 256
#define RT_NTB 4     // bins of the tie pass per reporter: n_scope, n_inferred, E, Q  (and the all-ones scalars of a layer)
#define RT_NRB 7     // bins of the report pass per reporter: n_rep, total, hits, mutual, n_out, H, U
#define RT_SLOTS 64  // tie slots a group walks per workgroup (report pass)

// the fixed point of a call (host-sized) and what the kernels refuse
struct RtFx {
  int sh_p, sh_q, sh_u;
  double lim_q;   // 2 max G_lambda, rounded up to a power of two: no q may exceed it
};

struct RtTie {
  double prob, rs, q;
  unsigned y;
};

// what both passes take from a tie's rho row; gla null: q is not needed
__device__ __forceinline__ RtTie rt_tie(const double* __restrict__ r, int K, const double* __restrict__ gla, int method, double threshold) {
  RtTie o;
  double mean;
  rho_row_prob_mean(r, K, o.prob, mean);
  o.y = rho_row_readout(r, K, method, threshold);
  double rs = 0.0, q = 0.0;
  for (int k = 0; k < K; ++k) {
    rs += r[k];
    if (gla) q += r[k] * gla[k];
  }
  o.rs = rs; o.q = q;
  return o;
}

// v in [0, lim] as a multiple of 2^-sh; NaN and values out of range are flagged and add nothing
__device__ __forceinline__ u64 rt_fx(double v, double lim, int sh, int* __restrict__ bad) {
  if (!(v >= 0.0 && v <= lim)) { atomicOr(bad, v != v ? 1 : 4); return 0ull; }
  return det_fx(v, sh);
}

// The pass over the ties of one layer.  perm: position -> tie of the layer (report lists: rho is stored by sorted position), or null.
// scal [RT_NTB]: the all-ones rows; bins [M][RT_NTB]: the partial rows.  HIST: the bins in LDS first.
template <bool HIST>
__global__ __launch_bounds__(RT_TPB) void k_rt_ties(PpcLayer p, const unsigned* __restrict__ perm, RtFx fx, int method, double threshold,
                                                    u64* __restrict__ scal, u64* __restrict__ bins, int* __restrict__ bad) {
  extern __shared__ u64 rt_hist[];   // HIST: [M][RT_NTB]
  __shared__ u64 tot[RT_NTB];
  if (threadIdx.x < RT_NTB) tot[threadIdx.x] = 0ull;
  if (HIST) for (int q = threadIdx.x; q < RT_NTB * p.M; q += RT_TPB) rt_hist[q] = 0ull;
  __syncthreads();
  u64* const o = HIST ? rt_hist : bins;
  u64 c[RT_NTB] = {0ull, 0ull, 0ull, 0ull};
  for (size_t pos = (size_t)blockIdx.x * RT_TPB + threadIdx.x; pos < p.T; pos += (size_t)gridDim.x * RT_TPB) {
    const size_t t = perm ? (size_t)perm[pos] : pos;
    if (t >= p.T) continue;   // (never: positions below T hold ties)
    const int cl = p.cls[t];
    if (cl == 0) continue;
    const RtTie v = rt_tie(p.rho + pos * p.K, p.K, p.gla, method, threshold);
    if (v.rs != v.rs || v.rs > 2.0) atomicOr(bad, v.rs != v.rs ? 1 : 4);
    const u64 e = rt_fx(v.prob, 2.0, fx.sh_p, bad), qf = rt_fx(v.q, fx.lim_q, fx.sh_q, bad), inf = v.y > 0u ? 1ull : 0ull;
    if (cl == 1) {
      c[0] += 1ull; c[1] += inf; c[2] += e; c[3] += qf;
    } else if (p.rq) {
      const unsigned a1 = p.rq[t + 1];
      for (unsigned a = p.rq[t]; a < a1; ++a) {
        const unsigned m = p.Rm[a];
        if (m >= (unsigned)p.M) continue;
        u64* b = o + (size_t)m * RT_NTB;
        atomicAdd(b, 1ull);
        if (inf) atomicAdd(b + 1, 1ull);
        if (e) atomicAdd(b + 2, e);
        if (qf) atomicAdd(b + 3, qf);
      }
    } else {
      for (int w = 0; w < p.W; ++w) {
        uint64_t bits = p.Rb[t * (size_t)p.W + w];
        while (bits) {
          const unsigned m = (unsigned)w * 64u + (unsigned)(__ffsll((long long)bits) - 1);
          bits &= bits - 1ull;
          if (m >= (unsigned)p.M) continue;
          u64* b = o + (size_t)m * RT_NTB;
          atomicAdd(b, 1ull);
          if (inf) atomicAdd(b + 1, 1ull);
          if (e) atomicAdd(b + 2, e);
          if (qf) atomicAdd(b + 3, qf);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < RT_NTB; ++k) {
    c[k] = wave_sum_ull(c[k]);
    if ((threadIdx.x & 63) == 0 && c[k]) atomicAdd(&tot[k], c[k]);
  }
  __syncthreads();
  if (threadIdx.x < RT_NTB && tot[threadIdx.x]) atomicAdd(scal + threadIdx.x, tot[threadIdx.x]);
  if (HIST) flush_bins(rt_hist, bins, RT_NTB * p.M, RT_TPB);
}

// The pass over the reports of one layer: a group of G lanes per ordered tie.  bins [M][RT_NRB].
template <bool HIST>
__global__ __launch_bounds__(RT_TPB) void k_rt_reports(PpcLayer p, int G, RtFx fx, int method, double threshold, double lim_u,
                                                       u64* __restrict__ bins, int* __restrict__ bad) {
  extern __shared__ u64 rt_hist[];   // HIST: [M][RT_NRB]
  if (HIST) for (int q = threadIdx.x; q < RT_NRB * p.M; q += RT_TPB) rt_hist[q] = 0ull;
  __syncthreads();
  u64* const o = HIST ? rt_hist : bins;
  const WalkGroup g = walk_group(G);
  const size_t gpb = RT_TPB / G;
  const size_t t_lim = ((size_t)blockIdx.x + 1) * gpb * RT_SLOTS, t_end = t_lim < p.T ? t_lim : p.T;
  for (size_t t = (size_t)blockIdx.x * gpb * RT_SLOTS + threadIdx.x / G; t < t_end; t += gpb) {   // (uniform over the group)
    const unsigned e0 = p.X ? 0u : p.ip[t], nc = p.X ? (unsigned)p.M : p.ip[t + 1] - e0;
    if (nc == 0u) continue;
    const MaskRow A = mask_row(p.cls, p.Rb, p.rq, p.Rm, p.W, t);
    const size_t i = t / p.N, j = t - i * p.N, tm = j * p.N + i;
    const MaskRow B = i != j ? mask_row(p.cls, p.Rb, p.rq, p.Rm, p.W, tm) : A;   // the mirror tie's row (a diagonal tie is its own mirror)
    bool have = false;
    unsigned y = 0;
    u64 e = 0;
    double rsm = 0.0;
    for (unsigned c0 = 0; c0 < nc; c0 += (unsigned)G) {
      const TieReport rp = tie_report(p, A, t, e0, nc, c0 + (unsigned)g.gl);
      const unsigned x = rp.x, m = rp.m;
      if (!(__ballot(x > 0u) & g.gmask)) continue;   // (uniform over the group)
      if (!have) {   // the tie's own row, and the mirror tie's sum: once per tie with a report
        const RtTie v = rt_tie(tie_rho(p, t), p.K, nullptr, method, threshold);
        y = v.y;
        e = rt_fx(v.prob, 2.0, fx.sh_p, bad);
        if (p.mut) {
          rsm = v.rs;
          if (i != j) {
            const double* r = tie_rho(p, tm);
            rsm = 0.0;
            for (int k = 0; k < p.K; ++k) rsm += r[k];
          }
          if (rsm != rsm || rsm > 2.0) { if (g.gl == 0) atomicOr(bad, rsm != rsm ? 1 : 4); rsm = 0.0; }
        }
        have = true;
      }
      if (x == 0u || m >= (unsigned)p.M) continue;
      u64* b = o + (size_t)m * RT_NRB;
      if (rp.in) {
        const bool mut = i != j && B.c != 0 && mirror_reported(p, B, tm, m);
        atomicAdd(b, 1ull);
        atomicAdd(b + 1, (u64)x);
        if (y) atomicAdd(b + 2, 1ull);
        if (mut) atomicAdd(b + 3, 1ull);
        if (e) atomicAdd(b + 5, e);
      } else {
        atomicAdd(b + 4, 1ull);
      }
      if (p.mut && row_has(B, m)) {   // x is X^T of the mirror tie, which reporter m's support holds
        const u64 u = rt_fx(rsm * (double)x, lim_u, fx.sh_u, bad);
        if (u) atomicAdd(b + 6, u);
      }
    }
  }
  __syncthreads();
  if (HIST) flush_bins(rt_hist, bins, RT_NRB * p.M, RT_TPB);
}

static double det_back_host(u64 u, int sh) { return ldexp((double)u, -sh); }

// The fixed point of a call, from what the host knows.  b = ceil(log2 N^2); e_l: G_lambda <= 2^e_l for every entry; e_x: sum X < 2^e_x.
//   E, H   terms prob <= 2 (checked), at most N^2 of them                      sh_p = 61 - b
//   Q      terms q <= 2 max G_lambda <= 2^(e_l + 1), at most N^2                sh_q = 61 - b - e_l
//   U      terms rs x with rs <= 2 (checked), all of them together <= 2 sum X   sh_u = 61 - e_x
// so every sum stays below 2^62.  A term is rounded to nearest: a reporter's sum of n terms is off by n 2^-sh / 2 at most.
static void rt_fixed_point(size_t T, double gla_max, double sum_x, RtFx& fx, double& lim_u) {
  const int b = ceil_log2((u64)T);
  int e_l = 0, e_x = 0;
  (void)frexp(gla_max, &e_l);            // gla_max = f 2^e_l, f in [0.5, 1)
  if (gla_max == 0.0) e_l = -1000;
  if (e_l < -900) e_l = -900;
  (void)frexp(sum_x + 1.0, &e_x);
  fx.sh_p = 61 - b;
  fx.sh_q = 61 - b - e_l;
  fx.sh_u = 61 - e_x;
  fx.lim_q = ldexp(1.0, e_l + 1);
  lim_u = ldexp(1.0, e_x + 1);
}

}  // namespace

extern "C" int vmr_reporter_table(vmr_handle h, int method, double threshold, int layer, uint64_t* counts, double* sums) {
  if (!h) return VMR_EINVAL;
  if (!counts && !sums) return fail(h, VMR_EINVAL, "vmr_reporter_table: counts and sums are both NULL");
  if (method != VMR_READ_RHO_MAX && method != VMR_READ_THRESHOLD)
    return fail(h, VMR_EINVAL, "vmr_reporter_table: the method must be VMR_READ_RHO_MAX or VMR_READ_THRESHOLD (a table of categories)");
  if (layer >= h->g.L) return fail(h, VMR_EINVAL, "vmr_reporter_table: layer out of range");
  if (!h->have_state) return fail(h, VMR_ESTATE, "vmr_set_state must be called before vmr_reporter_table");
  const Geo& g = h->g;
  const int L = g.L, M = g.M, K = g.K;
  const size_t T = (size_t)g.N * g.N, NS = (T + 63) / 64;
  if (T >= 0x7fffffffull) return fail(h, VMR_EINVAL, "vmr_reporter_table: 2^31 ties or more in one layer");
  HIPCHK(h, hipSetDevice(h->device));
  { const int rce = ensure_rho_ext(h); if (rce) return rce; }
  const int l0 = layer < 0 ? 0 : layer, l1 = layer < 0 ? L : layer + 1, Lq = l1 - l0;

  // the parameters the sums are put together from, and the fixed point
  std::vector<double> gth((size_t)L * M), gla((size_t)L * K);
  double gnu = 0.0, sum_x = 0.0, gla_max = 0.0;
  int rc;
  if ((rc = vmr_get_geometric(h, gth.data(), gla.data(), &gnu, nullptr)) || (rc = vmr_data_stats(h, &sum_x, nullptr))) return rc;
  if (!table_nonneg(gla.data() + (size_t)l0 * K, (size_t)Lq * K)) return fail(h, VMR_ENAN, "vmr_reporter_table: G_lambda is NaN, infinite or negative");
  for (size_t q = (size_t)l0 * K; q < (size_t)l1 * K; ++q) gla_max = std::max(gla_max, gla[q]);
  RtFx fx;
  double lim_u = 0.0;
  rt_fixed_point(T, gla_max, sum_x, fx, lim_u);

  Tmp tm(h);
  int* bad = nullptr;
  u64 *scal = nullptr, *tb = nullptr, *rb = nullptr;
  const size_t n_sc = (size_t)Lq * RT_NTB, n_tb = (size_t)Lq * M * RT_NTB, n_rb = (size_t)Lq * M * RT_NRB;
  if ((rc = tm.get(&bad, 4, "a flag")) || (rc = tm.get(&scal, n_sc * 8, "the all-ones rows' sums")) ||
      (rc = tm.get(&tb, n_tb * 8, "the reporters' bins of the ties")) || (rc = tm.get(&rb, n_rb * 8, "the reporters' bins of the reports")))
    return rc;
  HIPCHK(h, hipMemsetAsync(bad, 0, 4, h->stream));
  HIPCHK(h, hipMemsetAsync(scal, 0, n_sc * 8, h->stream));
  HIPCHK(h, hipMemsetAsync(tb, 0, n_tb * 8, h->stream));
  HIPCHK(h, hipMemsetAsync(rb, 0, n_rb * 8, h->stream));

  const bool hist = M <= PR_HIST_M;
  const size_t smem_t = hist ? (size_t)M * RT_NTB * 8 : 0, smem_r = hist ? (size_t)M * RT_NRB * 8 : 0;
  if (smem_t > 48 * 1024)
    HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(k_rt_ties<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_t));
  if (smem_r > 48 * 1024)
    HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(k_rt_reports<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_r));
  // lanes per tie of the report pass: dense tiles the whole row; report lists twice the mean row of the index
  const int G = h->sparse ? index_lanes(h) : pow2_lanes((size_t)M);
  const unsigned nb_t = (unsigned)std::max<size_t>(1, std::min<size_t>(2048, (T + RT_TPB - 1) / RT_TPB));
  const unsigned nb_r = walk_blocks(T, RT_TPB, G, RT_SLOTS);
  for (int l = l0; l < l1; ++l) {
    LayerPrep lp;
    if ((rc = ppc_prep_layer(h, tm, l, false, true, lp, true, false))) return rc;
    const unsigned* perm = h->sparse ? h->perm + (size_t)l * NS * 64 : nullptr;
    u64 *sc_l = scal + (size_t)(l - l0) * RT_NTB, *tb_l = tb + (size_t)(l - l0) * M * RT_NTB, *rb_l = rb + (size_t)(l - l0) * M * RT_NRB;
    if (hist) hipLaunchKernelGGL(k_rt_ties<true>, dim3(nb_t), dim3(RT_TPB), smem_t, h->stream, lp.p, perm, fx, method, threshold, sc_l, tb_l, bad);
    else hipLaunchKernelGGL(k_rt_ties<false>, dim3(nb_t), dim3(RT_TPB), 0, h->stream, lp.p, perm, fx, method, threshold, sc_l, tb_l, bad);
    HIPCHK(h, hipGetLastError());
    if (hist) hipLaunchKernelGGL(k_rt_reports<true>, dim3(nb_r), dim3(RT_TPB), smem_r, h->stream, lp.p, G, fx, method, threshold, lim_u, rb_l, bad);
    else hipLaunchKernelGGL(k_rt_reports<false>, dim3(nb_r), dim3(RT_TPB), 0, h->stream, lp.p, G, fx, method, threshold, lim_u, rb_l, bad);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    ppc_release_layer(tm, lp);
  }
  std::vector<u64> sc_h(n_sc), tb_h(n_tb), rb_h(n_rb);
  int b = 0;
  HIPCHK(h, hipMemcpyAsync(sc_h.data(), scal, n_sc * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(tb_h.data(), tb, n_tb * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(rb_h.data(), rb, n_rb * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(&b, bad, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (b & 1) return fail(h, VMR_ENAN, "vmr_reporter_table: a sum is NaN");
  if (b) return fail(h, VMR_EINVAL, "vmr_reporter_table: a row of rho sums to more than 2 (the fixed point of the sums is sized for normalised rows)");
  bool nan_seen = false;
  for (int l = l0; l < l1; ++l)
    for (int m = 0; m < M; ++m) {
      const size_t r = (size_t)(l - l0) * M + m;
      const u64 *s = &sc_h[(size_t)(l - l0) * RT_NTB], *t = &tb_h[r * RT_NTB], *q = &rb_h[r * RT_NRB];
      if (counts) {
        uint64_t* c = counts + r * VMR_RT_NCOUNT;
        c[0] = s[0] + t[0]; c[1] = q[0]; c[2] = q[1]; c[3] = s[1] + t[1]; c[4] = q[2]; c[5] = q[3]; c[6] = q[4];
      }
      if (sums) {
        double* d = sums + r * VMR_RT_NSUM;
        d[0] = det_back_host(s[2] + t[2], fx.sh_p);
        d[1] = det_back_host(q[5], fx.sh_p);
        d[2] = gth[(size_t)l * M + m] * det_back_host(s[3] + t[3], fx.sh_q);
        if (g.mut) d[2] += gnu * det_back_host(q[6], fx.sh_u);
        nan_seen = nan_seen || d[0] != d[0] || d[1] != d[1] || d[2] != d[2];
      }
    }
  if (nan_seen) return fail(h, VMR_ENAN, "vmr_reporter_table: a sum is NaN");
  return VMR_OK;
}
