// heldout.hip -- the log predictive density of reports the fit never saw, scored where rho lives: vmr_heldout_loglik
// (include/vimure_hip.h states the per-entry values, the per-layer sums and counts, and every refusal).
//
// The caller gives a LIST of entries (l,i,j,m) with their held-out counts x and, with mutuality, the mirrored counts to condition
// on; the handle gives rho and its mask, nothing else: its X is never read and no tie-major index of it is built.  The list is
// non-decreasing in l; a layer's segment runs against that layer's PpcLayer (ppc_layer.h: the mask for the in-mask count, the
// tie -> position table because report-list handles store rho by sorted position).
//   k_ho_check   a lane per entry: l in range and not below its predecessor's (else a flag and the call ends before the pass);
//                the lane at a layer's first entry writes the segment bounds seg[L + 1].
//   k_ho_lane    K <= 8, a lane per entry: the entry's subscripts (24 B, coalesced), the rho row of its tie (8 K B; K = 2 in one
//                16-byte load) -- a list sorted by (l,i,j,m) has the M entries of a tie in neighbouring lanes, which then read the
//                same row: the fast case --, K rates, the K terms b_k = x log mu_k - mu_k + log rho_k, their maximum and the sum
//                of exp(b_k - max) in ascending k.
//   k_ho_group   K > 8 (up to KGEN_MAX): a group of HO_G lanes per entry, lane g takes the categories g, g + HO_G, ..; a lane
//                keeps a running maximum and the sum scaled to it, and the group folds the pairs by shuffles in a fixed order.
//                The mean is added in ascending k all the same (the products travel to every lane by shuffles).
// Both write logp and mean per entry and reduce four doubles and four counts per workgroup: a workgroup owns HO_CHUNK
// consecutive entries of the segment, a thread adds its entries in order, the waves fold by shuffles, the workgroup by
// block_sum_n, and k_lik_finish adds a layer's per-workgroup partials in a fixed order.  The tree's shape depends on the segment
// length alone; there is no floating-point atomic and no ticket: the results are bit-identical from run to run.
// lgamma(x + 1): a table of the host's lgamma for x < HO_LGT, Stirling's series beyond (the library's device lgamma costs scratch).
// An entry whose subscripts are out of range or whose counts are negative sets a flag, reads nothing and adds nothing.
#include "report_lik.h"

namespace {

#define HO_TPB 256
#define HO_CHUNK 1024   // entries of a workgroup
#define HO_G 16         // lanes of an entry's group (K > KMAX)

// flag bits (LIK_BAD_NAN is bit 1)
#define HO_BAD_SUB 4
#define HO_BAD_NEG 8
#define HO_BAD_LAYER 16

static_assert(VMR_HO_NSUM == LIK_N && VMR_HO_NCOUNT == LIK_N && HO_TPB == LIK_TPB, "LikAcc, k_lik_finish");

struct HoIn {
  const int32_t *el, *ei, *ej, *em, *ex, *ext;   // ext may be null: no mirrored count
};

struct HoOut {
  double *logp, *mean;     // [n], either may be null
  double* part;            // [workgroups of the layer][VMR_HO_NSUM]
  u64* cpart;              // [workgroups of the layer][VMR_HO_NCOUNT]
};

// The subscripts of entry e, checked: false (and a flag) where the entry may not be read.
__device__ __forceinline__ bool ho_entry(const PpcLayer& p, const HoIn& in, size_t e, int& i, int& j, int& m, int& x, int& xt, int* __restrict__ bad) {
  const int l = in.el[e];
  i = in.ei[e]; j = in.ej[e]; m = in.em[e]; x = in.ex[e];
  xt = in.ext ? in.ext[e] : 0;
  int f = 0;
  if (l != p.l) f |= HO_BAD_LAYER;
  if ((unsigned)i >= (unsigned)p.N || (unsigned)j >= (unsigned)p.N || (unsigned)m >= (unsigned)p.M) f |= HO_BAD_SUB;
  if (x < 0 || xt < 0) f |= HO_BAD_NEG;
  if (f && bad) atomicOr(bad, f);   // (bad null: another lane of the entry's group reports it)
  return f == 0;
}

// K <= KMAX: a lane per entry of the segment [s0, s0 + ns).  th [M], la [K]: the layer's rows of the caller's tables.
template <bool K2>
__global__ __launch_bounds__(HO_TPB) void k_ho_lane(PpcLayer p, HoIn in, size_t s0, size_t ns, const double* __restrict__ th,
                                                    const double* __restrict__ la, double eta, const double* __restrict__ lgt, HoOut o,
                                                    int* __restrict__ bad) {
  __shared__ double red[16];
  __shared__ u64 redu[16];
  LikAcc a;
  const size_t base = (size_t)blockIdx.x * HO_CHUNK;
  for (int rd = 0; rd < HO_CHUNK / HO_TPB; ++rd) {
    const size_t q = base + (size_t)rd * HO_TPB + threadIdx.x;
    if (q >= ns) break;
    const size_t e = s0 + q;
    int i, j, m, x, xt;
    double lp = 0.0, mn = 0.0;
    if (ho_entry(p, in, e, i, j, m, x, xt, bad)) {
      const size_t t = (size_t)i * p.N + j;
      const double* row = tie_rho(p, t);
      lik_eval_lane<(K2 ? 2 : 0)>(p.K, row, th[m], la, eta, x, xt, lgt, lp, mn);
      const bool inm = row_has(mask_row(p.cls, p.Rb, p.rq, p.Rm, p.W, t), (unsigned)m);
      LIK_TAKE(a, lp, mn, x, inm, bad);
    }
    if (o.logp) o.logp[e] = lp;
    if (o.mean) o.mean[e] = mn;
  }
  lik_flush(a, o.part, o.cpart, red, redu);
}

// K > KMAX: HO_G lanes per entry
__global__ __launch_bounds__(HO_TPB) void k_ho_group(PpcLayer p, HoIn in, size_t s0, size_t ns, const double* __restrict__ th,
                                                     const double* __restrict__ la, double eta, const double* __restrict__ lgt, HoOut o,
                                                     int* __restrict__ bad) {
  __shared__ double red[16];
  __shared__ u64 redu[16];
  const int K = p.K, lane = threadIdx.x & 63, gl = lane & (HO_G - 1), g0 = lane - gl;
  LikAcc a;
  const size_t base = (size_t)blockIdx.x * HO_CHUNK;
  const int gpb = HO_TPB / HO_G;
  for (int rd = 0; rd < HO_CHUNK / gpb; ++rd) {
    const size_t q = base + (size_t)rd * gpb + threadIdx.x / HO_G;   // (uniform over the group, and so is all control flow below)
    if (q >= ns) break;
    const size_t e = s0 + q;
    int i, j, m, x, xt;
    double lp = 0.0, mn = 0.0;
    const bool ok = ho_entry(p, in, e, i, j, m, x, xt, gl == 0 ? bad : nullptr);
    if (ok) {
      const size_t t = (size_t)i * p.N + j;
      const double* row = tie_rho(p, t);
      const double thm = th[m], exy = eta * (double)xt, xd = (double)x;
      double mx = -INFINITY, s = 0.0;
      for (int k0 = 0; k0 < K; k0 += HO_G) {
        const int k = k0 + gl;
        double pr = 0.0;
        if (k < K) {
          const double r = row[k], mu = ho_rate(thm, la[k], exy);
          pr = ho_mul(r, mu);
          const double b = ho_term(r, mu, xd, x > 0);
          if (b != b) s = b;
          else if (b > -INFINITY) ho_fold(mx, s, b, 1.0);
        }
        const int lim = K - k0 < HO_G ? K - k0 : HO_G;
        for (int c = 0; c < lim; ++c) mn = ho_add(mn, __shfl(pr, g0 + c, 64));   // ascending k, in every lane
      }
#pragma unroll
      for (int w = HO_G >> 1; w > 0; w >>= 1) {
        const double mx2 = __shfl_xor(mx, w, 64), s2 = __shfl_xor(s, w, 64);
        ho_fold(mx, s, mx2, s2);
      }
      lp = ho_logp(mx, s, ho_lgam1((unsigned)x, lgt));
      if (gl == 0) {
        const bool inm = row_has(mask_row(p.cls, p.Rb, p.rq, p.Rm, p.W, t), (unsigned)m);
        LIK_TAKE(a, lp, mn, x, inm, bad);
      }
    }
    if (gl == 0) {
      if (o.logp) o.logp[e] = lp;
      if (o.mean) o.mean[e] = mn;
    }
  }
  lik_flush(a, o.part, o.cpart, red, redu);
}

// el in [0, L) and non-decreasing; seg[l] = the first entry of a layer >= l (seg[L] = n).  Every seg entry is written exactly once
// when the list is in order; otherwise the flag ends the call before seg is used.
__global__ __launch_bounds__(HO_TPB) void k_ho_check(const int32_t* __restrict__ el, size_t n, int L, u64* __restrict__ seg, int* __restrict__ bad) {
  for (size_t e = (size_t)blockIdx.x * HO_TPB + threadIdx.x; e < n; e += (size_t)gridDim.x * HO_TPB) {
    const int l = el[e];
    if (l < 0 || l >= L) { atomicOr(bad, HO_BAD_SUB); continue; }
    int prev = -1;
    if (e > 0) {
      prev = el[e - 1];
      if (prev > l) { atomicOr(bad, HO_BAD_LAYER); continue; }
      if (prev < 0 || prev >= L) continue;   // (flagged by its own lane)
    }
    for (int q = prev + 1; q <= l; ++q) seg[q] = (u64)e;
    if (e == n - 1)
      for (int q = l + 1; q <= L; ++q) seg[q] = (u64)n;
  }
}

}  // namespace

extern "C" int vmr_heldout_loglik(vmr_handle h, uint64_t n, const int32_t* el, const int32_t* ei, const int32_t* ej, const int32_t* em,
                                  const int32_t* ex, const int32_t* ext, int in_on_device, const double* theta, const double* lambda,
                                  double eta, double* logp, double* mean, int out_on_device, double* sums, uint64_t* counts) {
  if (!h) return VMR_EINVAL;
  if (!el || !ei || !ej || !em || !ex) return fail(h, VMR_EINVAL, "vmr_heldout_loglik: a subscript array or the count array is NULL");
  if (!logp && !mean && !sums && !counts) return fail(h, VMR_EINVAL, "vmr_heldout_loglik: every output is NULL");
  if (n == 0 || n >= 0x80000000ull) return fail(h, VMR_EINVAL, "vmr_heldout_loglik: n must lie in [1, 2^31)");
  if (!theta || !lambda) return fail(h, VMR_EINVAL, "vmr_heldout_loglik: theta or lambda is NULL");
  const Geo& g = h->g;
  const int L = g.L, M = g.M, K = g.K;
  if (!table_nonneg(theta, (size_t)L * M)) return fail(h, VMR_EINVAL, "vmr_heldout_loglik: theta must be finite and non-negative");
  if (!table_nonneg(lambda, (size_t)L * K)) return fail(h, VMR_EINVAL, "vmr_heldout_loglik: lambda must be finite and non-negative");
  if (!table_nonneg(&eta, 1)) return fail(h, VMR_EINVAL, "vmr_heldout_loglik: eta must be finite and non-negative");
  if (!h->have_state) return fail(h, VMR_ESTATE, "vmr_set_state must be called before vmr_heldout_loglik");
  const size_t T = (size_t)g.N * g.N;
  if (T >= 0x7fffffffull) return fail(h, VMR_EINVAL, "vmr_heldout_loglik: 2^31 ties or more in one layer");
  HIPCHK(h, hipSetDevice(h->device));
  { const int rce = ensure_rho_ext(h); if (rce) return rce; }

  // the caller's tables and the lgamma table, one upload: theta [L][M], lambda [L][K], lgamma(x + 1) for x < HO_LGT
  const size_t n_par = (size_t)L * M + (size_t)L * K + HO_LGT;
  std::vector<double> par_h(n_par);
  memcpy(par_h.data(), theta, (size_t)L * M * 8);
  memcpy(par_h.data() + (size_t)L * M, lambda, (size_t)L * K * 8);
  ho_lgt_fill(par_h.data() + (size_t)L * M + (size_t)L * K);

  const size_t nb_all = (size_t)((n + HO_CHUNK - 1) / HO_CHUNK) + (size_t)L;   // workgroups of all segments at most
  Tmp tm(h);
  int rc;
  int* bad = nullptr;
  int32_t* in_d = nullptr;
  u64 *seg_d = nullptr, *cpart = nullptr, *counts_d = nullptr;
  double *par_d = nullptr, *part = nullptr, *sums_d = nullptr, *logp_d = nullptr, *mean_d = nullptr;
  const int n_in = ext ? 6 : 5;
  if ((rc = tm.get(&bad, 4, "a flag")) || (rc = tm.get(&seg_d, (size_t)(L + 1) * 8, "the layers' segments")) ||
      (rc = tm.get(&par_d, n_par * 8, "the parameter tables")) || (rc = tm.get(&part, nb_all * VMR_HO_NSUM * 8, "the partial sums")) ||
      (rc = tm.get(&cpart, nb_all * VMR_HO_NCOUNT * 8, "the partial counts")) || (rc = tm.get(&sums_d, (size_t)L * VMR_HO_NSUM * 8, "the sums")) ||
      (rc = tm.get(&counts_d, (size_t)L * VMR_HO_NCOUNT * 8, "the counts")))
    return rc;
  if (!in_on_device && (rc = tm.get(&in_d, (size_t)n_in * n * 4, "the list of entries"))) return rc;
  if (logp && !out_on_device && (rc = tm.get(&logp_d, (size_t)n * 8, "the staging of logp"))) return rc;
  if (mean && !out_on_device && (rc = tm.get(&mean_d, (size_t)n * 8, "the staging of mean"))) return rc;

  HoIn in;
  if (in_on_device) {
    in.el = el; in.ei = ei; in.ej = ej; in.em = em; in.ex = ex; in.ext = ext;
  } else {
    const int32_t* src[6] = {el, ei, ej, em, ex, ext};
    for (int q = 0; q < n_in; ++q) HIPCHK(h, hipMemcpyAsync(in_d + (size_t)q * n, src[q], (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    in.el = in_d; in.ei = in_d + n; in.ej = in_d + 2 * n; in.em = in_d + 3 * n; in.ex = in_d + 4 * n;
    in.ext = ext ? in_d + 5 * n : nullptr;
  }
  HIPCHK(h, hipMemcpyAsync(par_d, par_h.data(), n_par * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemsetAsync(bad, 0, 4, h->stream));
  HIPCHK(h, hipMemsetAsync(seg_d, 0, (size_t)(L + 1) * 8, h->stream));
  HIPCHK(h, hipMemsetAsync(sums_d, 0, (size_t)L * VMR_HO_NSUM * 8, h->stream));
  HIPCHK(h, hipMemsetAsync(counts_d, 0, (size_t)L * VMR_HO_NCOUNT * 8, h->stream));

  const unsigned nb_c = (unsigned)std::max<size_t>(1, std::min<size_t>(4096, ((size_t)n + HO_TPB - 1) / HO_TPB));
  hipLaunchKernelGGL(k_ho_check, dim3(nb_c), dim3(HO_TPB), 0, h->stream, in.el, (size_t)n, L, seg_d, bad);
  HIPCHK(h, hipGetLastError());
  std::vector<u64> seg((size_t)L + 1, 0ull);
  int b = 0;
  HIPCHK(h, hipMemcpyAsync(seg.data(), seg_d, (size_t)(L + 1) * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(&b, bad, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (b & HO_BAD_SUB) return fail(h, VMR_EINVAL, "vmr_heldout_loglik: a layer subscript is out of range");
  if (b) return fail(h, VMR_EINVAL, "vmr_heldout_loglik: the list decreases in the layer subscript (el must be non-decreasing)");
  for (int l = 0; l < L; ++l)   // (what an ordered list gives; anything else would be a fault of the check, never used as a bound)
    if (seg[l] > seg[l + 1] || seg[l + 1] > n) return fail(h, VMR_EHIP, "vmr_heldout_loglik: the layers' segments are inconsistent");

  HoOut o;
  o.logp = logp ? (out_on_device ? logp : logp_d) : nullptr;
  o.mean = mean ? (out_on_device ? mean : mean_d) : nullptr;
  size_t blk0 = 0;
  for (int l = 0; l < L; ++l) {
    const size_t s0 = (size_t)seg[l], ns = (size_t)seg[l + 1] - s0;
    if (ns == 0) continue;
    const size_t nb = (ns + HO_CHUNK - 1) / HO_CHUNK;
    if (blk0 + nb > nb_all) return fail(h, VMR_EHIP, "vmr_heldout_loglik: the layers' segments are inconsistent");
    LayerPrep lp;
    if ((rc = ppc_prep_layer(h, tm, l, false, true, lp, false, false, false))) return rc;
    o.part = part + blk0 * VMR_HO_NSUM;
    o.cpart = cpart + blk0 * VMR_HO_NCOUNT;
    const double *th_l = par_d + (size_t)l * M, *la_l = par_d + (size_t)L * M + (size_t)l * K, *lgt = par_d + (size_t)L * M + (size_t)L * K;
    if (K == 2) hipLaunchKernelGGL(k_ho_lane<true>, dim3((unsigned)nb), dim3(HO_TPB), 0, h->stream, lp.p, in, s0, ns, th_l, la_l, eta, lgt, o, bad);
    else if (K <= KMAX) hipLaunchKernelGGL(k_ho_lane<false>, dim3((unsigned)nb), dim3(HO_TPB), 0, h->stream, lp.p, in, s0, ns, th_l, la_l, eta, lgt, o, bad);
    else hipLaunchKernelGGL(k_ho_group, dim3((unsigned)nb), dim3(HO_TPB), 0, h->stream, lp.p, in, s0, ns, th_l, la_l, eta, lgt, o, bad);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_lik_finish, dim3(1), dim3(HO_TPB), 0, h->stream, (const double*)o.part, (const u64*)o.cpart, nb,
                       sums_d + (size_t)l * VMR_HO_NSUM, counts_d + (size_t)l * VMR_HO_NCOUNT);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    ppc_release_layer(tm, lp);
    blk0 += nb;
  }
  HIPCHK(h, hipMemcpyAsync(&b, bad, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (b & HO_BAD_LAYER) return fail(h, VMR_EINVAL, "vmr_heldout_loglik: the list decreases in the layer subscript (el must be non-decreasing)");
  if (b & HO_BAD_SUB) return fail(h, VMR_EINVAL, "vmr_heldout_loglik: a subscript is out of range");
  if (b & HO_BAD_NEG) return fail(h, VMR_EINVAL, "vmr_heldout_loglik: a count is negative (ex and ext hold counts >= 0)");
  if (logp && !out_on_device) HIPCHK(h, hipMemcpyAsync(logp, logp_d, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
  if (mean && !out_on_device) HIPCHK(h, hipMemcpyAsync(mean, mean_d, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
  if (sums) HIPCHK(h, hipMemcpyAsync(sums, sums_d, (size_t)L * VMR_HO_NSUM * 8, hipMemcpyDeviceToHost, h->stream));
  if (counts) HIPCHK(h, hipMemcpyAsync(counts, counts_d, (size_t)L * VMR_HO_NCOUNT * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (b & LIK_BAD_NAN) return fail(h, VMR_ENAN, "vmr_heldout_loglik: a logp or a mean is NaN");
  return VMR_OK;
}
