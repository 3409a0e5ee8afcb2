// score_truth.hip -- the posterior scored against a ground-truth network where rho lives: vmr_score_truth (the f1_score /
// GridSearchCV scoring of the reference's synthetic experiments, notebooks/python/experiments/unreliable_reporters.py:189-200,
// 358-361, and utils.get_optimal_threshold, without a dense read-out per threshold and without rho crossing PCIe).
//
// One pass, k_sc_pass, walks the positions of a layer (grid (nb, L), nb of N only): a thread reads its tie's rho row once (8 K
// bytes) and the tie's one truth byte (through perm on report-list handles, where rho is stored by sorted position), and from
// them the score s, the arg-max a and the mean.  Everything it adds up is either an integer or goes through a fixed tree:
//   hist   thresholds (doubles) and the (n_thr + 1) x 2 histogram of 32-bit counters live in LDS; a tie finds its bin
//          c = #{thresholds <= s} by binary search.  In a sparse network almost every tie lands in ONE counter, which would make
//          that LDS address a serialisation point: the wave first peels two rounds of "every lane that shares the first pending
//          lane's counter" (a ballot, a popcount, one LDS add by that lane) and only what is still pending after both adds for
//          itself.  The workgroup's non-zero counters go out with one 64-bit global atomic each.
//   conf   ballots and popcounts (wave-uniform counters), one 64-bit global atomic per wave and count.
//   sums   per-thread doubles, a workgroup sum, part[l][block][4]; k_sc_finish adds a layer's partials in a fixed order.  No
//          floating-point atomics; the grid depends on N only, so the tree is the same on every device and in every run.
// The AUC (only when asked for): k_sc_pos compacts the positives' scores of a layer as order-preserving uint64 keys (slots from
// an integer cursor: the sort that follows makes their order immaterial), hipcub sorts them, and k_sc_rank lets every negative tie
// binary-search the sorted keys and add 2 #(pos > s) + #(pos = s) -- integers, one 64-bit atomic per workgroup.
#include "read_side.h"

namespace {

#define SC_TPB 256

struct ScTie {
  double s, mean;
  unsigned a;
};

// score, arg-max and mean of the row at r.  K2: K = 2, the row in one 16-byte load (rho is 256-byte aligned)
template <bool K2>
__device__ __forceinline__ ScTie sc_tie(const double* __restrict__ r, int K, int score) {
  ScTie o;
  if (K2) {
    const double2 v = *reinterpret_cast<const double2*>(r);
    const double q[2] = {v.x, v.y};
    double pr, mn;
    rho_row_prob_mean(q, 2, pr, mn);
    o.s = score == VMR_SCORE_RHO1 ? q[1] : pr;
    o.mean = mn;
    o.a = rho_row_argmax(q, 2);
  } else {
    double pr, mn;
    rho_row_prob_mean(r, K, pr, mn);
    o.s = score == VMR_SCORE_RHO1 ? r[1] : pr;
    o.mean = mn;
    o.a = rho_row_argmax(r, K);
  }
  return o;
}

// the tie of position pos of layer l, or T where the tie is left out (the diagonal with skip_diag)
__device__ __forceinline__ size_t sc_tie_of(const unsigned* __restrict__ perm, int l, size_t pos, size_t T, size_t NS, int N, int skip_diag) {
  const size_t t = perm ? (size_t)perm[(size_t)l * NS * 64 + pos] : pos;
  if (t >= T) return T;   // (never: positions below T hold ties)
  if (skip_diag) { const size_t i = t / (size_t)N; if (t - i * (size_t)N == i) return T; }
  return t;
}

// The pass.  Dynamic LDS: thr [n_thr] doubles, then cnt [(n_thr + 1) * 2] words (nothing when hist is null).
template <bool K2>
__global__ __launch_bounds__(SC_TPB) void k_sc_pass(const double* __restrict__ rho, const uint8_t* __restrict__ y, const unsigned* __restrict__ perm,
                                                    int N, int K, size_t T, size_t NS, int score, int skip_diag, int n_thr,
                                                    const double* __restrict__ thr_g, unsigned long long* __restrict__ hist,
                                                    unsigned long long* __restrict__ conf, double* __restrict__ part, int* __restrict__ bad) {
  extern __shared__ double sc_lds[];
  __shared__ double red[16];
  double* thr = sc_lds;
  unsigned* cnt = reinterpret_cast<unsigned*>(sc_lds + n_thr);
  const int l = blockIdx.y, lane = threadIdx.x & 63;
  const int nbin = hist ? (n_thr + 1) * 2 : 0;
  if (hist) {
    for (int q = threadIdx.x; q < n_thr; q += SC_TPB) thr[q] = thr_g[q];
    for (int q = threadIdx.x; q < nbin; q += SC_TPB) cnt[q] = 0u;
  }
  __syncthreads();
  unsigned c_tp = 0, c_fp = 0, c_fn = 0, c_eq = 0, c_p = 0;   // wave-uniform
  double s_all = 0.0, s_pos = 0.0, s_brier = 0.0, s_mse = 0.0;
  bool nan_seen = false;
  // (the loop bound is uniform over the workgroup: the ballots below see whole waves)
  for (size_t p0 = (size_t)blockIdx.x * SC_TPB; p0 < T; p0 += (size_t)gridDim.x * SC_TPB) {
    const size_t pos = p0 + threadIdx.x;
    size_t t = T;
    if (pos < T) t = sc_tie_of(perm, l, pos, T, NS, N, skip_diag);
    const bool in = t < T;
    ScTie v;
    v.s = 0.0; v.mean = 0.0; v.a = 0u;
    unsigned yt = 0u;
    if (in) {
      v = sc_tie<K2>(rho + ((size_t)l * T + pos) * K, K, score);
      yt = y[(size_t)l * T + t];
    }
    const bool b = yt > 0u;
    if (v.s != v.s) nan_seen = true;
    c_tp += (unsigned)__popcll(__ballot(in && v.a > 0u && b));
    c_fp += (unsigned)__popcll(__ballot(in && v.a > 0u && !b));
    c_fn += (unsigned)__popcll(__ballot(in && v.a == 0u && b));
    c_eq += (unsigned)__popcll(__ballot(in && v.a == yt));
    c_p += (unsigned)__popcll(__ballot(in && b));
    if (in) {
      const double d = v.s - (b ? 1.0 : 0.0), e = v.mean - (double)yt;
      s_all += v.s;
      if (b) s_pos += v.s;
      s_brier += d * d;
      s_mse += e * e;
    }
    if (hist) {
      // c = #{tau : thr[tau] <= s}: the first index whose threshold exceeds s
      int lo = 0, hi = in ? n_thr : 0;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (thr[mid] <= v.s) lo = mid + 1; else hi = mid;
      }
      const unsigned key = (unsigned)lo * 2u + (b ? 1u : 0u);   // (< nbin: lo <= n_thr)
      bool pending = in;
      for (int r = 0; r < 2; ++r) {
        const unsigned long long m = __ballot(pending);
        if (!m) break;   // (uniform over the wave)
        const int first = __ffsll((long long)m) - 1;
        const unsigned k0 = (unsigned)__shfl((int)key, first, 64);
        const bool mine = pending && key == k0;
        const unsigned long long same = __ballot(mine);
        if (lane == first) atomicAdd(&cnt[k0], (unsigned)__popcll(same));
        if (mine) pending = false;
      }
      if (pending) atomicAdd(&cnt[key], 1u);
    }
  }
  if (nan_seen) atomicOr(bad, 1);
  if (conf && lane == 0) {
    unsigned long long* o = conf + (size_t)l * VMR_SCORE_NCONF;
    if (c_tp) atomicAdd(o + 0, (unsigned long long)c_tp);
    if (c_fp) atomicAdd(o + 1, (unsigned long long)c_fp);
    if (c_fn) atomicAdd(o + 2, (unsigned long long)c_fn);
    if (c_eq) atomicAdd(o + 3, (unsigned long long)c_eq);
    if (c_p) atomicAdd(o + 4, (unsigned long long)c_p);
  }
  const double t0 = block_sum_n(s_all, red), t1 = block_sum_n(s_pos, red), t2 = block_sum_n(s_brier, red), t3 = block_sum_n(s_mse, red);
  if (part && threadIdx.x == 0) {
    double* o = part + ((size_t)l * gridDim.x + blockIdx.x) * VMR_SCORE_NSUM;
    o[0] = t0; o[1] = t1; o[2] = t2; o[3] = t3;
  }
  __syncthreads();   // (every wave's LDS adds are done)
  if (hist)
    for (int q = threadIdx.x; q < nbin; q += SC_TPB) {
      const unsigned c = cnt[q];
      if (c) atomicAdd(hist + (size_t)l * nbin + q, (unsigned long long)c);
    }
}

// second stage of the sums: one workgroup per layer adds the nb partials of each column in a fixed order
__global__ __launch_bounds__(SC_TPB) void k_sc_finish(const double* __restrict__ part, int nb, double* __restrict__ out) {
  __shared__ double red[16];
  const int l = blockIdx.x;
  for (int c = 0; c < VMR_SCORE_NSUM; ++c) {
    double a = 0.0;
    for (int b = threadIdx.x; b < nb; b += SC_TPB) a += part[((size_t)l * nb + b) * VMR_SCORE_NSUM + c];
    const double sum = block_sum_n(a, red);
    if (threadIdx.x == 0) out[l * VMR_SCORE_NSUM + c] = sum;
  }
}

// the positives' keys of layer l: keys[0, P), slots from the cursor (sorted afterwards, so any order will do)
template <bool K2>
__global__ __launch_bounds__(SC_TPB) void k_sc_pos(const double* __restrict__ rho, const uint8_t* __restrict__ y, const unsigned* __restrict__ perm,
                                                   int l, int N, int K, size_t T, size_t NS, int score, int skip_diag,
                                                   unsigned long long* __restrict__ keys, unsigned long long P, unsigned long long* __restrict__ cursor,
                                                   int* __restrict__ bad) {
  for (size_t pos = (size_t)blockIdx.x * SC_TPB + threadIdx.x; pos < T; pos += (size_t)gridDim.x * SC_TPB) {
    const size_t t = sc_tie_of(perm, l, pos, T, NS, N, skip_diag);
    if (t >= T || y[(size_t)l * T + t] == 0) continue;
    const ScTie v = sc_tie<K2>(rho + ((size_t)l * T + pos) * K, K, score);
    const unsigned long long at = atomicAdd(cursor, 1ull);
    if (at >= P) { atomicOr(bad, 2); continue; }   // (the count and the walk disagree: never written out of bounds)
    keys[at] = order_key(v.s);
  }
}

// every negative tie of layer l against the sorted positives pk[0, P): acc += 2 #(pos > s) + #(pos = s); *nneg += 1
template <bool K2>
__global__ __launch_bounds__(SC_TPB) void k_sc_rank(const double* __restrict__ rho, const uint8_t* __restrict__ y, const unsigned* __restrict__ perm,
                                                    int l, int N, int K, size_t T, size_t NS, int score, int skip_diag,
                                                    const unsigned long long* __restrict__ pk, unsigned long long P,
                                                    unsigned long long* __restrict__ acc) {
  __shared__ unsigned long long tot;
  if (threadIdx.x == 0) tot = 0ull;
  __syncthreads();
  unsigned long long mine = 0;
  for (size_t pos = (size_t)blockIdx.x * SC_TPB + threadIdx.x; pos < T; pos += (size_t)gridDim.x * SC_TPB) {
    const size_t t = sc_tie_of(perm, l, pos, T, NS, N, skip_diag);
    if (t >= T || y[(size_t)l * T + t] != 0) continue;
    const ScTie v = sc_tie<K2>(rho + ((size_t)l * T + pos) * K, K, score);
    const unsigned long long key = order_key(v.s);
    unsigned long long lo = 0, hi = P;   // first index with pk >= key
    while (lo < hi) {
      const unsigned long long mid = lo + ((hi - lo) >> 1);
      if (pk[mid] < key) lo = mid + 1; else hi = mid;
    }
    const unsigned long long first = lo;
    hi = P;                              // first index with pk > key
    while (lo < hi) {
      const unsigned long long mid = lo + ((hi - lo) >> 1);
      if (pk[mid] <= key) lo = mid + 1; else hi = mid;
    }
    mine += 2ull * (P - lo) + (lo - first);
  }
  mine = wave_sum_ull(mine);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&tot, mine);
  __syncthreads();
  if (threadIdx.x == 0 && tot) atomicAdd(acc, tot);
}

}  // namespace

extern "C" int vmr_score_truth(vmr_handle h, const uint8_t* y_true, int y_true_on_device, int score, int skip_diagonal, int n_thr,
                               const double* thresholds, uint64_t* hist, uint64_t* conf, double* sums, double* auc, uint64_t* auc_pairs) {
  if (!h) return VMR_EINVAL;
  if (!y_true) return fail(h, VMR_EINVAL, "vmr_score_truth: y_true is NULL");
  if (!hist && !conf && !sums && !auc && !auc_pairs) return fail(h, VMR_EINVAL, "vmr_score_truth: every output is NULL");
  if (score != VMR_SCORE_RHO1 && score != VMR_SCORE_PROB) return fail(h, VMR_EINVAL, "vmr_score_truth: score must be VMR_SCORE_RHO1 or VMR_SCORE_PROB");
  if (n_thr < 0 || n_thr > VMR_SCORE_MAX_THR) return fail(h, VMR_EINVAL, "vmr_score_truth: n_thr must lie in [0, VMR_SCORE_MAX_THR]");
  if (hist && n_thr > 0) {
    if (!thresholds) return fail(h, VMR_EINVAL, "vmr_score_truth: thresholds is NULL");
    for (int q = 0; q < n_thr; ++q) {
      if (!std::isfinite(thresholds[q])) return fail(h, VMR_EINVAL, "vmr_score_truth: a threshold is not finite");
      if (q && thresholds[q] < thresholds[q - 1]) return fail(h, VMR_EINVAL, "vmr_score_truth: the thresholds decrease");
    }
  }
  if (!h->have_state) return fail(h, VMR_ESTATE, "vmr_set_state must be called before vmr_score_truth");
  const Geo& g = h->g;
  const int L = g.L, K = g.K;
  const size_t T = (size_t)g.N * g.N, ties = (size_t)L * T, NS = (T + 63) / 64;
  const bool want_auc = auc || auc_pairs;
  // T < 2^32 (perm holds 32-bit ties), so 2 P Q <= T^2 / 2 < 2^63 always; the positives' sort takes an int count
  if (T >= 0xffffffffull) return fail(h, VMR_EINVAL, "vmr_score_truth: 2^32 ties or more in one layer");
  HIPCHK(h, hipSetDevice(h->device));
  { const int rce = ensure_rho_ext(h); if (rce) return rce; }

  const int nh = hist ? n_thr : 0;            // thresholds the pass uses
  const size_t nbin = (size_t)(nh + 1) * 2;
  const int nb = (int)grid_for(T, SC_TPB, 1024);      // (of N only: the summation tree is the same on every device)
  const size_t smem = hist ? (size_t)nh * 8 + nbin * 4 : 0;
  Tmp tm(h);
  int rc;
  int* bad = nullptr;
  uint8_t* yd = nullptr;
  double *thr_d = nullptr, *part = nullptr, *sums_d = nullptr;
  unsigned long long *hist_d = nullptr, *conf_d = nullptr;
  if ((rc = tm.get(&bad, 4, "a flag")) || (rc = tm.get(&conf_d, (size_t)L * VMR_SCORE_NCONF * 8, "the counts")) ||
      (rc = tm.get(&part, (size_t)L * nb * VMR_SCORE_NSUM * 8, "the partial sums")) || (rc = tm.get(&sums_d, (size_t)L * VMR_SCORE_NSUM * 8, "the sums")))
    return rc;
  if (hist && ((rc = tm.get(&hist_d, (size_t)L * nbin * 8, "the histogram")) || (rc = tm.get(&thr_d, (size_t)nh * 8, "the thresholds")))) return rc;
  const uint8_t* yt = y_true;
  if (!y_true_on_device) {
    if ((rc = tm.get(&yd, ties, "the ground truth"))) return rc;
    HIPCHK(h, hipMemcpyAsync(yd, y_true, ties, hipMemcpyHostToDevice, h->stream));
    yt = yd;
  }
  HIPCHK(h, hipMemsetAsync(bad, 0, 4, h->stream));
  HIPCHK(h, hipMemsetAsync(conf_d, 0, (size_t)L * VMR_SCORE_NCONF * 8, h->stream));
  if (hist) {
    HIPCHK(h, hipMemsetAsync(hist_d, 0, (size_t)L * nbin * 8, h->stream));
    if (nh) HIPCHK(h, hipMemcpyAsync(thr_d, thresholds, (size_t)nh * 8, hipMemcpyHostToDevice, h->stream));
  }
  {
    if (smem > 48 * 1024)
      HIPCHK(h, hipFuncSetAttribute(K == 2 ? reinterpret_cast<const void*>(k_sc_pass<true>) : reinterpret_cast<const void*>(k_sc_pass<false>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    if (K == 2) hipLaunchKernelGGL(k_sc_pass<true>, dim3((unsigned)nb, (unsigned)L), dim3(SC_TPB), smem, h->stream, (const double*)h->rho, yt, (const unsigned*)h->perm,
                                   g.N, K, T, NS, score, skip_diagonal ? 1 : 0, nh, (const double*)thr_d, hist_d, conf_d, part, bad);
    else hipLaunchKernelGGL(k_sc_pass<false>, dim3((unsigned)nb, (unsigned)L), dim3(SC_TPB), smem, h->stream, (const double*)h->rho, yt, (const unsigned*)h->perm,
                            g.N, K, T, NS, score, skip_diagonal ? 1 : 0, nh, (const double*)thr_d, hist_d, conf_d, part, bad);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_sc_finish, dim3((unsigned)L), dim3(SC_TPB), 0, h->stream, (const double*)part, nb, sums_d);
    HIPCHK(h, hipGetLastError());
  }
  std::vector<unsigned long long> conf_h((size_t)L * VMR_SCORE_NCONF, 0ull);
  HIPCHK(h, hipMemcpyAsync(conf_h.data(), conf_d, conf_h.size() * 8, hipMemcpyDeviceToHost, h->stream));
  if (hist) HIPCHK(h, hipMemcpyAsync(hist, hist_d, (size_t)L * nbin * 8, hipMemcpyDeviceToHost, h->stream));
  if (sums) HIPCHK(h, hipMemcpyAsync(sums, sums_d, (size_t)L * VMR_SCORE_NSUM * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (conf) memcpy(conf, conf_h.data(), conf_h.size() * 8);

  if (want_auc) {
    const unsigned long long n_ties = (unsigned long long)T - (skip_diagonal ? (unsigned long long)g.N : 0ull);
    unsigned long long Pmax = 0;
    for (int l = 0; l < L; ++l) {
      const unsigned long long P = conf_h[(size_t)l * VMR_SCORE_NCONF + 4];
      if (P >= 0x7fffffffull) return fail(h, VMR_EINVAL, "vmr_score_truth: 2^31 positives or more in a layer (the sort of their scores takes an int count)");
      if (P && n_ties - P && P > 0x3fffffffffffffffull / (n_ties - P))
        return fail(h, VMR_EINVAL, "vmr_score_truth: 2 P Q reaches 2^63 (the pair counts are 64-bit integers)");
      Pmax = std::max(Pmax, P);
    }
    unsigned long long *pk = nullptr, *pk2 = nullptr, *acc = nullptr;   // acc: per layer the pair count, then the cursor
    void* ts = nullptr;
    size_t tb = 0;
    if ((rc = tm.get(&acc, (size_t)L * 16, "the pair counts"))) return rc;
    HIPCHK(h, hipMemsetAsync(acc, 0, (size_t)L * 16, h->stream));
    if (Pmax) {
      if ((rc = tm.get(&pk, Pmax * 8, "the positives' scores")) || (rc = tm.get(&pk2, Pmax * 8, "the positives' scores"))) return rc;
      hipcub::DoubleBuffer<unsigned long long> db(pk, pk2);
      HIPCHK(h, hipcub::DeviceRadixSort::SortKeys(nullptr, tb, db, (int)Pmax, 0, 64, h->stream));
      if ((rc = tm.get(&ts, tb, "the sort of the positives"))) return rc;
    }
    const unsigned gridw = grid_for(T, SC_TPB, 8192);
    for (int l = 0; l < L; ++l) {
      const unsigned long long P = conf_h[(size_t)l * VMR_SCORE_NCONF + 4], Q = n_ties - P;
      if (!P || !Q) continue;
      hipcub::DoubleBuffer<unsigned long long> db(pk, pk2);
      size_t tb2 = tb;
      if (K == 2) hipLaunchKernelGGL(k_sc_pos<true>, dim3(gridw), dim3(SC_TPB), 0, h->stream, (const double*)h->rho, yt, (const unsigned*)h->perm, l, g.N, K, T, NS,
                                     score, skip_diagonal ? 1 : 0, pk, P, acc + 2 * l + 1, bad);
      else hipLaunchKernelGGL(k_sc_pos<false>, dim3(gridw), dim3(SC_TPB), 0, h->stream, (const double*)h->rho, yt, (const unsigned*)h->perm, l, g.N, K, T, NS,
                              score, skip_diagonal ? 1 : 0, pk, P, acc + 2 * l + 1, bad);
      HIPCHK(h, hipGetLastError());
      HIPCHK(h, hipcub::DeviceRadixSort::SortKeys(ts, tb2, db, (int)P, 0, 64, h->stream));
      const unsigned long long* sorted = db.Current();
      if (K == 2) hipLaunchKernelGGL(k_sc_rank<true>, dim3(gridw), dim3(SC_TPB), 0, h->stream, (const double*)h->rho, yt, (const unsigned*)h->perm, l, g.N, K, T, NS,
                                     score, skip_diagonal ? 1 : 0, sorted, P, acc + 2 * l);
      else hipLaunchKernelGGL(k_sc_rank<false>, dim3(gridw), dim3(SC_TPB), 0, h->stream, (const double*)h->rho, yt, (const unsigned*)h->perm, l, g.N, K, T, NS,
                              score, skip_diagonal ? 1 : 0, sorted, P, acc + 2 * l);
      HIPCHK(h, hipGetLastError());
      HIPCHK(h, hipStreamSynchronize(h->stream));   // (the next layer reuses the key buffers)
    }
    std::vector<unsigned long long> acc_h((size_t)L * 2, 0ull);
    HIPCHK(h, hipMemcpyAsync(acc_h.data(), acc, acc_h.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int l = 0; l < L; ++l) {
      const unsigned long long P = conf_h[(size_t)l * VMR_SCORE_NCONF + 4], Q = n_ties - P, U2 = acc_h[(size_t)2 * l];
      if (auc_pairs) { auc_pairs[2 * l] = U2; auc_pairs[2 * l + 1] = Q; }
      if (auc) auc[l] = (P && Q) ? (double)U2 / (2.0 * (double)P * (double)Q) : __builtin_nan("");
    }
  }
  int b = 0;
  HIPCHK(h, hipMemcpyAsync(&b, bad, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (b & 2) return fail(h, VMR_EHIP, "vmr_score_truth: the count of the positives and the walk over them disagree");
  if (b) return fail(h, VMR_ENAN, "vmr_score_truth: a score is NaN");
  return VMR_OK;
}
