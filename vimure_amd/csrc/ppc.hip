// ppc.hip -- posterior expected reports and their AUC on the device: vmr_mean_poisson_size, vmr_mean_poisson, vmr_report_auc
// (the reference's VimureModel._calculate_mean_poisson, model.py:1220-1293, and utils.calculate_AUC, utils.py:40-66, with mask = R).
//
// Over the support S = {(l,i,j,m) : R[l,i,j,m] != 0}, in lexicographic (l,i,j,m) order:
//     mp[l,i,j,m] = sum_k rho[l,i,j,k] (G_theta[l,m] G_lambda[l,k] + G_nu XT[l,i,j,m]),   XT = X[l,j,i,m] with mutuality, else 0
// One lane per support element, a lane group per tie: no sum crosses lanes, so every value is the same from run to run.
//
// The sweep layout (sweep_sl.h) keeps a tie's reports by sorted position, rotated, and reaches ties only through perm: neither
// a tie's own count of reporter m nor its mirror tie's is addressable.  Per call and per layer the reports are therefore
// re-indexed TIE-MAJOR: key tie << mb | m, value x << 1 | R, one radix sort, row starts by binary search in the sorted keys
// (layer-local: fewer than 2^31 slots per layer, hipcub's item count).  Dense tiles read X and the mask words directly.
//
// Support offsets: per tie in natural order the support size (M for all-ones rows, the list length of listed rows, the
// popcount of the mask words, 0 for empty rows) and the number of positives (support elements with X > 0), exclusive 64-bit
// scans of both.  An element's output index is its tie's offset plus its rank in the tie's walk (ballots inside the group), so
// positives and negatives land at fixed places without atomics.
//
// AUC = (#{(p,n) : mp_p > mp_n} + #{mp_p = mp_n} / 2) / (P Q): the positives' scores are sorted once (as order-preserving
// uint64 keys), the negatives' come in chunks of ties sized to free memory and hipcub's int item count; each chunk is sorted (a
// wave's binary searches then share cache lines) and every negative adds 2 #(pos > s) + #(pos = s), summed in uint64 -- exact,
// order-free, the same from run to run.
#include "read_side.h"

namespace {

#define PPC_XMASK 0xfffffu   // packed entries (sweep_sl.h): bits 0..19 y * Mp + m, bit 20 R, bits 21..31 x
#define PPC_MODE_WRITE 0
#define PPC_MODE_POS 1
#define PPC_MODE_NEG 2

// the score in the reference's order and roundings: PoissonMean_k = theta_m lambda_k + nu XT, then sum_k rho_k PoissonMean_k,
// k ascending, every product and sum rounded on its own (no contraction to FMA: the AUC counts exact ties, and a value one ulp
// off the reference's would split a tie it has).  The pragma is what holds the compiler to that: __dmul_rn / __dadd_rn are inlined
// header code and were contracted to v_fma_f64 / v_fmac_f64 all the same (rho_row.h's convention and its reason).
__device__ __forceinline__ double ppc_score(const PpcLayer& p, const double* __restrict__ r, unsigned m, unsigned xt) {
#pragma clang fp contract(off)
  const double gt = p.gth[m], nx = *p.gnu * (double)xt;
  double s = 0.0;
  for (int k = 0; k < p.K; ++k) {
    const double a = gt * p.gla[k];
    const double mu = a + nx;
    const double t = r[k] * mu;
    s = s + t;
  }
  return s;
}

// per tie: support size and positives; entry T of both is 0 (the exclusive scans then end in the totals)
__global__ __launch_bounds__(256) void k_ppc_count(PpcLayer p, unsigned long long* __restrict__ sup, unsigned long long* __restrict__ pc) {
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t <= p.T; t += (size_t)gridDim.x * 256) {
    if (t == p.T) { sup[t] = 0; if (pc) pc[t] = 0; continue; }
    const int c = p.cls[t];
    sup[t] = mask_row_size(p, t, c);
    if (!pc) continue;
    unsigned long long n = 0;
    if (c != 0) {
      if (p.X) {   // dense tiles: the support's non-zero counts
        for (int m = 0; m < p.M; ++m) {
          const bool in = c == 1 || ((p.Rb[t * p.W + (m >> 6)] >> (m & 63)) & 1ull);
          n += (in && p.X[t * p.Mp + m]) ? 1u : 0u;
        }
      } else {     // report lists: the tie's reports that R keeps
        for (unsigned e = p.ip[t]; e < p.ip[t + 1]; ++e) n += p.iv[e] & 1u;
      }
    }
    pc[t] = n;
  }
}

// tie-major keys of one layer's report lists: one wave per step of 64 sorted positions (sweep_sl.h); empty slots get the key
// T << mb, past every tie's
__global__ __launch_bounds__(256) void k_ppc_keys(const unsigned* __restrict__ El, const unsigned* __restrict__ EXl, const unsigned* __restrict__ rsl,
                                                  const unsigned* __restrict__ perml, size_t NS, int Mp, int mb, unsigned long long T,
                                                  unsigned long long* __restrict__ keys, unsigned* __restrict__ vals) {
  const int lane = threadIdx.x & 63;
  for (size_t s = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); s < NS; s += (size_t)gridDim.x * 4) {
    const unsigned ea = rsl[s], R = (rsl[s + 1] - ea) >> 6;
    const unsigned t = perml[s * 64 + lane];
    for (unsigned r = 0; r < R; ++r) {
      const size_t slot = (size_t)ea + (size_t)r * 64 + lane;
      const unsigned e = El[slot];
      unsigned row, xr;
      if (EXl) { row = e; xr = EXl[slot]; }
      else { row = e & PPC_XMASK; xr = ((e >> 21) << 1) | ((e >> 20) & 1u); }
      const bool on = (xr >> 1) != 0u && t != 0xffffffffu;
      keys[slot] = on ? (((unsigned long long)t << mb) | (row % (unsigned)Mp)) : (T << mb);
      vals[slot] = on ? xr : 0u;
    }
  }
}

// row starts of the sorted index: ip[t] = first key >= t << mb, t in [0, T]
__global__ __launch_bounds__(256) void k_ppc_rows(const unsigned long long* __restrict__ keys, unsigned n, int mb, size_t T, unsigned* __restrict__ ip) {
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t <= T; t += (size_t)gridDim.x * 256) {
    const unsigned long long key = (unsigned long long)t << mb;
    unsigned a = 0, b = n;
    while (a < b) { const unsigned c = a + ((b - a) >> 1); if (keys[c] < key) a = c + 1; else b = c; }
    ip[t] = a;
  }
}

// tie -> sorted position
__global__ __launch_bounds__(256) void k_ppc_inv(const unsigned* __restrict__ perml, size_t NP, unsigned* __restrict__ inv) {
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < NP; q += (size_t)gridDim.x * 256) {
    const unsigned t = perml[q];
    if (t != 0xffffffffu) inv[t] = (unsigned)q;
  }
}

// The walk: a group of G lanes per tie of [t0, t1) takes the tie's support reporters in ascending m, G at a time (the per-tie
// set-up and the per-lane reporter of read_side.h's support walk; the loop is its own: a window of ties, grid-stride, two ranks).
//   WRITE: subs (any pointer may be null) and vals at off[t] + rank - obase
//   POS:   keys of the positives at poff[t] + positive rank - obase
//   NEG:   keys of the negatives at off[t] - poff[t] + negative rank - obase
template <int MODE>
__global__ __launch_bounds__(256) void k_ppc_walk(PpcLayer p, int G, size_t t0, size_t t1, const unsigned long long* __restrict__ off,
                                                  const unsigned long long* __restrict__ poff, unsigned long long obase, unsigned long long lim,
                                                  int32_t* __restrict__ sl,
                                                  int32_t* __restrict__ si, int32_t* __restrict__ sj, int32_t* __restrict__ sm,
                                                  double* __restrict__ vals, unsigned long long* __restrict__ keys, int* __restrict__ bad) {
  const WalkGroup g = walk_group(G);
  const size_t gpb = 256 / G, ngr = (size_t)gridDim.x * gpb;
  for (size_t t = t0 + (size_t)blockIdx.x * gpb + threadIdx.x / G; t < t1; t += ngr) {   // (uniform over the group)
    const int c = p.cls[t];
    if (c == 0) continue;
    const WalkTie w = walk_tie(p, t, c);
    unsigned long long js = 0, jp = 0;
    const unsigned long long o_all = off[t], o_pos = (MODE == PPC_MODE_WRITE) ? 0ull : poff[t];
    for (unsigned c0 = 0; c0 < w.nc; c0 += (unsigned)G) {
      unsigned m;
      const bool in = walk_reporter(p, w, t, c0 + (unsigned)g.gl, m);
      unsigned x = 0, xt = 0;
      if (in) {
        if (MODE != PPC_MODE_WRITE) x = ppc_x(p, t, m);
        if (p.mut) xt = ppc_x(p, w.tm, m);
      }
      const bool pos = in && x != 0u;
      const unsigned long long bs = __ballot(in) & g.gmask, bp = __ballot(pos) & g.gmask;
      const unsigned long long rk = js + (unsigned long long)__popcll(bs & g.lt), rp = jp + (unsigned long long)__popcll(bp & g.lt);
      const bool take = in && (MODE == PPC_MODE_WRITE || (MODE == PPC_MODE_POS) == pos);
      if (take) {
        const double v = ppc_score(p, w.row, m, xt);
        if (v != v) atomicOr(bad, 1);
        const unsigned long long at = MODE == PPC_MODE_WRITE ? o_all + rk - obase
                                    : MODE == PPC_MODE_POS ? o_pos + rp - obase : (o_all - o_pos) + (rk - rp) - obase;
        if (at >= lim) {
          atomicOr(bad, 2);   // (the counts and the walk disagree: never written out of bounds)
        } else if (MODE == PPC_MODE_WRITE) {
          vals[at] = v;
          if (sl) sl[at] = p.l;
          if (si) si[at] = (int32_t)w.i;
          if (sj) sj[at] = (int32_t)w.j;
          if (sm) sm[at] = (int32_t)m;
        } else {
          keys[at] = order_key(v);
        }
      }
      js += (unsigned long long)__popcll(bs);
      jp += (unsigned long long)__popcll(bp);
    }
  }
}

// every negative s adds 2 #(pos > s) + #(pos = s); per-workgroup uint64 sums, one integer atomic each (order-free)
__global__ __launch_bounds__(256) void k_ppc_rank(const unsigned long long* __restrict__ pos, unsigned long long P, const unsigned long long* __restrict__ neg,
                                                  unsigned long long n, unsigned long long* __restrict__ acc) {
  __shared__ unsigned long long red[4];
  unsigned long long v = 0;
  for (unsigned long long q = (unsigned long long)blockIdx.x * 256 + threadIdx.x; q < n; q += (unsigned long long)gridDim.x * 256) {
    const unsigned long long s = neg[q];
    unsigned long long a = 0, b = P;
    while (a < b) { const unsigned long long c = a + ((b - a) >> 1); if (pos[c] < s) a = c + 1; else b = c; }
    unsigned long long u = a, e = P;
    while (u < e) { const unsigned long long c = u + ((e - u) >> 1); if (pos[c] <= s) u = c + 1; else e = c; }
    v += 2ull * (P - u) + (u - a);
  }
  v = wave_sum_ull(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long s = red[0] + red[1] + red[2] + red[3];
    if (s) atomicAdd(acc, s);
  }
}

}  // namespace

int ppc_layer_mask(vmr_ctx* h, int l, PpcLayer& p) {
  const Geo& g = h->g;
  const size_t T = (size_t)g.N * g.N;
  memset(&p, 0, sizeof p);
  p.l = l; p.N = g.N; p.M = g.M; p.Mp = g.Mp; p.K = g.K; p.W = g.W; p.mut = g.mut; p.T = T;
  p.mb = 1;
  while ((1ll << p.mb) < (long long)g.Mp) ++p.mb;
  p.cls = h->rcls + (size_t)l * T;
  p.Rb = h->Rb ? h->Rb + (size_t)l * T * g.W : nullptr;
  if (h->rq) {
    p.rq = h->rq + (size_t)l * (T + 1);
    unsigned long long rb = 0;
    HIPCHK(h, hipMemcpy(&rb, h->rbase + l, 8, hipMemcpyDeviceToHost));
    p.Rm = h->Rm + rb;
  }
  return VMR_OK;
}

int ppc_prep_layer(vmr_ctx* h, Tmp& tm, int l, bool positives, bool walk, LayerPrep& lp, bool want_index, bool offsets, bool mirror) {
  const Geo& g = h->g;
  const size_t T = (size_t)g.N * g.N, NS = (T + 63) / 64;
  const ParOff o = par_off(g.L, g.Mp, g.K);
  PpcLayer& p = lp.p;
  int rc;
  if ((rc = ppc_layer_mask(h, l, p))) return rc;
  p.rho = h->rho + (size_t)l * T * g.K;
  p.gth = h->par + o.G_th + (size_t)l * g.Mp;
  p.gla = h->par + o.G_la + (size_t)l * g.K;
  p.gnu = h->par + o.sc + SC_G_NU;
  auto take = [&](auto** q, size_t bytes, const char* what) { const int rc = tm.get(q, bytes, what); if (!rc) lp.mine.push_back(*q); return rc; };
  const bool index = h->sparse && (want_index || positives || (walk && g.mut && mirror));   // the counts are needed: positives, or XT
  if (h->sparse) {
    if (walk) {
      unsigned* inv = nullptr;
      if ((rc = take(&inv, T * 4, "the tie -> position table"))) return rc;
      hipLaunchKernelGGL(k_ppc_inv, dim3(grid_for(NS * 64)), dim3(256), 0, h->stream, h->perm + (size_t)l * NS * 64, NS * 64, inv);
      HIPCHK(h, hipGetLastError());
      p.inv = inv;
    }
    if (index) {
      unsigned long long eb = 0;
      unsigned slots = 0;
      HIPCHK(h, hipMemcpy(&eb, h->ebase + l, 8, hipMemcpyDeviceToHost));
      HIPCHK(h, hipMemcpy(&slots, h->rs + (size_t)l * (NS + 1) + NS, 4, hipMemcpyDeviceToHost));
      if (slots >= 0x7fffffffu) return fail(h, VMR_EINVAL, "more than 2^31 report slots in one layer (the tie-major index sorts a layer at once)");
      const int nsl = (int)slots;
      unsigned long long *k0 = nullptr, *k1 = nullptr;
      unsigned *v0 = nullptr, *v1 = nullptr, *ip = nullptr;
      void* ts = nullptr;
      if ((rc = take(&k0, (size_t)nsl * 8, "the report index")) || (rc = take(&k1, (size_t)nsl * 8, "the report index")) ||
          (rc = take(&v0, (size_t)nsl * 4, "the report index")) || (rc = take(&v1, (size_t)nsl * 4, "the report index")) ||
          (rc = take(&ip, (T + 1) * 4, "the report index rows")))
        return rc;
      int bits = p.mb;
      while (bits < 64 && ((unsigned long long)T >> (bits - p.mb)) != 0) ++bits;   // T << mb < 2^bits
      size_t tb = 0;
      HIPCHK(h, hipcub::DeviceRadixSort::SortPairs(nullptr, tb, k0, k1, v0, v1, nsl, 0, bits, h->stream));
      if ((rc = take(&ts, tb, "the report index sort"))) return rc;
      hipLaunchKernelGGL(k_ppc_keys, dim3(grid_for(NS, 4, 8192)), dim3(256), 0, h->stream, h->E + eb, h->EX ? h->EX + eb : nullptr,
                         h->rs + (size_t)l * (NS + 1), h->perm + (size_t)l * NS * 64, NS, g.Mp, p.mb, (unsigned long long)T, k0, v0);
      HIPCHK(h, hipGetLastError());
      HIPCHK(h, hipcub::DeviceRadixSort::SortPairs(ts, tb, k0, k1, v0, v1, nsl, 0, bits, h->stream));
      hipLaunchKernelGGL(k_ppc_rows, dim3(grid_for(T + 1)), dim3(256), 0, h->stream, k1, (unsigned)nsl, p.mb, T, ip);
      HIPCHK(h, hipGetLastError());
      tm.release(ts); tm.release(k0); tm.release(v0);
      p.ik = k1; p.iv = v1; p.ip = ip;
    }
  } else {
    p.X = h->X + (size_t)l * T * g.Mp;
  }
  if (!offsets) return VMR_OK;
  unsigned long long *sup = nullptr, *pc = nullptr;
  if ((rc = take(&sup, (T + 1) * 8, "the support sizes")) || (rc = take(&lp.off, (T + 1) * 8, "the support offsets"))) return rc;
  if (positives && ((rc = take(&pc, (T + 1) * 8, "the positives' counts")) || (rc = take(&lp.poff, (T + 1) * 8, "the positives' offsets")))) return rc;
  hipLaunchKernelGGL(k_ppc_count, dim3(grid_for(T + 1)), dim3(256), 0, h->stream, p, sup, pc);
  HIPCHK(h, hipGetLastError());
  size_t tb = 0;
  void* ts = nullptr;
  HIPCHK(h, hipcub::DeviceScan::ExclusiveSum(nullptr, tb, sup, lp.off, (int)(T + 1), h->stream));
  if ((rc = take(&ts, tb, "the support scan"))) return rc;
  HIPCHK(h, hipcub::DeviceScan::ExclusiveSum(ts, tb, sup, lp.off, (int)(T + 1), h->stream));
  if (positives) HIPCHK(h, hipcub::DeviceScan::ExclusiveSum(ts, tb, pc, lp.poff, (int)(T + 1), h->stream));
  HIPCHK(h, hipMemcpyAsync(&lp.nsup, lp.off + T, 8, hipMemcpyDeviceToHost, h->stream));
  if (positives) HIPCHK(h, hipMemcpyAsync(&lp.npos, lp.poff + T, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  tm.release(ts); tm.release(sup);
  if (pc) tm.release(pc);
  return VMR_OK;
}

void ppc_release_layer(Tmp& tm, LayerPrep& lp) {
  for (void* q : lp.mine) tm.release(q);
  lp.mine.clear();
}

namespace {

// the last tie t1 in (t0, T] with f(t1) - f(t0) <= cap, where f(t) = a[t] - (b ? b[t] : 0) (a row never exceeds M <= cap)
static int cut_ties(vmr_ctx* h, const unsigned long long* a, const unsigned long long* b, size_t t0, size_t T, unsigned long long cap, size_t* t1) {
  auto f = [&](size_t t, unsigned long long* v) {
    unsigned long long x = 0, y = 0;
    HIPCHK(h, hipMemcpy(&x, a + t, 8, hipMemcpyDeviceToHost));
    if (b) HIPCHK(h, hipMemcpy(&y, b + t, 8, hipMemcpyDeviceToHost));
    *v = x - y;
    return VMR_OK;
  };
  unsigned long long f0 = 0, fT = 0;
  int rc;
  if ((rc = f(t0, &f0)) || (rc = f(T, &fT))) return rc;
  if (fT - f0 <= cap) { *t1 = T; return VMR_OK; }
  size_t lo = t0 + 1, hi = T;   // f(lo) - f0 <= cap (one row), f(hi) - f0 > cap
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    unsigned long long fm = 0;
    if ((rc = f(mid, &fm))) return rc;
    if (fm - f0 <= cap) lo = mid; else hi = mid;
  }
  *t1 = lo;
  return VMR_OK;
}

static int check_handle(vmr_ctx* h, int layer, const char* fn) {
  if (!h->have_state) return fail(h, VMR_ESTATE, (std::string("vmr_set_state must be called before ") + fn).c_str());
  if (layer >= h->g.L) return fail(h, VMR_EINVAL, (std::string(fn) + ": layer out of range").c_str());
  HIPCHK(h, hipSetDevice(h->device));
  return ensure_rho_ext(h);
}

static int bad_check(vmr_ctx* h, const int* bad_dev, const char* fn) {
  int bad = 0;
  HIPCHK(h, hipMemcpyAsync(&bad, bad_dev, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (bad & 2) return fail(h, VMR_EHIP, (std::string(fn) + ": the support counts and the walk over it disagree").c_str());
  if (bad) return fail(h, VMR_ENAN, (std::string(fn) + ": an expected report is NaN").c_str());
  return VMR_OK;
}

}  // namespace

extern "C" int vmr_mean_poisson_size(vmr_handle h, int layer, uint64_t* n) {
  if (!h || !n) return VMR_EINVAL;
  int rc = check_handle(h, layer, "vmr_mean_poisson_size");
  if (rc) return rc;
  Tmp tm(h);
  unsigned long long tot = 0;
  for (int l = (layer < 0 ? 0 : layer); l < (layer < 0 ? h->g.L : layer + 1); ++l) {
    LayerPrep lp;
    if ((rc = ppc_prep_layer(h, tm, l, false, false, lp))) return rc;
    tot += lp.nsup;
    ppc_release_layer(tm, lp);
  }
  *n = tot;
  return VMR_OK;
}

extern "C" int vmr_mean_poisson(vmr_handle h, int layer, uint64_t n, int32_t* sl, int32_t* si, int32_t* sj, int32_t* sm, double* vals,
                                int out_on_device) {
  if (!h || !vals) return VMR_EINVAL;
  int rc = check_handle(h, layer, "vmr_mean_poisson");
  if (rc) return rc;
  const int l0 = layer < 0 ? 0 : layer, l1 = layer < 0 ? h->g.L : layer + 1;
  uint64_t need = 0;
  if ((rc = vmr_mean_poisson_size(h, layer, &need))) return rc;
  if (n < need) {
    char msg[160];
    snprintf(msg, sizeof msg, "vmr_mean_poisson: the output holds %llu values, the support has %llu", (unsigned long long)n, (unsigned long long)need);
    return fail(h, VMR_EINVAL, msg);
  }
  Tmp tm(h);
  int* bad = nullptr;
  if ((rc = tm.get(&bad, 4, "a flag"))) return rc;
  HIPCHK(h, hipMemsetAsync(bad, 0, 4, h->stream));
  const int G = pow2_lanes((size_t)h->g.M);
  const size_t T = (size_t)h->g.N * h->g.N;
  unsigned long long base = 0;   // output index of the layer's first value
  for (int l = l0; l < l1; ++l) {
    LayerPrep lp;
    if ((rc = ppc_prep_layer(h, tm, l, false, true, lp))) return rc;
    if (out_on_device) {
      hipLaunchKernelGGL(k_ppc_walk<PPC_MODE_WRITE>, dim3(grid_for(T * G, 256, 65536)), dim3(256), 0, h->stream, lp.p, G, (size_t)0, T, lp.off,
                         (const unsigned long long*)nullptr, 0ull, lp.nsup, sl ? sl + base : nullptr, si ? si + base : nullptr, sj ? sj + base : nullptr,
                         sm ? sm + base : nullptr, vals + base, (unsigned long long*)nullptr, bad);
      HIPCHK(h, hipGetLastError());
    } else if (lp.nsup) {
      // host output: chunks of ties through device staging
      const unsigned long long cap = std::min<unsigned long long>(lp.nsup, 1ull << 25);
      const int nsubs = (sl != nullptr) + (si != nullptr) + (sj != nullptr) + (sm != nullptr);
      double* dv = nullptr;
      int32_t* ds = nullptr;
      if ((rc = tm.get(&dv, cap * 8, "the staging of the expected reports")) ||
          (nsubs && (rc = tm.get(&ds, cap * 4 * nsubs, "the staging of the subscripts"))))
        return rc;
      int32_t* dsub[4] = {nullptr, nullptr, nullptr, nullptr};
      int32_t* hsub[4] = {sl, si, sj, sm};
      for (int q = 0, u = 0; q < 4; ++q) if (hsub[q]) dsub[q] = ds + (size_t)(u++) * cap;
      for (size_t t0 = 0; t0 < T;) {
        size_t t1 = T;
        if ((rc = cut_ties(h, lp.off, nullptr, t0, T, cap, &t1))) return rc;
        unsigned long long a = 0, b = 0;
        HIPCHK(h, hipMemcpy(&a, lp.off + t0, 8, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(&b, lp.off + t1, 8, hipMemcpyDeviceToHost));
        hipLaunchKernelGGL(k_ppc_walk<PPC_MODE_WRITE>, dim3(grid_for((t1 - t0) * G, 256, 65536)), dim3(256), 0, h->stream, lp.p, G, t0, t1, lp.off,
                           (const unsigned long long*)nullptr, a, b - a, dsub[0], dsub[1], dsub[2], dsub[3], dv, (unsigned long long*)nullptr, bad);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(vals + base + a, dv, (b - a) * 8, hipMemcpyDeviceToHost, h->stream));
        for (int q = 0; q < 4; ++q)
          if (hsub[q]) HIPCHK(h, hipMemcpyAsync(hsub[q] + base + a, dsub[q], (b - a) * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        t0 = t1;
      }
      tm.release(dv);
      if (ds) tm.release(ds);
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    base += lp.nsup;
    ppc_release_layer(tm, lp);
  }
  return bad_check(h, bad, "vmr_mean_poisson");
}

extern "C" int vmr_report_auc(vmr_handle h, int layer, double* auc, uint64_t* n_pos, uint64_t* n_neg) {
  if (!h || !auc) return VMR_EINVAL;
  int rc = check_handle(h, layer, "vmr_report_auc");
  if (rc) return rc;
  const int l0 = layer < 0 ? 0 : layer, l1 = layer < 0 ? h->g.L : layer + 1;
  const size_t T = (size_t)h->g.N * h->g.N;
  const int G = pow2_lanes((size_t)h->g.M);
  Tmp tm(h);
  // sizes: positives and support of every layer
  std::vector<unsigned long long> P_l(h->g.L, 0), S_l(h->g.L, 0);
  unsigned long long P = 0, S = 0;
  for (int l = l0; l < l1; ++l) {
    LayerPrep lp;
    if ((rc = ppc_prep_layer(h, tm, l, true, false, lp))) return rc;
    P_l[l] = lp.npos; S_l[l] = lp.nsup;
    P += lp.npos; S += lp.nsup;
    ppc_release_layer(tm, lp);
  }
  const unsigned long long Q = S - P;
  if (n_pos) *n_pos = P;
  if (n_neg) *n_neg = Q;
  if (P == 0 || Q == 0) { *auc = __builtin_nan(""); return VMR_OK; }
  if (P >= 0x7fffffffull) return fail(h, VMR_EINVAL, "vmr_report_auc: 2^31 positives or more (the sort of their scores takes an int count)");
  if (P > 0x3fffffffffffffffull / Q) return fail(h, VMR_EINVAL, "vmr_report_auc: 2 P Q reaches 2^63 (the pair counts are 64-bit integers)");
  int* bad = nullptr;
  unsigned long long *pk = nullptr, *pk2 = nullptr, *acc = nullptr;
  if ((rc = tm.get(&bad, 4, "a flag")) || (rc = tm.get(&acc, 8, "the pair count")) || (rc = tm.get(&pk, P * 8, "the positives' scores")) ||
      (rc = tm.get(&pk2, P * 8, "the positives' scores")))
    return rc;
  HIPCHK(h, hipMemsetAsync(bad, 0, 4, h->stream));
  HIPCHK(h, hipMemsetAsync(acc, 0, 8, h->stream));
  // the positives' scores, sorted
  unsigned long long pb = 0;
  for (int l = l0; l < l1; ++l) {
    if (!P_l[l]) continue;
    LayerPrep lp;
    if ((rc = ppc_prep_layer(h, tm, l, true, true, lp))) return rc;
    hipLaunchKernelGGL(k_ppc_walk<PPC_MODE_POS>, dim3(grid_for(T * G, 256, 65536)), dim3(256), 0, h->stream, lp.p, G, (size_t)0, T, lp.off, lp.poff,
                       0ull, P_l[l], (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (double*)nullptr, pk + pb, bad);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    pb += P_l[l];
    ppc_release_layer(tm, lp);
  }
  {
    hipcub::DoubleBuffer<unsigned long long> db(pk, pk2);
    size_t tb = 0;
    void* ts = nullptr;
    HIPCHK(h, hipcub::DeviceRadixSort::SortKeys(nullptr, tb, db, (int)P, 0, 64, h->stream));
    if ((rc = tm.get(&ts, tb, "the sort of the positives"))) return rc;
    HIPCHK(h, hipcub::DeviceRadixSort::SortKeys(ts, tb, db, (int)P, 0, 64, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    tm.release(ts);
    if (db.Current() != pk) std::swap(pk, pk2);
    tm.release(pk2);
  }
  // the negatives, in chunks of ties: scores, sort, ranks against the positives
  for (int l = l0; l < l1; ++l) {
    const unsigned long long Ql = S_l[l] - P_l[l];
    if (!Ql) continue;
    LayerPrep lp;
    if ((rc = ppc_prep_layer(h, tm, l, true, true, lp))) return rc;
    size_t fr = 0, tot = 0;
    HIPCHK(h, hipMemGetInfo(&fr, &tot));
    // 16 B per negative (keys and the sort's second buffer) plus the sort's scratch: a third of the free memory at most
    unsigned long long cap = std::min<unsigned long long>(Ql, std::min<unsigned long long>(1ull << 30, (unsigned long long)(fr / 3 / 16)));
    cap = std::max<unsigned long long>(cap, (unsigned long long)h->g.M);
    unsigned long long *nk = nullptr, *nk2 = nullptr;
    void* ts = nullptr;
    size_t tb = 0;
    if ((rc = tm.get(&nk, cap * 8, "the negatives' scores")) || (rc = tm.get(&nk2, cap * 8, "the negatives' scores"))) return rc;
    {
      hipcub::DoubleBuffer<unsigned long long> db(nk, nk2);
      HIPCHK(h, hipcub::DeviceRadixSort::SortKeys(nullptr, tb, db, (int)cap, 0, 64, h->stream));
    }
    if ((rc = tm.get(&ts, tb, "the sort of the negatives"))) return rc;
    for (size_t t0 = 0; t0 < T;) {
      size_t t1 = T;
      if ((rc = cut_ties(h, lp.off, lp.poff, t0, T, cap, &t1))) return rc;
      unsigned long long a0 = 0, a1 = 0, b0 = 0, b1 = 0;
      HIPCHK(h, hipMemcpy(&a0, lp.off + t0, 8, hipMemcpyDeviceToHost));
      HIPCHK(h, hipMemcpy(&a1, lp.off + t1, 8, hipMemcpyDeviceToHost));
      HIPCHK(h, hipMemcpy(&b0, lp.poff + t0, 8, hipMemcpyDeviceToHost));
      HIPCHK(h, hipMemcpy(&b1, lp.poff + t1, 8, hipMemcpyDeviceToHost));
      const unsigned long long nb = (a1 - b1) - (a0 - b0);
      if (nb) {
        hipLaunchKernelGGL(k_ppc_walk<PPC_MODE_NEG>, dim3(grid_for((t1 - t0) * G, 256, 65536)), dim3(256), 0, h->stream, lp.p, G, t0, t1, lp.off, lp.poff,
                           a0 - b0, nb, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (double*)nullptr, nk, bad);
        HIPCHK(h, hipGetLastError());
        hipcub::DoubleBuffer<unsigned long long> db(nk, nk2);
        size_t tb2 = tb;
        HIPCHK(h, hipcub::DeviceRadixSort::SortKeys(ts, tb2, db, (int)nb, 0, 64, h->stream));
        hipLaunchKernelGGL(k_ppc_rank, dim3(grid_for(nb, 256, 8192)), dim3(256), 0, h->stream, pk, P, db.Current(), nb, acc);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipStreamSynchronize(h->stream));
      }
      t0 = t1;
    }
    tm.release(ts); tm.release(nk); tm.release(nk2);
    ppc_release_layer(tm, lp);
  }
  if ((rc = bad_check(h, bad, "vmr_report_auc"))) return rc;
  unsigned long long U2 = 0;
  HIPCHK(h, hipMemcpy(&U2, acc, 8, hipMemcpyDeviceToHost));
  *auc = (double)U2 / (2.0 * (double)P * (double)Q);
  return VMR_OK;
}
