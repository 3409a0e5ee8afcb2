// read_side.h -- what the read-side units share beyond one layer's view (ppc_layer.h) and one rho row (rho_row.h): the small device
// and host helpers, the two walks over a tie's reporters -- the support walk (a tie's mask row in ascending m: ppc.hip,
// report_scores.hip, influence.hip) and the report walk (a tie's non-zero counts: reporter_table.hip, ppc_rep.hip) -- and the
// host driver of a walk that counts, scans and fills a table of flagged elements.  Everything here is static or inline.
#ifndef VMR_READ_SIDE_H
#define VMR_READ_SIDE_H
#include <type_traits>
#include "vmr_internal.h"
#include "ppc_layer.h"
#include "rho_row.h"

typedef unsigned long long u64;

// flag bits every walk shares (a unit's own bits start at 4)
#define WALK_BAD_NAN 1
#define WALK_BAD_WALK 2

// ------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------
// the rho row of tie t: by tie, or by sorted position through inv
__device__ __forceinline__ const double* tie_rho(const PpcLayer& p, size_t t) { return p.rho + (p.inv ? (size_t)p.inv[t] : t) * p.K; }

// reporters the mask keeps for a tie of class c
__device__ __forceinline__ unsigned mask_row_size(const PpcLayer& p, size_t t, int c) {
  if (c == 1) return (unsigned)p.M;
  if (c != 2) return 0u;
  if (p.rq) return p.rq[t + 1] - p.rq[t];
  unsigned s = 0;
  for (int w = 0; w < p.W; ++w) s += (unsigned)__popcll(p.Rb[t * p.W + w]);
  return s;
}

// a lane's place in its group of G lanes (a power of two up to 64): the lane in the group, the group's lanes and the lanes below
struct WalkGroup {
  int gl;
  u64 gmask, lt;
};
__device__ __forceinline__ WalkGroup walk_group(int G) {
  const int lane = threadIdx.x & 63;
  WalkGroup g;
  g.gl = lane & (G - 1);
  g.gmask = (G == 64 ? ~0ull : ((1ull << G) - 1ull)) << (lane - g.gl);
  g.lt = (1ull << lane) - 1ull;
  return g;
}

__device__ __forceinline__ u64 wave_sum_ull(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (u64)__shfl_xor((long long)v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned wave_sum_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned wave_min_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o, 64));
  return v;
}
__device__ __forceinline__ unsigned wave_max_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// the workgroup's sum in thread 0: the waves in index order (every thread calls it; red holds a slot per wave)
__device__ __forceinline__ u64 block_sum_ull(u64 v, u64* red) {
  v = wave_sum_ull(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  u64 r = 0;
  if (threadIdx.x == 0)
    for (unsigned w = 0; w < (blockDim.x >> 6); ++w) r += red[w];
  return r;
}

// c = #{tau : edges[tau] <= s}; a NaN lands in bin 0 (the call then ends in VMR_ENAN)
__device__ __forceinline__ int edge_bin(const double* __restrict__ edges, int n, double s) {
  int a = 0, b = n;
  while (a < b) { const int c = a + ((b - a) >> 1); if (edges[c] <= s) a = c + 1; else b = c; }
  return a;
}

// order-preserving key of a double (-0 as +0): equal keys <=> equal values
__device__ __forceinline__ u64 order_key(double v) {
  const u64 u = (u64)__double_as_longlong(v + 0.0);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// the workgroup's n LDS bins (32- or 64-bit words) -> 64-bit global ones, the non-zero ones, by integer atomics (tpb threads)
template <class W>
__device__ __forceinline__ void flush_bins(const W* lds, u64* __restrict__ bins, int n, int tpb) {
  for (int q = threadIdx.x; q < n; q += tpb) {
    const W u = lds[q];
    if (u) atomicAdd(bins + q, (u64)u);
  }
}

// A count pass' integer bins -- n_rep words of reporters' bins, then n_hist of histogram -- where its lanes add to them: the
// workgroup's dynamic LDS (zeroed here) for those the host put there, else global.  FILL: nothing is added, nothing zeroed.
struct WalkBins {
  u64 *rep, *hist;
};
template <bool FILL>
__device__ __forceinline__ WalkBins walk_bins(u64* lds, int n_rep, int n_hist, int rep_lds, int hist_lds, u64* rep_g, u64* hist_g, int tpb) {
  if (!FILL) {
    const int n_lds = (rep_lds ? n_rep : 0) + (hist_lds ? n_hist : 0);
    for (int q = threadIdx.x; q < n_lds; q += tpb) lds[q] = 0ull;
    __syncthreads();
  }
  WalkBins b;
  b.rep = rep_lds ? lds : rep_g;
  b.hist = hist_lds ? lds + (rep_lds ? n_rep : 0) : hist_g;
  return b;
}
// ... and out of LDS once the workgroup's lanes are done
__device__ __forceinline__ void walk_bins_flush(const u64* lds, int n_rep, int n_hist, int rep_lds, int hist_lds, u64* rep_g, u64* hist_g, int tpb) {
  __syncthreads();
  if (rep_lds) flush_bins(lds, rep_g, n_rep, tpb);
  if (hist_lds) flush_bins(lds + (rep_lds ? n_rep : 0), hist_g, n_hist, tpb);
}

// --- the report walk: candidate q of a tie's nc -- entry e0 + q of the tie-major index, or reporter q of the dense row ---
struct TieReport {
  unsigned m, x;   // the reporter and the count
  bool in;         // a count x > 0 that the tie's mask row A keeps
};
__device__ __forceinline__ TieReport tie_report(const PpcLayer& p, const MaskRow& A, size_t t, unsigned e0, unsigned nc, unsigned q) {
  TieReport r;
  r.m = 0u; r.x = 0u; r.in = false;
  if (q >= nc) return r;
  if (p.X) {
    r.m = q;
    r.x = p.X[t * p.Mp + q];
    r.in = r.x && row_has(A, q);
  } else {
    const unsigned w = p.iv[e0 + q];
    r.m = (unsigned)(p.ik[e0 + q] & ((1ull << p.mb) - 1ull));
    r.x = w >> 1;
    r.in = r.x && (w & 1u);
  }
  return r;
}

// does the mirror tie tm hold a report of reporter m inside its mask row B?
__device__ __forceinline__ bool mirror_reported(const PpcLayer& p, const MaskRow& B, size_t tm, unsigned m) {
  if (p.X) return p.X[tm * p.Mp + m] != 0 && row_has(B, m);
  unsigned lo = p.ip[tm], hi = p.ip[tm + 1];
  const unsigned end = hi;
  const u64 key = ((u64)tm << p.mb) | m;
  while (lo < hi) { const unsigned c = lo + ((hi - lo) >> 1); if (p.ik[c] < key) lo = c + 1; else hi = c; }
  return lo < end && p.ik[lo] == key && (p.iv[lo] & 1u) && (p.iv[lo] >> 1) != 0u;
}

// --- the support walk: a group of G lanes takes a tie's support reporters in ascending m, G at a time ---
// a tie of class c != 0 as its group sees it: nc candidates -- the reporter list, or [0, M) tested against the mask words
struct WalkTie {
  bool listed, bits;
  unsigned nc;
  const unsigned short* lst;
  size_t i, j, tm;
  const double* row;
};
__device__ __forceinline__ WalkTie walk_tie(const PpcLayer& p, size_t t, int c) {
  WalkTie w;
  w.listed = c == 2 && p.rq != nullptr;
  w.bits = c == 2 && p.rq == nullptr;
  w.nc = w.listed ? p.rq[t + 1] - p.rq[t] : (unsigned)p.M;
  w.lst = w.listed ? p.Rm + p.rq[t] : nullptr;
  w.i = t / p.N; w.j = t - w.i * p.N; w.tm = w.j * p.N + w.i;
  w.row = tie_rho(p, t);
  return w;
}
// candidate q of the tie: its reporter m, and whether the support holds it
__device__ __forceinline__ bool walk_reporter(const PpcLayer& p, const WalkTie& w, size_t t, unsigned q, unsigned& m) {
  m = w.listed ? (q < w.nc ? (unsigned)w.lst[q] : 0u) : q;
  return q < w.nc && m < (unsigned)p.M && (!w.bits || ((p.Rb[t * p.W + (m >> 6)] >> (m & 63)) & 1ull));
}

// The walk of a workgroup of NT threads over its ties [blockIdx.x * gpb * SLOTS, ..), gpb = NT / G groups, and both of its
// passes.  tie(row) runs once per walked tie, elem(row, m, x, xt) once per support element and returns whether the element is
// flagged.  Count pass: cnt[t] = the tie's flagged elements (cnt comes zeroed).  Fill pass (cnt: the exclusive sum, T + 1 long),
// only over ties that hold a row: a flagged element's row is its tie's offset plus its ballot rank in the group -- lexicographic
// order, no atomics -- the six integer columns are written here and put(at) writes the rest; a row at or past a.lim sets
// WALK_BAD_WALK and is not written.  Args holds cnt, lim, sl si sj sm x xt (any may be null) and bad.
template <bool FILL, int NT, int SLOTS, class Args, class Tie, class Elem, class Put>
__device__ __forceinline__ void support_walk(const PpcLayer& p, int G, const Args& a, Tie tie, Elem elem, Put put) {
  const WalkGroup g = walk_group(G);
  const size_t gpb = NT / G;
  const size_t t_lim = ((size_t)blockIdx.x + 1) * gpb * SLOTS, t_end = t_lim < p.T ? t_lim : p.T;
  for (size_t t = (size_t)blockIdx.x * gpb * SLOTS + threadIdx.x / G; t < t_end; t += gpb) {   // (uniform over the group)
    const int c = p.cls[t];
    u64 o_t = 0;
    if (FILL) {
      o_t = a.cnt[t];
      if (c == 0 || a.cnt[t + 1] == o_t) continue;   // no row of this tie
    } else if (c == 0) {
      continue;                                      // (cnt comes zeroed)
    }
    const WalkTie w = walk_tie(p, t, c);
    tie(w.row);
    u64 jf = 0;
    for (unsigned c0 = 0; c0 < w.nc; c0 += (unsigned)G) {
      unsigned m;
      const bool in = walk_reporter(p, w, t, c0 + (unsigned)g.gl, m);
      bool flag = false;
      int x = 0, xt = 0;
      if (in) {
        x = (int)ppc_x(p, t, m);
        if (p.mut) xt = (int)ppc_x(p, w.tm, m);
        flag = elem(w.row, m, x, xt);
      }
      const u64 bf = __ballot(flag) & g.gmask;
      if (FILL && flag) {
        const u64 at = o_t + jf + (u64)__popcll(bf & g.lt);
        if (at >= a.lim) {
          atomicOr(a.bad, WALK_BAD_WALK);   // (the count pass and the fill pass disagree: never written out of bounds)
        } else {
          if (a.sl) a.sl[at] = p.l;
          if (a.si) a.si[at] = (int32_t)w.i;
          if (a.sj) a.sj[at] = (int32_t)w.j;
          if (a.sm) a.sm[at] = (int32_t)m;
          if (a.x) a.x[at] = x;
          if (a.xt) a.xt[at] = xt;
          put(at);
        }
      }
      jf += (u64)__popcll(bf);
    }
    if (!FILL && g.gl == 0) a.cnt[t] = jf;
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// lanes per tie, a power of two up to 64: the longest row a group walks
static inline int pow2_lanes(size_t longest) {
  int G = 1;
  while (G < 64 && (size_t)G < longest) G <<= 1;
  return G;
}

// lanes per tie of a walk over the tie-major index of a report-list handle: twice the mean row (a longer row takes more rounds)
static inline int index_lanes(const vmr_ctx* h) {
  const size_t ties = (size_t)h->g.L * h->g.N * h->g.N;
  const size_t mean2 = ties ? (size_t)((2 * h->nnz + ties - 1) / ties) : 1;
  return pow2_lanes(std::min<size_t>((size_t)h->g.M, std::max<size_t>(1, mean2)));
}

// smallest b with 2^b >= v
static inline int ceil_log2(u64 v) {
  int b = 0;
  while (b < 63 && (1ull << b) < v) ++b;
  return b;
}

static inline unsigned grid_for(size_t n, size_t per = 256, size_t cap = 16384) {
  return (unsigned)std::max<size_t>(1, std::min<size_t>(cap, (n + per - 1) / per));
}

// the checks of a caller's table: finite and non-negative; finite; histogram edges, finite and non-decreasing
static inline bool table_nonneg(const double* v, size_t n) {
  for (size_t q = 0; q < n; ++q)
    if (!(v[q] >= 0.0 && v[q] <= 1.79769313486231570815e308)) return false;
  return true;
}
static inline bool table_finite(const double* v, size_t n) {
  for (size_t q = 0; q < n; ++q)
    if (!(v[q] >= -1.79769313486231570815e308 && v[q] <= 1.79769313486231570815e308)) return false;
  return true;
}
// what a call refuses of its histogram arguments, or null; range: the unit's text for n_edges outside [0, max_edges]
static inline const char* hist_refusal(const void* hist, int n_edges, int max_edges, const char* range, const double* edges) {
  if (n_edges < 0 || n_edges > max_edges) return range;
  if (hist && n_edges > 0 && !edges) return "hist is asked for and edges is NULL";
  for (int q = 0; hist && q < n_edges; ++q)
    if (!table_finite(edges + q, 1) || (q && edges[q] < edges[q - 1])) return "the edges must be finite and non-decreasing";
  return nullptr;
}

// workgroups of a walk that gives each of its tpb / G groups `slots` consecutive ties
static inline unsigned walk_blocks(size_t T, int tpb, int G, int slots) {
  const size_t per = (size_t)(tpb / G) * slots;
  return (unsigned)((T + per - 1) / per);
}

// the shape of a support walk's count pass: lanes per tie (a support row holds up to M reporters), workgroups, and which of its
// integer bins -- n_rep words of reporters' bins, then the histogram's [n_edges + 1][2] -- go to LDS first (lds_max bytes at most)
struct WalkShape {
  int G;
  unsigned nb;
  size_t n_hist, smem;
  bool rep_lds, hist_lds;
};
static inline WalkShape walk_shape(const vmr_ctx* h, int tpb, int slots, bool hist, int n_edges, size_t n_rep, size_t lds_max) {
  WalkShape s;
  s.G = pow2_lanes((size_t)h->g.M);
  s.nb = walk_blocks((size_t)h->g.N * h->g.N, tpb, s.G, slots);
  s.n_hist = hist ? 2 * ((size_t)n_edges + 1) : 0;
  s.rep_lds = n_rep && h->g.M <= PR_HIST_M;
  s.hist_lds = hist && ((s.rep_lds ? n_rep : 0) + s.n_hist) * 8 <= lds_max;
  s.smem = ((s.rep_lds ? n_rep : 0) + (s.hist_lds ? s.n_hist : 0)) * 8;
  return s;
}

// Launches pick(kc)(args...) on nb workgroups of tpb threads; kc carries the kernel's K variant as a constant: 2, 0 (any
// K <= KMAX) or -1 (K > KMAX).
template <class Pick, class... A>
static int launch_by_k(vmr_ctx* h, int K, unsigned nb, unsigned tpb, size_t smem, Pick pick, const A&... args) {
  auto go = [&](auto kern) -> int {
    if (smem > 48 * 1024) HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL(kern, dim3(nb), dim3(tpb), smem, h->stream, args...);
    HIPCHK(h, hipGetLastError());
    return VMR_OK;
  };
  if (K == 2) return go(pick(std::integral_constant<int, 2>()));
  if (K <= KMAX) return go(pick(std::integral_constant<int, 0>()));
  return go(pick(std::integral_constant<int, -1>()));
}

// the table a count-and-fill call may write: six int32 columns (sl si sj sm x xt) and n_dbl <= WALK_MAX_DBL double columns, any of
// them null
#define WALK_MAX_DBL 4
struct WalkTable {
  bool rows;             // the table is asked for, n its capacity
  uint64_t n;
  int32_t* const* sub;
  double* const* dbl;
  int n_dbl;
  int out_on_device;
  uint64_t* n_out;       // the row count, or null
};

// The host side of support_walk's two passes over the layers [l0, l1); a is the kernels' argument struct -- a.bad the caller's
// flag word (a temporary of tm, cleared here); cnt, lim and the six integer columns are set here -- and b returns the flag bits.
// One callback per pass, and one between them:
//   count(l, p)        sets the layer's fields of a and launches the count pass (and what follows it on the stream)
//   totals(flagged)    after the count pass (the stream is idle, b is read): fetches what holds the layers' flagged counts and
//                      fills flagged[l - l0]; what it refuses ends the call
//   fill(l, p, d64)    sets the layer's fields of a, d64 its double columns, and launches the fill pass
// A table that holds fewer rows than are flagged is refused; the fill pass runs over the layers that hold a row, straight into
// device outputs or through per-layer staging into host outputs, and is left out once WALK_BAD_NAN is set.
template <class Args, class Count, class Totals, class Fill>
static int walk_count_fill(vmr_ctx* h, const char* fn, Tmp& tm, int l0, int l1, const WalkTable& w, Args& a, int& b, Count count, Totals totals,
                           Fill fill) {
  const size_t T = (size_t)h->g.N * h->g.N;
  const int Lq = l1 - l0;
  int rc;
  int* const bad = a.bad;
  u64 *cnt = nullptr, *off = nullptr;
  void* ts = nullptr;
  size_t tb = 0;
  if ((rc = tm.get(&cnt, (T + 1) * 8, "the ties' flagged counts"))) return rc;
  if (w.rows) {   // a tie's first row, every layer's: kept until the capacity is checked against all of them
    if ((rc = tm.get(&off, (size_t)Lq * (T + 1) * 8, "the ties' row offsets"))) return rc;
    HIPCHK(h, hipcub::DeviceScan::ExclusiveSum(nullptr, tb, cnt, off, (int)(T + 1), h->stream));
    if ((rc = tm.get(&ts, tb, "the scan of the flagged counts"))) return rc;
  }
  HIPCHK(h, hipMemsetAsync(bad, 0, 4, h->stream));

  // the count pass, layer by layer
  for (int l = l0; l < l1; ++l) {
    LayerPrep lp;
    if ((rc = ppc_prep_layer(h, tm, l, false, true, lp, true, false))) return rc;
    a.cnt = cnt;
    HIPCHK(h, hipMemsetAsync(cnt, 0, (T + 1) * 8, h->stream));
    if ((rc = count(l, lp.p))) return rc;
    if (w.rows) HIPCHK(h, hipcub::DeviceScan::ExclusiveSum(ts, tb, cnt, off + (size_t)(l - l0) * (T + 1), (int)(T + 1), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    ppc_release_layer(tm, lp);
  }
  std::vector<u64> flagged((size_t)Lq, 0ull);
  b = 0;
  HIPCHK(h, hipMemcpyAsync(&b, bad, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if ((rc = totals(flagged.data()))) return rc;
  u64 total = 0;
  for (int q = 0; q < Lq; ++q) total += flagged[q];
  if (w.n_out) *w.n_out = total;
  if (w.rows && w.n < total) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: the table holds %llu rows, %llu elements are flagged", fn, (unsigned long long)w.n, (unsigned long long)total);
    return fail(h, VMR_EINVAL, msg);
  }
  if (!w.rows || !total || (b & WALK_BAD_NAN)) return VMR_OK;

  // the fill pass: the layers that hold a row
  double* d64[WALK_MAX_DBL];
  u64 base = 0;
  for (int l = l0; l < l1; ++l) {
    const u64 nl = flagged[l - l0];
    if (!nl) continue;
    LayerPrep lp;
    if ((rc = ppc_prep_layer(h, tm, l, false, true, lp, true, false))) return rc;
    a.cnt = off + (size_t)(l - l0) * (T + 1);
    a.lim = nl;
    int32_t* d32[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int32_t* st32 = nullptr;
    double* st64 = nullptr;
    if (w.out_on_device) {
      for (int q = 0; q < 6; ++q) d32[q] = w.sub[q] ? w.sub[q] + base : nullptr;
      for (int q = 0; q < w.n_dbl; ++q) d64[q] = w.dbl[q] ? w.dbl[q] + base : nullptr;
    } else {   // host outputs: the layer's rows through device staging
      int n32 = 0, n64 = 0;
      for (int q = 0; q < 6; ++q) n32 += w.sub[q] != nullptr;
      for (int q = 0; q < w.n_dbl; ++q) n64 += w.dbl[q] != nullptr;
      if ((n32 && (rc = tm.get(&st32, (size_t)n32 * nl * 4, "the staging of the rows"))) ||
          (n64 && (rc = tm.get(&st64, (size_t)n64 * nl * 8, "the staging of the rows"))))
        return rc;
      for (int q = 0, u = 0; q < 6; ++q) if (w.sub[q]) d32[q] = st32 + (size_t)(u++) * nl;
      for (int q = 0, u = 0; q < w.n_dbl; ++q) d64[q] = w.dbl[q] ? st64 + (size_t)(u++) * nl : nullptr;
    }
    a.sl = d32[0]; a.si = d32[1]; a.sj = d32[2]; a.sm = d32[3]; a.x = d32[4]; a.xt = d32[5];
    if ((rc = fill(l, lp.p, d64))) return rc;
    if (!w.out_on_device) {
      for (int q = 0; q < 6; ++q)
        if (w.sub[q]) HIPCHK(h, hipMemcpyAsync(w.sub[q] + base, d32[q], (size_t)nl * 4, hipMemcpyDeviceToHost, h->stream));
      for (int q = 0; q < w.n_dbl; ++q)
        if (w.dbl[q]) HIPCHK(h, hipMemcpyAsync(w.dbl[q] + base, d64[q], (size_t)nl * 8, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (st32) tm.release(st32);
    if (st64) tm.release(st64);
    ppc_release_layer(tm, lp);
    base += nl;
  }
  HIPCHK(h, hipMemcpyAsync(&b, bad, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (b & WALK_BAD_WALK) return fail(h, VMR_EHIP, (std::string(fn) + ": the count pass and the fill pass disagree").c_str());
  return VMR_OK;
}

#endif  // VMR_READ_SIDE_H
