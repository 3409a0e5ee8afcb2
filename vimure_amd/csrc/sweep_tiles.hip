// sweep_tiles.hip -- the dense tile path: FP64 streaming passes over the dense uint8 report tensor X[L,N,N,Mp] and the
// bit-packed reporter mask R (sweep_tiles.h; data layout and byte accounting: DESIGN.md).
//   k_rho          "tile-pair" sweep over X: a workgroup stages the (I,J) tile of ties and its mirror (J,I) in
//                  LDS so that X[l,j,i,m] (the reference's data_T_vals) is an LDS byte read; the non-zero counts
//                  of the pair are compacted into wave-local queues and walked twice: per-tie sums for the rho
//                  update, then the sufficient statistics H[l,y,m,k] of the new rho (and the ELBO data terms).
//   k_hist         the same sweep building H from the current rho (start of a realisation).
// Host side: the LDS sizes, the geometry of a handle (choose_geo) and the two launch entries tiles_hist / tiles_rho.
#include "sweep_tiles.h"

// Non-zero-byte flags of a 16-byte chunk, 16 bits spread over a dword: bit 8*b + i (+4 when hi) is set
// iff byte b of dword i is non-zero.  Two chunks (hi = 0/1) share one dword, four one 64-bit word.
template <int SH>   // SH = 0 or 4
__device__ __forceinline__ unsigned nz_flags16(uint4 v) {
  const unsigned M = 0x7f7f7f7fu;
  unsigned t0 = ((v.x & M) + M) | v.x, t1 = ((v.y & M) + M) | v.y;
  unsigned t2 = ((v.z & M) + M) | v.z, t3 = ((v.w & M) + M) | v.w;   // bit 7 of each byte = byte != 0
  unsigned f = (t0 >> (7 - SH)) & (0x01010101u << SH);
  f |= (t1 >> (6 - SH)) & (0x02020202u << SH);
  f |= (t2 >> (5 - SH)) & (0x04040404u << SH);
  f |= (t3 >> (4 - SH)) & (0x08080808u << SH);
  return f;
}
// flag position (0..63 in a 64-bit word of four chunks) -> chunk-in-word (0..3) and byte-in-chunk (0..15)
__device__ __forceinline__ void flag_pos(int bit, int& chunk, int& byte) {
  const int lo = bit & 31;                       // position inside the dword of a chunk pair
  chunk = ((bit >> 5) << 1) | ((lo >> 2) & 1);   // dword half, then the +4 flag
  byte = ((lo & 3) << 2) | (lo >> 3);            // dword i = lo & 3, byte b = lo >> 3  ->  4*i + b
}

// decode pair index p -> (I,J), I <= J, row-major over the upper triangle of an nb x nb grid
__device__ __forceinline__ void pair_decode(long long p, int nb, int& I, int& J) {
  double d = (2.0 * nb + 1.0);
  long long i = (long long)((d - sqrt(d * d - 8.0 * (double)p)) * 0.5);
  if (i < 0) i = 0;
  if (i > nb - 1) i = nb - 1;
  auto off = [&](long long r) { return r * nb - r * (r - 1) / 2; };
  while (i > 0 && off(i) > p) --i;
  while (i < nb - 1 && off(i + 1) <= p) ++i;
  I = (int)i;
  J = (int)(i + (p - off(i)));
}

// Register-staged stream of tile pairs.  The 16-B chunks a thread stages are the same slots of
// every tile pair, so their byte offsets from the two sub-tile bases (I,J) / (J,I) and their LDS
// offsets are computed once; fetch() is one saddr+voffset global_load_dwordx4 per slot and the
// loads stay in flight while the previous tile pair is processed.  Reads never need a bounds
// check: X is allocated with b*N+b rows of slack, and rows outside the network are never used.
template <int PF>
struct TileStream {
  uint4 buf[PF];
  unsigned goff[PF];
  unsigned loff[PF];
  unsigned valid, second;   // bit u: slot exists / belongs to the mirrored sub-tile
  __device__ __forceinline__ void init(const Geo& g) {
    valid = 0; second = 0;
    const int bb = g.b * g.b;
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      int q = threadIdx.x + u * TPB;
      int tau = q / g.nchunk, c = q - tau * g.nchunk;
      bool ok = tau < g.nt, sec = tau >= bb;
      int v = sec ? tau - bb : tau;
      int p = v >> g.lb, qq = v & (g.b - 1);
      goff[u] = ok ? (unsigned)((p * g.N + qq) * g.Mp + c * 16) : 0u;
      loff[u] = ok ? (unsigned)(tau * g.stride + c * 16) : 0u;
      valid |= (ok ? 1u : 0u) << u;
      second |= (sec ? 1u : 0u) << u;
    }
  }
  __device__ __forceinline__ void fetch(const uint8_t* __restrict__ Xl, const Geo& g, int I0, int J0) {
    const uint8_t* baseA = Xl + ((size_t)I0 * g.N + J0) * g.Mp;
    const uint8_t* baseB = Xl + ((size_t)J0 * g.N + I0) * g.Mp;
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      // (assign every slot unconditionally: a conditionally written array would live in scratch)
      uint4 v = make_uint4(0, 0, 0, 0);
      if ((valid >> u) & 1u) {
        const uint8_t* base = ((second >> u) & 1u) ? baseB : baseA;
        v = *reinterpret_cast<const uint4*>(base + goff[u]);
      }
      buf[u] = v;
    }
  }
  __device__ __forceinline__ void store(unsigned char* xt) {
#pragma unroll
    for (int u = 0; u < PF; ++u)
      if ((valid >> u) & 1u) *reinterpret_cast<uint4*>(xt + loff[u]) = buf[u];
  }
};

// The same staging for the tile pair's mask rows (64-bit words), 3 words per thread at most.
struct MaskStream {
  uint64_t buf[3];
  unsigned goff[3];
  unsigned valid, second;
  __device__ __forceinline__ void init(const Geo& g) {
    valid = 0; second = 0;
    const int bb = g.b * g.b;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      int q = threadIdx.x + u * TPB;
      int tau = q / g.W, w = q - tau * g.W;
      bool ok = tau < g.nt, sec = tau >= bb;
      int v = sec ? tau - bb : tau;
      int p = v >> g.lb, qq = v & (g.b - 1);
      goff[u] = ok ? (unsigned)((p * g.N + qq) * g.W + w) : 0u;
      valid |= (ok ? 1u : 0u) << u;
      second |= (sec ? 1u : 0u) << u;
    }
  }
  __device__ __forceinline__ void fetch(const uint64_t* __restrict__ Rl, const Geo& g, int I0, int J0) {
    const uint64_t* baseA = Rl + ((size_t)I0 * g.N + J0) * g.W;
    const uint64_t* baseB = Rl + ((size_t)J0 * g.N + I0) * g.W;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      uint64_t v = 0ull;
      if ((valid >> u) & 1u) v = (((second >> u) & 1u) ? baseB : baseA)[goff[u]];
      buf[u] = v;
    }
  }
  __device__ __forceinline__ void store(uint64_t* rw) {
#pragma unroll
    for (int u = 0; u < 3; ++u)
      if ((valid >> u) & 1u) rw[threadIdx.x + u * TPB] = buf[u];
  }
};

// Weights of the cache refresh (model.py:685-693) without a divide per report:
//   w1 = z1/(z1 + z2) = 1/(1 + c y),  c[m][k] = G_nu / (G_theta[m] G_lambda[k])  (LDS table, built per launch)
// y = 0 gives exactly 1; a z1 that underflows to 0 gives c = inf and w1 = 0 at EVERY y: at y = 0 by the reference's den==0 -> 1
// rule, beyond it as z1/z2 = 0 (G_nu = 0 as well: the rule again) -- selected before the reciprocal, whose Newton step makes
// 1/inf a NaN.
template <int K>
__device__ __forceinline__ void build_ct(double* ct, const double* Gth, const double (&Gla)[K], double gnu, int Mp) {
  for (int m = threadIdx.x; m < Mp; m += TPB) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      double z1 = Gth[m] * Gla[k];
      ct[(size_t)m * K + k] = (z1 == 0.0) ? (double)INFINITY : gnu / z1;
    }
  }
}
template <int K>
__device__ __forceinline__ void weights(double (&w)[K], const double* ct, int m, unsigned y) {
  const double dy = (double)y;
  const double* p = ct + (size_t)m * K;
  if (K == 2) {   // one reciprocal for both categories: 1/a0 = a1/(a0 a1)
    const double c0 = p[0], c1 = p[1];
    if (c0 < (double)INFINITY && c1 < (double)INFINITY) {
      const double a0 = 1.0 + c0 * dy, a1 = 1.0 + c1 * dy;
      const double r = fast_rcp(a0 * a1);
      w[0] = a1 * r; w[1] = a0 * r;   // y = 0: a0 = a1 = 1 and r = 1 exactly
      return;
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double c = p[k];
    const double r = fast_rcp(1.0 + c * dy);   // y = 0: 1 exactly; c = inf: a NaN (inf 0, or the Newton step), not taken
    w[k] = (c < (double)INFINITY) ? r : 0.0;
  }
}

// Per-tie accumulators a report may feed (reduced over the wave when a heavy share is processed cooperatively)
struct NoAcc {
  __device__ __forceinline__ void zero() {}
  __device__ __forceinline__ void wave_reduce() {}
};

#define QCAP 6   // a lane queues at most this many non-zero dwords; larger shares are "heavy"

// The non-zero counts of the tile rows owned by one wave.  Lane (tau, s) owns the 16-B chunks {s, s+S, ..}
// of row tau.
//   build(): phase 1 (no divergence): one flag per DWORD of the lane's chunks (v_min_u32 + v_lshl_or); then the
//            flags of all 64 lanes are compacted into a wave-local LDS queue of (lane, dword) entries
//            (ballot/mbcnt prefix sums) -- without it a wave runs max-over-lanes(non-zeros) trips at ~30 % lane
//            utilisation.  Heavy shares (a true tie is reported by most reporters: ~100 non-zeros in a row whose
//            neighbours have 2-5) are not queued.
//   walk():  every lane takes queue entries; f(tau_e, m, x, acc) handles one report of tie slot tau_e,
//            commit(tau_e, acc) adds acc to that tie's sums.  Heavy shares: all lanes take one dword each, sums
//            come back through a wave reduction.  walk() may be called several times per build().
// Both must be called by every lane of the wave (act = false for lanes without a tie).
struct TileScan {
  unsigned lo, hi, tot;
  bool heavy, simple;

  __device__ __forceinline__ void build(const unsigned char* xt, const Geo& g, int tau, int s, bool act,
                                        unsigned short* wq) {
    const int S = g.S, nchunk = g.nchunk;
    const unsigned char* row = xt + tau * g.stride;
    lo = 0; hi = 0; tot = 0; heavy = false;
    simple = (nchunk + S - 1) / S > 12;   // huge M (b = 1): plain chunk-by-chunk walk, nothing to build
    if (simple) return;
    // phase 1: bit 4*j + i <-> dword i of chunk s + j*S   (lo: chunks 0..7, hi: chunks 8..11)
    if (act) {
#pragma unroll
      for (int j = 0; j < 12; ++j) {
        if (j * S < nchunk) {   // wave-uniform
          const int c = s + j * S;
          const int cl = c < nchunk ? c : nchunk - 1;
          const uint4 v = *reinterpret_cast<const uint4*>(row + cl * 16);
          unsigned f4 = min(v.x, 1u) | (min(v.y, 1u) << 1) | (min(v.z, 1u) << 2) | (min(v.w, 1u) << 3);
          f4 = c < nchunk ? f4 : 0u;
          if (j < 8) lo |= f4 << (4 * j); else hi |= f4 << (4 * (j - 8));
        }
      }
    }
    const int cnt = __popc(lo) + __popc(hi);   // non-zero dwords of the share
    if (g.dbg & 4) { lo = (cnt == 0x7fffffff) ? 1u : 0u; hi = 0; return; }   // timing experiment: phase 1 only
    const int lane = threadIdx.x & 63;
    heavy = cnt > QCAP;
    const unsigned cl_ = heavy ? 0u : (unsigned)cnt;   // 0..QCAP (< 8)
    unsigned pre = 0;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const uint64_t bal = __ballot((cl_ >> b) & 1u);
      pre += __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u)) << b;
      tot += (unsigned)__popcll(bal) << b;
    }
    if (!heavy) {
      unsigned l2 = lo, h2 = hi, j = pre;
      while (l2 | h2) {
        int p;
        if (l2) { p = __builtin_ctz(l2); l2 &= l2 - 1; } else { p = 32 + __builtin_ctz(h2); h2 &= h2 - 1; }
        wq[j++] = (unsigned short)((lane << 6) | p);
      }
    }
    __builtin_amdgcn_wave_barrier();
  }

  template <class TieAcc, class F, class C>
  __device__ __forceinline__ void walk(const unsigned char* xt, const Geo& g, int tau, int s, bool act,
                                       const unsigned short* wq, F&& f, C&& commit) const {
    const int S = g.S, nchunk = g.nchunk;
    if (simple) {
      if (!act) return;
      const unsigned char* row = xt + tau * g.stride;
      TieAcc a;
      a.zero();
      for (int c = s; c < nchunk; c += S) {
        unsigned nzm = nz_flags16<0>(*reinterpret_cast<const uint4*>(row + c * 16));
        while (nzm) {
          int bit = __builtin_ctz(nzm), ch, by;
          nzm &= nzm - 1;
          flag_pos(bit, ch, by);
          f(tau, c * 16 + by, (unsigned)row[c * 16 + by], a);
        }
      }
      commit(tau, a);
      return;
    }
    const int lane = threadIdx.x & 63;
    const int wave_base = threadIdx.x & ~63;
    for (unsigned e0 = 0; e0 < tot; e0 += 64) {   // wave-uniform trip count
      const unsigned e = e0 + lane;
      if (e < tot) {
        const unsigned ent = wq[e];
        const int ls = ent >> 6, p = ent & 63;
        const int tau_e = (wave_base | ls) >> g.lS, s_e = ls & (S - 1);
        const int off = (s_e + (p >> 2) * S) * 16 + (p & 3) * 4;
        unsigned d = *reinterpret_cast<const unsigned*>(xt + tau_e * g.stride + off);
        TieAcc a;
        a.zero();
        while (d) {
          const int sh = __builtin_ctz(d) & ~7;
          const unsigned x = (d >> sh) & 0xffu;
          d &= ~(0xffu << sh);
          f(tau_e, off + (sh >> 3), x, a);
        }
        commit(tau_e, a);
      }
    }
    // heavy shares: lane p < 48 takes dword p of the share
    uint64_t hm = __ballot(heavy);
    while (hm) {
      const int h = __builtin_ctzll(hm);
      hm &= hm - 1;
      const int tau_h = (wave_base | h) >> g.lS, s_h = h & (S - 1);
      const unsigned lo_h = __builtin_amdgcn_readlane((int)lo, h), hi_h = __builtin_amdgcn_readlane((int)hi, h);
      TieAcc a;
      a.zero();
      const bool mine = lane < 32 ? ((lo_h >> lane) & 1u) : (lane < 48 ? ((hi_h >> (lane - 32)) & 1u) : false);
      if (mine) {
        const int off = (s_h + (lane >> 2) * S) * 16 + (lane & 3) * 4;
        unsigned d = *reinterpret_cast<const unsigned*>(xt + tau_h * g.stride + off);
        while (d) {
          const int sh = __builtin_ctz(d) & ~7;
          const unsigned x = (d >> sh) & 0xffu;
          d &= ~(0xffu << sh);
          f(tau_h, off + (sh >> 3), x, a);
        }
      }
      a.wave_reduce();
      if (lane == 0) commit(tau_h, a);
    }
    __builtin_amdgcn_wave_barrier();
  }
};

// ------------------------------------------------------------------------------------------
// Sufficient statistics of the reports:  H[l,y,m,k] = sum over ties t of x * rho_k(t), taken over the non-zero
// counts x = X[l,t,m] whose mirrored count X^T[l,t,m] equals y (y = 0 always when mutuality is off).
// Everything the gamma, phi and nu updates need from X is linear in rho with weights that depend on (m, y, k) only:
//   gamma_shp[l,m] = alpha + sum_{y,k} w1_k(m,y) H    (model.py:698-703, 832-859; w1 with the OLD parameters)
//   phi_shp[l,k]   = alpha + sum_{m,y} w1_k(m,y) H    (model.py:731-733, 861-887; w1 with the NEW E[log theta])
//   nu_shp         = alpha + sum_{l,m,y>0,k} w2_k(m,y) H   (model.py:822-825; H of the NEW rho)
// so one pass over X per sweep (the rho pass, which rebuilds H from the new rho) replaces three.  H is tiny
// ([L][Y][Mp][K] doubles, Y = max count + 1); mirror counts 0..HC-1 are accumulated in LDS, the rest with global
// f64 atomics.  k_hist builds H from the current rho (start of a fit, sub-step tests).
// ------------------------------------------------------------------------------------------

struct HistArgs {
  const uint8_t* X; const double* rho; double* Hg;
  int Gl;   // workgroups per layer of this launch
};

// common per-tile bookkeeping of the tile-pair kernels
struct TileIter {
  int I, J, nb, b, lb, bb, N;
  __device__ __forceinline__ void init(const Geo& g, long long p0) {
    nb = g.nb; b = g.b; lb = g.lb; bb = g.b * g.b; N = g.N;
    pair_decode(p0, nb, I, J);
  }
  __device__ __forceinline__ void next() { if (++J == nb) { ++I; J = I; } }
  __device__ __forceinline__ bool diag() const { return I == J; }
  // tie slot tau -> (i,j); false when the slot is unused in this pair or lies outside the network
  __device__ __forceinline__ bool coords(int tau, int& i, int& j) const {
    const bool second = tau >= bb;
    const int u = second ? tau - bb : tau;
    const int p = u >> lb, q = u & (b - 1);
    i = (second ? J : I) * b + p;
    j = (second ? I : J) * b + q;
    return tau < (diag() ? bb : 2 * bb) && i < N && j < N;
  }
  __device__ __forceinline__ int mirror(int tau) const {
    const bool second = tau >= bb;
    const int u = second ? tau - bb : tau;
    const int m = ((u & (b - 1)) << lb) | (u >> lb);
    return diag() ? m : (second ? m : bb + m);
  }
};

// one report into H: LDS cache for small mirror counts, global atomics beyond
template <int K>
__device__ __forceinline__ void hist_add(double* Hc, double* Hl /*this workgroup's copy [Y][Mp][K]*/, int Mp, int m, unsigned y,
                                         double dx, const double* r, unsigned hc) {
  if (y < hc) {
    double* d = Hc + ((size_t)y * Mp + m) * K;
#pragma unroll
    for (int k = 0; k < K; ++k) atomicAdd(&d[k], dx * r[k]);
  } else {
    double* d = Hl + ((size_t)y * Mp + m) * K;
#pragma unroll
    for (int k = 0; k < K; ++k) atomicAdd(&d[k], dx * r[k]);
  }
}
__device__ __forceinline__ void hist_flush(const double* Hc, double* Hl, int n) {
  for (int q = threadIdx.x; q < n; q += TPB) {
    const double v = Hc[q];
    if (v != 0.0) atomicAdd(&Hl[q], v);
  }
}

template <int K, bool MUT, int PF>
__global__ __launch_bounds__(TPB, VMR_LB_COUNTS) void k_hist(HistArgs a, Geo g) {
  extern __shared__ __align__(16) unsigned char smem[];
  unsigned char* xt = smem;
  double* rt = reinterpret_cast<double*>(smem + (size_t)g.nt * g.stride);   // rho of the pair's ties [nt][K]
  double* Hc = rt + (size_t)g.nt * K;                                        // [HC][Mp][K]
  const int nHc = g.hc * g.Mp * K;
  unsigned short* wq = reinterpret_cast<unsigned short*>(Hc + nHc) + (threadIdx.x >> 6) * (64 * QCAP);
  const int l = blockIdx.x / a.Gl, gb = blockIdx.x - l * a.Gl;
  const long long p0 = (long long)gb * g.P / a.Gl, p1 = (long long)(gb + 1) * g.P / a.Gl;
  for (int q = threadIdx.x; q < nHc; q += TPB) Hc[q] = 0.0;
  double* Hl = a.Hg + ((size_t)l * NH + (gb % NH)) * g.Y * g.Mp * K;
  TileIter it;
  it.init(g, p0);
  const int tau = threadIdx.x >> g.lS, s = threadIdx.x & (g.S - 1);
  const uint8_t* Xl = a.X + (size_t)l * g.N * g.N * g.Mp;
  const double* rl = a.rho + (size_t)l * g.N * g.N * K;
  TileStream<PF> ts;
  ts.init(g);
  double rn[K];   // rho of this lane's tie in the NEXT pair (prefetched like the X chunks)
  auto fetch_rho = [&]() {
    int i, j;
    const bool ok = it.coords(tau, i, j);
#pragma unroll
    for (int k = 0; k < K; ++k) rn[k] = ok ? rl[((size_t)i * g.N + j) * K + k] : 0.0;
  };
  if (p0 < p1) { ts.fetch(Xl, g, it.I * g.b, it.J * g.b); fetch_rho(); }
  __syncthreads();
  for (long long p = p0; p < p1; ++p) {
    ts.store(xt);
    int i, j;
    const bool act = it.coords(tau, i, j);
    if (s == 0 && tau < g.nt) {
#pragma unroll
      for (int k = 0; k < K; ++k) rt[tau * K + k] = rn[k];
    }
    const TileIter cur = it;
    __syncthreads();
    it.next();
    if (p + 1 < p1) { ts.fetch(Xl, g, it.I * g.b, it.J * g.b); fetch_rho(); }   // flies while this pair is scanned
    TileScan sc;
    sc.build(xt, g, tau, s, act, wq);
    sc.walk<NoAcc>(xt, g, tau, s, act, wq,
      [&](int te, int m, unsigned x, NoAcc&) {
        const unsigned y = MUT ? (unsigned)xt[cur.mirror(te) * g.stride + m] : 0u;
        hist_add<K>(Hc, Hl, g.Mp, m, y, (double)x, rt + te * K, (unsigned)g.hc);
      },
      [&](int, const NoAcc&) {});
    __syncthreads();
  }
  hist_flush(Hc, Hl, nHc);
}

// ------------------------------------------------------------------------------------------
// rho (+ H of the new rho, + ELBO data terms)   model.py:763-818, 889-923; ELBO :948-995, :1013
// slotR[slot][4]: [1] ELBO linear+entropy terms, [2] ELBO log terms,
//                 [3] sum_t (sum_k rho_k) Q_t  (multiplied by -E[nu] in k_fin_rho)
// Walk 1 over the pair's non-zero counts collects U_k per tie; after the per-tie update the same queue is
// walked again with the NEW rho to rebuild H (and, on ELBO sweeps, the log terms and the mirror sums Q).
// ------------------------------------------------------------------------------------------
struct RhoArgs {
  const uint8_t* X; const uint64_t* Rb; double* rho; const double* logpr; const double* par;
  double* slotR;
  const double* lutg;   // nibble LUT of E[theta], [L][W*256]
  double* Hg;
  double* slotF;
  int Gl;
};

template <int K>
struct SumU {
  double U[K];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int k = 0; k < K; ++k) U[k] = 0.0;
  }
  __device__ __forceinline__ void wave_reduce() {
#pragma unroll
    for (int k = 0; k < K; ++k) U[k] = wave_sum(U[k]);
  }
};
struct SumQ {   // ELBO walk: the mirror tie's masked count
  unsigned q;
  __device__ __forceinline__ void zero() { q = 0u; }
  __device__ __forceinline__ void wave_reduce() {
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) q += __shfl_xor(q, o2, 64);
  }
};

template <int K, bool MUT, bool UPDATE, bool ELBO, int PF>
__global__ __launch_bounds__(TPB, ELBO ? 2 : VMR_LB_RHO) void k_rho(RhoArgs a, Geo g) {   // ELBO variants: 2 resident (LDS), so 256 VGPRs
  extern __shared__ __align__(16) unsigned char smem[];
  unsigned char* xt = smem;
  size_t off = (size_t)g.nt * g.stride;
  uint64_t* rw = reinterpret_cast<uint64_t*>(smem + off); off += (size_t)g.nt * g.W * 8;
  double* wsum = reinterpret_cast<double*>(smem + off); off += (size_t)g.W * 8;
  double* lth = reinterpret_cast<double*>(smem + off); off += (size_t)g.Mp * 8;
  double* red = reinterpret_cast<double*>(smem + off); off += 8 * 8;
  double* ct = reinterpret_cast<double*>(smem + off); off += MUT ? (size_t)g.Mp * K * 8 : 0;
  double* ut = reinterpret_cast<double*>(smem + off); off += (size_t)g.nt * K * 8;    // U per tie; exp(rho) in the ELBO walk
  double* rt = reinterpret_cast<double*>(smem + off); off += (size_t)g.nt * K * 8;    // (new) rho per tie
  const bool do_hist = UPDATE && !g.two_pass;
  const int nHc = do_hist ? g.hc * g.Mp * K : 0;
  double* Hc = reinterpret_cast<double*>(smem + off); off += (size_t)nHc * 8;
  double* Gth = reinterpret_cast<double*>(smem + off); off += ELBO ? (size_t)g.Mp * 8 : 0;
  unsigned* qs = reinterpret_cast<unsigned*>(smem + off); off += ELBO ? (size_t)g.nt * 4 : 0;
  unsigned short* wq = reinterpret_cast<unsigned short*>(smem + off) + (threadIdx.x >> 6) * (64 * QCAP);
  const ParOff o = par_off(g.L, g.Mp, g.K);
  const int l = blockIdx.x / a.Gl, gb = blockIdx.x - l * a.Gl;
  const long long p0 = (long long)gb * g.P / a.Gl, p1 = (long long)(gb + 1) * g.P / a.Gl;
  for (int m = threadIdx.x; m < g.Mp; m += TPB) {
    lth[m] = a.par[o.l_th + (size_t)l * g.Mp + m];
    if (ELBO) Gth[m] = a.par[o.G_th + (size_t)l * g.Mp + m];
  }
  for (int q = threadIdx.x; q < nHc; q += TPB) Hc[q] = 0.0;
  // lut[n][e] = sum of E[theta_m] over the set bits e of reporters 4n..4n+3 (global, L1/L2 resident);
  // wsum[w] = sum over the 64 reporters of word w (shortcut for all-ones words)
  const double* lut = a.lutg + (size_t)l * g.W * 256;
  for (int w = threadIdx.x; w < g.W; w += TPB) {
    double v = 0.0;
    for (int n = 0; n < 16; ++n) v += lut[(w * 16 + n) * 16 + 15];
    wsum[w] = v;
  }
  double Ela[K], lla[K], Gla[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    Ela[k] = a.par[o.E_la + l * K + k]; lla[k] = a.par[o.l_la + l * K + k]; Gla[k] = a.par[o.G_la + l * K + k];
  }
  // UPDATE: the weights use the current G_nu; stand-alone ELBO: the stale one (model.py:970)
  const double gnu = a.par[o.sc + (UPDATE ? SC_G_NU : SC_G_NU_STALE)];
  const double eps = g.eps;
  double e_lin = 0.0, e_q = 0.0, e_log = 0.0;
  double accF[K];   // sum of the new rho over this workgroup's ties whose mask row is all ones
#pragma unroll
  for (int k = 0; k < K; ++k) accF[k] = 0.0;
  const int lastrem = g.M - (g.W - 1) * 64;
  const uint64_t lastfull = lastrem >= 64 ? ~0ull : ((1ull << lastrem) - 1ull);
  if (MUT) build_ct<K>(ct, a.par + o.G_th + (size_t)l * g.Mp, Gla, gnu, g.Mp);
  double* Hl = a.Hg + ((size_t)l * NH + (gb % NH)) * g.Y * g.Mp * K;

  TileIter it;
  it.init(g, p0);
  const int tau = threadIdx.x >> g.lS, s = threadIdx.x & (g.S - 1);
  const size_t T = (size_t)g.N * g.N;
  const uint8_t* Xl = a.X + (size_t)l * T * g.Mp;
  const uint64_t* Rl = a.Rb + (size_t)l * T * g.W;
  double* rl = a.rho + (size_t)l * T * K;
  const double* lpl = a.logpr + (size_t)l * T * K;
  TileStream<PF> ts;
  ts.init(g);
  MaskStream ms;
  ms.init(g);
  double lpn[K], rn[K];   // log prior (and rho, ELBO-only) of this lane's tie in the NEXT pair
  auto fetch_tie = [&]() {
    int i, j;
    const bool ok = it.coords(tau, i, j);
    const size_t t_ = ok ? ((size_t)i * g.N + j) : 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      lpn[k] = ok ? lpl[t_ * K + k] : 0.0;
      rn[k] = (!UPDATE && ok) ? rl[t_ * K + k] : 0.0;
    }
  };
  if (p0 < p1) { ts.fetch(Xl, g, it.I * g.b, it.J * g.b); ms.fetch(Rl, g, it.I * g.b, it.J * g.b); fetch_tie(); }
  __syncthreads();
  for (long long p = p0; p < p1; ++p) {
    ts.store(xt);
    ms.store(rw);
    int i, j;
    const bool act = it.coords(tau, i, j);
    const size_t tg = act ? ((size_t)i * g.N + j) : 0;
    const TileIter cur = it;
    double lp[K], r[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { lp[k] = lpn[k]; r[k] = rn[k]; }
    if (UPDATE && s == 0 && tau < g.nt) {
#pragma unroll
      for (int k = 0; k < K; ++k) ut[tau * K + k] = 0.0;
    }
    __syncthreads();
    it.next();
    if (p + 1 < p1) { ts.fetch(Xl, g, it.I * g.b, it.J * g.b); ms.fetch(Rl, g, it.I * g.b, it.J * g.b); fetch_tie(); }
    double Tt = 0.0;
    int rowfull = 1;
    if (act) {
      // T = sum_m R E[theta_m] (model.py:766-792): whole-word shortcut, else nibble look-ups
      const uint64_t* rwt = rw + (size_t)tau * g.W;
      for (int w = s; w < g.W; w += g.S) {
        uint64_t bits = rwt[w];
        rowfull &= (bits == (w == g.W - 1 ? lastfull : ~0ull)) ? 1 : 0;
        if (bits == ~0ull) { Tt += wsum[w]; continue; }
        for (int n = 0; bits != 0; ++n, bits >>= 4) Tt += lut[((w * 16 + n) << 4) + (unsigned)(bits & 15u)];
      }
    }
    Tt = group_sum(Tt, g.S);
    if (UPDATE && g.fuse_full) {
      for (int o2 = g.S >> 1; o2 > 0; o2 >>= 1) rowfull &= __shfl_xor(rowfull, o2, 64);
    }
    TileScan sc;
    sc.build(xt, g, tau, s, act, wq);
    if (UPDATE) {
      sc.walk<SumU<K>>(xt, g, tau, s, act, wq,
        [&](int te, int m, unsigned x, SumU<K>& acc) {
          const double dx = (double)x, lt = lth[m];
          if (MUT) {
            double w[K];
            weights<K>(w, ct, m, (unsigned)xt[cur.mirror(te) * g.stride + m]);
#pragma unroll
            for (int k = 0; k < K; ++k) acc.U[k] += (lt + lla[k]) * (dx * w[k]);
          } else {
#pragma unroll
            for (int k = 0; k < K; ++k) acc.U[k] += (lt + lla[k]) * dx;
          }
        },
        [&](int te, const SumU<K>& t) {   // the tie's sums live in LDS; a tie belongs to one wave
#pragma unroll
          for (int k = 0; k < K; ++k) atomicAdd(&ut[te * K + k], t.U[k]);
        });
      double sum = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const double u = (tau < g.nt) ? ut[tau * K + k] : 0.0;
        r[k] = exp((lp[k] + u) - Tt * Ela[k]);   // no max-subtraction, as model.py:807
        sum += r[k];
      }
      if (sum > 0.0) {   // model.py:808-811; a true divide: 1/sum overflows when sum is subnormal
#pragma unroll
        for (int k = 0; k < K; ++k) r[k] /= sum;
      }
      if (act && s == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
          rl[tg * K + k] = r[k];
          accF[k] += (g.fuse_full && rowfull) ? r[k] : 0.0;
        }
      }
    }
    if (s == 0 && tau < g.nt) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        rt[tau * K + k] = r[k];
        if (ELBO) ut[tau * K + k] = exp(r[k]);   // exp(rho), model.py:971 (U is consumed)
      }
      if (ELBO) qs[tau] = 0u;
    }
    if (ELBO) __syncthreads(); else __builtin_amdgcn_wave_barrier();   // Q crosses waves, the rest is wave-local
    // walk 2: H of the new rho; ELBO log terms and mirror sums
    if (do_hist || ELBO) sc.walk<SumQ>(xt, g, tau, s, act, wq,
      [&](int te, int m, unsigned x, SumQ& acc) {
        const double dx = (double)x;
        const int mt = cur.mirror(te);
        const unsigned y = MUT ? (unsigned)xt[mt * g.stride + m] : 0u;
        if (do_hist) hist_add<K>(Hc, Hl, g.Mp, m, y, dx, rt + te * K, (unsigned)g.hc);
        if (ELBO) {
          const bool in_r = (rw[te * g.W + (m >> 6)] >> (m & 63)) & 1ull;
          double inner = 0.0;
          if (in_r) {
            const double z2 = gnu * (double)y, gt = Gth[m];
            const double* er = ut + te * K;
#pragma unroll
            for (int k = 0; k < K; ++k) inner += er[k] * (gt * Gla[k] + z2);
          }
          e_log += dx * log(inner + eps);
          if (MUT && ((rw[mt * g.W + (m >> 6)] >> (m & 63)) & 1ull)) acc.q += x;   // R[mirror] X^T[mirror]
        }
      },
      [&](int te, const SumQ& t) {   // Q of the MIRROR tie: sum_m R[mirror,m] X[this,m]
        if (ELBO && t.q) atomicAdd(&qs[cur.mirror(te)], t.q);
      });
    if (ELBO) {
      __syncthreads();
      if (act && s == 0) {
        double sr = 0.0, se = 0.0, ent = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          sr += r[k]; se += r[k] * Ela[k];
          ent += r[k] * lp[k] - r[k] * log(r[k] + eps);   // model.py:1306-1313
        }
        e_lin += ent - se * Tt;
        e_q += sr * (double)qs[tau];
      }
    }
    __syncthreads();
  }
  if (do_hist) hist_flush(Hc, Hl, nHc);
  if (UPDATE && g.fuse_full) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      double v = block_sum(accF[k], red);
      if (threadIdx.x == 0) atomicAdd(&a.slotF[((size_t)l * NSLOT + (gb % NSLOT)) * K + k], v);
    }
  }
  if (ELBO) {
    double v1 = block_sum(e_lin, red);
    double v2 = block_sum(e_log, red);
    double v3 = block_sum(e_q, red);
    if (threadIdx.x == 0) {
      double* out = a.slotR + (size_t)(blockIdx.x % NSLOT) * 4;
      atomicAdd(&out[1], v1); atomicAdd(&out[2], v2); atomicAdd(&out[3], v3);
    }
  }
}

static size_t shmem_ct(const Geo& g) { return g.mut ? (size_t)g.Mp * g.K * 8 : 0; }
static size_t shmem_q() { return (size_t)(TPB / 64) * 64 * QCAP * 2; }
static size_t shmem_hc(const Geo& g) { return (size_t)g.hc * g.Mp * g.K * 8; }
size_t shmem_hist(const Geo& g) {
  return (size_t)g.nt * g.stride + (size_t)g.nt * g.K * 8 + shmem_hc(g) + shmem_q() + 16;
}
size_t shmem_rho(const Geo& g, bool update, bool elbo) {
  size_t n = (size_t)g.nt * g.stride + (size_t)g.nt * g.W * 8 + (size_t)g.W * 8 + (size_t)g.Mp * 8 + 64 + shmem_ct(g) +
             2 * (size_t)g.nt * g.K * 8 + shmem_q();
  if (update && !g.two_pass) n += shmem_hc(g);
  if (elbo) n += (size_t)g.Mp * 8 + (size_t)g.nt * 4;
  return n + 16;
}

// K and the prefetch depth (4, 8 or 12 sixteen-byte chunks per thread)
#define DISPATCH_KP(K_, PF_, ...)                                     \
  switch (PF_) {                                                      \
    case 4: { constexpr int PP = 4; DISPATCH_K(K_, __VA_ARGS__); } break;   \
    case 8: { constexpr int PP = 8; DISPATCH_K(K_, __VA_ARGS__); } break;   \
    default: { constexpr int PP = 12; DISPATCH_K(K_, __VA_ARGS__); } break; \
  }

// lists_only: a vmr_create_coo handle, which never launches the dense tiles (their LDS bound does not limit M there)
int choose_geo(Geo& g, int ncu, std::string& err, bool lists_only) {
  g.Mp = (g.M + 15) / 16 * 16;
  g.nchunk = g.Mp / 16;
  g.stride = (g.nchunk % 2 == 1) ? g.Mp : g.Mp + 16;
  g.W = (g.M + 63) / 64;
  const size_t budget = 48 * 1024;
  // per-reporter LDS tables of the rho pass beside the tile pair (see shmem_rho): they cap the tile edge too
  const size_t tables = (size_t)g.Mp * 8 * (2 + (g.mut ? g.K : 0)) + (size_t)g.W * 8 + shmem_q() + 256;
  auto lds = [&](int b_) { return (size_t)2 * b_ * b_ * (g.stride + (size_t)g.W * 8 + 2 * g.K * 8 + 4) + tables; };
  int b = 8;
  while (b > 1 && ((size_t)2 * b * b * g.stride > budget || lds(b) > 160 * 1024)) b >>= 1;
  if ((size_t)2 * b * b * g.stride > budget && !lists_only) { err = "M too large for the LDS tile (M <= ~24500 supported)"; return VMR_EINVAL; }
  g.b = b; g.lb = (b == 8) ? 3 : (b == 4) ? 2 : (b == 2) ? 1 : 0;
  g.nb = (g.N + b - 1) / b;
  g.nt = 2 * b * b;
  g.S = TPB / g.nt; if (g.S > 64) g.S = 64;
  g.lS = 0; while ((1 << g.lS) < g.S) ++g.lS;
  g.P = (long long)g.nb * (g.nb + 1) / 2;
  g.Gl = 0;   // per launch, see grid_per_layer()
  g.Y = 1;    // set by vmr_create once the largest count is known
  g.hc = 0;
  g.two_pass = 0;
  g.farl = 0;
  g.fuse_full = 0;
  long long T = (long long)g.N * g.N;
  long long gm = (long long)ncu * 8 / g.L; if (gm < 1) gm = 1;
  long long maxgm = (T + 255) / 256; if (gm > maxgm) gm = maxgm; if (gm < 1) gm = 1;
  g.Gm = (int)gm;
  int need = (g.nt * g.nchunk + TPB - 1) / TPB;
  g.pf = need <= 4 ? 4 : need <= 8 ? 8 : 12;
  return VMR_OK;
}

int tiles_hist(vmr_ctx* h) {
  const Geo& g = h->g;
  HistArgs a{h->X, h->rho, h->Hg, 1};
  size_t sm = shmem_hist(g);
  int rc = VMR_OK;
  if (g.mut) {
    DISPATCH_KP(g.K, g.pf, if ((rc = grid_per_layer(h, k_hist<KK, true, PP>, sm, &a.Gl))) return rc;
                hipLaunchKernelGGL((k_hist<KK, true, PP>), dim3(g.L * a.Gl), dim3(TPB), sm, h->stream, a, g));
  } else {
    DISPATCH_KP(g.K, g.pf, if ((rc = grid_per_layer(h, k_hist<KK, false, PP>, sm, &a.Gl))) return rc;
                hipLaunchKernelGGL((k_hist<KK, false, PP>), dim3(g.L * a.Gl), dim3(TPB), sm, h->stream, a, g));
  }
  return VMR_OK;
}

int tiles_rho(vmr_ctx* h, int mode, size_t sm) {
  const Geo& g = h->g;
  RhoArgs a{h->X, h->Rb, h->rho, h->logpr, h->par, h->slotR, h->lutg, h->Hg, h->slotF, 1};
  dim3 blk(TPB);
  int rc = VMR_OK;
#define LRHO(MUT_, UPD_, ELB_)                                                                  \
  DISPATCH_KP(g.K, g.pf, if ((rc = grid_per_layer(h, k_rho<KK, MUT_, UPD_, ELB_, PP>, sm, &a.Gl))) return rc; \
              hipLaunchKernelGGL((k_rho<KK, MUT_, UPD_, ELB_, PP>), dim3(g.L * a.Gl), blk, sm, h->stream, a, g))
  if (g.mut) {
    if (mode == 0) { LRHO(true, true, false); } else if (mode == 1) { LRHO(true, true, true); } else { LRHO(true, false, true); }
  } else {
    if (mode == 0) { LRHO(false, true, false); } else if (mode == 1) { LRHO(false, true, true); } else { LRHO(false, false, true); }
  }
#undef LRHO
  return VMR_OK;
}
