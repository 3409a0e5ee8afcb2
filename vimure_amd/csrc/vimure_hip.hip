// libvimure_hip.so -- MI355X (gfx950 / CDNA4) CAVI engine for the VIMuRe model.
//
// Implements the reference's hot path (latentnetworks/vimure, src/python/vimure/model.py:
// _update_CAVI :623-660, _update_cache :662-696, _update_gamma :698-727, _update_phi :729-761,
// _update_rho :763-818, _update_nu :820-830, __ELBO :948-1019) behind the C-ABI of include/vimure_hip.h.
// Design notes, data layout and byte accounting: DESIGN.md.
//
// This file is the engine proper: the set-state kernels, the mask sums, the finalize kernels, the launch logic of a sweep
// (launch_hist / launch_gamma / launch_phi / launch_rho), step_n, the fit loops, the lockstep batch, and the state, read-out
// and profile API.  What a sweep launches lives in units of its own:
//   sweep_sl.hip     the sweep kernel over the sorted report lists, one object per K (sweep_sl.h)     -- the default format
//   sweep_gen.hip    the general kernels: any K, wide entries (sweep_gen.h)
//   sweep_tiles.hip  the dense tile path: k_hist, k_rho, the geometry and the LDS sizes (sweep_tiles.h)
// and what makes a handle does too:
//   create.hip       vmr_create, the shared tail of both creators, vmr_destroy (create.h)
//   create_coo.hip   vmr_create_coo
//   sorted_lists.hip the sorted report lists and the permutation kernels of the boundary functions
//
// One sweep:  mask sums A -> k_fin_gamma -> the rho pass (which rebuilds the statistics H) -> k_fin_rho.
//   k_gamma_mask   A[l,m,k] = sum_ij R rho: mask words become the EXEC mask of K v_add_f64 (lane <-> reporter).
//   k_mask_lists   the same sums from the mask lists of partial rows that hold few reporters.
//   k_fin_*        gamma, phi, nu from H and A, the Gamma expectations (digamma/log/exp), ELBO assembly -- no host round
//                  trip inside a sweep.
//   k_far_hist     the statistics of the reports of the levels beyond the LDS ones (Geo::farl).
#include "vmr_internal.h"
#include "sweep_sl.h"
#include "sweep_gen.h"
#include "sweep_tiles.h"
#include "create.h"
#include "sample_draw.h"

thread_local std::string g_create_err;

// ------------------------------------------------------------------------------------------
// set-state kernels
// ------------------------------------------------------------------------------------------
__global__ void k_init_rho(const double* __restrict__ pr, double* __restrict__ rho, double* __restrict__ logpr,
                           size_t n, double eps) {
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < n; q += (size_t)gridDim.x * blockDim.x) {
    double v = pr[q];
    rho[q] = v;
    logpr[q] = log(v + eps);
  }
}

// the same for a handle whose rho / log prior live in sorted position order (sweep_sl.h): pr is in tie order
// (rs / not_onehot: does every tie of a step WITHOUT reports carry the one-hot prior (1, 0, .., 0) the reference gives ties nobody
// reported on (model.py:536-556)?  Then the sweeps need not read the log prior of those steps -- SlArgs::lp0)
__global__ void k_init_rho_pos(const double* __restrict__ pr, double* __restrict__ rho, double* __restrict__ logpr,
                               const unsigned* __restrict__ perm, size_t T, size_t NS, int L, int K, double eps,
                               const unsigned* __restrict__ rs, int* __restrict__ not_onehot) {
  const size_t n = (size_t)L * T * K;
  bool bad = false;
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < n; q += (size_t)gridDim.x * blockDim.x) {
    const size_t row = q / K, k = q - row * K, l = row / T, pos = row - l * T;
    const double v = pr[(l * T + perm[l * NS * 64 + pos]) * K + k];
    rho[q] = v;
    logpr[q] = log(v + eps);
    const unsigned* rsl = rs + l * (NS + 1);
    const size_t st = pos >> 6;
    if (rsl[st + 1] == rsl[st] && v != (k == 0 ? 1.0 : 0.0)) bad = true;
  }
  if (bad) atomicOr(not_onehot, 1);
}

// K = 2 (SlArgs::lpd): lpd[row] = logpr[row][1] - logpr[row][0] over the L T rows by position (lpd null: VMR_NO_LPD), and the layers' bounds
// lpb[l][k] = max |logpr[l][.][k]| (non-negative doubles order as their bit patterns: an integer max; a NaN bound fails every test)
__global__ __launch_bounds__(256) void k_lpd(const double* __restrict__ logpr, double* __restrict__ lpd, unsigned long long* __restrict__ lpb, size_t T, int L) {
  for (int l = 0; l < L; ++l) {
    unsigned long long m0 = 0ull, m1 = 0ull;
    for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < T; q += (size_t)gridDim.x * blockDim.x) {
      const size_t row = (size_t)l * T + q;
      const double v0 = logpr[row * 2], v1 = logpr[row * 2 + 1];
      if (lpd) lpd[row] = v1 - v0;
      m0 = max(m0, (unsigned long long)__double_as_longlong(fabs(v0)));
      m1 = max(m1, (unsigned long long)__double_as_longlong(fabs(v1)));
    }
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) {
      m0 = max(m0, (unsigned long long)__shfl_xor((long long)m0, o2, 64));
      m1 = max(m1, (unsigned long long)__shfl_xor((long long)m1, o2, 64));
    }
    if ((threadIdx.x & 63) == 0) { atomicMax(&lpb[2 * l], m0); atomicMax(&lpb[2 * l + 1], m1); }
  }
}

// nibble LUT of E[theta] for wide masks: lut[l][n][e] = sum of E[theta_m] over the set bits e of reporters 4n..4n+3
__global__ void k_build_lut(const double* __restrict__ par, double* __restrict__ lutg, Geo g) {
  const ParOff o = par_off(g.L, g.Mp, g.K);
  const int l = blockIdx.x;
  const double* Eth = par + o.E_th + (size_t)l * g.Mp;
  for (int q = threadIdx.x; q < g.W * 256; q += blockDim.x) {
    int n = q >> 4, e = q & 15;
    double v = 0.0;
    for (int u = 0; u < 4; ++u) {
      int m = n * 4 + u;
      if (((e >> u) & 1) && m < g.Mp) v += Eth[m];
    }
    lutg[(size_t)l * g.W * 256 + q] = v;
  }
}

// derived expectations of all Gamma factors from shp/rte (used after vmr_set_state)
__global__ void k_derive_all(double* par, Geo g) {
  ParOff o = par_off(g.L, g.Mp, g.K);
  int tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
  for (int q = tid; q < g.L * g.Mp; q += nth) {
    int m = q % g.Mp;
    if (m < g.M) {
      double s = par[o.g_shp + q], r = par[o.g_rte + q];
      double l = digamma_pos(s) - log(r);
      par[o.E_th + q] = s / r; par[o.l_th + q] = l; par[o.G_th + q] = exp(l);
    } else {
      par[o.E_th + q] = 0.0; par[o.l_th + q] = 0.0; par[o.G_th + q] = 0.0;
    }
  }
  for (int q = tid; q < g.L * g.K; q += nth) {
    double s = par[o.p_shp + q], r = par[o.p_rte + q];
    double l = digamma_pos(s) - log(r);
    par[o.E_la + q] = s / r; par[o.l_la + q] = l; par[o.G_la + q] = exp(l);
  }
  if (tid == 0) {
    double* sc = par + o.sc;
    double gn = g.mut ? exp(digamma_pos(sc[SC_NU_SHP]) - log(sc[SC_NU_RTE])) : 0.0;  // model.py:596-600
    sc[SC_G_NU] = gn; sc[SC_G_NU_STALE] = gn;
    sc[SC_E_NU] = sc[SC_NU_SHP] / sc[SC_NU_RTE];
  }
}

// ------------------------------------------------------------------------------------------
// gamma, mask half:  A[l,m,k] = sum_{i,j} R[l,i,j,m] rho[l,i,j,k]
// (gives gamma_rte = beta + sum_k E[lambda_k] A  -- model.py:704-718 -- and, with the new
//  E[theta], phi_rte = beta + sum_m E[theta_m] A -- model.py:742-749 -- from ONE pass over R)
// Output: slotA[l][slot][m][k] accumulated with global f64 atomics (zeroed by k_fin_gamma).
// ------------------------------------------------------------------------------------------
// A wave takes 64 consecutive ties per trip, lane <-> tie for the (coalesced, prefetched) loads of
// the R-row words and rho.  Rows whose words are all ones only feed a per-lane sum (one v_add_f64
// per k and 64 ties); every other row is broadcast with v_readlane and added under EXEC = its bits
// (lane <-> reporter).
// DET (Geo::det): a wave's sums -- ties in a fixed order, so the same bits every run -- go as fixed-point integers (det_sha) into
// the shadow of slotA's slot 0 (detA, vmr_ctx::det_buf), where the order of the adds does not matter; det_fold makes them doubles.
template <int K, int NC, bool DET>
__global__ __launch_bounds__(TPB) void k_gamma_mask(const uint64_t* __restrict__ Rb, const double* __restrict__ rho,
                                                    const uint8_t* __restrict__ rcls, double* __restrict__ slotA,
                                                    int skip_full, const unsigned* __restrict__ perm /* rho by sorted position, or null */, Geo g,
                                                    unsigned long long* __restrict__ detA) {
  __shared__ double sacc[NC * 64 * K];
  const int l = blockIdx.x / g.Gm, gb = blockIdx.x - l * g.Gm;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const long long T = (long long)g.N * g.N;
  const long long nw = (long long)g.Gm * (TPB / 64), gw = (long long)gb * (TPB / 64) + wave;
  const long long t0 = gw * T / nw, t1 = (gw + 1) * T / nw;
  const uint64_t* Rl = Rb + (size_t)l * T * g.W;
  const double* rl = rho + (size_t)l * T * K;
  const uint8_t* cl = rcls + (size_t)l * T;
  const unsigned* pl = perm ? perm + (size_t)l * ((T + 63) / 64) * 64 : nullptr;
  const int Wp = g.W * 64;
  for (int cg = 0; cg < g.W; cg += NC) {
    const int nc = min(NC, g.W - cg);   // == NC except in the last group of a wide mask
    double acc[NC][K], accF[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      accF[k] = 0.0;
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c][k] = 0.0;
    }
    uint64_t wq[NC];
    double rq[K];
    unsigned cq = 0;   // the row's class: "all ones" must mean the whole row, not just this group's words
    auto fetch = [&](long long tb) {
      long long t = tb + lane;
      bool ok = t < t1;
      const long long pc = ok ? t : t1 - 1;              // position (= tie when rho is in tie order)
      const long long tc = pl ? (long long)pl[pc] : pc;   // the tie whose mask row this is
#pragma unroll
      for (int c = 0; c < NC; ++c) wq[c] = (ok && c < nc) ? Rl[tc * g.W + cg + c] : 0ull;
#pragma unroll
      for (int k = 0; k < K; ++k) rq[k] = ok ? rl[pc * K + k] : 0.0;
      cq = ok ? (unsigned)cl[tc] : 0u;
    };
    if (t0 < t1) fetch(t0);
    for (long long tb = t0; tb < t1; tb += 64) {
      uint64_t w[NC];
      double r[K];
#pragma unroll
      for (int c = 0; c < NC; ++c) w[c] = wq[c];
#pragma unroll
      for (int k = 0; k < K; ++k) r[k] = rq[k];
      const bool full = cq == 1u;
      if (tb + 64 < t1) fetch(tb + 64);   // in flight during this batch
      bool any = false;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (c < nc) any = any || (w[c] != 0ull);
      }
#pragma unroll
      for (int k = 0; k < K; ++k) accF[k] += (full && !skip_full) ? r[k] : 0.0;   // skip_full: the rho pass summed them
      uint64_t todo = __ballot(any && !full);
      while (todo) {
        int i = __builtin_ctzll(todo);
        todo &= todo - 1;
        double ri[K];
#pragma unroll
        for (int k = 0; k < K; ++k) ri[k] = readlane_f64(r[k], i);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          if (c < nc) {
            uint64_t wi = readlane64(w[c], i);
            if (__builtin_amdgcn_inverse_ballot_w64(wi)) {
#pragma unroll
              for (int k = 0; k < K; ++k) acc[c][k] += ri[k];
            }
          }
        }
      }
    }
    // all-ones rows: every reporter of the group gets the same sum
#pragma unroll
    for (int k = 0; k < K; ++k) {
      double u = wave_sum(accF[k]);
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < nc && (cg + c) * 64 + lane < g.M) acc[c][k] += u;
    }
    if (DET) {
      unsigned long long* outd = detA + ((size_t)l * Wp + cg * 64) * K;
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (c < nc && acc[c][k] != 0.0) atomicAdd(&outd[(c * 64 + lane) * K + k], det_fx(acc[c][k], g.det_sha));
      continue;
    }
    // combine the 4 waves in LDS, then one global atomic per (m,k) and workgroup
    for (int q = threadIdx.x; q < NC * 64 * K; q += TPB) sacc[q] = 0.0;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int k = 0; k < K; ++k) atomicAdd(&sacc[(c * 64 + lane) * K + k], acc[c][k]);
    __syncthreads();
    double* out = slotA + (((size_t)l * NSLOT + (gb % NSLOT)) * Wp + cg * 64) * K;
    for (int q = threadIdx.x; q < nc * 64 * K; q += TPB) atomicAdd(&out[q], sacc[q]);
    __syncthreads();
  }
}

// A[l,m,k] += rho[l,t,k] over the listed reporters of the partial rows (model.py:704-718, 742-749); all-ones rows
// were summed by the rho pass.  One thread per tie, A of the workgroup in LDS, one global add per value at the end.
// (The mask lists rq / Rm: create.hip, beside k_rm_count.)
template <int K>
__global__ __launch_bounds__(TPB) void k_mask_lists(const unsigned* __restrict__ rq, const unsigned short* __restrict__ Rm,
                                                    const unsigned long long* __restrict__ rbase, const uint8_t* __restrict__ rcls,
                                                    const double* __restrict__ rho, double* __restrict__ slotA, int Gl,
                                                    const unsigned* __restrict__ perm /* rho by sorted position, or null */, Geo g) {
  extern __shared__ double As[];   // [Mp][K]
  const int l = blockIdx.x / Gl, gb = blockIdx.x - l * Gl;
  const size_t T = (size_t)g.N * g.N;
  const unsigned* rql = rq + (size_t)l * (T + 1);
  const unsigned short* Rml = Rm + rbase[l];
  const uint8_t* cl = rcls + (size_t)l * T;
  const double* rl = rho + (size_t)l * T * K;
  for (int q = threadIdx.x; q < g.Mp * K; q += TPB) As[q] = 0.0;
  __syncthreads();
  const size_t t0 = (size_t)gb * T / Gl, t1 = (size_t)(gb + 1) * T / Gl;
  const unsigned* pl = perm ? perm + (size_t)l * ((T + 63) / 64) * 64 : nullptr;
  for (size_t p = t0 + threadIdx.x; p < t1; p += TPB) {
    const size_t t = pl ? (size_t)pl[p] : p;
    if (cl[t] != 2) continue;
    const unsigned q0 = rql[t], q1 = rql[t + 1];
    double r[K];
#pragma unroll
    for (int k = 0; k < K; ++k) r[k] = rl[p * K + k];
    for (unsigned q = q0; q < q1; ++q) {
      const int m = Rml[q];
#pragma unroll
      for (int k = 0; k < K; ++k) atomicAdd(&As[m * K + k], r[k]);
    }
  }
  __syncthreads();
  double* out = slotA + ((size_t)l * NSLOT + (gb % NSLOT)) * (size_t)g.W * 64 * K;
  for (int q = threadIdx.x; q < g.M * K; q += TPB) {
    const double v = As[q];
    if (v != 0.0) atomicAdd(&out[q], v);
  }
}

// ------------------------------------------------------------------------------------------
// H is accumulated in NH copies (workgroup gb adds into copy gb % NH; adding the rare high levels to one copy
// only was tried: the rho pass ran 1.8x longer on the contended addresses).  Before anything reads it the copies
// are folded into copy 0 by many workgroups (k_fin_rho does it on its way, k_h_reduce otherwise): one workgroup
// per layer reading 8 x 50 KB was most of the finalize kernels' time.
__device__ __forceinline__ double h_fold(double* Hl0, size_t copy_stride, size_t idx) {
  double v[NH];
#pragma unroll
  for (int c = 0; c < NH; ++c) v[c] = Hl0[c * copy_stride + idx];   // all copies in flight at once
  double t = 0.0;
#pragma unroll
  for (int c = 0; c < NH; ++c) {
    t += v[c];
    if (c > 0) Hl0[c * copy_stride + idx] = 0.0;
  }
  Hl0[idx] = t;
  return t;
}
// Fold the K values of one (y, m) item.  Report lists (Cl != null) accumulate categories 1..K-1 and, in slot 0, the
// deficit sum x (1 - sum_k rho_k) of irregular ties; with Cl[y][m] = sum x over the item's reports (a constant of the
// data, from the count-mode launch of vmr_create): H_0 = C - deficit - sum_{k>0} H_k.
__device__ __forceinline__ void h_fold_item(double* Hl0, size_t copy_stride, size_t item, int K, const double* Cl, double* out) {
  double rest = 0.0;
  for (int k = K - 1; k >= 0; --k) {
    double v = h_fold(Hl0, copy_stride, item * K + k);
    if (k > 0) rest += v;
    else if (Cl) { v = Cl[item] - v - rest; Hl0[item * K] = v; }
    out[k] = v;
  }
}
__global__ __launch_bounds__(TPB) void k_h_reduce(double* Hg, const double* Cg, Geo g) {
  const size_t items = (size_t)g.Y * g.Mp, hcs = items * g.K, n = (size_t)g.L * items;
  double tmp[KMAX];
  for (size_t q = (size_t)blockIdx.x * TPB + threadIdx.x; q < n; q += (size_t)gridDim.x * TPB) {
    const size_t l = q / items, it = q - l * items;
    h_fold_item(Hg + l * NH * hcs, hcs, it, g.K, Cg ? Cg + l * items : nullptr, tmp);
  }
}
// count-mode result -> the constants C[l][y][m], leaving H zeroed
__global__ __launch_bounds__(TPB) void k_take_counts(double* Hg, double* Cg, Geo g) {
  const size_t items = (size_t)g.Y * g.Mp, hcs = items * g.K, n = (size_t)g.L * items;
  for (size_t q = (size_t)blockIdx.x * TPB + threadIdx.x; q < n; q += (size_t)gridDim.x * TPB) {
    const size_t l = q / items, it = q - l * items;
    double* Hl0 = Hg + l * NH * hcs;
    Cg[q] = h_fold(Hl0, hcs, it * g.K + 1);   // count mode put sum x into category 1
    Hl0[it * g.K + 1] = 0.0;
  }
}
template <bool ZERO>
__device__ __forceinline__ double h_sum(double* Hl0, size_t, size_t idx) {   // folded H: copy 0
  const double v = Hl0[idx];
  if (ZERO) Hl0[idx] = 0.0;
  return v;
}
__device__ __forceinline__ double h_at(const double* Hl0, size_t, size_t idx) { return Hl0[idx]; }

#ifndef FIN_TPB
#define FIN_TPB 512   // (1024: 128 registers, 16-33 spilled, +2 us per launch; 256: +5 us)
#endif
__device__ __forceinline__ double block_sum_fin(double v, double* red /*16*/) {   // result valid in thread 0
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x == 0) {
    for (int w = 0; w < FIN_TPB / 64; ++w) r += red[w];
  }
  return r;
}

// finalize kernels
// ------------------------------------------------------------------------------------------
// gamma_shp from H with the current (old) weights (model.py:698-703), gamma_rte from A (model.py:704-718), then phi_rte from
// the same A with the new E[theta] (model.py:742-749) and phi_shp from H with the new E[log theta] (model.py:731-733, 861-887;
// mutuality off: from the level-0 sums), the factor table F of the rho pass, the LUT of E[theta].
// FG_G workgroups per layer, each owning a range of REPORTERS: everything of gamma is local to a reporter, so a workgroup
// reads the (y, m) items of its own reporters (kept in registers for the second, phi, use when they are few), finishes their
// gamma and adds its share of the 2 K sums that lambda needs to `fin` with device-scope atomics; the workgroup that draws the
// layer's last ticket finishes lambda and builds F and the LUT from the theta values the others published (release before
// the ticket, acquire after it).  One workgroup per layer (rounds 1-2) kept 4 of 256 CUs busy for 25 us per sweep.
// consume = 1 (fused sweep): H and slotF are read for the last time here and left zeroed for the rho pass.
// (bx: the workgroup's index in its handle's grid -- the launch's, or the handle's share of a lockstep launch, k_fin_gamma_b)
template <bool det /*Geo::det: sums whose order would vary are integer or in slots (its own instantiation: the code costs the plain one 3 us)*/>
__device__ __forceinline__ void fin_gamma_body(double* par, double* Hg, const double* __restrict__ Cg, double* slotA, double* slotF,
                                               double* lutg, double* Fg, double* fin /*[L][2 KMAX + 2]*/, double* nu_acc,
                                               int nh /*copies of H to fold: NH, or 1 when folded already*/, int do_phi, int consume, const Geo& g,
                                               const int bx, const int fg = FG_G /*workgroups per layer of this launch (<= FG_G)*/) {
  extern __shared__ double dyn[];   // s1[mper]: sum_{y,k} w1 H per reporter; gthn[mper]: the new G_theta
  __shared__ double red[16];
  __shared__ double ela_old[KMAX], gla_old[KMAX], fk[KMAX];
  __shared__ double lla_n[KMAX], gla_n[KMAX];   // the new E[log lambda], G_lambda (for the factor table F)
  __shared__ int last;
  const ParOff o = par_off(g.L, g.Mp, g.K);
  const int l = bx / fg, gq = bx - l * fg, K = g.K, Wp = g.W * 64, tid = threadIdx.x;
  const int mper = (g.M + fg - 1) / fg, m0 = gq * mper, m1 = min(g.M, m0 + mper), nm = max(0, m1 - m0);
  double* s1 = dyn;
  double* gthn = dyn + mper;
  double* finl = fin + (size_t)l * (2 * KMAX + 2);
  if (tid < K) {
    double fv[NSLOT], f = 0.0;   // all-ones mask rows, summed by the rho pass (zero when the mask kernel handled them)
#pragma unroll
    for (int sl = 0; sl < NSLOT; ++sl) fv[sl] = slotF[((size_t)l * NSLOT + sl) * K + tid];   // loads first, all in flight
#pragma unroll
    for (int sl = 0; sl < NSLOT; ++sl) f += fv[sl];
    fk[tid] = f;
    ela_old[tid] = par[o.p_shp + l * K + tid] / par[o.p_rte + l * K + tid];
    gla_old[tid] = par[o.G_la + l * K + tid];
  }
  for (int m = tid; m < mper; m += FIN_TPB) { s1[m] = 0.0; gthn[m] = 0.0; }
  __syncthreads();
  const double gnu = par[o.sc + SC_G_NU];
  const size_t hcs = (size_t)g.Y * g.Mp * K;
  double* Hl = Hg + (size_t)l * NH * hcs;
  const int items = g.Y * nm;                 // (y, m) items of this workgroup's reporters
  const bool phi2 = do_phi && g.mut;          // a second use of H follows (phi_shp with the new E[log theta])
  const bool cached = items <= FIN_TPB;       // one item per thread: its K values stay in registers for that second use
  double hv[KMAX], p0[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) { hv[k] = 0.0; p0[k] = 0.0; }
  // One (y, m) item: its K values summed over the nh copies the workgroups of the pass added into (all loads in flight at
  // once).  Report lists (Cl != null) accumulate categories 1..K-1 and, in slot 0, the deficit of irregular ties:
  // H_0 = C - deficit - sum_{k>0} H_k with C[y][m] = sum x a constant of the data.  zero: leave the copies zeroed.
  const double* Cl = Cg ? Cg + (size_t)l * g.Y * g.Mp : nullptr;
  auto item = [&](int y, int m, double (&h_)[KMAX], bool zero) {
    const size_t base = ((size_t)y * g.Mp + m) * K;
    double rest = 0.0;
#pragma unroll
    for (int k = KMAX - 1; k >= 0; --k) {
      if (k < K) {
        double v[NH], t = 0.0;
#pragma unroll
        for (int c = 0; c < NH; ++c) v[c] = c < nh ? Hl[(size_t)c * hcs + base + k] : 0.0;   // loads first, all in flight
#pragma unroll
        for (int c = 0; c < NH; ++c) {
          t += v[c];
          if (zero && c < nh) Hl[(size_t)c * hcs + base + k] = 0.0;
        }
        if (k > 0) rest += t;
        else if (Cl && nh > 1) t = Cl[(size_t)y * g.Mp + m] - t - rest;   // (a folded H holds H_0 itself)
        h_[k] = t;
      }
    }
  };
  for (int it = tid; it < items; it += FIN_TPB) {
    const int y = it / nm, m = m0 + (it - y * nm);
    const double gth = par[o.G_th + (size_t)l * g.Mp + m];   // still the old value
    double acc = 0.0;
    item(y, m, hv, consume && (!phi2 || cached));
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (k < K) {
        acc += (g.mut ? w1_of(gth * gla_old[k], gnu * (double)y) : 1.0) * hv[k];
        if (y == 0) p0[k] += hv[k];
      }
    }
    if (acc != 0.0) {
      if (det) atomicAdd(reinterpret_cast<unsigned long long*>(&s1[m - m0]), det_fx(acc, g.det_sh));   // (threads of several waves add here)
      else atomicAdd(&s1[m - m0], acc);
    }
  }
  __syncthreads();
  if (det) {
    for (int m = tid; m < mper; m += FIN_TPB) s1[m] = det_back(*reinterpret_cast<unsigned long long*>(&s1[m]), g.det_sh);
    __syncthreads();
  }
  double pr[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) pr[k] = 0.0;
  for (int mi = tid; mi < nm; mi += FIN_TPB) {
    const int m = m0 + mi;
    const size_t q = (size_t)l * g.Mp + m;
    double A[KMAX], rte = 0.0;
    const double pa_th = par[o.a_th + q], pb_th = par[o.b_th + q];
    for (int k = 0; k < K; ++k) {
      double av[NSLOT], ak = 0.0;
      if (slotA) {   // (null: the mask has no partial rows, nothing ever lands in the slots -- a memory round trip less)
#pragma unroll
        for (int sl = 0; sl < NSLOT; ++sl) av[sl] = slotA[(((size_t)l * NSLOT + sl) * Wp + m) * K + k];   // loads first
#pragma unroll
        for (int sl = 0; sl < NSLOT; ++sl) {
          ak += av[sl];
          slotA[(((size_t)l * NSLOT + sl) * Wp + m) * K + k] = 0.0;   // consume: the slots are zero again for the next sweep
        }
      }
      ak += fk[k];
      A[k] = ak;
      rte += ela_old[k] * ak;
    }
    double shp = pa_th + s1[mi];
    rte = pb_th + rte;
    par[o.g_shp + q] = shp; par[o.g_rte + q] = rte;
    double e = shp / rte, lg = digamma_pos(shp) - log(rte);
    const double gn = exp(lg);
    par[o.E_th + q] = e; par[o.l_th + q] = lg; par[o.G_th + q] = gn;
    gthn[mi] = gn;
    for (int k = 0; k < K; ++k) pr[k] += e * A[k];
  }
  __syncthreads();
  // phi_shp's share of this workgroup: H with the NEW E[log theta] of its reporters (model.py:731-733, 861-887)
  double ps[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) ps[k] = 0.0;
  if (phi2) {
    if (cached) {
      if (tid < items) {
        const int y = tid / nm, mi = tid - y * nm;
        const double gth = gthn[mi];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) if (k < K) ps[k] = w1_of(gth * gla_old[k], gnu * (double)y) * hv[k];
      }
    } else {
      for (int it = tid; it < items; it += FIN_TPB) {
        const int y = it / nm, mi = it - y * nm;
        const double gth = gthn[mi];
        double h2[KMAX];
        item(y, m0 + mi, h2, consume != 0);
        for (int k = 0; k < K; ++k) ps[k] += w1_of(gth * gla_old[k], gnu * (double)y) * h2[k];
      }
    }
  } else if (!g.mut) {
#pragma unroll
    for (int k = 0; k < KMAX; ++k) ps[k] = p0[k];   // mutuality off: phi_shp = alpha + sum x rho_k
  }
  // this workgroup's shares of the 2 K sums, then its ticket
  for (int k = 0; k < K; ++k) {
    const double v = block_sum_fin(pr[k], red);
    const double w = block_sum_fin(ps[k], red);
    if (tid == 0) {
      if (det) { double* sl_ = fin + (size_t)g.L * (2 * KMAX + 2) + ((size_t)l * FG_G + gq) * 2 * KMAX; sl_[k] = v; sl_[KMAX + k] = w; }   // its own slot
      else { atomicAdd(&finl[k], v); atomicAdd(&finl[KMAX + k], w); }
    }
  }
  // publish this workgroup's theta values (every storing wave drained, then one agent-scope release) before the ticket
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    if (fg == 1) last = 1;   // (one workgroup has the whole layer: nothing to publish, no ticket, no fences)
    else {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const double t = atomicAdd(&finl[2 * KMAX], 1.0);
      last = (t == (double)(fg - 1));
      if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  if (!last) return;
  // ---- the layer's last workgroup: lambda, the factor table F, the LUT -------------------------------------------------
  if (tid < K) {
    const int k = tid, q = l * K + k;
    double sr, ss;
    if (det) {   // the workgroups' slots in order (published like the theta values: release before the ticket, acquire after it)
      sr = 0.0; ss = 0.0;
      const double* sl_ = fin + (size_t)g.L * (2 * KMAX + 2) + (size_t)l * FG_G * 2 * KMAX;
      for (int q = 0; q < FG_G; ++q) { sr += __builtin_nontemporal_load(&sl_[q * 2 * KMAX + k]); ss += __builtin_nontemporal_load(&sl_[q * 2 * KMAX + KMAX + k]); }
    } else { sr = atomicAdd(&finl[k], 0.0); ss = atomicAdd(&finl[KMAX + k], 0.0); }   // (device-scope reads)
    const double rte = par[o.b_la + q] + sr;
    if (g.mut && !do_phi) {
      par[o.p_rte_pend + q] = rte;   // the PHI sub-step commits (k_fin_phi)
    } else {
      const double shp = par[o.a_la + q] + ss;
      par[o.p_shp + q] = shp; par[o.p_rte + q] = rte;
      if (g.mut) par[o.p_rte_pend + q] = rte;
      const double lg = digamma_pos(shp) - log(rte);
      par[o.E_la + q] = shp / rte; par[o.l_la + q] = lg; par[o.G_la + q] = exp(lg);
      lla_n[k] = lg; gla_n[k] = exp(lg);
    }
  }
  __syncthreads();
  if (tid == 0) { for (int k = 0; k < 2 * KMAX + 1; ++k) finl[k] = 0.0; }   // scratch ready for the next sweep
  if (consume && tid < K) {
#pragma unroll
    for (int sl = 0; sl < NSLOT; ++sl) slotF[((size_t)l * NSLOT + sl) * K + tid] = 0.0;   // (every workgroup of the layer has read it)
  }
  // (fused sweep, report lists) the factor table F of the rho pass from the new theta, lambda and the current nu
  if (do_phi && Fg) {
    const int all = g.Y * g.Mp;
    double* Fl = Fg + (size_t)l * all * K;
    const double* lthn = par + o.l_th + (size_t)l * g.Mp;
    const double* gthg = par + o.G_th + (size_t)l * g.Mp;
    for (int it = tid; it < all; it += FIN_TPB) {
      const int y = it / g.Mp, m = it - y * g.Mp;
      const double lt = (m < g.M) ? lthn[m] : 0.0, gt = (m < g.M) ? gthg[m] : 0.0;
      for (int k = 0; k < K; ++k)
        Fl[(size_t)it * K + k] = (m < g.M) ? f_entry(g.mut, lt, gt, lla_n[k], gla_n[k], gnu, y) : 0.0;
    }
  }
  const double* Eth = par + o.E_th + (size_t)l * g.Mp;
  for (int q = tid; q < g.W * 256; q += FIN_TPB) {
    int n = q >> 4, e = q & 15;
    double v = 0.0;
    for (int u = 0; u < 4; ++u) {
      int m = n * 4 + u;
      if (((e >> u) & 1) && m < g.Mp) v += Eth[m];
    }
    lutg[(size_t)l * g.W * 256 + q] = v;
  }
  // (fused sweep, sorted lists) the constant part of the nu update the rho pass finishes itself (SlArgs::nu_acc):
  // sum_{y>0,m} w2_0(m, y) C[l][y][m] with the new theta, lambda and the current nu
  if (nu_acc && do_phi && g.mut && Cl) {
    const double* gthg = par + o.G_th + (size_t)l * g.Mp;
    double c0 = 0.0;
    for (int it = tid; it < g.Y * g.Mp; it += FIN_TPB) {
      const int y = it / g.Mp, m = it - y * g.Mp;
      if (y > 0 && m < g.M) {
        const double z2 = gnu * (double)y, den = gthg[m] * gla_n[0] + z2;
        if (den != 0.0) c0 += (z2 / den) * Cl[it];
      }
    }
    c0 = block_sum_fin(c0, red);
    if (tid == 0) nu_acc[2 + l] = c0;
  }
}
__global__ __launch_bounds__(FIN_TPB) void k_fin_gamma(double* par, double* Hg, const double* __restrict__ Cg, double* slotA, double* slotF,
                                                       double* lutg, double* Fg, double* fin, double* nu_acc, int nh, int do_phi, int consume, Geo g) {
  fin_gamma_body<false>(par, Hg, Cg, slotA, slotF, lutg, Fg, fin, nu_acc, nh, do_phi, consume, g, (int)blockIdx.x);
}
__global__ __launch_bounds__(FIN_TPB) void k_fin_gamma_det(double* par, double* Hg, const double* __restrict__ Cg, double* slotA, double* slotF,
                                                           double* lutg, double* Fg, double* fin, double* nu_acc, int nh, int do_phi, int consume, Geo g) {
  fin_gamma_body<true>(par, Hg, Cg, slotA, slotF, lutg, Fg, fin, nu_acc, nh, do_phi, consume, g, (int)blockIdx.x);
}
// the finalize kernels of many small handles in one launch (vmr_fit_loop_batch): workgroup -> unit through blk_unit
struct FinUnit {
  double *par, *Hg; const double* Cg; double *slotA, *slotF, *lutg, *fin_g, *nu_acc, *slotR, *elbo;   // (elbo: 8 doubles, as vmr_ctx::elbo_dev)
  Geo g; int fg_blk0, fr_blk0, fr_nblk;
};
// (fg workgroups per layer: 16 of them -- the latency of one handle's finalize -- times many units would queue up on the CUs)
__global__ __launch_bounds__(FIN_TPB) void k_fin_gamma_b(const FinUnit* __restrict__ units, const int* __restrict__ blk_unit, int fg) {
  const FinUnit& u = units[blk_unit[blockIdx.x]];
  fin_gamma_body<false>(u.par, u.Hg, u.Cg, u.slotA, u.slotF, u.lutg, nullptr, u.fin_g, u.nu_acc, NH, 1, 1, u.g, (int)blockIdx.x - u.fg_blk0, fg);
}

// phi commit, mutuality on: phi_shp from H with the NEW E[log theta] (model.py:731-733, 861-887; the cache
// refresh of :647 sits between the two updates), phi_rte as computed by k_fin_gamma (model.py:742-749)
__global__ __launch_bounds__(TPB) void k_fin_phi(double* par, const double* __restrict__ Hg, Geo g) {
  __shared__ double red[8];
  __shared__ double gla_old[KMAX];
  const ParOff o = par_off(g.L, g.Mp, g.K);
  const int l = blockIdx.x, K = g.K;
  if ((int)threadIdx.x < K) gla_old[threadIdx.x] = par[o.G_la + l * K + threadIdx.x];
  __syncthreads();
  const double gnu = par[o.sc + SC_G_NU];
  const size_t hcs = (size_t)g.Y * g.Mp * K;
  const double* Hl = Hg + (size_t)l * NH * hcs;
  double ps[KMAX];
  for (int k = 0; k < KMAX; ++k) ps[k] = 0.0;
  for (int m = threadIdx.x; m < g.M; m += TPB) {
    const double gth = par[o.G_th + (size_t)l * g.Mp + m];   // new
    for (int y = 0; y < g.Y; ++y)
      for (int k = 0; k < K; ++k) ps[k] += w1_of(gth * gla_old[k], gnu * (double)y) * h_at(Hl, hcs, ((size_t)y * g.Mp + m) * K + k);
  }
  for (int k = 0; k < K; ++k) {
    double v = block_sum(ps[k], red);
    if (threadIdx.x == 0) {
      const int q = l * K + k;
      double shp = par[o.a_la + q] + v, rte = par[o.p_rte_pend + q];
      par[o.p_shp + q] = shp; par[o.p_rte + q] = rte;
      double lg = digamma_pos(shp) - log(rte);
      par[o.E_la + q] = shp / rte; par[o.l_la + q] = lg; par[o.G_la + q] = exp(lg);
    }
  }
}

__device__ __forceinline__ double gamma_elbo_term(double pa, double pb, double qa, double qb) {
  // model.py:1300-1303
  return lgamma(qa) - pa * log(qb) + (pa - qa) * digamma_pos(qa) + qa * (1.0 - pb / qb);
}

// nu from H of the new rho (model.py:694-696, 822-825: sum x w2_k rho_k) and/or ELBO assembly (model.py:997-1013).
// One workgroup per layer adds its share to fin[0..1] with device-scope atomics; the workgroup that draws the
// last ticket (fin[2]) finishes the scalars and clears the scratch.
__device__ __forceinline__ void fin_rho_body(double* par, double* Hg, const double* Cg, double* slotR, double* elbo_out,
                                             double* fin, int do_nu, int do_elbo, int fold, int skip_nu /* the pass finished nu itself */, const Geo& g,
                                             const int bx, const int gx, double* slots = nullptr /*deterministic mode: [gx][2] partial sums, summed in order*/) {
  __shared__ double red[8];
  __shared__ int last;
  const ParOff o = par_off(g.L, g.Mp, g.K);
  double* sc = par + o.sc;
  const int l = bx / FR_G, gs = bx - l * FR_G;
  double a0 = 0.0, gt = 0.0;
  if (!skip_nu && (g.mut || fold)) {   // threads take (y, m) items of H; fold: the NH copies are summed into copy 0 on the way
    const double gnu = sc[SC_G_NU];
    const size_t hcs = (size_t)g.Y * g.Mp * g.K;
    double* Hl = Hg + (size_t)l * (g.gen ? 1 : NH) * hcs;   // (the general kernels keep one copy of H, every category in it)
    const long long items = (long long)g.Y * g.Mp, i0 = (long long)gs * items / FR_G, i1 = (long long)(gs + 1) * items / FR_G;
    for (long long it = i0 + (int)threadIdx.x; it < i1; it += TPB) {
      const int y = (int)(it / g.Mp), m = (int)(it - (long long)y * g.Mp);
      if (m >= g.M || (y == 0 && !fold)) continue;
      const double gth = par[o.G_th + (size_t)l * g.Mp + m], z2 = gnu * (double)y;
      if (fold) {   // (specialised kernels only: K <= KMAX)
        double hk[KMAX];
        h_fold_item(Hl, hcs, (size_t)it, g.K, Cg ? Cg + (size_t)l * items : nullptr, hk);
        for (int k = 0; k < g.K; ++k)
          if (g.mut && y > 0) a0 += w2_of(gth * par[o.G_la + l * g.K + k], z2) * hk[k];
      } else if (g.mut && y > 0) {
        for (int k = 0; k < g.K; ++k) {   // (general kernels, deterministic mode: the cells hold integers, sweep_gen.hip)
          const double hv = g.det ? det_back(reinterpret_cast<const unsigned long long*>(Hl)[(size_t)it * g.K + k], g.det_sh) : Hl[(size_t)it * g.K + k];
          if (hv != 0.0) a0 += w2_of(gth * par[o.G_la + l * g.K + k], z2) * hv;
        }
      }
    }
  }
  if (do_elbo) {
    for (int m = gs * TPB + threadIdx.x; m < g.M; m += FR_G * TPB) {
      const size_t q = (size_t)l * g.Mp + m;
      gt += gamma_elbo_term(par[o.a_th + q], par[o.b_th + q], par[o.g_shp + q], par[o.g_rte + q]);
    }
    if (gs == 0) {
      for (int k = threadIdx.x; k < g.K; k += TPB) {
        const int q = l * g.K + k;
        gt += gamma_elbo_term(par[o.a_la + q], par[o.b_la + q], par[o.p_shp + q], par[o.p_rte + q]);
      }
    }
  }
  a0 = block_sum(a0, red);
  gt = block_sum(gt, red);
  if (threadIdx.x == 0) {
    if (slots) { slots[2 * bx] = a0; slots[2 * bx + 1] = gt; __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); }
    else { atomicAdd(&fin[0], a0); atomicAdd(&fin[1], gt); }
    // the two adds are performed at the memory side before the ticket is drawn: they stay counted until they are (a full
    // __threadfence() -- L2 write-back and invalidate, ~3.5 us -- orders plain stores, of which the ticket publishes none)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const double t = atomicAdd(&fin[2], 1.0);
    last = (t == (double)(gx - 1));
  }
  __syncthreads();
  if (!last) return;
  double a1 = 0, a2 = 0, a3 = 0;
  if (g.gen && g.det) {
    // (the general kernels' deterministic pass added integers here, two words each: slots 0 .. NSLOT/2 - 1 at 2^-det_shr, the
    // others at 2^-(det_shr + DET_SH2), sweep_gen.hip's gen_fx2.  How they split over the slots depends on which workgroup drew which
    // step: summed as integers, then converted once -- a slot beyond 2^53 would round on its own)
    if (threadIdx.x == 0) {
      unsigned long long* pi = reinterpret_cast<unsigned long long*>(slotR);
      unsigned long long s[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
      for (int q = 0; q < NSLOT; ++q) {
        const int w = q < NSLOT / 2 ? 0 : 3;
        for (int i = 1; i <= 3; ++i) { s[w + i - 1] += pi[q * 4 + i]; pi[q * 4 + i] = 0ull; }
        pi[q * 4] = 0ull;
      }
      a1 = det_back(s[0], g.det_shr) + det_back(s[3], g.det_shr + DET_SH2);
      a2 = det_back(s[1], g.det_shr) + det_back(s[4], g.det_shr + DET_SH2);
      a3 = det_back(s[2], g.det_shr) + det_back(s[5], g.det_shr + DET_SH2);
    }
  } else if (threadIdx.x < NSLOT) {
    double* ps = slotR + (size_t)threadIdx.x * 4;
    a1 = ps[1]; a2 = ps[2]; a3 = ps[3];
    ps[0] = ps[1] = ps[2] = ps[3] = 0.0;   // consume
  }
  a1 = block_sum(a1, red); a2 = block_sum(a2, red); a3 = block_sum(a3, red);
  if (threadIdx.x == 0) {
    if (slots) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      a0 = 0.0; gt = 0.0;
      for (int q = 0; q < gx; ++q) { a0 += __builtin_nontemporal_load(&slots[2 * q]); gt += __builtin_nontemporal_load(&slots[2 * q + 1]); }
    } else {
      a0 = atomicAdd(&fin[0], 0.0);   // device-scope reads of the other workgroups' sums
      gt = atomicAdd(&fin[1], 0.0);
    }
    fin[0] = 0.0; fin[1] = 0.0; fin[2] = 0.0;
    if (do_nu && g.mut) {
      sc[SC_G_NU_STALE] = sc[SC_G_NU];           // what the last cache refresh held (model.py:684)
      sc[SC_NU_SHP] = sc[SC_A_ETA] + a0;
      sc[SC_G_NU] = exp(digamma_pos(sc[SC_NU_SHP]) - log(sc[SC_NU_RTE]));
      sc[SC_E_NU] = sc[SC_NU_SHP] / sc[SC_NU_RTE];
    }
    if (do_elbo) {
      double e = a1 + a2 - sc[SC_E_NU] * a3 + gt;
      e += gamma_elbo_term(sc[SC_A_ETA], sc[SC_B_ETA], sc[SC_NU_SHP], sc[SC_NU_RTE]);
      elbo_out[0] = e;
    }
    // raw pieces for fits whose layers are spread over several handles (vmr_sweep_local)
    if (!skip_nu) elbo_out[1] = a0;   // sum x w2 rho over the local layers (nu_shp - alpha_eta)
    elbo_out[2] = a1 + a2 + gt;   // local ELBO terms that do not involve nu
    elbo_out[3] = a3;             // local sum_t (sum_k rho) Q_t, enters the ELBO as -E[nu] * (.)
  }
}
__global__ __launch_bounds__(TPB) void k_fin_rho(double* par, double* Hg, const double* Cg, double* slotR, double* elbo_out,
                                                 double* fin, int do_nu, int do_elbo, int fold, int skip_nu, Geo g, double* slots) {
  fin_rho_body(par, Hg, Cg, slotR, elbo_out, fin, do_nu, do_elbo, fold, skip_nu, g, (int)blockIdx.x, (int)gridDim.x, slots);
}
// (lockstep launch: the ELBO of a sweep whose pass finished nu itself)
__global__ __launch_bounds__(TPB) void k_fin_rho_b(const FinUnit* __restrict__ units, const int* __restrict__ blk_unit) {
  const FinUnit& u = units[blk_unit[blockIdx.x]];
  fin_rho_body(u.par, u.Hg, u.Cg, u.slotR, u.elbo, u.elbo + 4, 0, 1, 0, 1, u.g, (int)blockIdx.x - u.fr_blk0, u.fr_nblk);
}

// commit a nu_shp that was summed over several handles (layer-sharded fits)
__global__ void k_commit_nu(double* par, double nu_partial_total, const double* total_dev, Geo g) {
  const ParOff o = par_off(g.L, g.Mp, g.K);
  double* sc = par + o.sc;
  if (total_dev) nu_partial_total = total_dev[0];   // (summed over the owners on the device: no host hop)
  if (threadIdx.x == 0 && blockIdx.x == 0 && g.mut) {
    sc[SC_G_NU_STALE] = sc[SC_G_NU];
    sc[SC_NU_SHP] = sc[SC_A_ETA] + nu_partial_total;
    sc[SC_G_NU] = exp(digamma_pos(sc[SC_NU_SHP]) - log(sc[SC_NU_RTE]));
    sc[SC_E_NU] = sc[SC_NU_SHP] / sc[SC_NU_RTE];
  }
}

// posterior read-out per tie (model.py:1099-1188, utils.py:200-217): argmax_k rho, sum_k k rho_k, rho_1 >= threshold
__global__ __launch_bounds__(256) void k_readout(const double* __restrict__ rho, void* __restrict__ out, size_t ties, int K,
                                                 int method, double threshold, const unsigned* __restrict__ perm, size_t T, size_t NS) {
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < ties; q += (size_t)gridDim.x * blockDim.x) {
    const double* r = rho + q * K;
    size_t t = q;
    if (perm) { const size_t l = q / T, pos = q - l * T; t = l * T + perm[l * NS * 64 + pos]; }   // rho by sorted position, answers by tie
    if (method == VMR_READ_RHO_MAX) {
      int best = 0;
      double bv = r[0];
      for (int k = 1; k < K; ++k) if (r[k] > bv) { bv = r[k]; best = k; }   // first maximum, as np.argmax
      reinterpret_cast<uint8_t*>(out)[t] = (uint8_t)best;
    } else if (method == VMR_READ_RHO_MEAN) {
      double m = 0.0;
      for (int k = 1; k < K; ++k) m += (double)k * r[k];
      reinterpret_cast<double*>(out)[t] = m;
    } else {
      reinterpret_cast<uint8_t*>(out)[t] = r[1] >= threshold ? 1 : 0;
    }
  }
}


// ------------------------------------------------------------------------------------------
// Posterior samples of Y on the device: `sample_inferred_model` (model.py:1062-1096) draws, per tie, n_trials categorical
// trials from rho and keeps the most frequent category (first maximum): Generator.multinomial(n, rho).argmax(-1).  Here the
// uniforms come from Philox4x32-10 with key = seed and counter = (tie index in [L,N,N] order, trial pair), so a draw depends on
// (seed, tie, trial) only -- reproducible, and the same for every data layout -- not on NumPy's PCG64 stream, which a GPU cannot
// follow (the host class keeps that exact mode; this one is checked by distribution).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sample(const double* __restrict__ rho, uint8_t* __restrict__ out, size_t ties, int K, int n_trials,
                                                unsigned long long seed, const unsigned* __restrict__ perm, size_t T, size_t NS) {
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < ties; q += (size_t)gridDim.x * blockDim.x) {
    const double* r = rho + q * K;
    size_t t = q;
    if (perm) { const size_t l = q / T, pos = q - l * T; t = l * T + perm[l * NS * 64 + pos]; }
    const int best = draw_tie<false>(r, K, n_trials, seed, t, nullptr);   // (sample_draw.h)
    out[t] = (uint8_t)best;
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------

// Launch shape of one sweep over the sorted lists: the handle's block size and table levels, shrunk until the workgroup fits in LDS
SlShape sl_shape(const vmr_ctx* h, bool update, bool elbo, bool hist) {
  const Geo& g = h->g;
  SlShape s{std::max(64, std::min((update || elbo) ? h->sp_tpb : h->st_tpb, sl_tpb_max(g.K, elbo, h->all_full != 0, update)) & ~63), update ? g.yt : 0, hist ? g.hc : 0, 0};
  auto bytes = [&]() { return sl_smem(g, s.yt, s.hc, update, elbo, hist); };
  while (bytes() > SP_LDS_MAX && (s.yt > 0 || s.hc > 0)) { if (s.yt >= s.hc && s.yt > 0) --s.yt; else --s.hc; }
  s.smem = bytes();
  return s;
}
SlArgs sl_args(const vmr_ctx* h, const SlShape& sh, int do_hist, int sum_a) {
  return SlArgs{h->E, h->rs, h->ebase, h->perm, h->sy, h->cls_p, h->Qt_p, h->Rb, h->rq, h->Rm, h->rbase, h->rm2, h->rho, h->logpr, h->par, h->slotR,
                h->lutg, h->Hg, h->slotF, h->slotA, 1, do_hist, sh.yt, sh.hc, sum_a, nullptr, nullptr, 0, 0, nullptr, h->lp0 ? 1 : 0, h->g.farl, (do_hist == 1 && h->g.two_pass && sh.hc >= 1) ? h->h0s : nullptr, (do_hist == 1 && h->g.two_pass && sh.hc >= 1 && h->h0s) ? h->x0p : nullptr,
                (h->h0s && h->g.two_pass && !h->opt.no_lv0r) ? 1 : 0, h->E + h->n_slots, 0, h->lpd, h->lpb};   // (level 0 must be among the LDS levels: its deficits go there)
}
int sl_launch(vmr_ctx* h, int mode, const SlShape& sh, SlArgs& a) {
  sl_launch_fn fn = vmr_sl_launcher(h->g.K);
  if (!fn) return fail(h, VMR_EINVAL, "this build of libvimure_hip.so holds no sweep kernel for this K");
  return fn(h, mode, sh, a);
}

// The statistics of the far reports: H[y][m][k] += x rho_k (k >= 1; the deficits of ties whose rho does not sum to 1 in slot 0)
// for the reports of levels y >= hc, which the pass left out -- the next LF levels in LDS (float atomics, as the pass' own), any
// beyond those as global adds -- and their share of nu_shp - alpha = sum x rho_k w2_k (model.py:820-830).  The grid's last
// workgroup finishes nu exactly as the pass' does where it keeps every level (sweep_sl.hip).  rho is gathered by position: a few
// per cent of the reports.  count: the constants' pass of vmr_create (every tie "is" category 1).
template <int K>
__global__ __launch_bounds__(1024) void k_far_hist(const unsigned* __restrict__ far_pos, const unsigned* __restrict__ far_ent,
                                                   const unsigned long long* __restrict__ fbase, const double* __restrict__ rho, double* Hg, double* par,
                                                   double* nu_acc, double* elbo_dev, int count, int commit_nu, int Gl, int LF, Geo g) {
  extern __shared__ double Hf[];   // [K][LF][Mp], 16 doubles for the block sums
  const int Mp = g.Mp, tid = threadIdx.x, nthr = (int)blockDim.x;
  const int l = (int)blockIdx.x / Gl, gb = (int)blockIdx.x - l * Gl;
  const unsigned lfm = (unsigned)LF * (unsigned)Mp, hcm = (unsigned)g.hc * (unsigned)Mp;
  double* red = Hf + (size_t)K * lfm;
  for (unsigned q = tid; q < (unsigned)K * lfm; q += nthr) Hf[q] = 0.0;
  __syncthreads();
  const ParOff o = par_off(g.L, Mp, g.K);
  const size_t T = (size_t)g.N * g.N;
  double Gla[K];
#pragma unroll
  for (int k = 0; k < K; ++k) Gla[k] = par[o.G_la + l * K + k];
  const double gnu = par[o.sc + SC_G_NU];
  const double* gth = par + o.G_th + (size_t)l * Mp;
  const double* rl = rho + (size_t)l * T * K;
  double* Hl = Hg + ((size_t)l * NH + (gb % NH)) * g.Y * Mp * K;
  double share = 0.0;
  const unsigned long long i1 = fbase[l + 1];
  constexpr int FB = 4;   // reports in flight per thread (the gathers of rho are what this kernel waits for)
  for (unsigned long long i0 = fbase[l] + (unsigned long long)gb * nthr * FB + tid; i0 < i1; i0 += (unsigned long long)Gl * nthr * FB) {
    unsigned pos[FB], ent[FB];
    double r[FB][K];
#pragma unroll
    for (int u = 0; u < FB; ++u) {
      const unsigned long long i = i0 + (unsigned long long)u * nthr;
      const bool on = i < i1;
      pos[u] = on ? far_pos[i] : 0u;
      ent[u] = on ? far_ent[i] : 0u;
    }
#pragma unroll
    for (int u = 0; u < FB; ++u) {
#pragma unroll
      for (int k = 0; k < K; ++k) r[u][k] = count ? (k == 1 ? 1.0 : 0.0) : (ent[u] ? rl[(size_t)pos[u] * K + k] : 0.0);
    }
#pragma unroll
    for (int u = 0; u < FB; ++u) {
      if (ent[u] == 0u) continue;
      const unsigned ym = SL_YM(ent[u]), rel = ym - hcm;
      const double dx = (double)SL_X(ent[u]);
      double sm = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) sm += r[u][k];
      double dfc = 1.0 - sm;
      if (fabs(dfc) <= 1e-14) dfc = 0.0;   // (as the pass decides it)
      if (rel < lfm) {
#pragma unroll
        for (int k = 1; k < K; ++k) atomicAdd(&Hf[(unsigned)k * lfm + rel], dx * r[u][k]);
        if (dfc != 0.0) atomicAdd(&Hf[rel], dx * dfc);
      } else {
        double* d = Hl + (size_t)ym * K;
#pragma unroll
        for (int k = 1; k < K; ++k) atomicAdd(&d[k], dx * r[u][k]);
        if (dfc != 0.0) atomicAdd(&d[0], dx * dfc);
      }
      if (nu_acc) {
        const unsigned y = ym / (unsigned)Mp, m = ym - y * (unsigned)Mp;
        const double z2 = gnu * (double)y, gt = gth[m];
        const double w0 = w2_of(gt * Gla[0], z2);
        share -= w0 * dx * dfc;
#pragma unroll
        for (int k = 1; k < K; ++k) share += (w2_of(gt * Gla[k], z2) - w0) * dx * r[u][k];
      }
    }
  }
  __syncthreads();
  for (unsigned q = tid; q < (unsigned)K * lfm; q += nthr) {
    const double v = Hf[q];
    if (v != 0.0) { const unsigned k = q / lfm, rel = q - k * lfm; atomicAdd(&Hl[(size_t)(hcm + rel) * K + k], v); }
  }
  if (!nu_acc) return;
  share = block_sum_n(share, red);
  __shared__ int last;
  if (tid == 0) {
    atomicAdd(&nu_acc[0], share);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (this workgroup's share is performed at the memory side before the ticket is drawn)
    const double t = atomicAdd(&nu_acc[1], 1.0);
    last = (t == (double)(gridDim.x - 1u));
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      double tot = atomicAdd(&nu_acc[0], 0.0);   // the pass' workgroups' shares and this kernel's (device-scope read)
      for (int ll = 0; ll < g.L; ++ll) tot += nu_acc[2 + ll];
      nu_acc[0] = 0.0; nu_acc[1] = 0.0;
      elbo_dev[1] = tot;   // the raw piece, for fits whose layers are spread over several handles (vmr_sweep_local)
      if (commit_nu) {
        double* sc = par + o.sc;
        sc[SC_G_NU_STALE] = sc[SC_G_NU];           // what the last cache refresh held (model.py:684)
        sc[SC_NU_SHP] = sc[SC_A_ETA] + tot;
        sc[SC_G_NU] = exp(digamma_pos(sc[SC_NU_SHP]) - log(sc[SC_NU_RTE]));
        sc[SC_E_NU] = sc[SC_NU_SHP] / sc[SC_NU_RTE];
      }
    }
  }
}
// SlArgs::h0s: the level-0 statistics of the rounds that took them as per-tie products, put into copy 0 of H with the marginals the
// finalize kernels read -- sum_m H[0][m][k] = S_k (the pass' sums), sum_k H[0][m][k] = R_m = C[0][m] - deficits (rebuilt from the
// constant as for every level, h_fold_item; the deficits: slot 0 of the copies the pass added into): H[0][m][k] += R_m S_k / sum_m R_m
// for k >= 1.  In proportion to R_m, not to the constant: a reporter whose reports all sit on all-zero rows (R_m = 0) gets exactly
// the zeros it has, so that the finalize may find its new G_theta to be 0 and drop its row (w1_of) without the other rows' column
// sums being off by what the spread had put there.  One workgroup per layer; consumes h0s.
__global__ __launch_bounds__(256) void k_level0_spread(double* Hg, const double* __restrict__ Cg, double* h0s, Geo g) {
  __shared__ double Sk[KMAX];
  __shared__ double red[16];
  __shared__ double tot;
  const int l = blockIdx.x, K = g.K, Mp = g.Mp;
  const size_t hcs = (size_t)g.Y * Mp * K;
  double* H0 = Hg + (size_t)l * NH * hcs;
  const double* C0 = Cg + (size_t)l * g.Y * Mp;
  auto marginal = [&](int m) {
    double d = 0.0;
#pragma unroll
    for (int c = 0; c < NH; ++c) d += H0[(size_t)c * hcs + (size_t)m * K];
    return C0[m] - d;
  };
  double s = 0.0;
  for (int m = threadIdx.x; m < g.M; m += 256) s += marginal(m);
  s = block_sum_n(s, red);
  if (threadIdx.x == 0) tot = s;
  __syncthreads();
  if ((int)threadIdx.x < K) {
    double sk = 0.0;
    for (int sl = 0; sl < NSLOT; ++sl) { sk += h0s[((size_t)l * NSLOT + sl) * K + threadIdx.x]; h0s[((size_t)l * NSLOT + sl) * K + threadIdx.x] = 0.0; }
    Sk[threadIdx.x] = tot > 0.0 ? sk / tot : 0.0;
  }
  __syncthreads();
  for (int q = threadIdx.x; q < g.M * (K - 1); q += 256) {   // (writes slots k >= 1 of copy 0 only: the marginals read slot 0)
    const int m = q / (K - 1), k = 1 + (q - m * (K - 1));
    const double c = marginal(m);
    if (c != 0.0 && Sk[k] != 0.0) H0[(size_t)m * K + k] += c * Sk[k];
  }
}
// the count-mode launch of vmr_create is done: its result becomes the constants (create.h)
int take_counts(vmr_ctx* h) {
  const Geo& g = h->g;
  const size_t nit = (size_t)g.L * g.Y * g.Mp;
  hipLaunchKernelGGL(k_take_counts, dim3((unsigned)std::min<size_t>(1024, (nit + TPB - 1) / TPB)), dim3(TPB), 0, h->stream, h->Hg, h->Cg, g);
  CK(hipGetLastError());
  return VMR_OK;
}

// nu: -1 = no nu sum in this sweep; 0 = the raw sum to elbo_dev[1]; 1 = nu committed too (as launch_hist's)
int launch_far(vmr_ctx* h, int count, int nu) {
  const Geo& g = h->g;
  if (!g.farl || h->far_off.empty() || h->far_off.back() == 0ull) {
    if (nu >= 0 && g.farl) return fail(h, VMR_ESTATE, "far lists missing");   // (cannot happen: farl is only chosen with far reports)
    return VMR_OK;
  }
  const size_t lb = (size_t)g.Mp * g.K * 8;
  const int LF = (int)std::max<size_t>(1, std::min<size_t>((size_t)(g.Y - g.hc), ((size_t)150 * 1024 - 256) / lb));
  const size_t sm = (size_t)LF * lb + 16 * 8;
  unsigned long long most = 0;
  for (int l = 0; l < g.L; ++l) most = std::max(most, h->far_off[l + 1] - h->far_off[l]);
  const int Gl = (int)std::max<unsigned long long>(1, std::min<unsigned long long>((most + 4095) / 4096, std::max(1, h->ncu / g.L)));
  double* nu_acc = (nu >= 0 && g.mut) ? h->nu_acc : nullptr;
  Prof p(h, VMR_KERNEL_GAMMA_COUNTS);
  DISPATCH_K(g.K, if (sm > 48 * 1024) HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(k_far_hist<KK>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm));
             hipLaunchKernelGGL((k_far_hist<KK>), dim3(g.L * Gl), dim3(1024), sm, h->stream, h->far_pos, h->far_ent, h->far_base, h->rho, h->Hg, h->par,
                                nu_acc, h->elbo_dev, count, nu > 0 ? 1 : 0, Gl, LF, g));
  HIPCHK(h, hipGetLastError());
  return VMR_OK;
}

// k_fin_rho: nu and/or the ELBO; folds the NH copies of H into copy 0 on its way when they are not folded yet
static int launch_fin_rho(vmr_ctx* h, int do_nu, int do_elbo, int skip_nu = 0) {
  const Geo& g = h->g;
  const int fold = (!skip_nu && h->h_valid && !h->h_reduced && !g.gen) ? 1 : 0;
  {
    Prof p(h, VMR_KERNEL_FINALIZE);
    hipLaunchKernelGGL(k_fin_rho, dim3(g.L * FR_G), dim3(TPB), 0, h->stream, h->par, h->Hg, h->Cg, h->slotR, h->elbo_dev,
                       h->elbo_dev + 4, do_nu, do_elbo, fold, skip_nu, g, g.det ? h->fr_slots : nullptr);
  }
  HIPCHK(h, hipGetLastError());
  if (fold) h->h_reduced = true;
  return VMR_OK;
}
// before k_fin_gamma / k_fin_phi read H outside the fused sweep
static int ensure_h_folded(vmr_ctx* h) {
  if (h->h_reduced) return VMR_OK;
  const Geo& g = h->g;
  const size_t n = (size_t)g.L * g.Y * g.Mp * g.K;
  hipLaunchKernelGGL(k_h_reduce, dim3((unsigned)std::min<size_t>(1024, (n + TPB - 1) / TPB)), dim3(TPB), 0, h->stream, h->Hg, h->Cg, g);
  HIPCHK(h, hipGetLastError());
  h->h_reduced = true;
  return VMR_OK;
}

// The pass about to be launched adds the mask-list sums of its rho into slotA: whatever an earlier pass left there unconsumed goes
static int begin_sum_a(vmr_ctx* h, hipStream_t st) {
  const Geo& g = h->g;
  if (!h->a_zero) HIPCHK(h, hipMemsetAsync(h->slotA, 0, (size_t)g.L * NSLOT * g.W * 64 * g.K * 8, st));
  h->a_zero = false;
  return VMR_OK;
}
// H of the current rho (start of a fit / after vmr_set_state; the rho pass keeps it current afterwards)
// Deterministic mode: the integer shadows a pass left (SlArgs::det) become the doubles the finalize kernels read -- copy 0 of H,
// slot 0 of the mask sums, of the all-ones sums and of the ELBO partials (the other copies / slots stay zero) -- and are zeroed.
__global__ __launch_bounds__(256) void k_det_fold(unsigned long long* __restrict__ d, double* __restrict__ Hg, double* __restrict__ slotA,
                                                 double* __restrict__ slotF, double* __restrict__ slotR, Geo g) {
  const size_t nH = (size_t)g.Y * g.Mp * g.K, nA = (size_t)g.W * 64 * g.K, L = (size_t)g.L, K = (size_t)g.K;
  const size_t tot = L * nH + L * nA + L * K + 4;
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < tot; q += (size_t)gridDim.x * 256) {
    const unsigned long long u = d[q];
    if (u == 0ull) continue;
    d[q] = 0ull;
    if (q < L * nH) { const size_t l = q / nH, i = q - l * nH; Hg[l * NH * nH + i] += det_back(u, g.det_sh); }
    else if (q < L * nH + L * nA) { const size_t r = q - L * nH, l = r / nA, i = r - l * nA; slotA[l * NSLOT * nA + i] += det_back(u, g.det_sha); }
    else if (q < L * nH + L * nA + L * K) { const size_t r = q - L * nH - L * nA, l = r / K, k = r - l * K; slotF[l * NSLOT * K + k] += det_back(u, g.det_sha); }
    else { const size_t r = q - L * nH - L * nA - L * K; slotR[r] += det_back(u, g.det_shr); }
  }
}
static int det_fold(vmr_ctx* h) {
  const Geo& g = h->g;
  if (!g.det) return VMR_OK;
  const size_t tot = (size_t)g.L * g.Y * g.Mp * g.K + (size_t)g.L * g.W * 64 * g.K + (size_t)g.L * g.K + 4;
  hipLaunchKernelGGL(k_det_fold, dim3((unsigned)std::min<size_t>(1024, (tot + 255) / 256)), dim3(256), 0, h->stream, h->det_buf, h->Hg, h->slotA, h->slotF,
                     h->slotR, g);
  HIPCHK(h, hipGetLastError());
  return VMR_OK;
}

// The last sweep used its new rho without writing it (launch_rho, store = false): write it now -- the same update once more, from the
// same log prior, theta, lambda and the nu of before that sweep's commit (SC_G_NU_STALE); no statistics, no sums, nothing else
// changes.  Called by everything that reads rho; vmr_step and the fit loops leave no stale rho behind, so this only runs after a
// loop that failed half way.
static int ensure_rho(vmr_ctx* h) {
  if (!h->rho_stale) return VMR_OK;
  const SlShape shs = sl_shape(h, true, false, false);
  SlArgs as = sl_args(h, shs, 0, 0);
  as.slotF = nullptr; as.slotA = nullptr;
  as.nu_stale = h->g.mut ? 1 : 0;
  int rc = sl_launch(h, 0, shs, as);
  if (rc) return rc;
  HIPCHK(h, hipGetLastError());
  h->rho_stale = false;
  return VMR_OK;
}

int ensure_rho_ext(vmr_ctx* h) { return ensure_rho(h); }

// nu: -1 = the pass leaves nu alone; 0 = it leaves the raw sum in elbo_dev[1]; 1 = it also commits nu (sorted lists, see SlArgs::nu_acc)
static int launch_hist(vmr_ctx* h, int nu = -1) {
  const Geo& g = h->g;
  if (g.gen) return gen_hist(h);
  { int rce = ensure_rho(h); if (rce) return rce; }
  HIPCHK(h, hipMemsetAsync(h->Hg, 0, (size_t)g.L * NH * g.Y * g.Mp * g.K * 8, h->stream));
  if (h->sparse) {
    HIPCHK(h, hipMemsetAsync(h->slotF, 0, (size_t)g.L * NSLOT * g.K * 8, h->stream));   // (the pass sums rho over all-ones mask rows)
    h->f_valid = g.fuse_full != 0;
    if (g.ml) { int rc = begin_sum_a(h, h->stream); if (rc) return rc; h->a_valid = true; }
    Prof p(h, VMR_KERNEL_GAMMA_COUNTS);
    const SlShape shs = sl_shape(h, false, false, true);
    SlArgs as = sl_args(h, shs, 1, g.ml);
    if (nu >= 0 && g.mut) { as.nu_acc = h->nu_acc; as.elbo_dev = h->elbo_dev; as.commit_nu = nu; }
    as.det = g.det ? h->det_buf : nullptr;
    int rcs = sl_launch(h, 3, shs, as);
    if (rcs) return rcs;
    HIPCHK(h, hipGetLastError());
    if (g.farl && (rcs = launch_far(h, 0, (nu >= 0 && g.mut) ? nu : -1))) return rcs;
    if (as.h0s) {
      hipLaunchKernelGGL(k_level0_spread, dim3(g.L), dim3(256), 0, h->stream, h->Hg, h->Cg, h->h0s, g);
      HIPCHK(h, hipGetLastError());
    }
    if ((rcs = det_fold(h))) return rcs;
  } else {
    Prof p(h, VMR_KERNEL_GAMMA_COUNTS);
    int rc = tiles_hist(h);
    if (rc) return rc;
  }
  HIPCHK(h, hipGetLastError());
  h->h_valid = true;
  h->h_zero = false;
  h->h_reduced = false;
  return VMR_OK;
}

static int launch_gamma(vmr_ctx* h, bool with_phi) {
  const Geo& g = h->g;
  h->prte_valid = !with_phi;   // (a gamma finalize on its own leaves phi's rate pending; in a sweep the rho pass follows)
  if (g.gen) return gen_gamma(h, with_phi);
  if (h->sparse && !h->h_valid) {   // report lists: the statistics pass also sums rho over the all-ones mask rows (slotF)
    int rc = launch_hist(h);
    if (rc) return rc;
  }
  // fork: the mask sums A = sum_ij R rho (memory-bound) run beside the statistics pass when one is needed
  hipStream_t ms = h->h_valid ? h->stream : h->stream2;
  if (ms != h->stream) {
    HIPCHK(h, hipEventRecord(h->ev_fork, h->stream));
    HIPCHK(h, hipStreamWaitEvent(ms, h->ev_fork, 0));
  }
  // mask rows that are all ones were already summed by the last rho pass (slotF); the mask kernel then only
  // handles partial rows, and is not needed at all when R has none
  const int skip_full = (g.fuse_full && h->f_valid) ? 1 : 0;
  if (skip_full && h->n_partial > 0 && h->rq && h->a_valid) {
    // the last rho / statistics pass summed the lists on its way (SpArgs::sum_a): nothing to launch
  } else if (skip_full && h->n_partial > 0 && h->rq) {   // partial rows only, and they are short lists
    { int rc = begin_sum_a(h, ms); if (rc) return rc; }
    Prof p(h, VMR_KERNEL_GAMMA_MASK, ms);
    const size_t T_ = (size_t)g.N * g.N;
    int gl = (int)std::min<size_t>(std::max<size_t>(1, (size_t)h->ncu / g.L), (T_ + 4 * TPB - 1) / (4 * TPB));
    const size_t lsm = (size_t)g.Mp * g.K * 8;
    if (lsm > 48 * 1024 && !h->ml_attr) {
      DISPATCH_K(g.K, HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(k_mask_lists<KK>),
                                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lsm)));
      h->ml_attr = true;
    }
    DISPATCH_K(g.K, hipLaunchKernelGGL((k_mask_lists<KK>), dim3(g.L * gl), dim3(TPB), lsm, ms, h->rq, h->Rm, h->rbase,
                                       h->rcls, h->rho, h->slotA, gl, h->perm, g));
  } else if (!skip_full || h->n_partial > 0) {
    Prof p(h, VMR_KERNEL_GAMMA_MASK, ms);
    dim3 grid(g.L * g.Gm), blk(TPB);
    // (deterministic handles are on report lists: their statistics are valid here, so ms is the handle's stream and det_fold follows in order)
    unsigned long long* detA = g.det ? h->det_buf + (size_t)g.L * g.Y * g.Mp * g.K : nullptr;
#define GMASK(NC_)                                                                                                                              \
  do {                                                                                                                                          \
    if (g.det) { DISPATCH_K(g.K, hipLaunchKernelGGL((k_gamma_mask<KK, NC_, true>), grid, blk, 0, ms, h->Rb, h->rho, h->rcls, h->slotA, skip_full, h->perm, g, detA)); } \
    else { DISPATCH_K(g.K, hipLaunchKernelGGL((k_gamma_mask<KK, NC_, false>), grid, blk, 0, ms, h->Rb, h->rho, h->rcls, h->slotA, skip_full, h->perm, g, detA)); }    \
  } while (0)
    switch (g.W >= 4 ? 4 : g.W) {
      case 1: GMASK(1); break;
      case 2: GMASK(2); break;
      case 3: GMASK(3); break;
      default: GMASK(4); break;
    }
#undef GMASK
    if (g.det) {
      if (ms != h->stream) return fail(h, VMR_ESTATE, "deterministic mask sums beside a statistics pass");
      HIPCHK(h, hipGetLastError());
      int rcd = det_fold(h);
      if (rcd) return rcd;
    }
  }
  if (ms != h->stream) {
    HIPCHK(h, hipEventRecord(h->ev_join, ms));
    int rc = launch_hist(h);
    if (rc) return rc;
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_join, 0));   // join
  } else if (!h->h_valid) {
    int rc = launch_hist(h);
    if (rc) return rc;
  }
  {
    Prof p(h, VMR_KERNEL_FINALIZE);
    // fused sweep: this is the last reader of H and slotF before the rho pass rebuilds them, so it leaves them zeroed.  It
    // sums the NH copies the workgroups of the pass added into on its way (nh = 1 when something folded them already).
    const int consume = (with_phi && !g.two_pass) ? 1 : 0;
    const int nh = h->h_reduced ? 1 : NH;
    const size_t fsm = (size_t)2 * ((g.M + FG_G - 1) / FG_G) * 8;
    hipLaunchKernelGGL(g.det ? k_fin_gamma_det : k_fin_gamma, dim3(g.L * FG_G), dim3(FIN_TPB), fsm, h->stream, h->par, h->Hg, h->sparse ? h->Cg : nullptr,
                       (h->sparse && skip_full && h->n_partial == 0) ? nullptr : h->slotA,   // (lists, every mask row all ones: the pass summed them into slotF)
                       h->slotF, h->lutg, nullptr, h->fin_g, h->sparse ? h->nu_acc : nullptr, nh,
                       with_phi ? 1 : 0, consume, g);
    h->a_valid = false; h->a_zero = true;   // (k_fin_gamma zeroes the slots of A as it reads them)
    if (consume) { h->h_valid = false; h->f_valid = false; h->h_zero = true; }
  }
  HIPCHK(h, hipGetLastError());
  return VMR_OK;
}

static int launch_phi(vmr_ctx* h) {
  const Geo& g = h->g;
  if (g.gen) return gen_phi(h);
  if (!g.mut) return VMR_OK;   // committed by k_fin_gamma
  if (!h->h_valid) { int rc = launch_hist(h); if (rc) return rc; }
  { int rc = ensure_h_folded(h); if (rc) return rc; }
  {
    Prof p(h, VMR_KERNEL_FINALIZE);
    hipLaunchKernelGGL(k_fin_phi, dim3(g.L), dim3(TPB), 0, h->stream, h->par, h->Hg, g);
  }
  HIPCHK(h, hipGetLastError());
  return VMR_OK;
}

// mode: 0 = rho update (+nu), 1 = rho update + fused ELBO, 2 = ELBO only
// raw_nu: leave the raw nu sum in elbo_dev[1] although nu is not committed (vmr_sweep_local)
// store = false (mode 0 on report lists in one pass only): the pass uses its new rho without writing it (vmr_ctx::rho_stale)
static int launch_rho(vmr_ctx* h, int mode, bool commit_nu, bool raw_nu = false, bool store = true) {
  const Geo& g = h->g;
  if (mode != 2) h->prte_valid = false;   // a new rho: the pending rate of phi is another rho's
  if (g.gen) return gen_rho(h, mode, commit_nu, raw_nu, [](vmr_ctx* hh, int do_nu, int do_elbo, int skip_nu) { return launch_fin_rho(hh, do_nu, do_elbo, skip_nu); });
  if (h->sparse && g.farl && h->elbo_split && mode == 1) {
    // An ELBO sweep of a handle whose fused variant would drop an LDS level: the plain update pass (with the far reports' kernel and
    // nu), then the ELBO-only pass on the new rho with the G_nu of before the commit -- what the fused pass evaluates (model.py:970).
    int rc2 = launch_rho(h, 0, commit_nu, raw_nu, true);
    if (rc2) return rc2;
    const SlShape she = sl_shape(h, false, true, false);
    SlArgs ae = sl_args(h, she, 0, 0);
    ae.elbo_cur = commit_nu ? 0 : 1;
    {
      Prof p(h, VMR_KERNEL_ELBO);
      if ((rc2 = sl_launch(h, 2, she, ae))) return rc2;
    }
    HIPCHK(h, hipGetLastError());
    return launch_fin_rho(h, 0, 1, 1);
  }
  size_t sm = shmem_rho(g, mode != 2, mode != 0);
  int rc = VMR_OK;
  if (mode != 2 && !h->h_zero) {   // (after a fused k_fin_gamma both are zero already)
    if (g.fuse_full) HIPCHK(h, hipMemsetAsync(h->slotF, 0, (size_t)g.L * NSLOT * g.K * 8, h->stream));
    if (!g.two_pass) HIPCHK(h, hipMemsetAsync(h->Hg, 0, (size_t)g.L * NH * g.Y * g.Mp * g.K * 8, h->stream));   // rebuilt from the new rho
  }
  if (mode != 2) h->h_zero = false;
  // sorted lists with mutuality: the pass that builds H finishes nu itself -- no finalize launch on plain sweeps
  const bool nu_in_pass = h->sparse && g.mut && mode != 2 && (commit_nu || raw_nu);
  if (mode == 2 && (rc = ensure_rho(h))) return rc;
  if (h->sparse) {
    const int do_hist = (mode != 2 && !g.two_pass) ? 1 : 0;
    const int sum_a = (g.ml && do_hist) ? 1 : 0;   // (two passes: the statistics pass that follows sums the lists)
    if (mode != 2) h->a_valid = false;
    if (sum_a) { if ((rc = begin_sum_a(h, h->stream))) return rc; h->a_valid = true; }
    const SlShape shs = sl_shape(h, mode != 2, mode != 0, do_hist != 0);
    SlArgs as = sl_args(h, shs, do_hist, sum_a);
    if (nu_in_pass && do_hist) { as.nu_acc = h->nu_acc; as.elbo_dev = h->elbo_dev; as.commit_nu = commit_nu ? 1 : 0; }
    as.det = g.det ? h->det_buf : nullptr;
    // the rho of a sweep that the next one overwrites unread is not written: only with mutuality's nu committed inside the pass
    // (the re-write of ensure_rho takes the nu before that commit from SC_G_NU_STALE) or without mutuality, in one pass per sweep
    // -- and only where the pass itself sums rho over the mask rows: the mask kernels of launch_gamma read rho from memory
    const bool lazy = !store && mode == 0 && do_hist && (nu_in_pass ? commit_nu : !g.mut) && g.fuse_full && (h->n_partial == 0 || g.ml) &&
                      !g.farl && !h->opt.always_store_rho;   // (k_far_hist reads rho)
    {
      Prof p(h, lazy ? VMR_KERNEL_RHO_NOSTORE : mode == 2 ? VMR_KERNEL_ELBO : mode == 1 ? VMR_KERNEL_RHO_ELBO : VMR_KERNEL_RHO);
      if ((rc = sl_launch(h, lazy ? 4 : mode, shs, as))) return rc;
    }
    if (mode != 2) h->rho_stale = lazy;
    if (g.farl && do_hist && (rc = launch_far(h, 0, nu_in_pass ? (commit_nu ? 1 : 0) : -1))) return rc;
    if ((rc = det_fold(h))) return rc;
  } else {
    Prof p(h, mode == 2 ? VMR_KERNEL_ELBO : mode == 1 ? VMR_KERNEL_RHO_ELBO : VMR_KERNEL_RHO);
    if ((rc = tiles_rho(h, mode, sm))) return rc;
  }
  if (mode != 2) {
    h->f_valid = g.fuse_full != 0;
    h->h_valid = !g.two_pass;
    if (!g.two_pass) h->h_reduced = false;
    if (g.two_pass && (rc = launch_hist(h, nu_in_pass ? (commit_nu ? 1 : 0) : -1))) return rc;   // wide reporter dimension: second pass rebuilds H
  }
  HIPCHK(h, hipGetLastError());
  if (nu_in_pass || (h->sparse && mode != 2 && !g.mut)) {
    // nu is done (or there is none): the finalize kernel only assembles an ELBO
    if (mode != 0 && (rc = launch_fin_rho(h, 0, 1, 1))) return rc;
  } else if (mode != 0 || commit_nu) {
    if ((rc = launch_fin_rho(h, (mode != 2 && commit_nu) ? 1 : 0, mode != 0 ? 1 : 0))) return rc;
  }
  return VMR_OK;
}

extern "C" {

const char* vmr_version(void) { return VMR_VERSION; }

const char* vmr_last_error(vmr_handle h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int vmr_data_stats(vmr_handle h, double* sum_x, uint8_t* coverage) {
  if (!h) return VMR_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  // every copy is ordered on the handle's stream: it is a non-blocking stream, which plain hipMemcpy (null stream)
  // does not wait for
  unsigned long long v = 0;
  if (sum_x) HIPCHK(h, hipMemcpyAsync(&v, h->sumx, 8, hipMemcpyDeviceToHost, h->stream));
  if (coverage) HIPCHK(h, hipMemcpyAsync(coverage, h->cov, (size_t)h->g.L * h->g.N * h->g.N, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (sum_x) *sum_x = (double)v;
  return VMR_OK;
}

// host [L,M] -> device [L,Mp]
static int upload_lm(vmr_ctx* h, size_t off, const double* src, double pad) {
  const Geo& g = h->g;
  std::vector<double> buf((size_t)g.L * g.Mp, pad);
  for (int l = 0; l < g.L; ++l) memcpy(&buf[(size_t)l * g.Mp], src + (size_t)l * g.M, (size_t)g.M * 8);
  HIPCHK(h, hipMemcpyAsync(h->par + off, buf.data(), buf.size() * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // buf is a pageable temporary: it must outlive the copy
  return VMR_OK;
}
// small host -> device copy ordered on the handle's stream (the stream is non-blocking: a null-stream hipMemcpy
// would not wait for kernels queued on it)
static int h2d(vmr_ctx* h, void* dst, const void* src, size_t n) {
  HIPCHK(h, hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, h->stream));
  return VMR_OK;
}
static int d2h(vmr_ctx* h, void* dst, const void* src, size_t n) {
  HIPCHK(h, hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, h->stream));
  return VMR_OK;
}

int vmr_set_priors(vmr_handle h, const double* alpha_theta, const double* beta_theta, const double* alpha_lambda,
                   const double* beta_lambda, double alpha_eta, double beta_eta) {
  if (!h || !alpha_theta || !beta_theta || !alpha_lambda || !beta_lambda) return fail(h, VMR_EINVAL, "NULL prior array");
  HIPCHK(h, hipSetDevice(h->device));
  const Geo& g = h->g;
  ParOff o = par_off(g.L, g.Mp, g.K);
  int rc;
  if ((rc = upload_lm(h, o.a_th, alpha_theta, 1.0))) return rc;
  if ((rc = upload_lm(h, o.b_th, beta_theta, 1.0))) return rc;
  if ((rc = h2d(h, h->par + o.a_la, alpha_lambda, (size_t)g.L * g.K * 8))) return rc;
  if ((rc = h2d(h, h->par + o.b_la, beta_lambda, (size_t)g.L * g.K * 8))) return rc;
  double ab[2] = {alpha_eta, beta_eta};
  if ((rc = h2d(h, h->par + o.sc + SC_A_ETA, ab, 16))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->have_priors = true;
  return VMR_OK;
}

static void drop_graphs(vmr_ctx* h);
int vmr_set_state(vmr_handle h, const double* gamma_shp, const double* gamma_rte, const double* phi_shp,
                  const double* phi_rte, double nu_shp, double nu_rte, const double* pr_rho, int pr_rho_on_device) {
  if (!h || !gamma_shp || !gamma_rte || !phi_shp || !phi_rte || !pr_rho) return fail(h, VMR_EINVAL, "NULL state array");
  if (!h->have_priors) return fail(h, VMR_ESTATE, "vmr_set_priors must be called before vmr_set_state");
  HIPCHK(h, hipSetDevice(h->device));
  const Geo& g = h->g;
  ParOff o = par_off(g.L, g.Mp, g.K);
  int rc;
  if ((rc = upload_lm(h, o.g_shp, gamma_shp, 1.0))) return rc;
  if ((rc = upload_lm(h, o.g_rte, gamma_rte, 1.0))) return rc;
  if ((rc = h2d(h, h->par + o.p_shp, phi_shp, (size_t)g.L * g.K * 8))) return rc;
  if ((rc = h2d(h, h->par + o.p_rte, phi_rte, (size_t)g.L * g.K * 8))) return rc;
  double nu[2] = {nu_shp, nu_rte};
  if ((rc = h2d(h, h->par + o.sc + SC_NU_SHP, nu, 16))) return rc;   // (the stream is synchronised below, before nu[] dies)
  const size_t n = (size_t)g.L * g.N * g.N * g.K;
  const double* src = pr_rho;
  if (h->perm) {   // sorted lists: rho and the log prior are stored by position
    if (!pr_rho_on_device) {
      if (!h->nat) HIPCHK(h, hipMalloc(&h->nat, n * 8));
      HIPCHK(h, hipMemcpyAsync(h->nat, pr_rho, n * 8, hipMemcpyHostToDevice, h->stream));
      src = h->nat;
    }
    const size_t T_ = (size_t)g.N * g.N;
    int* flag = reinterpret_cast<int*>(h->elbo_dev + 7);   // (the spare double of the ELBO scratch)
    HIPCHK(h, hipMemsetAsync(flag, 0, 4, h->stream));
    hipLaunchKernelGGL(k_init_rho_pos, dim3(4096), dim3(256), 0, h->stream, src, h->rho, h->logpr, h->perm, T_, (T_ + 63) / 64, g.L, g.K, g.eps,
                       h->rs, flag);
    int nf = 1;
    HIPCHK(h, hipMemcpyAsync(&nf, flag, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->lp0 = nf == 0 && !h->opt.no_lp0;
    if (g.K == 2 && !g.gen) {   // the bounds of the log prior and (unless VMR_NO_LPD) its difference (SlArgs::lpd)
      if (!h->lpb) HIPCHK(h, hipMalloc(&h->lpb, (size_t)g.L * 2 * 8));
      if (!h->lpd && !h->opt.no_lpd) {
        HIPCHK(h, hipMalloc(&h->lpd, ((size_t)g.L * T_ + 64) * 8));
        HIPCHK(h, hipMemsetAsync(h->lpd + (size_t)g.L * T_, 0, (size_t)64 * 8, h->stream));
      }
      HIPCHK(h, hipMemsetAsync(h->lpb, 0, (size_t)g.L * 2 * 8, h->stream));
      hipLaunchKernelGGL(k_lpd, dim3(1024), dim3(256), 0, h->stream, h->logpr, h->lpd, reinterpret_cast<unsigned long long*>(h->lpb), T_, g.L);
      HIPCHK(h, hipGetLastError());
    }
  } else {
    if (!pr_rho_on_device) {
      // stage through logpr (overwritten by k_init_rho element-wise after being read)
      HIPCHK(h, hipMemcpyAsync(h->logpr, pr_rho, n * 8, hipMemcpyHostToDevice, h->stream));
      src = h->logpr;
    }
    hipLaunchKernelGGL(k_init_rho, dim3(4096), dim3(256), 0, h->stream, src, h->rho, h->logpr, n, g.eps);
  }
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(k_derive_all, dim3(8), dim3(256), 0, h->stream, h->par, g);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(k_build_lut, dim3(g.L), dim3(256), 0, h->stream, h->par, h->lutg, g);
  HIPCHK(h, hipGetLastError());
  // (queued before the wait: the lockstep loop runs this handle's kernels on another handle's stream, so nothing of this call
  // may still be pending on the handle's own stream when it returns)
  HIPCHK(h, hipMemsetAsync(h->slotF, 0, (size_t)g.L * NSLOT * g.K * 8, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  drop_graphs(h);   // (a realisation's arguments may differ: SlArgs::lp0)
  h->have_state = true;
  h->restored = false;
  h->rho_stale = false;
  h->h_valid = false;
  h->f_valid = false;
  h->a_valid = false;
  h->h_zero = false; h->a_zero = false;   // (whatever an earlier, possibly failed, sweep left behind)
  h->prte_valid = false;
  if (h->h0s) HIPCHK(h, hipMemsetAsync(h->h0s, 0, (size_t)h->g.L * NSLOT * h->g.K * 8, h->stream));   // (the slots, not the constants behind them)
  if (h->gen_s1) HIPCHK(h, hipMemsetAsync(h->gen_s1, 0, (size_t)h->g.L * (h->g.Mp + h->g.K) * 8, h->stream));
  return VMR_OK;
}

int vmr_draw_pr_rho(vmr_handle h, int nblk, const int64_t* tie_cuts, const uint32_t* mt_keys, const int32_t* mt_pos,
                    double bias0, int undirected, double* out, int out_on_device) {
  if (!h) return VMR_EINVAL;
  if (!tie_cuts || !mt_keys || !mt_pos || !out) return fail(h, VMR_EINVAL, "vmr_draw_pr_rho: NULL argument");
  if (nblk <= 0) return fail(h, VMR_EINVAL, "vmr_draw_pr_rho: nblk must be positive");
  const Geo& g = h->g;
  if (g.K > KGEN_MAX) return fail(h, VMR_EINVAL, "vmr_draw_pr_rho: K must be at most 256");
  const int64_t ties = (int64_t)g.L * g.N * g.N;
  for (int b = 0; b < nblk; ++b)
    if (tie_cuts[b + 1] <= tie_cuts[b]) return fail(h, VMR_EINVAL, "vmr_draw_pr_rho: the tie cuts must be increasing");
  if (tie_cuts[0] != 0 || tie_cuts[nblk] != ties) return fail(h, VMR_EINVAL, "vmr_draw_pr_rho: the tie cuts must span [0, L*N*N]");
  for (int b = 0; b < nblk; ++b)
    if (mt_pos[b] < 0 || mt_pos[b] > 624) return fail(h, VMR_EINVAL, "vmr_draw_pr_rho: a generator position outside [0, 624]");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t cb = (size_t)(nblk + 1) * 8, kb = (size_t)nblk * 624 * 4, need = cb + kb + (size_t)nblk * 4;
  if (h->drw_cap < need) {
    if (h->drw) HIPCHK(h, hipFree(h->drw));
    h->drw = nullptr;
    h->drw_cap = 0;
    HIPCHK(h, hipMalloc(&h->drw, need));
    h->drw_cap = need;
  }
  char* base = static_cast<char*>(h->drw);
  int rc;
  if ((rc = h2d(h, base, tie_cuts, cb))) return rc;
  if ((rc = h2d(h, base + cb, mt_keys, kb))) return rc;
  if ((rc = h2d(h, base + cb + kb, mt_pos, (size_t)nblk * 4))) return rc;
  const size_t n = (size_t)ties * g.K;
  double* dst = out;
  if (!out_on_device) HIPCHK(h, hipMalloc(&dst, n * 8));   // (the host form, for tests: the handle's own buffers may hold a state)
  rc = draw_pr_rho_launch(h, nblk, reinterpret_cast<const int64_t*>(base), reinterpret_cast<const uint32_t*>(base + cb),
                          reinterpret_cast<const int32_t*>(base + cb + kb), bias0, undirected, dst);
  if (rc == VMR_OK && !out_on_device) rc = d2h(h, out, dst, n * 8);
  hipError_t e = hipStreamSynchronize(h->stream);   // (the host arrays are only read during the call)
  if (!out_on_device) (void)hipFree(dst);
  if (rc != VMR_OK) return rc;
  HIPCHK(h, e);
  return VMR_OK;
}

static int read_elbo(vmr_ctx* h, double* out) {
  HIPCHK(h, hipMemcpyAsync(out, h->elbo_dev, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (isnan(*out)) return fail(h, VMR_ENAN, "ELBO is NaN!!!!");
  return VMR_OK;
}

static int sweep(vmr_ctx* h, int mode, bool store = true) {
  int rc;
  if ((rc = launch_gamma(h, true))) return rc;   // gamma and phi are finished by one kernel
  return launch_rho(h, mode, true, false, store);
}

// After a committed sweep the handle is in a fixed point of its bookkeeping: the next sweep is the same two or three launches with
// the same arguments.  Such sweeps are captured once (per count, kind of last sweep and bookkeeping state) and replayed as one
// graph launch.
static bool sweep_steady(const vmr_ctx* h) {
  return h->have_state && h->h_valid && !h->h_zero && h->f_valid == (h->g.fuse_full != 0) && (!h->g.ml || h->a_valid) && !h->prof;
}
static unsigned state_sig(const vmr_ctx* h) {
  return (h->h_valid ? 1u : 0u) | (h->h_reduced ? 2u : 0u) | (h->h_zero ? 4u : 0u) | (h->f_valid ? 8u : 0u) | (h->a_valid ? 16u : 0u) | (h->a_zero ? 32u : 0u) |
         (h->rho_stale ? 64u : 0u);
}
static void state_set(vmr_ctx* h, unsigned s) {
  h->h_valid = s & 1u; h->h_reduced = s & 2u; h->h_zero = s & 4u; h->f_valid = s & 8u; h->a_valid = s & 16u; h->a_zero = s & 32u; h->rho_stale = s & 64u;
}
static void drop_graphs(vmr_ctx* h) {
  for (auto& e : h->graphs) (void)hipGraphExecDestroy(e.ex);
  h->graphs.clear();
}
// n plain sweeps from the handle's present state, the last one with (lazy_last) or without leaving rho unwritten
static int graph_for(vmr_ctx* h, int n, bool lazy_last, const vmr_ctx::GraphEntry** out) {
  const unsigned sig0 = state_sig(h);
  for (auto& e : h->graphs) if (e.n == n && e.lazy_last == lazy_last && e.sig0 == sig0) { *out = &e; return VMR_OK; }
  hipGraph_t gr = nullptr;
  HIPCHK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
  int rc = VMR_OK;
  for (int i = 0; i < n && rc == VMR_OK; ++i) rc = sweep(h, 0, i == n - 1 ? !lazy_last : false);   // (queues nothing: the launches are recorded)
  const unsigned sig1 = state_sig(h);
  state_set(h, sig0);   // nothing ran yet
  hipError_t e = hipStreamEndCapture(h->stream, &gr);
  if (rc != VMR_OK || e != hipSuccess || !gr) {
    if (gr) (void)hipGraphDestroy(gr);
    (void)hipGetLastError();
    h->use_graphs = false;   // eager from now on
    if (rc == VMR_OK) { h->err = std::string("hipStreamEndCapture: ") + hipGetErrorString(e); rc = VMR_EHIP; }
    return rc;
  }
  hipGraphExec_t ex = nullptr;
  e = hipGraphInstantiate(&ex, gr, nullptr, nullptr, 0);
  (void)hipGraphDestroy(gr);
  if (e != hipSuccess) { (void)hipGetLastError(); h->use_graphs = false; h->err = std::string("hipGraphInstantiate: ") + hipGetErrorString(e); return VMR_EHIP; }
  h->graphs.push_back({n, lazy_last, sig0, sig1, ex});
  *out = &h->graphs.back();
  return VMR_OK;
}

// n sweeps.  rho is written by the LAST sweep of the call (and by ELBO sweeps) only: the rho of a sweep inside the call is overwritten
// by the next one before anyone can read it.  store_last = false: the caller runs an ELBO sweep next (the fit loops), so not even that.
static int step_n(vmr_ctx* h, int n_iters, double* elbo_out, bool store_last);
int vmr_step(vmr_handle h, int n_iters, double* elbo_out) {
  if (!h) return VMR_EINVAL;
  if (!h->have_state) return fail(h, VMR_ESTATE, "vmr_set_state must be called before vmr_step");
  if (h->restored) return fail(h, VMR_ESTATE, "vmr_step after vmr_restore: the restored state is read-only until the next vmr_set_state");
  if (n_iters < 0) return fail(h, VMR_EINVAL, "n_iters < 0");
  // (VMR_DEBUG_LAZY_RHO=1, diagnostics / tests: leave even the call's last rho unwritten, so that every reader goes through ensure_rho)
  return step_n(h, n_iters, elbo_out, !h->opt.debug_lazy_rho);
}
static int step_n(vmr_ctx* h, int n_iters, double* elbo_out, bool store_last) {
  HIPCHK(h, hipSetDevice(h->device));
  if (n_iters > 0) h->prte_valid = false;   // (a replayed graph runs no launch helper: the sweeps change rho all the same)
  int rc;
  int it = 0;
  const int plain = elbo_out ? n_iters - 1 : n_iters;   // sweeps without an ELBO
  if (h->use_graphs && plain >= 2) {
    if (!sweep_steady(h)) { if ((rc = sweep(h, 0, false))) return rc; it = 1; }   // (more sweeps follow: its rho is overwritten unread)
    while (h->use_graphs && sweep_steady(h) && plain - it >= 2) {
      const int n = (plain - it >= 9) ? 9 : (plain - it);   // the fit loop asks for 9 between two ELBO checks (model.py:1036)
      const bool ends = it + n == n_iters;   // the call's last sweep is in this graph (no ELBO sweep behind it)
      const vmr_ctx::GraphEntry* ge = nullptr;
      if (graph_for(h, n, !(ends && store_last), &ge) != VMR_OK) break;   // capture failed: the eager loop below takes over
      HIPCHK(h, hipGraphLaunch(ge->ex, h->stream));
      state_set(h, ge->sig1);
      h->prte_valid = false;
      it += n;
    }
  }
  for (; it < n_iters; ++it) {
    const bool last = it == n_iters - 1;
    if ((rc = sweep(h, (last && elbo_out) ? 1 : 0, last && store_last))) return rc;
  }
  if (elbo_out) {
    if (n_iters == 0) return vmr_elbo(h, elbo_out);
    return read_elbo(h, elbo_out);
  }
  return VMR_OK;
}

// the convergence loop of `fit` for one realisation (model.py:405-426, 1021-1056), without a host-language round trip
// per iteration: one call per realisation, so several fits driven from host threads do not queue for an interpreter lock.
// (st: where the loop stands -- a fresh realisation, or one whose first iterations ran elsewhere, see vmr_fit_loop_batch)
struct LoopState { int it = 1, coincide = 0, reached = 0, rows = 0; double elbo = -1e10; /* INF of the reference (model.py:24) */ };
static int fit_loop_core(vmr_ctx* h, LoopState& st, int max_iter, double tol, int decision, int cap, int* row_iter, double* row_elbo,
                         double* row_runtime, int* row_reached) {
  int rc;
  while (!st.reached && st.it <= max_iter) {
    // the ELBO is evaluated at iteration 1, every 10th and the last (model.py:1036-1039); the sweeps in between are queued at once
    const int it = st.it;
    const int nxt = (it == 1 || it % 10 == 0 || it == max_iter) ? it : std::min(max_iter, (it / 10 + 1) * 10);
    if (nxt > it) {
      if ((rc = step_n(h, nxt - it, nullptr, false))) return rc;   // (an ELBO sweep follows: it writes rho)
      st.it = nxt;
      HIPCHK(h, hipStreamSynchronize(h->stream));   // so that the runtime below is this iteration's sweep, as in the reference
    }
    const auto t0 = std::chrono::steady_clock::now();
    const double old = st.elbo;
    if ((rc = step_n(h, 1, &st.elbo, true))) return rc;
    const double runtime = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    st.coincide = (fabs(st.elbo - old) < tol) ? st.coincide + 1 : 0;
    if (st.coincide > decision) st.reached = 1;
    ++st.it;
    if ((st.it - 1) % 10 == 0 && st.rows < cap) {
      row_iter[st.rows] = st.it - 1; row_elbo[st.rows] = st.elbo; row_runtime[st.rows] = runtime; row_reached[st.rows] = st.reached;
      ++st.rows;
    }
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return VMR_OK;
}
int vmr_fit_loop(vmr_handle h, int max_iter, double tol, int decision, int cap, int* n_rows, int* row_iter, double* row_elbo,
                 double* row_runtime, int* row_reached, double* elbo_out, int* iters_out, int* converged_out) {
  if (!h || !n_rows || !elbo_out || !iters_out || !converged_out) return VMR_EINVAL;
  if (!h->have_state) return fail(h, VMR_ESTATE, "vmr_set_state must be called before vmr_fit_loop");
  if (h->restored) return fail(h, VMR_ESTATE, "vmr_fit_loop after vmr_restore: the restored state is read-only until the next vmr_set_state");
  if (cap > 0 && (!row_iter || !row_elbo || !row_runtime || !row_reached)) return fail(h, VMR_EINVAL, "trace arrays missing");
  LoopState st;
  int rc = fit_loop_core(h, st, max_iter, tol, decision, cap, row_iter, row_elbo, row_runtime, row_reached);
  if (rc) return rc;
  *n_rows = st.rows; *elbo_out = st.elbo; *iters_out = st.it - 1; *converged_out = st.reached;
  return VMR_OK;
}

// ---- many small fits in lockstep -----------------------------------------------------------------------------------
// A sweep of a Karnataka-sized layer (N = 200-800, L = 1) is two dependent launches of 20-40 us each that leave the GPU nearly
// empty, and launches of different streams of one process hardly overlap (8 host threads: 1.4x one thread's sweeps per
// second).  Here the realisations of n handles advance together: every sweep is ONE launch of the finalize kernel and ONE of
// the pass for all of them (k_fin_gamma_b, k_sweep_sl_b; on ELBO sweeps k_fin_rho_b and one copy of n ELBOs), each handle's
// workgroups reading its own arguments from a table in device memory.  A handle that converges leaves the tables.
// Handles of another kind than the first (K, mutuality, mask kind, report lists in one pass) run their loops one by one.
static bool batch_steady(const vmr_ctx* h) {
  const Geo& g = h->g;
  return h->have_state && !h->restored && h->sparse && !g.two_pass && !g.farl && h->h_valid && !h->h_reduced && !h->h_zero &&
         h->f_valid == (g.fuse_full != 0) && (!g.ml || h->a_valid) && !h->prof;
}
static bool batch_kind(const vmr_ctx* h, const vmr_ctx* h0) {
  // (a sweep of such a handle is k_fin_gamma + the pass, + k_fin_rho with an ELBO: the pass sums rho over the mask itself)
  return h->sparse && !h->g.gen && !h->g.two_pass && !h->g.farl && !h->g.det && !h->prof && h->g.fuse_full && (h->n_partial == 0 || h->g.ml) && h->device == h0->device &&
         h->g.K == h0->g.K && h->g.mut == h0->g.mut && (h->all_full != 0) == (h0->all_full != 0) && !memcmp(&h->opt, &h0->opt, sizeof h->opt);
}
namespace {
struct BatchTables {   // device copies of the unit tables of one lockstep loop
  SlUnit* su[3] = {nullptr, nullptr, nullptr};   // mode 0 / 1; [2]: the statistics pass of a realisation's first sweep
  int* smap[3] = {nullptr, nullptr, nullptr};
  FinUnit* fu = nullptr;
  int *gmap = nullptr, *rmap = nullptr;
  double* be = nullptr;                 // [n][8]: every unit's elbo_dev
  int nb[3] = {0, 0, 0}, ngb = 0, nrb = 0, tpb[3] = {0, 0, 0}, fg = FG_G;
  size_t smem[3] = {0, 0, 0}, fsm = 0;
  ~BatchTables() { for (void* p : {(void*)su[0], (void*)su[1], (void*)su[2], (void*)smap[0], (void*)smap[1], (void*)smap[2], (void*)fu, (void*)gmap, (void*)rmap, (void*)be}) if (p) (void)hipFree(p); }
};
}  // namespace
// (re)builds the tables for the units listed in `act`
static int batch_tables(vmr_ctx* const* hs, const std::vector<int>& act, int n_all, BatchTables& bt, hipStream_t st) {
  vmr_ctx* h0 = hs[act[0]];
  const int K = h0->g.K, allfull = h0->all_full != 0;
  long long steps = 0;
  for (int u : act) steps += (((long long)hs[u]->g.N * hs[u]->g.N + 63) / 64) * hs[u]->g.L;
  std::vector<FinUnit> fu(act.size());
  std::vector<int> gmap, rmap;
  for (int m = 0; m < 3; ++m) {
    const int tpb = sl_tpb_max_b(K, m == 1, allfull), nw = tpb / 64;
    // steps per wave: about one workgroup per CU in all (the tables in LDS allow few more, and a second round of workgroups
    // costs a workgroup's fixed part -- its tables, its share of nu: some ten steps' worth -- again), at least 4 steps each, at
    // most 64 (192 fits of N = 200..800, lockstep loops: cap 8 1.05 s, 16 0.88, 32 0.78, 64 0.72, none 0.96 -- a small unit
    // then is one workgroup that walks all its steps)
    long long per = std::max<long long>(4, std::min<long long>(64, (steps + (long long)nw * h0->ncu - 1) / ((long long)nw * h0->ncu)));
    {
      // ... but never a FEW workgroups more than are resident at once: every workgroup of the launch gets the largest unit's LDS
      // (a village of N = 900: 130 KB, one workgroup per CU), and with 293 workgroups on 256 CUs the launch takes two rounds for
      // the sake of 37.  Then rather more steps per wave, until one round holds them all.
      size_t smem_max = 0;
      for (int u : act) smem_max = std::max(smem_max, sl_shape(hs[u], m != 2, m == 1, true).smem);
      const int wpc = std::max<int>(1, std::min<int>((int)(SP_LDS_MAX / std::max<size_t>(smem_max, 1)), 4 * sl_wpe_b(K, m == 1, allfull) / nw));
      const long long cap_wgs = (long long)h0->ncu * wpc;
      auto total = [&](long long p_) {
        long long t = 0;
        for (int u : act) { const Geo& g = hs[u]->g; const long long NS = ((long long)g.N * g.N + 63) / 64; t += (long long)g.L * ((NS + nw * p_ - 1) / (nw * p_)); }
        return t;
      };
      if (total(per) > cap_wgs) {
        long long p2 = per;
        while (p2 < 512 && total(p2) > cap_wgs) p2 += std::max<long long>(1, p2 / 16);
        if (total(p2) <= cap_wgs) per = p2;
      }
    }
    std::vector<SlUnit> su(act.size());
    std::vector<int> map;
    size_t smem = 0;
    for (size_t i = 0; i < act.size(); ++i) {
      vmr_ctx* h = hs[act[i]];
      const Geo& g = h->g;
      const SlShape sh = sl_shape(h, m != 2, m == 1, true);
      SlArgs a = sl_args(h, sh, 1, g.ml ? 1 : 0);
      a.elbo_dev = bt.be + (size_t)act[i] * 8;
      if (g.mut && m != 2) { a.nu_acc = h->nu_acc; a.commit_nu = 1; }   // (the statistics of the initial rho leave nu alone)
      const long long NS = ((long long)g.N * g.N + 63) / 64;
      a.Gl = (int)std::max<long long>(1, std::min<long long>(4096, (NS + nw * per - 1) / (nw * per)));
      su[i].a = a; su[i].g = g; su[i].blk0 = (int)map.size(); su[i].nblk = g.L * a.Gl;
      map.insert(map.end(), (size_t)su[i].nblk, (int)i);
      smem = std::max(smem, sh.smem);
    }
    HIPCHK(h0, hipMemcpyAsync(bt.su[m], su.data(), su.size() * sizeof(SlUnit), hipMemcpyHostToDevice, st));
    HIPCHK(h0, hipMemcpyAsync(bt.smap[m], map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(h0, hipStreamSynchronize(st));   // (the host vectors go away)
    bt.nb[m] = (int)map.size(); bt.tpb[m] = tpb; bt.smem[m] = smem;
  }
  bt.fsm = 0;
  {   // workgroups per layer of the finalize launch: about one per CU in all, 2..FG_G per layer
    long long layers = 0;
    for (int u : act) layers += hs[u]->g.L;
    bt.fg = (int)std::max<long long>(2, std::min<long long>(FG_G, (1LL * h0->ncu) / std::max<long long>(1, layers)));   // (64 units: 4 -- measured 1 / 2 / 4 / 8 / 16: 3.29 / 3.06 / 2.95 / 3.11 / 3.33 s of loops)
    if (h0->opt.batch_fg) bt.fg = h0->opt.batch_fg;   // (experiments)
  }
  for (size_t i = 0; i < act.size(); ++i) {
    vmr_ctx* h = hs[act[i]];
    const Geo& g = h->g;
    fu[i] = FinUnit{h->par, h->Hg, h->Cg, h->slotA, h->slotF, h->lutg, h->fin_g, h->nu_acc, h->slotR, bt.be + (size_t)act[i] * 8, g,
                    (int)gmap.size(), (int)rmap.size(), g.L * FR_G};
    gmap.insert(gmap.end(), (size_t)g.L * bt.fg, (int)i);
    rmap.insert(rmap.end(), (size_t)g.L * FR_G, (int)i);
    bt.fsm = std::max(bt.fsm, (size_t)2 * ((g.M + bt.fg - 1) / bt.fg) * 8);
  }
  HIPCHK(h0, hipMemcpyAsync(bt.fu, fu.data(), fu.size() * sizeof(FinUnit), hipMemcpyHostToDevice, st));
  HIPCHK(h0, hipMemcpyAsync(bt.gmap, gmap.data(), gmap.size() * sizeof(int), hipMemcpyHostToDevice, st));
  HIPCHK(h0, hipMemcpyAsync(bt.rmap, rmap.data(), rmap.size() * sizeof(int), hipMemcpyHostToDevice, st));
  HIPCHK(h0, hipStreamSynchronize(st));
  bt.ngb = (int)gmap.size(); bt.nrb = (int)rmap.size();
  (void)n_all;
  return VMR_OK;
}

int vmr_fit_loop_batch(vmr_handle* hs, int n, int max_iter, double tol, int decision, int cap, int* n_rows, int* row_iter, double* row_elbo,
                       double* row_runtime, int* row_reached, double* elbo_out, int* iters_out, int* converged_out, int* rc_out) {
  if (!hs || n <= 0 || !n_rows || !elbo_out || !iters_out || !converged_out || !rc_out) return VMR_EINVAL;
  if (cap > 0 && (!row_iter || !row_elbo || !row_runtime || !row_reached)) return VMR_EINVAL;
  for (int u = 0; u < n; ++u) {
    if (!hs[u]) return VMR_EINVAL;
    for (int v = 0; v < u; ++v) if (hs[v] == hs[u]) return fail(hs[u], VMR_EINVAL, "vmr_fit_loop_batch: a handle is listed twice");
    rc_out[u] = VMR_OK;
  }
  std::vector<LoopState> ls(n);
  auto rows_of = [&](int u, int*& ri, double*& re, double*& rr, int*& rq) {
    ri = cap > 0 ? row_iter + (size_t)u * cap : nullptr; re = cap > 0 ? row_elbo + (size_t)u * cap : nullptr;
    rr = cap > 0 ? row_runtime + (size_t)u * cap : nullptr; rq = cap > 0 ? row_reached + (size_t)u * cap : nullptr;
  };
  auto solo = [&](int u) {   // this unit's loop (or the rest of it) on its own
    int* ri; double* re; double* rr; int* rq;
    rows_of(u, ri, re, rr, rq);
    vmr_ctx* h = hs[u];
    if (!h->have_state) { rc_out[u] = fail(h, VMR_ESTATE, "vmr_set_state must be called before vmr_fit_loop_batch"); return; }
    if (h->restored) { rc_out[u] = fail(h, VMR_ESTATE, "vmr_fit_loop_batch after vmr_restore: the restored state is read-only until the next vmr_set_state"); return; }
    rc_out[u] = fit_loop_core(h, ls[u], max_iter, tol, decision, cap, ri, re, rr, rq);
  };
  auto finish = [&]() {
    int worst = VMR_OK;
    for (int u = 0; u < n; ++u) {
      n_rows[u] = ls[u].rows; elbo_out[u] = ls[u].elbo; iters_out[u] = ls[u].it - 1; converged_out[u] = ls[u].reached;
      if (rc_out[u] && !worst) worst = rc_out[u];
    }
    return worst;
  };
  // the units of the first batchable handle's kind advance together; the others run alone
  int lead = -1;
  for (int u = 0; u < n && lead < 0; ++u) if (hs[u]->have_state && !hs[u]->restored && batch_kind(hs[u], hs[u])) lead = u;
  std::vector<int> act;
  for (int u = 0; u < n; ++u) {
    if (lead >= 0 && hs[u]->have_state && !hs[u]->restored && batch_kind(hs[u], hs[lead]) && vmr_sl_batch_launcher(hs[u]->g.K)) act.push_back(u);
    else solo(u);
  }
  if (act.size() < 2 || max_iter < 2) { for (int u : act) solo(u); return finish(); }
  vmr_ctx* h0 = hs[act[0]];
  // Every failure from here on leaves through ONE exit: the code goes into rc_out of every unit still in the lockstep loop (their
  // traces, ELBOs and iteration counts are then meaningless) and into the return value.
  auto lockstep = [&]() -> int {
  HIPCHK(h0, hipSetDevice(h0->device));
  // the loop runs every unit's kernels on ONE stream (the first unit's): whatever a unit's own stream still holds -- the tail of
  // vmr_set_state, an earlier sweep -- is waited for here, once
  for (int u : act) HIPCHK(h0, hipStreamSynchronize(hs[u]->stream));
  // Iteration 1 (the ELBO is evaluated there, model.py:1036) also builds the statistics of the initial rho -- launches the
  // steady sweeps do not have.  Handles that come straight from vmr_set_state take it inside the tables (below); if some do
  // not, every handle runs it on its own stream.
  bool fresh = true;
  for (int u : act) fresh = fresh && !hs[u]->h_valid && !hs[u]->prof;
  if (!fresh) {
    for (int u : act) { rc_out[u] = sweep(hs[u], 1); }
    for (size_t i = 0; i < act.size();) {
      const int u = act[i];
      if (!rc_out[u]) rc_out[u] = read_elbo(hs[u], &ls[u].elbo);
      if (rc_out[u]) { (void)hipStreamSynchronize(hs[u]->stream); act.erase(act.begin() + i); continue; }
      ls[u].coincide = (fabs(ls[u].elbo - (-1e10)) < tol) ? 1 : 0;
      if (ls[u].coincide > decision) ls[u].reached = 1;
      ls[u].it = 2;
      if (ls[u].reached) { act.erase(act.begin() + i); continue; }
      if (!batch_steady(hs[u])) { solo(u); act.erase(act.begin() + i); continue; }
      ++i;
    }
  }
  if (act.size() < 2) { for (int u : act) solo(u); act.clear(); return VMR_OK; }
  h0 = hs[act[0]];
  hipStream_t st = h0->stream;
  const int K = h0->g.K, allfull = h0->all_full != 0;
  sl_launch_batch_fn pass = vmr_sl_batch_launcher(K);
  BatchTables bt;
  {
    size_t blocks = 0, gb = 0, rb = 0;
    for (int u : act) {
      const Geo& g = hs[u]->g;
      blocks += (size_t)g.L * 4096; gb += (size_t)g.L * FG_G; rb += (size_t)g.L * FR_G;
    }
    for (int m = 0; m < 3; ++m) {
      HIPCHK(h0, hipMalloc(&bt.su[m], act.size() * sizeof(SlUnit)));
      HIPCHK(h0, hipMalloc(&bt.smap[m], blocks * sizeof(int)));
    }
    HIPCHK(h0, hipMalloc(&bt.fu, act.size() * sizeof(FinUnit)));
    HIPCHK(h0, hipMalloc(&bt.gmap, gb * sizeof(int)));
    HIPCHK(h0, hipMalloc(&bt.rmap, rb * sizeof(int)));
    HIPCHK(h0, hipMalloc(&bt.be, (size_t)n * 8 * 8));
    HIPCHK(h0, hipMemsetAsync(bt.be, 0, (size_t)n * 8 * 8, st));
  }
  std::vector<double> be_host((size_t)n * 8);
  int rc = batch_tables(hs, act, n, bt, st);
  if (rc) return rc;
  const bool lazy_rho = !h0->opt.always_store_rho;   // plain sweeps do not write rho: the ELBO sweep every loop ends with does
  auto launch_sweeps = [&](int mode) -> int {
    hipLaunchKernelGGL(k_fin_gamma_b, dim3(bt.ngb), dim3(FIN_TPB), bt.fsm, st, bt.fu, bt.gmap, bt.fg);
    const int pm = (mode == 0 && lazy_rho) ? 4 : mode;
    int r = pass(h0, st, pm, allfull, bt.su[mode], bt.smap[mode], bt.nb[mode], bt.tpb[mode], bt.smem[mode]);
    for (int u : act) { hs[u]->rho_stale = pm == 4; hs[u]->prte_valid = false; }
    if (r) return r;
    if (mode == 1) hipLaunchKernelGGL(k_fin_rho_b, dim3(bt.nrb), dim3(TPB), 0, st, bt.fu, bt.rmap);
    HIPCHK(h0, hipGetLastError());
    return VMR_OK;
  };
  int it = fresh ? 1 : 2;   // every active unit stands at the same iteration
  while (!act.empty() && it <= max_iter) {
    const int nxt = (it == 1 || it % 10 == 0 || it == max_iter) ? it : std::min(max_iter, (it / 10 + 1) * 10);
    for (; it < nxt; ++it) if ((rc = launch_sweeps(0))) break;
    if (rc) break;
    HIPCHK(h0, hipStreamSynchronize(st));
    const auto t0 = std::chrono::steady_clock::now();
    if (it == 1) {
      // the first sweep of the realisations: H, the all-ones sums and the mask sums of the initial rho (launch_hist, for all units)
      for (int u : act) {
        vmr_ctx* h = hs[u];
        const Geo& g = h->g;
        HIPCHK(h0, hipMemsetAsync(h->Hg, 0, (size_t)g.L * NH * g.Y * g.Mp * g.K * 8, st));
        HIPCHK(h0, hipMemsetAsync(h->slotF, 0, (size_t)g.L * NSLOT * g.K * 8, st));
        if (g.ml) HIPCHK(h0, hipMemsetAsync(h->slotA, 0, (size_t)g.L * NSLOT * g.W * 64 * g.K * 8, st));
      }
      if ((rc = pass(h0, st, 3, allfull, bt.su[2], bt.smap[2], bt.nb[2], bt.tpb[2], bt.smem[2]))) break;
      for (int u : act) {   // (where a sweep leaves a handle: statistics of the current rho in place, nothing folded or zeroed)
        vmr_ctx* h = hs[u];
        h->h_valid = true; h->h_zero = false; h->h_reduced = false; h->f_valid = h->g.fuse_full != 0; h->a_valid = h->g.ml != 0; h->a_zero = false;
      }
    }
    if ((rc = launch_sweeps(1))) break;
    HIPCHK(h0, hipMemcpyAsync(be_host.data(), bt.be, (size_t)n * 8 * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(h0, hipStreamSynchronize(st));
    const double runtime = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    ++it;
    bool changed = false;
    for (size_t i = 0; i < act.size();) {
      const int u = act[i];
      LoopState& s = ls[u];
      const double old = s.elbo;
      s.elbo = be_host[(size_t)u * 8];
      s.it = it;
      bool out = false;
      if (isnan(s.elbo)) { rc_out[u] = fail(hs[u], VMR_ENAN, "ELBO is NaN!!!!"); out = true; }
      else {
        s.coincide = (fabs(s.elbo - old) < tol) ? s.coincide + 1 : 0;
        if (s.coincide > decision) s.reached = 1;
        if ((it - 1) % 10 == 0 && s.rows < cap) {
          int* ri; double* re; double* rr; int* rq;
          rows_of(u, ri, re, rr, rq);
          ri[s.rows] = it - 1; re[s.rows] = s.elbo; rr[s.rows] = runtime; rq[s.rows] = s.reached;
          ++s.rows;
        }
        out = s.reached != 0;
      }
      if (out) { act.erase(act.begin() + i); changed = true; } else ++i;
    }
    if (changed && !act.empty() && it <= max_iter && (rc = batch_tables(hs, act, n, bt, st))) break;
  }
  (void)hipStreamSynchronize(st);
  return rc;
  };
  const int rc_all = lockstep();
  if (rc_all) {
    (void)hipStreamSynchronize(h0->stream);
    for (int u : act) if (!rc_out[u]) { rc_out[u] = rc_all; if (hs[u] != h0) hs[u]->err = h0->err; }
  }
  return finish();
}

int vmr_elbo(vmr_handle h, double* out) {
  if (!h || !out) return VMR_EINVAL;
  if (!h->have_state) return fail(h, VMR_ESTATE, "vmr_set_state must be called before vmr_elbo");
  if (h->restored) return fail(h, VMR_ESTATE, "vmr_elbo after vmr_restore: the restored state is read-only until the next vmr_set_state");
  HIPCHK(h, hipSetDevice(h->device));
  int rc;
  if ((rc = launch_rho(h, 2, false))) return rc;
  return read_elbo(h, out);
}

int vmr_sweep_local(vmr_handle h, int want_elbo, double* out3) {
  if (!h || !out3) return VMR_EINVAL;
  if (!h->have_state) return fail(h, VMR_ESTATE, "vmr_set_state must be called before vmr_sweep_local");
  if (h->restored) return fail(h, VMR_ESTATE, "vmr_sweep_local after vmr_restore: the restored state is read-only until the next vmr_set_state");
  HIPCHK(h, hipSetDevice(h->device));
  int rc;
  if ((rc = launch_gamma(h, true))) return rc;
  if ((rc = launch_rho(h, want_elbo ? 1 : 0, false, true))) return rc;   // rho updated, nu NOT committed
  if (!want_elbo && !h->sparse) {   // launch_rho skipped the finalize kernel: run it for the raw pieces only
    if ((rc = launch_fin_rho(h, 0, 0))) return rc;   // (sorted lists: the pass left the raw nu sum itself)
  }
  double v[4];
  HIPCHK(h, hipMemcpyAsync(v, h->elbo_dev, 32, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  out3[0] = v[1]; out3[1] = v[2]; out3[2] = v[3];
  return VMR_OK;
}

int vmr_commit_nu(vmr_handle h, double nu_partial_total) {
  if (!h) return VMR_EINVAL;
  if (!h->have_state) return fail(h, VMR_ESTATE, "vmr_set_state must be called before vmr_commit_nu");
  if (h->restored) return fail(h, VMR_ESTATE, "vmr_commit_nu after vmr_restore: the restored state is read-only until the next vmr_set_state");
  HIPCHK(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(k_commit_nu, dim3(1), dim3(64), 0, h->stream, h->par, nu_partial_total, (const double*)nullptr, h->g);
  HIPCHK(h, hipGetLastError());
  return VMR_OK;
}

// the same exchange with the three doubles left on the device (RCCL all-reduce on the handle's stream, see vmr_stream)
int vmr_sweep_local_dev(vmr_handle h, int want_elbo, double* out3_dev) {
  if (!h || !out3_dev) return VMR_EINVAL;
  if (!h->have_state) return fail(h, VMR_ESTATE, "vmr_set_state must be called before vmr_sweep_local_dev");
  if (h->restored) return fail(h, VMR_ESTATE, "vmr_sweep_local_dev after vmr_restore: the restored state is read-only until the next vmr_set_state");
  HIPCHK(h, hipSetDevice(h->device));
  int rc;
  if ((rc = launch_gamma(h, true))) return rc;
  if ((rc = launch_rho(h, want_elbo ? 1 : 0, false, true))) return rc;
  if (!want_elbo && !h->sparse && (rc = launch_fin_rho(h, 0, 0))) return rc;
  HIPCHK(h, hipMemcpyAsync(out3_dev, h->elbo_dev + 1, 24, hipMemcpyDeviceToDevice, h->stream));
  return VMR_OK;
}

int vmr_commit_nu_dev(vmr_handle h, const double* nu_partial_total_dev) {
  if (!h || !nu_partial_total_dev) return VMR_EINVAL;
  if (!h->have_state) return fail(h, VMR_ESTATE, "vmr_set_state must be called before vmr_commit_nu_dev");
  if (h->restored) return fail(h, VMR_ESTATE, "vmr_commit_nu_dev after vmr_restore: the restored state is read-only until the next vmr_set_state");
  HIPCHK(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(k_commit_nu, dim3(1), dim3(64), 0, h->stream, h->par, 0.0, nu_partial_total_dev, h->g);
  HIPCHK(h, hipGetLastError());
  return VMR_OK;
}

void* vmr_stream(vmr_handle h) { return h ? (void*)h->stream : nullptr; }

int vmr_sub_step(vmr_handle h, int which) {
  if (!h) return VMR_EINVAL;
  if (!h->have_state) return fail(h, VMR_ESTATE, "vmr_set_state must be called before vmr_sub_step");
  if (h->restored) return fail(h, VMR_ESTATE, "vmr_sub_step after vmr_restore: the restored state is read-only until the next vmr_set_state");
  HIPCHK(h, hipSetDevice(h->device));
  if (h->g.det) return fail(h, VMR_ESTATE, "vmr_sub_step is not available with VMR_DETERMINISTIC=1 (whole sweeps only: vmr_step, vmr_fit_loop)");
  { const int rce = ensure_rho(h); if (rce) return rce; }
  switch (which) {
    case VMR_STEP_GAMMA: return launch_gamma(h, false);
    case VMR_STEP_PHI:
      // phi's rate is finished by the gamma finalize (one pass over the mask sums for both): without one since the last change of
      // rho there is none to commit -- silently committing the last one gave a rate of another rho, or of another realisation
      if (h->g.mut && !h->prte_valid)
        return fail(h, VMR_ESTATE, "VMR_STEP_PHI commits the rate that VMR_STEP_GAMMA prepares: no VMR_STEP_GAMMA since rho last changed");
      return launch_phi(h);
    // the rho pass also rebuilds the statistics H the nu update reads; nu is committed by the NU sub-step
    case VMR_STEP_RHO: return launch_rho(h, 0, false);
    case VMR_STEP_NU: {
      if (!h->g.mut) return VMR_OK;
      if (!h->h_valid) { int rc = launch_hist(h); if (rc) return rc; }
      return launch_fin_rho(h, 1, 0);
    }
    default: return fail(h, VMR_EINVAL, "unknown sub-step");
  }
}

// the whole parameter block in ONE copy (tens of KB): the getters of the small posteriors are called once per realisation of every
// small fit, from several host threads -- six small copies with a synchronisation each cost them a millisecond per call
static int fetch_par(vmr_ctx* h, std::vector<double>& buf) {
  buf.resize(h->par_doubles);
  HIPCHK(h, hipMemcpyAsync(buf.data(), h->par, h->par_doubles * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return VMR_OK;
}
static void rows_lm(const Geo& g, const std::vector<double>& buf, size_t off, double* dst) {
  for (int l = 0; l < g.L; ++l) memcpy(dst + (size_t)l * g.M, &buf[off + (size_t)l * g.Mp], (size_t)g.M * 8);
}

int vmr_get_state(vmr_handle h, double* gamma_shp, double* gamma_rte, double* phi_shp, double* phi_rte,
                  double* nu_shp, double* nu_rte, double* rho) {
  if (!h) return VMR_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  const Geo& g = h->g;
  ParOff o = par_off(g.L, g.Mp, g.K);
  int rc;
  if (gamma_shp || gamma_rte || phi_shp || phi_rte || nu_shp || nu_rte) {
    std::vector<double> buf;
    if ((rc = fetch_par(h, buf))) return rc;
    if (gamma_shp) rows_lm(g, buf, o.g_shp, gamma_shp);
    if (gamma_rte) rows_lm(g, buf, o.g_rte, gamma_rte);
    if (phi_shp) memcpy(phi_shp, &buf[o.p_shp], (size_t)g.L * g.K * 8);
    if (phi_rte) memcpy(phi_rte, &buf[o.p_rte], (size_t)g.L * g.K * 8);
    if (nu_shp) *nu_shp = buf[o.sc + SC_NU_SHP];
    if (nu_rte) *nu_rte = buf[o.sc + SC_NU_RTE];
  }
  if (rho) {
    { const int rce = ensure_rho(h); if (rce) return rce; }
    const size_t nr = (size_t)g.L * g.N * g.N * g.K;
    const double* src = h->rho;
    if (h->perm) {   // back to tie order
      if (!h->nat) HIPCHK(h, hipMalloc(&h->nat, nr * 8));
      if ((rc = sl_permute_rows(h, h->rho, h->nat, false))) return rc;
      src = h->nat;
    }
    if ((rc = d2h(h, rho, src, nr * 8))) return rc;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return VMR_OK;
}

int vmr_get_geometric(vmr_handle h, double* g_theta, double* g_lambda, double* g_nu, double* g_nu_cache) {
  if (!h) return VMR_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  const Geo& g = h->g;
  ParOff o = par_off(g.L, g.Mp, g.K);
  int rc;
  std::vector<double> buf;
  if ((rc = fetch_par(h, buf))) return rc;
  if (g_theta) rows_lm(g, buf, o.G_th, g_theta);
  if (g_lambda) memcpy(g_lambda, &buf[o.G_la], (size_t)g.L * g.K * 8);
  if (g_nu) *g_nu = buf[o.sc + SC_G_NU];
  if (g_nu_cache) *g_nu_cache = buf[o.sc + SC_G_NU_STALE];
  return VMR_OK;
}

// `_update_optimal_parameters` (model.py:925-942) without a host round trip: keep a device copy of the posteriors
int vmr_snapshot(vmr_handle h) {
  if (!h) return VMR_EINVAL;
  if (!h->have_state) return fail(h, VMR_ESTATE, "vmr_set_state must be called before vmr_snapshot");
  HIPCHK(h, hipSetDevice(h->device));
  { const int rce = ensure_rho(h); if (rce) return rce; }
  const Geo& g = h->g;
  const size_t nr = (size_t)g.L * g.N * g.N * g.K * 8, np_ = h->par_doubles * 8;
  if (!h->rho_snap) { HIPCHK(h, hipMalloc(&h->rho_snap, nr)); HIPCHK(h, hipMalloc(&h->par_snap, np_)); }
  HIPCHK(h, hipMemcpyAsync(h->rho_snap, h->rho, nr, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->par_snap, h->par, np_, hipMemcpyDeviceToDevice, h->stream));
  h->have_snap = true;
  return VMR_OK;
}

// make the snapshot the current state again (rho and every parameter; the statistics are rebuilt on the next sweep)
int vmr_restore(vmr_handle h) {
  if (!h) return VMR_EINVAL;
  if (!h->have_snap) return fail(h, VMR_ESTATE, "vmr_snapshot must be called before vmr_restore");
  HIPCHK(h, hipSetDevice(h->device));
  const Geo& g = h->g;
  HIPCHK(h, hipMemcpyAsync(h->rho, h->rho_snap, (size_t)g.L * g.N * g.N * g.K * 8, hipMemcpyDeviceToDevice, h->stream));
  // the posteriors and what is derived from them, NOT the priors: those are the handle's (a vmr_set_priors since the snapshot holds)
  {
    const ParOff o = par_off(g.L, g.Mp, g.K);
    const size_t rng[3][2] = {{o.g_shp, o.a_la}, {o.p_shp, o.sc}, {o.sc + SC_NU_SHP, o.total}};
    for (const auto& r : rng)
      HIPCHK(h, hipMemcpyAsync(h->par + r[0], h->par_snap + r[0], (r[1] - r[0]) * 8, hipMemcpyDeviceToDevice, h->stream));
  }
  h->h_valid = false; h->f_valid = false; h->a_valid = false; h->h_zero = false; h->prte_valid = false;
  h->restored = true;   // the log prior on the device is the LAST realisation's: reading is fine, sweeping is not
  h->rho_stale = false;
  HIPCHK(h, hipMemsetAsync(h->slotF, 0, (size_t)g.L * NSLOT * g.K * 8, h->stream));
  hipLaunchKernelGGL(k_build_lut, dim3(g.L), dim3(256), 0, h->stream, h->par, h->lutg, g);
  HIPCHK(h, hipGetLastError());
  return VMR_OK;
}

int vmr_readout(vmr_handle h, int method, double threshold, void* out, int out_on_device) {
  if (!h || !out) return VMR_EINVAL;
  if (!h->have_state) return fail(h, VMR_ESTATE, "vmr_set_state must be called before vmr_readout");
  if (method < VMR_READ_RHO_MAX || method > VMR_READ_THRESHOLD) return fail(h, VMR_EINVAL, "unknown read-out method");
  HIPCHK(h, hipSetDevice(h->device));
  { const int rce = ensure_rho(h); if (rce) return rce; }
  const Geo& g = h->g;
  const size_t ties = (size_t)g.L * g.N * g.N, bytes = ties * (method == VMR_READ_RHO_MEAN ? 8 : 1);
  void* dst = out;
  if (!out_on_device) HIPCHK(h, hipMalloc(&dst, bytes));
  const size_t T_ = (size_t)g.N * g.N;
  hipLaunchKernelGGL(k_readout, dim3((unsigned)std::min<size_t>(4096, (ties + 255) / 256)), dim3(256), 0, h->stream, h->rho, dst, ties,
                     g.K, method, threshold, h->perm, T_, (T_ + 63) / 64);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && !out_on_device) e = hipMemcpyAsync(out, dst, bytes, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (!out_on_device) (void)hipFree(dst);
  if (e != hipSuccess) { h->err = std::string("vmr_readout: ") + hipGetErrorString(e); (void)hipGetLastError(); return VMR_EHIP; }
  return VMR_OK;
}

int vmr_sample(vmr_handle h, uint64_t seed, int n_trials, uint8_t* out, int out_on_device) {
  if (!h || !out) return VMR_EINVAL;
  if (!h->have_state) return fail(h, VMR_ESTATE, "vmr_set_state must be called before vmr_sample");
  if (n_trials < 1) return fail(h, VMR_EINVAL, "n_trials must be positive");
  HIPCHK(h, hipSetDevice(h->device));
  { const int rce = ensure_rho(h); if (rce) return rce; }
  const Geo& g = h->g;
  const size_t T_ = (size_t)g.N * g.N, ties = (size_t)g.L * T_;
  uint8_t* dst = out;
  if (!out_on_device) HIPCHK(h, hipMalloc(&dst, ties));
  if (g.K > KMAX) { const int rcg = gen_sample(h, (unsigned long long)seed, n_trials, dst); if (rcg) { if (!out_on_device) (void)hipFree(dst); return rcg; } }
  else hipLaunchKernelGGL(k_sample, dim3((unsigned)std::min<size_t>(4096, (ties + 255) / 256)), dim3(256), 0, h->stream, h->rho, dst, ties, g.K,
                          n_trials, (unsigned long long)seed, h->perm, T_, (T_ + 63) / 64);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && !out_on_device) e = hipMemcpyAsync(out, dst, ties, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (!out_on_device) (void)hipFree(dst);
  if (e != hipSuccess) { h->err = std::string("vmr_sample: ") + hipGetErrorString(e); (void)hipGetLastError(); return VMR_EHIP; }
  return VMR_OK;
}

int vmr_sync(vmr_handle h) {
  if (!h) return VMR_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return VMR_OK;
}

static int prof_collect(vmr_ctx* h) {
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (auto& e : h->evs) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) { h->prof_ms[e.cls] += ms; h->prof_n[e.cls] += 1; }
    (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b);
  }
  h->evs.clear();
  return VMR_OK;
}

int vmr_profile(vmr_handle h, int enable) {
  if (!h) return VMR_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  int rc = prof_collect(h);
  if (rc) return rc;
  h->prof = enable != 0;
  // enable = 2: only the passes over the data (the roofline kernels); the small finalize kernels run unbracketed -- two event
  // records per launch are ~4 us on the stream, 9 % of a config-3 sweep when every kernel carries them
  h->prof_mask = enable == 2 ? ((1u << VMR_KERNEL_GAMMA_COUNTS) | (1u << VMR_KERNEL_RHO) | (1u << VMR_KERNEL_ELBO) | (1u << VMR_KERNEL_RHO_ELBO) | (1u << VMR_KERNEL_RHO_NOSTORE)) : ~0u;
  if (enable) { memset(h->prof_ms, 0, sizeof h->prof_ms); memset(h->prof_n, 0, sizeof h->prof_n); }
  return VMR_OK;
}

int vmr_profile_read(vmr_handle h, int kernel_class, double* total_ms, int64_t* launches) {
  if (!h || kernel_class < 0 || kernel_class >= VMR_KERNEL_COUNT) return VMR_EINVAL;
  HIPCHK(h, hipSetDevice(h->device));
  int rc = prof_collect(h);
  if (rc) return rc;
  if (total_ms) *total_ms = h->prof_ms[kernel_class];
  if (launches) *launches = h->prof_n[kernel_class];
  return VMR_OK;
}

int vmr_data_format(vmr_handle h, int* sparse, uint64_t* nnz) {
  if (!h) return VMR_EINVAL;
  if (sparse) *sparse = h->sparse;
  if (nnz) *nnz = h->nnz;
  return VMR_OK;
}

int vmr_mask_format(vmr_handle h, int* lists, uint64_t* listed) {
  if (!h) return VMR_EINVAL;
  if (lists) *lists = h->rq ? 1 : 0;
  if (listed) *listed = h->n_rm;
  return VMR_OK;
}

int vmr_sweep_shape(vmr_handle h, int* passes, int* lds_levels, uint64_t* far_reports) {
  if (!h) return VMR_EINVAL;
  if (passes) *passes = h->g.two_pass ? 2 : 1;
  if (lds_levels) *lds_levels = h->g.gen ? 0 : h->g.hc;
  if (far_reports) *far_reports = (h->g.farl && !h->far_off.empty()) ? h->far_off.back() : 0ull;
  return VMR_OK;
}

int vmr_kernel_bytes(vmr_handle h, int kernel_class, double* bytes) {
  if (!h || !bytes) return VMR_EINVAL;
  const Geo& g = h->g;
  const double V = (double)g.L * g.N * g.N * g.M;   // canonical: X 1 B/elt, R 1 bit/elt
  const double SX = V, SR = V / 8.0, Srho = 8.0 * g.L * (double)g.N * g.N * g.K;
  if (h->sparse) {   // report lists: 4 B per non-zero count + 4 B per tie; mask words only for partial rows
    const double ties = (double)g.L * g.N * g.N;
    // entries (without the rounds' padding); step pointers: two per 64 ties in the step layout, one in the sorted lists
    const double E = (g.wide ? 8.0 : 4.0) * (double)h->nnz, RP = 4.0 * (ties / 64.0 + g.L);   // (two-word entries: 8 B per report)
    const double mask = h->all_full ? 0.0 : ties + (h->rq ? 4.0 * ties + 2.0 * (double)h->n_rm : (double)h->n_partial * g.W * 8.0);
    const double Q = g.mut ? 4.0 * ties : 0.0;
    const double Slp = h->lpd ? 8.0 * ties : Srho;   // log prior of the update passes without ELBO: K = 2, its difference (SlArgs::lpd)
    switch (kernel_class) {
      case VMR_KERNEL_GAMMA_MASK: *bytes = ties + (h->rq ? 4.0 * ties + 2.0 * (double)h->n_rm : (double)h->n_partial * g.W * 8.0) + Srho; break;
      case VMR_KERNEL_GAMMA_COUNTS:   // (x0p: the rounds of level 0 only are not read -- a count per tie instead)
        *bytes = ((h->x0p && g.two_pass) ? 4.0 * (double)h->stat_slots + 4.0 * ties : E) + RP + Srho;
        break;
      case VMR_KERNEL_RHO: *bytes = E + RP + mask + Slp + Srho; break;
      case VMR_KERNEL_RHO_NOSTORE: *bytes = E + RP + mask + Slp; break;   // (the log prior is read, rho is not written)
      case VMR_KERNEL_ELBO: *bytes = E + RP + mask + Q + 2.0 * Srho; break;
      case VMR_KERNEL_RHO_ELBO: *bytes = E + RP + mask + Q + 2.0 * Srho; break;
      default: *bytes = 0.0; break;
    }
    return VMR_OK;
  }
  switch (kernel_class) {
    case VMR_KERNEL_GAMMA_MASK: *bytes = SR + Srho; break;
    case VMR_KERNEL_GAMMA_COUNTS: *bytes = SX + Srho; break;   // statistics pass (once per realisation)
    case VMR_KERNEL_PHI: *bytes = 0.0; break;                  // no pass of its own: phi_shp comes from H
    case VMR_KERNEL_RHO: *bytes = SX + SR + 2.0 * Srho; break;
    case VMR_KERNEL_ELBO: *bytes = SX + SR + 2.0 * Srho; break;
    case VMR_KERNEL_RHO_ELBO: *bytes = SX + SR + 2.0 * Srho; break;
    default: *bytes = 0.0; break;
  }
  return VMR_OK;
}

}  // extern "C"
