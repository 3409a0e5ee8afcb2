// mixing.hip -- mixing by node attribute and overlap between layers of the posterior on the device: vmr_sample_mixing,
// vmr_expected_mixing.
//
// The other read-outs treat the nodes as unlabelled and every layer on its own.  Given a group code per node (g_i in [0, C), -1:
// the node is left out) vmr_sample_mixing draws S posterior samples of Y in chunks (sampled_side.h: sample s is what
// vmr_sample(h, seed + s, n_trials) writes) and returns, per sample,
//     mix[l][a][b]     #{(i,j) : g_i = a, g_j = b, Y_lij > 0}                    the mixing matrix of layer l
//     mutual[l][a][b]  #{(i,j) : g_i = a, g_j = b, Y_lij > 0 and Y_lji > 0}      its reciprocated part (ordered pairs)
//     overlap[l][l']   #{(i,j) : Y_lij > 0 and Y_l'ij > 0}                       over ALL nodes, labelled or not
// (include/vimure_hip.h has the contract).
//
// Layout.  A chunk's Y[c][L][N][N] bytes are reduced in natural order by k_mix_reduce, one workgroup (4 waves) per (strip of 64
// rows, sample) -- the strip walk of sampled_side.h with the layer loop INSIDE the tile loop, so the L bytes of one tie meet in one
// thread, which keeps them as a bit mask per row (L <= 32) -- a ballot per layer and a popcount per pair of layers give the
// overlap.  The transposed tile of a layer is loaded for `mutual` only.  The group codes (int8) of the strip's rows sit in LDS for
// the whole walk, the code of a lane's column in a register for the tile.  The counters are 32-bit words of the workgroup's LDS -- mix and mutual of LB layers at a
// time ([LB][C][C] each, MIX_LDS_BINS bytes at most: the walk is repeated per round of LB layers, only the first round reads every
// layer and forms the overlap), then [L][L].  A row's edges reach them by one LDS atomic instruction per (row, layer): per tile
// lane b < C keeps the ballot of the columns of group b, the row's ballot of edges ANDed with it and popcounted is what lane b adds
// to bin (g_row, b) -- a bin per lane, so no two lanes of the instruction meet, and never more adds than the row has edges
// (samples are sparse: a few edges per row of 64 ties; rows without an edge add nothing).  The non-zero counters are flushed with
// 64-bit global atomics: sums of integers, the same from run to run in any order.
// A chunk's Y is read once or, with `mutual`, twice per round.
//
// vmr_expected_mixing: the same tables in expectation under q(Y) = prod rho.  P comes from ns_exp_p; the host sorts the labelled
// nodes by group (order, goff: group b is order[goff[b] .. goff[b + 1]), ascending node), so that one wave per (row, layer) sums
// the row's columns group by group -- a fixed lane stride and a fixed shuffle tree per group -- into Rw[l][i][b], and one thread
// per (l, a, b) adds the rows of group a in ascending i.  The overlap: one wave per row and a pair of layers at a time, then one
// thread per pair over the rows in ascending i.  No atomics, grids of N, L and C only: bit-identical from run to run.
#include "sampled_side.h"

namespace {

#define MIX_LDS_BINS (40 << 10)   // bytes of mix / mutual counters a workgroup keeps in LDS at most: the layers of one round

// One workgroup per (strip bi of 64 rows, sample s).  group: int8 [N] or null (no mix, no mutual); mixg / mutg: [c][L][C][C],
// ovg: [c][L][L], any of them null.  LB: layers per round (L when there are no group tables).  MUT: mutg is asked for.
template <bool MUT>
__global__ __launch_bounds__(256) void k_mix_reduce(const uint8_t* __restrict__ Y, const int8_t* __restrict__ group, int N, int L, int C, int LB, int skip,
                                                    u64* __restrict__ mixg, u64* __restrict__ mutg, u64* __restrict__ ovg) {
  extern __shared__ unsigned bins_s[];   // [LB][C][C] mix, [LB][C][C] mutual (each when asked for), [L][L] overlap (when asked for)
  __shared__ uint8_t Bs[MUT ? SS_TILE * SS_BSTRIDE : 4];
  __shared__ int gi_s[SS_TILE];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int bi = blockIdx.x, s = blockIdx.y;
  const size_t T = (size_t)N * N;
  const uint8_t* Ys = Y + (size_t)s * L * T;
  const int i0 = bi * SS_TILE, nb = (N + SS_TILE - 1) / SS_TILE, C2 = C * C;
  const bool grp_any = mixg != nullptr || (MUT && mutg != nullptr);
  unsigned* mixb = mixg ? bins_s : nullptr;
  unsigned* mutb = bins_s + (mixg ? LB * C2 : 0);
  const int ngrp = grp_any ? ((mixg ? 1 : 0) + (MUT ? 1 : 0)) * LB * C2 : 0;
  unsigned* ovb = bins_s + ngrp;
  if (threadIdx.x < SS_TILE) gi_s[threadIdx.x] = (grp_any && i0 + (int)threadIdx.x < N) ? (int)group[i0 + threadIdx.x] : -1;
  if (ovg)
    for (int q = threadIdx.x; q < L * L; q += 256) ovb[q] = 0u;
  for (int l0 = 0; l0 < L; l0 += LB) {
    const int l1 = l0 + LB < L ? l0 + LB : L;
    const bool ov = ovg != nullptr && l0 == 0;   // the first round reads every layer of a tie
    for (int q = threadIdx.x; q < ngrp; q += 256) bins_s[q] = 0u;
    __syncthreads();
    for (int bj = 0; bj < nb; ++bj) {
      const int j0 = bj * SS_TILE, j = j0 + lane;
      const int gc = (grp_any && j < N) ? (int)group[j] : -1;
      u64 cmv = 0ull;   // lane b < C: the tile's columns of group b (a column out of range or left out is in no group)
      for (int b = 0; b < C; ++b) {
        const u64 mb = __ballot(gc == b);
        if (lane == b) cmv = mb;
      }
      unsigned m[SS_TILE / 4];   // bit l of m[it]: tie (row 4 it + w, column lane) is an edge of layer l
#pragma unroll
      for (int it = 0; it < SS_TILE / 4; ++it) m[it] = 0u;
      for (int l = ov ? 0 : l0; l < (ov ? L : l1); ++l) {
        const uint8_t* Yl = Ys + (size_t)l * T;
        const bool grp = grp_any && l >= l0 && l < l1;   // (uniform over the workgroup)
        if (MUT && grp) {
          __syncthreads();   // (the last tile's reads of Bs are done)
          tile_transposed(Bs, Yl, i0, j0, N);
          __syncthreads();
        }
#pragma unroll
        for (int it = 0; it < SS_TILE / 4; ++it) {
          const int r = it * 4 + w, i = i0 + r;
          const bool in = i < N && j < N && !(skip && i == j);
          const bool a = in && Yl[(size_t)i * N + j] > 0;
          m[it] |= (unsigned)a << (l & 31);
          const u64 ba = __ballot(a);   // the row's edges in this tile
          const int gr = gi_s[r];
          if (grp && gr >= 0 && ba) {   // (uniform over the wave) lane b adds the row's edges into group b: one bin per lane
            const int q = (l - l0) * C2 + gr * C + lane;
            const unsigned n = (unsigned)__popcll(ba & cmv);
            if (mixb && n) atomicAdd(&mixb[q], n);
            if (MUT) {
              const u64 bm = __ballot(a && Bs[lane * SS_BSTRIDE + r] > 0);   // Y[j][i] > 0: in range, and off the skipped diagonal, as a is
              const unsigned nm = (unsigned)__popcll(bm & cmv);
              if (nm) atomicAdd(&mutb[q], nm);
            }
          }
        }
      }
      if (ov) {
#pragma unroll
        for (int it = 0; it < SS_TILE / 4; ++it) {
          if (!__ballot(m[it] != 0u)) continue;   // (uniform over the wave) no edge in this row of the tile, in any layer
          for (int l = 0; l < L; ++l) {
            const u64 bl = __ballot((m[it] >> l) & 1u);
            if (!bl) continue;
            for (int l2 = l; l2 < L; ++l2) {
              const unsigned c = (unsigned)__popcll(bl & __ballot((m[it] >> l2) & 1u));
              if (c && lane == 0) {
                atomicAdd(&ovb[l * L + l2], c);
                if (l2 != l) atomicAdd(&ovb[l2 * L + l], c);
              }
            }
          }
        }
      }
    }
    __syncthreads();
    const size_t o = ((size_t)s * L + l0) * C2;
    if (mixg) flush_bins(mixb, mixg + o, (l1 - l0) * C2, 256);
    if (MUT && mutg) flush_bins(mutb, mutg + o, (l1 - l0) * C2, 256);
    __syncthreads();   // (the next round zeroes the counters)
  }
  if (ovg) flush_bins(ovb, ovg + (size_t)s * L * L, L * L, 256);
}

// ------------------------------------------------------------------------------------------
// expectations
// ------------------------------------------------------------------------------------------

// One wave per (row i = 4 blockIdx.x + wave, layer blockIdx.y), rows of labelled nodes only: over the columns of group b, in
// the order of `order` with a lane stride of 64 and one shuffle tree, Rw[l][i][b] = sum p_ij and Rm[l][i][b] = sum p_ij p_ji
// (Rm may be null).
__global__ __launch_bounds__(256) void k_mix_exp_rows(const double* __restrict__ P, int N, int C, const int32_t* __restrict__ order,
                                                      const int32_t* __restrict__ goff, const int8_t* __restrict__ group, int skip,
                                                      double* __restrict__ Rw, double* __restrict__ Rm) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6), l = blockIdx.y;
  if (i >= N || group[i] < 0) return;   // (the same in every lane of the wave)
  const double* Pl = P + (size_t)l * N * N;
  for (int b = 0; b < C; ++b) {
    double sw = 0.0, sm = 0.0;
    for (int q = goff[b] + lane; q < goff[b + 1]; q += 64) {
      const int j = order[q];
      if (skip && j == i) continue;
      const double p = Pl[(size_t)i * N + j];
      sw += p;
      if (Rm) sm += p * Pl[(size_t)j * N + i];
    }
    sw = wave_sum(sw);
    if (Rm) sm = wave_sum(sm);
    if (lane == 0) {
      const size_t o = ((size_t)l * N + i) * C + b;
      Rw[o] = sw;
      if (Rm) Rm[o] = sm;
    }
  }
}

// one thread per (l, a, b): the rows of group a in ascending i
__global__ __launch_bounds__(256) void k_mix_exp_groups(const double* __restrict__ Rw, const double* __restrict__ Rm, int N, int L, int C,
                                                        const int32_t* __restrict__ order, const int32_t* __restrict__ goff, double* __restrict__ mix,
                                                        double* __restrict__ mut) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= L * C * C) return;
  const int l = t / (C * C), a = (t - l * C * C) / C, b = t - l * C * C - a * C;
  double sw = 0.0, sm = 0.0;
  for (int q = goff[a]; q < goff[a + 1]; ++q) {
    const size_t o = ((size_t)l * N + order[q]) * C + b;
    sw += Rw[o];
    if (Rm) sm += Rm[o];
  }
  if (mix) mix[t] = sw;
  if (mut) mut[t] = sm;
}

// One wave per row i = 4 blockIdx.x + wave, a pair of layers l <= l2 at a time: Ro[i][l][l2] = sum_j p_lij p_l2ij, sum_j p_lij
// for l2 = l (the upper triangle only).
__global__ __launch_bounds__(256) void k_mix_exp_ov_rows(const double* __restrict__ P, int N, int L, int skip, double* __restrict__ Ro) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;   // (the same in every lane of the wave)
  const size_t T = (size_t)N * N;
  for (int l = 0; l < L; ++l)
    for (int l2 = l; l2 < L; ++l2) {
      const double* Pa = P + (size_t)l * T + (size_t)i * N;
      const double* Pb = P + (size_t)l2 * T + (size_t)i * N;
      double sv = 0.0;
      for (int j = lane; j < N; j += 64) {
        if (skip && j == i) continue;
        sv += l2 == l ? Pa[j] : Pa[j] * Pb[j];
      }
      sv = wave_sum(sv);
      if (lane == 0) Ro[((size_t)i * L + l) * L + l2] = sv;
    }
}

// one thread per pair l <= l2: the rows in ascending i; both halves of the table get the same double
__global__ __launch_bounds__(256) void k_mix_exp_ov(const double* __restrict__ Ro, int N, int L, double* __restrict__ ov) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= L * L) return;
  const int l = t / L, l2 = t - l * L;
  if (l2 < l) return;
  double sv = 0.0;
  for (int i = 0; i < N; ++i) sv += Ro[((size_t)i * L + l) * L + l2];
  ov[l * L + l2] = sv;
  ov[l2 * L + l] = sv;
}

// what both calls refuse of their arguments (fn: the call's name), or VMR_OK
int mix_check_args(vmr_ctx* h, const char* fn, const int32_t* group, int C, bool want_grp, bool want_ov) {
  char msg[256];
  if (!want_grp && !want_ov) {
    snprintf(msg, sizeof msg, "%s: mix, mutual and overlap are all NULL", fn);
    return fail(h, VMR_EINVAL, msg);
  }
  if (want_grp) {
    if (C < 1 || C > VMR_MIX_CMAX) {
      snprintf(msg, sizeof msg, "%s: C = %d, the groups of mix and mutual are 1 to %d", fn, C, VMR_MIX_CMAX);
      return fail(h, VMR_EINVAL, msg);
    }
    if (!group) {
      snprintf(msg, sizeof msg, "%s: group is NULL while mix or mutual is asked for", fn);
      return fail(h, VMR_EINVAL, msg);
    }
    for (int i = 0; i < h->g.N; ++i)
      if (group[i] < -1 || group[i] >= C) {
        snprintf(msg, sizeof msg, "%s: group[%d] = %d is outside [-1, C = %d)", fn, i, (int)group[i], C);
        return fail(h, VMR_EINVAL, msg);
      }
  }
  if (want_ov && h->g.L > VMR_MIX_LMAX) {
    snprintf(msg, sizeof msg, "%s: overlap takes %d layers at most, the handle has L = %d", fn, VMR_MIX_LMAX, h->g.L);
    return fail(h, VMR_EINVAL, msg);
  }
  return VMR_OK;
}

}  // namespace

extern "C" int vmr_sample_mixing(vmr_handle h, uint64_t seed, int n_samples, int n_trials, const int32_t* group, int C, int skip_diagonal,
                                 uint64_t* mix, uint64_t* mutual, uint64_t* overlap) {
  const bool want_grp = mix || mutual;
  int rc;
  if ((rc = sampled_counts(h, "vmr_sample_mixing", n_samples, n_trials)) ||
      (rc = mix_check_args(h, "vmr_sample_mixing", group, C, want_grp, overlap != nullptr)) || (rc = expected_begin(h, "vmr_sample_mixing")))
    return rc;
  const Geo& g = h->g;
  if (!want_grp) C = 0;
  const size_t ties = (size_t)g.L * g.N * g.N, C2 = (size_t)C * C, grp_b = (size_t)g.L * C2 * 8, ov_b = (size_t)g.L * g.L * 8;
  SampledOut out[3] = {{mix, grp_b, true, "vmr_sample_mixing: the mixing counts"},
                       {mutual, grp_b, true, "vmr_sample_mixing: the mutual counts"},
                       {overlap, ov_b, true, "vmr_sample_mixing: the overlap counts"}};
  const size_t per = ties + (mix ? grp_b : 0) + (mutual ? grp_b : 0) + (overlap ? ov_b : 0);   // device bytes per sample of a chunk
  size_t S;
  if ((rc = chunk_samples(h, "vmr_sample_mixing", (size_t)n_samples, per, 0, &S))) return rc;
  std::vector<int8_t> codes;   // (outlives the temporaries: their release waits for the copy)
  Tmp tm(h);
  uint8_t* Y = nullptr;
  int8_t* gd = nullptr;
  if ((rc = tm.get(&Y, S * ties, "vmr_sample_mixing: the samples"))) return rc;
  if (want_grp) {
    codes.assign(group, group + g.N);
    if ((rc = tm.get(&gd, (size_t)g.N, "vmr_sample_mixing: the group codes"))) return rc;
    HIPCHK(h, hipMemcpyAsync(gd, codes.data(), (size_t)g.N, hipMemcpyHostToDevice, h->stream));
  }
  // layers whose mix / mutual counters a workgroup holds at once, and its LDS words
  const size_t grp_w = ((mix ? 1 : 0) + (mutual ? 1 : 0)) * C2;
  const int LB = want_grp ? (int)std::max<size_t>(1, std::min<size_t>((size_t)g.L, MIX_LDS_BINS / (grp_w * 4))) : g.L;
  const size_t smem = ((want_grp ? (size_t)LB * grp_w : 0) + (overlap ? (size_t)g.L * g.L : 0)) * 4;
  const unsigned nstrip = (unsigned)((g.N + SS_TILE - 1) / SS_TILE);
  const auto kern = mutual ? k_mix_reduce<true> : k_mix_reduce<false>;
  return sampled_chunks(h, tm, (size_t)n_samples, S, seed, n_trials, Y, out, [&](size_t, int c) -> int {
    hipLaunchKernelGGL(kern, dim3(nstrip, (unsigned)c), dim3(256), smem, h->stream, Y, gd, g.N, g.L, C, LB,
                       skip_diagonal != 0, out[0].as<u64>(), out[1].as<u64>(), out[2].as<u64>());
    HIPCHK(h, hipGetLastError());
    return VMR_OK;
  });
}

extern "C" int vmr_expected_mixing(vmr_handle h, const int32_t* group, int C, int skip_diagonal, double* mix, double* mutual, double* overlap) {
  if (!h) return VMR_EINVAL;
  const bool want_grp = mix || mutual;
  int rc;
  if ((rc = mix_check_args(h, "vmr_expected_mixing", group, C, want_grp, overlap != nullptr)) || (rc = expected_begin(h, "vmr_expected_mixing"))) return rc;
  const Geo& g = h->g;
  if (!want_grp) C = 0;
  const size_t T = (size_t)g.N * g.N, ties = (size_t)g.L * T, C2 = (size_t)C * C;
  const int nbp = exp_p_blocks(T);
  const int skip = skip_diagonal != 0;
  const unsigned nquad = (unsigned)((g.N + 3) / 4);
  std::vector<int8_t> codes;   // (these outlive the temporaries: their release waits for the copies)
  std::vector<int32_t> order, goff;
  Tmp tm(h);
  double *P = nullptr, *wpart = nullptr;
  if ((rc = tm.get(&P, ties * 8, "vmr_expected_mixing: the edge probabilities")) ||
      (rc = tm.get(&wpart, (size_t)g.L * nbp * 32, "vmr_expected_mixing: partial sums")))
    return rc;
  if ((rc = ns_exp_p(h, P, wpart, nbp))) return rc;
  if (want_grp) {   // the labelled nodes sorted by group, ascending node inside a group
    codes.assign(group, group + g.N);
    goff.assign((size_t)C + 1, 0);
    for (int i = 0; i < g.N; ++i)
      if (group[i] >= 0) ++goff[group[i] + 1];
    for (int b = 0; b < C; ++b) goff[b + 1] += goff[b];
    order.assign((size_t)std::max(1, goff[C]), 0);
    std::vector<int32_t> at(goff.begin(), goff.end() - 1);
    for (int i = 0; i < g.N; ++i)
      if (group[i] >= 0) order[at[group[i]]++] = i;
    int8_t* gd = nullptr;
    int32_t *ordd = nullptr, *goffd = nullptr;
    double *Rw = nullptr, *Rm = nullptr, *md = nullptr, *ud = nullptr;
    const size_t rows_b = (size_t)g.L * g.N * C * 8, out_b = (size_t)g.L * C2 * 8;
    if ((rc = tm.get(&gd, (size_t)g.N, "vmr_expected_mixing: the group codes")) ||
        (rc = tm.get(&ordd, order.size() * 4, "vmr_expected_mixing: the nodes by group")) ||
        (rc = tm.get(&goffd, goff.size() * 4, "vmr_expected_mixing: the groups' offsets")) ||
        (rc = tm.get(&Rw, rows_b, "vmr_expected_mixing: the rows' sums")) || (mutual && (rc = tm.get(&Rm, rows_b, "vmr_expected_mixing: the rows' sums"))) ||
        (mix && (rc = tm.get(&md, out_b, "vmr_expected_mixing: the result"))) || (mutual && (rc = tm.get(&ud, out_b, "vmr_expected_mixing: the result"))))
      return rc;
    HIPCHK(h, hipMemcpyAsync(gd, codes.data(), (size_t)g.N, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(ordd, order.data(), order.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(goffd, goff.data(), goff.size() * 4, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_mix_exp_rows, dim3(nquad, (unsigned)g.L), dim3(256), 0, h->stream, P, g.N, C, ordd, goffd, gd, skip, Rw, Rm);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_mix_exp_groups, dim3(grid_for((size_t)g.L * C2)), dim3(256), 0, h->stream, Rw, Rm, g.N, g.L, C, ordd, goffd, md, ud);
    HIPCHK(h, hipGetLastError());
    if (mix) HIPCHK(h, hipMemcpyAsync(mix, md, out_b, hipMemcpyDeviceToHost, h->stream));
    if (mutual) HIPCHK(h, hipMemcpyAsync(mutual, ud, out_b, hipMemcpyDeviceToHost, h->stream));
  }
  if (overlap) {
    double *Ro = nullptr, *od = nullptr;
    const size_t ov_b = (size_t)g.L * g.L * 8;
    if ((rc = tm.get(&Ro, (size_t)g.N * ov_b, "vmr_expected_mixing: the rows' sums")) || (rc = tm.get(&od, ov_b, "vmr_expected_mixing: the result"))) return rc;
    hipLaunchKernelGGL(k_mix_exp_ov_rows, dim3(nquad), dim3(256), 0, h->stream, P, g.N, g.L, skip, Ro);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_mix_exp_ov, dim3(grid_for((size_t)g.L * g.L)), dim3(256), 0, h->stream, Ro, g.N, g.L, od);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(overlap, od, ov_b, hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return VMR_OK;
}
