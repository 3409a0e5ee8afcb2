// triads.hip -- triad statistics of the posterior on the device: vmr_sample_triads, vmr_expected_triads.
//
// vmr_sample_stats (netstats.hip) stops at dyads; what measurement error distorts most is the triadic structure -- a missed or
// invented tie opens or closes up to N - 2 triads.  vmr_sample_triads draws S posterior samples of Y in chunks (sampled_side.h: sample
// s is what vmr_sample(h, seed + s, n_trials) writes) and returns per sample and layer, for A = (Y > 0) with the diagonal cleared
// and U = A | A^T:  transitive, cyclic, two_paths, triangles_u, wedges_u, edges_u (include/vimure_hip.h has the definitions) and,
// per node, the triangles of U through it and its degree in U.
//
// Layout.  A chunk's Y[c][L][N][N] bytes are packed into the bit rows Aout and Ain (sampled_side.h has the layout) by k_tri_pack,
// the strip walk of sampled_side.h: a wave's ballot over 64 consecutive bytes of a row is one word of Aout, the transposed tile
// gives the word of Ain.
// k_tri_count: one wave per (node i, layer, sample).  It lists the neighbours of i in U (block of TRI_BLK words at a time: a
// wave scan of the words' popcounts gives every lane its place in the wave's LDS list), then walks the list 64 / G neighbours per
// step, G = the largest power of two <= min(W, 64) lanes striding over the W words of a neighbour's rows:
//     j in out(i):  popc(Aout_i & Aout_j)  -> transitive  (k with i->k, j->k),   popc(Ain_i & Aout_j) -> cyclic (k with k->i, j->k)
//     j in U(i):    popc(U_i & U_j)        -> 2 node_tri[i],                      U = Aout | Ain formed on the fly
// and two_paths, wedges_u, edges_u come from the popcounts of row i.  Lanes reduce once at the end; LDS atomics, then one 64-bit
// global atomic per workgroup and statistic -- sums of integers, the same from run to run in any order.
//
// vmr_expected_triads: the same six in expectation under q(Y) = prod rho.  P (k_ns_exp_p through ns_exp_p, diagonal zeroed) and
// U (u_ij = 1 - (1 - p_ij)(1 - p_ji)) are written once; k_tri_exp_prod is a tiled FP64 product whose output is never stored:
// the workgroup of output tile (I, K) accumulates its 64 x 64 tiles of P P^T, P P and U U over j in registers (4 x 4 per thread,
// operands in LDS), multiplies them into P_ik, P_ki and U_ik and reduces, together with the tile's elementwise sums.  Per-workgroup
// partials on a grid that depends on N only, one workgroup per layer to finish in a fixed order -- no floating-point atomics.
#include "sampled_side.h"

namespace {

#define TRI_BLK 32       // words of row i whose neighbours are listed at a time
#define TRI_LIST (TRI_BLK * 64)

// One workgroup (4 waves) per (strip bi of 64 rows, layer l, sample s).  For every column tile bj wave w takes rows r = 4 it + w
// with lane = column c: ballot(Y[i0 + r][j0 + c] > 0) is word bj of Aout's row, ballot(Y[j0 + c][i0 + r] > 0), read from the
// transposed tile in LDS, word bj of Ain's row; lane `it` keeps the two words of row 4 it + w and stores them.  Out of range reads
// as 0, so do the diagonal elements: the pad bits and the diagonal bit are zero.
__global__ __launch_bounds__(256) void k_tri_pack(const uint8_t* __restrict__ Y, int N, int L, int W, unsigned long long* __restrict__ Aout,
                                                  unsigned long long* __restrict__ Ain) {
  __shared__ uint8_t Bs[SS_TILE * SS_BSTRIDE];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int bi = blockIdx.x, l = blockIdx.y, s = blockIdx.z;
  const size_t T = (size_t)N * N, sl = (size_t)s * L + l;
  const uint8_t* Ys = Y + sl * T;
  const int i0 = bi * SS_TILE;
  for (int bj = 0; bj < W; ++bj) {
    const int j0 = bj * SS_TILE;
    __syncthreads();   // (the last tile's reads of Bs are done)
    tile_transposed(Bs, Ys, i0, j0, N);
    __syncthreads();
    const int j = j0 + lane;
    unsigned long long wo = 0ull, wi = 0ull;
    for (int it = 0; it < SS_TILE / 4; ++it) {
      const int r = it * 4 + w, i = i0 + r;
      const bool in = i < N && j < N && i != j;
      const unsigned a = in ? Ys[(size_t)i * N + j] : 0u;
      const unsigned b = in ? Bs[lane * SS_BSTRIDE + r] : 0u;
      const unsigned long long ba = __ballot(a > 0u), bb = __ballot(b > 0u);
      if (lane == it) { wo = ba; wi = bb; }
    }
    if (lane < SS_TILE / 4) {
      const int i = i0 + lane * 4 + w;
      if (i < N) {
        const size_t o = (sl * N + i) * W + bj;
        Aout[o] = wo;
        Ain[o] = wi;
      }
    }
  }
}

// One wave per (node i = 4 blockIdx.x + wave, layer, sample); G = 1 << lG lanes per neighbour, 64 / G neighbours per step.
// counts[s][l]: 0 transitive, 1 cyclic, 2 two_paths, 3 sum_i 2 node_tri[i] (= 6 triangles), 4 wedges, 5 sum_i d_i (= 2 edges);
// the host divides columns 3 and 5.
__global__ __launch_bounds__(256) void k_tri_count(const unsigned long long* __restrict__ Aout, const unsigned long long* __restrict__ Ain, int N, int L,
                                                   int W, int lG, unsigned long long* __restrict__ counts, int32_t* __restrict__ node_tri,
                                                   int32_t* __restrict__ node_deg) {
  __shared__ unsigned short list_s[4][TRI_LIST];
  __shared__ unsigned long long tot[VMR_TRIAD_NSTAT];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wv, l = blockIdx.y, s = blockIdx.z;
  const size_t sl = (size_t)s * L + l;
  const int G = 1 << lG, nps = 64 >> lG, sub = lane >> lG, wl = lane & (G - 1);
  unsigned short* list = list_s[wv];
  if (threadIdx.x < VMR_TRIAD_NSTAT) tot[threadIdx.x] = 0ull;
  __syncthreads();
  if (i < N) {   // (the same in every lane of the wave)
    const unsigned long long* Ao = Aout + sl * N * W;
    const unsigned long long* Ai = Ain + sl * N * W;
    const unsigned long long* ao_i = Ao + (size_t)i * W;
    const unsigned long long* ai_i = Ai + (size_t)i * W;
    unsigned dout = 0, din = 0, mut = 0, deg = 0;
    for (int w = lane; w < W; w += 64) {
      const unsigned long long a = ao_i[w], b = ai_i[w];
      dout += (unsigned)__popcll(a); din += (unsigned)__popcll(b); mut += (unsigned)__popcll(a & b); deg += (unsigned)__popcll(a | b);
    }
    const bool one = W <= G;   // (W a power of two up to 64) a lane meets one word of a row only: row i's stay in registers
    const unsigned long long aoi1 = (one && wl < W) ? ao_i[wl] : 0ull, aii1 = (one && wl < W) ? ai_i[wl] : 0ull;
    unsigned long long trans = 0, cyc = 0, tri2 = 0;   // per lane
    for (int wb = 0; wb < W; wb += TRI_BLK) {
      const int w = wb + lane;
      unsigned long long a = 0ull, b = 0ull;
      if (lane < TRI_BLK && w < W) { a = ao_i[w]; b = ai_i[w]; }
      unsigned long long u = a | b;
      const unsigned c = (unsigned)__popcll(u);
      unsigned inc = c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
      const int n = __builtin_amdgcn_readfirstlane((int)__shfl(inc, 63, 64));   // neighbours in this block of words, <= TRI_LIST
      unsigned off = inc - c;
      wave_sync();   // (the walk of the last block is done with the list)
      while (u) {
        const int bit = __ffsll((long long)u) - 1;
        list[off++] = (unsigned short)((lane * 64 + bit) | (int)((a >> bit) & 1ull) << 15);   // bit 15: j is in out(i)
        u &= u - 1ull;
      }
      wave_sync();
      for (int t = 0; t < n; t += nps) {
        const int idx = t + sub;
        if (idx < n) {
          const unsigned e = list[idx];
          const int j = wb * 64 + (int)(e & 0x7fffu);   // < N: the pad bits are zero
          const bool isout = (e >> 15) != 0u;
          const unsigned long long* ao_j = Ao + (size_t)j * W;
          const unsigned long long* ai_j = Ai + (size_t)j * W;
          if (one) {
            if (wl < W) {
              const unsigned long long aoj = ao_j[wl], aij = ai_j[wl];
              tri2 += (unsigned)__popcll((aoi1 | aii1) & (aoj | aij));
              if (isout) { trans += (unsigned)__popcll(aoi1 & aoj); cyc += (unsigned)__popcll(aii1 & aoj); }
            }
          } else {
            for (int ww = wl; ww < W; ww += G) {
              const unsigned long long aoi = ao_i[ww], aii = ai_i[ww], aoj = ao_j[ww], aij = ai_j[ww];
              tri2 += (unsigned)__popcll((aoi | aii) & (aoj | aij));
              if (isout) { trans += (unsigned)__popcll(aoi & aoj); cyc += (unsigned)__popcll(aii & aoj); }
            }
          }
        }
      }
    }
    trans = wave_sum_ull(trans); cyc = wave_sum_ull(cyc); tri2 = wave_sum_ull(tri2);
    const unsigned long long so = wave_sum_ull(dout), si = wave_sum_ull(din), sm = wave_sum_ull(mut), sd = wave_sum_ull(deg);
    if (lane == 0) {
      const unsigned long long two = si * so - sm, wedges = sd * (sd - (sd ? 1ull : 0ull)) / 2ull;
      if (trans) atomicAdd(&tot[0], trans);
      if (cyc) atomicAdd(&tot[1], cyc);
      if (two) atomicAdd(&tot[2], two);
      if (tri2) atomicAdd(&tot[3], tri2);
      if (wedges) atomicAdd(&tot[4], wedges);
      if (sd) atomicAdd(&tot[5], sd);
      if (node_tri) node_tri[sl * N + i] = (int32_t)(tri2 / 2ull);
      if (node_deg) node_deg[sl * N + i] = (int32_t)sd;
    }
  }
  __syncthreads();
  if (threadIdx.x < VMR_TRIAD_NSTAT && tot[threadIdx.x]) atomicAdd(counts + sl * VMR_TRIAD_NSTAT + threadIdx.x, tot[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------
// expectations
// ------------------------------------------------------------------------------------------

// U[l][i][j] = 1 - (1 - p_ij)(1 - p_ji) off the diagonal (bitwise symmetric: the product commutes), 0 on it; P's diagonal is
// zeroed in place (only the thread of (i, i) reads or writes P_ii)
__global__ __launch_bounds__(256) void k_tri_exp_u(double* __restrict__ P, double* __restrict__ U, int N) {
  const int l = blockIdx.y;
  const size_t T = (size_t)N * N;
  double* Pl = P + (size_t)l * T;
  double* Ul = U + (size_t)l * T;
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < T; t += (size_t)gridDim.x * 256) {
    const size_t i = t / N, j = t - i * N;
    if (i == j) { Pl[t] = 0.0; Ul[t] = 0.0; }
    else Ul[t] = 1.0 - (1.0 - Pl[t]) * (1.0 - Pl[j * N + i]);
  }
}

#define TE_T 64     // output tile edge
#define TE_J 16     // j per LDS stage
#define TE_S 66     // doubles per LDS row: 16-byte aligned, and the transposed stores of a wave spread over the banks
#define TE_NPART 8  // partial sums per workgroup

// Output tile (I, K) = (blockIdx.x / nt, blockIdx.x % nt) of layer blockIdx.y; thread (ty, tx) = (tid / 16, tid % 16) holds
// rows i = 4 ty + a and columns k = 4 tx + b.  Per stage of TE_J values of j, in LDS as [jj][.]:
//   PI[jj][i] = p_ij   PK[jj][k] = p_kj   PJ[jj][k] = p_jk   UI[jj][i] = u_ji = u_ij   UK[jj][k] = u_jk
//   c1 += p_ij p_kj  (P P^T)_ik     c2 += p_ij p_jk  (P P)_ik     c3 += u_ij u_jk  (U U)_ik
// and at the end, over the tile: part = (sum c1 p_ik, sum c2 p_ki, sum c2, sum p_ik p_ki, sum c3 u_ik, sum c3, sum u_ik^2,
// sum_{i<k} u_ik).  Out of range loads as 0.
__global__ __launch_bounds__(256) void k_tri_exp_prod(const double* __restrict__ P, const double* __restrict__ U, int N, int nt,
                                                      double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double PI[TE_J * TE_S], PK[TE_J * TE_S], PJ[TE_J * TE_S], UI[TE_J * TE_S], UK[TE_J * TE_S];
  __shared__ double red[16];
  const int tid = threadIdx.x, l = blockIdx.y;
  const int I = blockIdx.x / nt, K = blockIdx.x - I * nt;
  const int i0 = I * TE_T, k0 = K * TE_T;
  const int ty = tid >> 4, tx = tid & 15;
  const size_t T = (size_t)N * N;
  const double* Pl = P + (size_t)l * T;
  const double* Ul = U + (size_t)l * T;
  double c1[4][4], c2[4][4], c3[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) { c1[a][b] = 0.0; c2[a][b] = 0.0; c3[a][b] = 0.0; }
  for (int j0 = 0; j0 < N; j0 += TE_J) {
    __syncthreads();   // (the last stage's reads are done)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      {   // rows of P across j: element (x, jj) of the tile rows i0 + x and k0 + x
        const int jj = tid & 15, x = (tid >> 4) + 16 * q, j = j0 + jj;
        PI[jj * TE_S + x] = (i0 + x < N && j < N) ? Pl[(size_t)(i0 + x) * N + j] : 0.0;
        PK[jj * TE_S + x] = (k0 + x < N && j < N) ? Pl[(size_t)(k0 + x) * N + j] : 0.0;
      }
      {   // rows j across the tile's columns
        const int x = tid & 63, jj = (tid >> 6) + 4 * q, j = j0 + jj;
        PJ[jj * TE_S + x] = (k0 + x < N && j < N) ? Pl[(size_t)j * N + k0 + x] : 0.0;
        UK[jj * TE_S + x] = (k0 + x < N && j < N) ? Ul[(size_t)j * N + k0 + x] : 0.0;
        UI[jj * TE_S + x] = (i0 + x < N && j < N) ? Ul[(size_t)j * N + i0 + x] : 0.0;
      }
    }
    __syncthreads();
#pragma unroll 4
    for (int jj = 0; jj < TE_J; ++jj) {
      double pi[4], pk[4], pj[4], ui[4], uk[4];
#pragma unroll
      for (int a = 0; a < 4; a += 2) {
        const double2 v0 = *reinterpret_cast<const double2*>(&PI[jj * TE_S + 4 * ty + a]);
        const double2 v1 = *reinterpret_cast<const double2*>(&PK[jj * TE_S + 4 * tx + a]);
        const double2 v2 = *reinterpret_cast<const double2*>(&PJ[jj * TE_S + 4 * tx + a]);
        const double2 v3 = *reinterpret_cast<const double2*>(&UI[jj * TE_S + 4 * ty + a]);
        const double2 v4 = *reinterpret_cast<const double2*>(&UK[jj * TE_S + 4 * tx + a]);
        pi[a] = v0.x; pi[a + 1] = v0.y; pk[a] = v1.x; pk[a + 1] = v1.y; pj[a] = v2.x; pj[a + 1] = v2.y;
        ui[a] = v3.x; ui[a + 1] = v3.y; uk[a] = v4.x; uk[a + 1] = v4.y;
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          c1[a][b] = fma(pi[a], pk[b], c1[a][b]);
          c2[a][b] = fma(pi[a], pj[b], c2[a][b]);
          c3[a][b] = fma(ui[a], uk[b], c3[a][b]);
        }
    }
  }
  double acc[TE_NPART];
#pragma unroll
  for (int c = 0; c < TE_NPART; ++c) acc[c] = 0.0;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int i = i0 + 4 * ty + a, k = k0 + 4 * tx + b;
      if (i < N && k < N) {
        const double pik = Pl[(size_t)i * N + k], pki = Pl[(size_t)k * N + i], uik = Ul[(size_t)i * N + k];
        acc[0] += c1[a][b] * pik;
        acc[1] += c2[a][b] * pki;
        acc[2] += c2[a][b];
        acc[3] += pik * pki;
        acc[4] += c3[a][b] * uik;
        acc[5] += c3[a][b];
        acc[6] += uik * uik;
        if (i < k) acc[7] += uik;
      }
    }
  double* o = part + ((size_t)l * gridDim.x + blockIdx.x) * TE_NPART;
#pragma unroll
  for (int c = 0; c < TE_NPART; ++c) {
    const double sum = block_sum_n(acc[c], red);
    if (tid == 0) o[c] = sum;
  }
}

// second stage: one workgroup per layer sums the nb partials of each column in a fixed order and forms the six expectations
__global__ __launch_bounds__(256) void k_tri_exp_finish(const double* __restrict__ part, int nb, double* __restrict__ out) {
  __shared__ double red[16];
  __shared__ double tot[TE_NPART];
  const int l = blockIdx.x;
  for (int c = 0; c < TE_NPART; ++c) {
    const double sum = partials_col_sum(part + (size_t)l * nb * TE_NPART, nb, TE_NPART, c, red);
    if (threadIdx.x == 0) tot[c] = sum;
  }
  if (threadIdx.x == 0) {
    double* o = out + (size_t)l * VMR_TRIAD_NSTAT;
    o[0] = tot[0];
    o[1] = tot[1];
    o[2] = tot[2] - tot[3];
    o[3] = tot[4] / 6.0;
    o[4] = (tot[5] - tot[6]) / 2.0;
    o[5] = tot[7];
  }
}

}  // namespace

int tri_pack_chunk(vmr_ctx* h, const uint8_t* Y, int c, unsigned long long* Aout, unsigned long long* Ain) {
  const Geo& g = h->g;
  const unsigned nstrip = (unsigned)((g.N + SS_TILE - 1) / SS_TILE);
  hipLaunchKernelGGL(k_tri_pack, dim3(nstrip, (unsigned)g.L, (unsigned)c), dim3(256), 0, h->stream, Y, g.N, g.L, (g.N + 63) / 64, Aout, Ain);
  HIPCHK(h, hipGetLastError());
  return VMR_OK;
}

extern "C" int vmr_sample_triads(vmr_handle h, uint64_t seed, int n_samples, int n_trials, uint64_t* counts, int32_t* node_tri,
                                 int32_t* node_deg) {
  if (!h) return VMR_EINVAL;
  if (!counts) return fail(h, VMR_EINVAL, "vmr_sample_triads: counts is NULL");
  int rc;
  if ((rc = sampled_begin(h, "vmr_sample_triads", n_samples, n_trials))) return rc;
  const Geo& g = h->g;
  if (g.N > 65536) return fail(h, VMR_EINVAL, "vmr_sample_triads: the triangles through a node are 32-bit counts: N <= 65536");
  const BitRows b = bit_rows(g);
  const size_t node_b = b.LN * 4;
  SampledOut out[3] = {{counts, (size_t)g.L * VMR_TRIAD_NSTAT * 8, true, "vmr_sample_triads: the counts"},
                       {node_tri, node_b, false, "vmr_sample_triads: the node triangles"},
                       {node_deg, node_b, false, "vmr_sample_triads: the node degrees"}};
  const size_t per = b.per() + out[0].bytes + (node_tri ? node_b : 0) + (node_deg ? node_b : 0);   // device bytes per sample of a chunk
  size_t C;
  if ((rc = chunk_samples(h, "vmr_sample_triads", (size_t)n_samples, per, 0, &C))) return rc;
  Tmp tm(h);
  uint8_t* Y = nullptr;
  u64 *Ao = nullptr, *Ai = nullptr;
  if ((rc = bit_rows_get(tm, b, C, "vmr_sample_triads", "samples", &Y, &Ao, &Ai))) return rc;
  const unsigned nquad = (unsigned)((g.N + 3) / 4);
  rc = sampled_chunks(h, tm, (size_t)n_samples, C, seed, n_trials, Y, out, [&](size_t, int c) -> int {
    int rc2;
    if ((rc2 = tri_pack_chunk(h, Y, c, Ao, Ai))) return rc2;
    hipLaunchKernelGGL(k_tri_count, dim3(nquad, (unsigned)g.L, (unsigned)c), dim3(256), 0, h->stream, Ao, Ai, g.N, g.L, b.W, b.lG,
                       out[0].as<unsigned long long>(), out[1].as<int32_t>(), out[2].as<int32_t>());
    HIPCHK(h, hipGetLastError());
    return VMR_OK;
  });
  if (rc) return rc;
  // every node counted its triangles twice and every triangle has three nodes; every edge of U has two ends
  for (size_t q = 0; q < (size_t)n_samples * g.L; ++q) {
    counts[q * VMR_TRIAD_NSTAT + 3] /= 6;
    counts[q * VMR_TRIAD_NSTAT + 5] /= 2;
  }
  return VMR_OK;
}

extern "C" int vmr_expected_triads(vmr_handle h, double* out) {
  if (!h) return VMR_EINVAL;
  if (!out) return fail(h, VMR_EINVAL, "vmr_expected_triads: out is NULL");
  int rc;
  if ((rc = expected_begin(h, "vmr_expected_triads"))) return rc;
  const Geo& g = h->g;
  const size_t T = (size_t)g.N * g.N, ties = (size_t)g.L * T;
  const int nbp = exp_p_blocks(T);
  const int nt = (g.N + TE_T - 1) / TE_T;
  if ((size_t)nt * nt > 0x7fffffffu) return fail(h, VMR_EINVAL, "vmr_expected_triads: N is too large");
  const int nb = nt * nt;   // (of N only: the tree is the same on every device)
  Tmp tm(h);
  double *P = nullptr, *U = nullptr, *wpart = nullptr, *part = nullptr, *od = nullptr;
  if ((rc = tm.get(&P, ties * 8, "vmr_expected_triads: the edge probabilities")) || (rc = tm.get(&U, ties * 8, "vmr_expected_triads: the pair probabilities")) ||
      (rc = tm.get(&wpart, (size_t)g.L * nbp * 32, "vmr_expected_triads: partial sums")) ||
      (rc = tm.get(&part, (size_t)g.L * nb * TE_NPART * 8, "vmr_expected_triads: partial sums")) ||
      (rc = tm.get(&od, (size_t)g.L * VMR_TRIAD_NSTAT * 8, "vmr_expected_triads: the result")))
    return rc;
  if ((rc = ns_exp_p(h, P, wpart, nbp))) return rc;
  hipLaunchKernelGGL(k_tri_exp_u, dim3((unsigned)nbp, (unsigned)g.L), dim3(256), 0, h->stream, P, U, g.N);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(k_tri_exp_prod, dim3((unsigned)nb, (unsigned)g.L), dim3(256), 0, h->stream, P, U, g.N, nt, part);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(k_tri_exp_finish, dim3((unsigned)g.L), dim3(256), 0, h->stream, part, nb, od);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(out, od, (size_t)g.L * VMR_TRIAD_NSTAT * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return VMR_OK;
}
