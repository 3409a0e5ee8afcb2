// census.hip -- the Holland-Leinhardt triad census of the posterior on the device: vmr_sample_triad_census, vmr_network_triad_census.
//
// The census sorts every unordered triple of nodes into one of 16 isomorphism classes, named M A N (mutual, asymmetric and null
// dyads) plus a letter -- 003 012 102 021D 021U 021C 111D 111U 030T 030C 201 120D 120U 120C 210 300, the order of
// `networkx.triadic_census` -- for A = (Y > 0) with the diagonal cleared.  vmr_sample_triad_census draws S posterior samples of Y
// in chunks (sampled_side.h: sample s is what vmr_sample(h, seed + s, n_trials) writes) and packs them into bit rows
// (sampled_side.h has the layout); vmr_network_triad_census uploads the caller's networks in chunks and packs them the same way.
//
// The scheme.  Seen from i a node k is in one of four states, st(i, k) = 0 none, 1 out (i -> k), 2 in (k -> i), 3 both; per word
// of row i of Aout (o) and Ain (n) their masks are ~(o | n), o & ~n, n & ~o and o & n.  For a CONNECTED pair i < j and states
// (a, b) the thirds k with st(i, k) = a and st(j, k) = b are popc(mask_i[a] & mask_j[b]) summed over the words, and the class of
// (i, j, k) follows from (st(i, j), a, b): cen_class.  The 15 combinations other than (none, none) are counted -- bit j is cleared
// from row i's words and bit i from row j's first (the diagonal bits i of row i and j of row j are zero already), so that neither
// i nor j passes as a third: both fall into (none, none), like the pad bits at and above N, and (none, none) is never
// popcounted.  The thirds tied to neither are N - 2 - the sum of the 15: 012 when the pair is asymmetric, 102 when it is mutual.
// A triad with c connected dyads is counted once from each of them, c = 1, 2 or 3, the first plus the second digit of its name:
// the host divides (exactly) and sets 003 = C(N, 3) - the rest.  The work is proportional to ties x W; no pass runs over the N^2
// pairs.
//
// k_census: one wave per (node i, layer, sample), the neighbour-list walk of k_tri_count (triads.hip).  It lists the neighbours
// j > i of i in U = Aout | Ain, a block of CEN_BLK words of row i at a time from the block that holds bit i on (a wave scan of the
// words' popcounts gives every lane its place in the wave's LDS list; an entry is the bit's place in the block and st(i, j)), then
// walks the list 64 / G neighbours per step, G = the largest power of two <= min(W, 64) lanes striding over the W words of the
// neighbour's rows; row i's words stay in registers when W <= G.  A lane keeps the 15 counts of its neighbour in registers and
// adds them at the neighbour's end into 15 per-lane class counters: the class of each of the 3 x 15 (st(i, j), a, b) is a
// compile-time constant, so every register index is static, and the one run-time choice, st(i, j), is three 0/1 factors.  After a
// block the wave sums the 15 counters (32 bits: at most CEN_LIST (N - 2) per block) and adds them to the workgroup's 64-bit
// totals in LDS; one 64-bit global atomic per workgroup and class at the end -- sums of integers, the same from run to run in any
// order.  Class totals exceed 2^32 (C(4097, 3) = 1.1e13): everything past the block sums is 64-bit.
#include <utility>
#include "sampled_side.h"

namespace {

#define CEN_BLK 32       // words of row i whose neighbours are listed at a time
#define CEN_LIST (CEN_BLK * 64)
#define CEN_NCOMB 15     // the combinations (a, b) other than (none, none); combination q is a = (q + 1) / 4, b = (q + 1) % 4

// The class of the triple (i, j, k) with t = st(i, j) in 1..3, a = st(i, k), b = st(j, k); states 0 none, 1 out, 2 in, 3 both, as
// seen from the first node.  (t, 0, 0) is 012 for an asymmetric pair and 102 for a mutual one.
__host__ __device__ constexpr int cen_class(int t, int a, int b) {
  constexpr unsigned char T[48] = {1, 5, 4, 6,  3, 8, 8,  11, 5, 9,  8,  13, 7,  13, 12, 14,    // i -> j
                                   1, 3, 5, 7,  5, 8, 9,  13, 4, 8,  8,  12, 6,  11, 13, 14,    // j -> i
                                   2, 7, 6, 10, 7, 12, 13, 14, 6, 13, 11, 14, 10, 14, 14, 15};  // both
  return T[(t - 1) * 16 + a * 4 + b];
}

// cnt[q] += the thirds of one word in combination q, from the word's bits of row i (oi, ni) and of row j (oj, nj)
__device__ __forceinline__ void cen_count(u64 oi, u64 ni, u64 oj, u64 nj, unsigned (&cnt)[CEN_NCOMB]) {
  const u64 mi[4] = {~(oi | ni), oi & ~ni, ni & ~oi, oi & ni};
  const u64 mj[4] = {~(oj | nj), oj & ~nj, nj & ~oj, oj & nj};
#pragma unroll
  for (int q = 0; q < CEN_NCOMB; ++q) cnt[q] += (unsigned)__popcll(mi[(q + 1) >> 2] & mj[(q + 1) & 3]);
}

// cls[class of (T_, a, b)] += is * cnt[(a, b)] for the 15 combinations, is = 1 when st(i, j) = T_ and 0 otherwise (cnt < 2^24)
template <int T_, int... Q>
__device__ __forceinline__ void cen_route(unsigned is, const unsigned (&cnt)[CEN_NCOMB], unsigned (&cls)[VMR_CENSUS_NCLASS],
                                          std::integer_sequence<int, Q...>) {
  ((cls[cen_class(T_, (Q + 1) >> 2, (Q + 1) & 3)] += __umul24(is, cnt[Q])), ...);
}

// One wave per (node i = 4 blockIdx.x + wave, layer, sample); G = 1 << lG lanes per neighbour, 64 / G neighbours per step.
// counts[s][l][c], c >= 1: the triads of class c, each counted once per connected dyad; the host divides and fills class 0.
__global__ __launch_bounds__(256) void k_census(const u64* __restrict__ Aout, const u64* __restrict__ Ain, int N, int L, int W, int lG,
                                                u64* __restrict__ counts) {
  __shared__ unsigned short list_s[4][CEN_LIST];
  __shared__ u64 tot[VMR_CENSUS_NCLASS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wv, l = blockIdx.y, s = blockIdx.z;
  const size_t sl = (size_t)s * L + l;
  const int G = 1 << lG, nps = 64 >> lG, sub = lane >> lG, wl = lane & (G - 1);
  unsigned short* list = list_s[wv];
  if (threadIdx.x < VMR_CENSUS_NCLASS) tot[threadIdx.x] = 0ull;
  __syncthreads();
  if (i < N) {   // (the same in every lane of the wave)
    const u64* Ao = Aout + sl * N * W;
    const u64* Ai = Ain + sl * N * W;
    const u64* ao_i = Ao + (size_t)i * W;
    const u64* ai_i = Ai + (size_t)i * W;
    const int iw = i >> 6;
    const u64 ibit = 1ull << (i & 63);
    const u64 thirds = (u64)(N - 2);   // (N >= 3 wherever a pair is connected and a count is added; unused otherwise)
    const bool one = W <= G;   // (W a power of two up to 64) a lane meets one word of a row only: row i's stay in registers
    const u64 aoi1 = (one && wl < W) ? ao_i[wl] : 0ull, aii1 = (one && wl < W) ? ai_i[wl] : 0ull;
    for (int wb = iw & ~(CEN_BLK - 1); wb < W; wb += CEN_BLK) {   // (the blocks below hold no j > i)
      const int w = wb + lane;
      u64 a = 0ull, b = 0ull;
      if (lane < CEN_BLK && w < W) { a = ao_i[w]; b = ai_i[w]; }
      const u64 gt = w > iw ? ~0ull : (w == iw ? (~0ull << (i & 63)) << 1 : 0ull);   // the bits of word w that are some j > i
      a &= gt; b &= gt;
      u64 u = a | b;
      const unsigned c = (unsigned)__popcll(u);
      unsigned npair_a = (unsigned)__popcll(a ^ b), npair_m = (unsigned)__popcll(a & b);   // asymmetric and mutual pairs (i, j)
      unsigned inc = c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
      const int n = __builtin_amdgcn_readfirstlane((int)__shfl(inc, 63, 64));   // neighbours in this block of words, <= CEN_LIST
      unsigned off = inc - c;
      wave_sync();   // (the walk of the last block is done with the list)
      while (u) {
        const int bit = __ffsll((long long)u) - 1;
        list[off++] = (unsigned short)((lane * 64 + bit) | (int)((a >> bit) & 1ull) << 14 | (int)((b >> bit) & 1ull) << 15);   // bits 14, 15: st(i, j)
        u &= u - 1ull;
      }
      wave_sync();
      unsigned cls[VMR_CENSUS_NCLASS];   // per lane; [1] and [2] collect the 15 counts of the asymmetric and of the mutual pairs
#pragma unroll
      for (int q = 0; q < VMR_CENSUS_NCLASS; ++q) cls[q] = 0u;
      for (int t = 0; t < n; t += nps) {
        const int idx = t + sub;
        if (idx < n) {
          const unsigned e = list[idx];
          const int j = wb * 64 + (int)(e & 0x3fffu);   // < N: the pad bits are zero
          const unsigned st = e >> 14;                  // 1 out, 2 in, 3 both
          const int jw = j >> 6;
          const u64 jbit = 1ull << (j & 63);
          const u64* ao_j = Ao + (size_t)j * W;
          const u64* ai_j = Ai + (size_t)j * W;
          unsigned cnt[CEN_NCOMB];
#pragma unroll
          for (int q = 0; q < CEN_NCOMB; ++q) cnt[q] = 0u;
          if (one) {
            if (wl < W) {
              const u64 ki = wl == jw ? ~jbit : ~0ull, kj = wl == iw ? ~ibit : ~0ull;
              cen_count(aoi1 & ki, aii1 & ki, ao_j[wl] & kj, ai_j[wl] & kj, cnt);
            }
          } else {
            for (int ww = wl; ww < W; ww += G) {
              const u64 ki = ww == jw ? ~jbit : ~0ull, kj = ww == iw ? ~ibit : ~0ull;
              cen_count(ao_i[ww] & ki, ai_i[ww] & ki, ao_j[ww] & kj, ai_j[ww] & kj, cnt);
            }
          }
          unsigned all = 0u;
#pragma unroll
          for (int q = 0; q < CEN_NCOMB; ++q) all += cnt[q];
          const unsigned is1 = st == 1u ? 1u : 0u, is2 = st == 2u ? 1u : 0u, is3 = st == 3u ? 1u : 0u;
          const std::make_integer_sequence<int, CEN_NCOMB> comb{};
          cen_route<1>(is1, cnt, cls, comb);
          cen_route<2>(is2, cnt, cls, comb);
          cen_route<3>(is3, cnt, cls, comb);
          cls[1] += __umul24(is1 + is2, all);
          cls[2] += __umul24(is3, all);
        }
      }
#pragma unroll
      for (int q = 1; q < VMR_CENSUS_NCLASS; ++q) cls[q] = wave_sum_u(cls[q]);
      npair_a = wave_sum_u(npair_a); npair_m = wave_sum_u(npair_m);
      if (lane == 0) {
        const u64 t012 = (u64)npair_a * thirds - cls[1], t102 = (u64)npair_m * thirds - cls[2];   // the thirds tied to neither
        if (t012) atomicAdd(&tot[1], t012);
        if (t102) atomicAdd(&tot[2], t102);
#pragma unroll
        for (int q = 3; q < VMR_CENSUS_NCLASS; ++q)
          if (cls[q]) atomicAdd(&tot[q], (u64)cls[q]);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < VMR_CENSUS_NCLASS && tot[threadIdx.x]) atomicAdd(counts + sl * VMR_CENSUS_NCLASS + threadIdx.x, tot[threadIdx.x]);
}

// the packed chunk of c samples (or networks), counts[c][L][16] zeroed -> the class sums, each triad once per connected dyad
int census_chunk(vmr_ctx* h, const BitRows& b, int c, const u64* Ao, const u64* Ai, u64* counts) {
  const Geo& g = h->g;
  hipLaunchKernelGGL(k_census, dim3((unsigned)((g.N + 3) / 4), (unsigned)g.L, (unsigned)c), dim3(256), 0, h->stream, Ao, Ai, g.N, g.L, b.W, b.lG,
                     counts);
  HIPCHK(h, hipGetLastError());
  return VMR_OK;
}

// counts[n][16] as the kernel leaves them -> the census: a triad of class c was counted once from each of its connected dyads
// (1, 2 or 3: the first plus the second digit of the class name), and 003 is what is left of the C(N, 3) triples
void census_finish(uint64_t* counts, size_t n, int N) {
  static const uint64_t dyads[VMR_CENSUS_NCLASS] = {1, 1, 1, 2, 2, 2, 2, 2, 3, 3, 2, 3, 3, 3, 3, 3};
  const uint64_t m = (uint64_t)N;
  const uint64_t triples = N < 3 ? 0 : m * (m - 1) / 2 * (m - 2) / 3;   // (m (m - 1) / 2 is exact, and the product of three consecutive numbers divides by 3)
  for (size_t q = 0; q < n; ++q) {
    uint64_t* o = counts + q * VMR_CENSUS_NCLASS;
    uint64_t rest = 0;
    for (int c = 1; c < VMR_CENSUS_NCLASS; ++c) {
      o[c] /= dyads[c];
      rest += o[c];
    }
    o[0] = triples - rest;
  }
}

}  // namespace

extern "C" int vmr_sample_triad_census(vmr_handle h, uint64_t seed, int n_samples, int n_trials, uint64_t* counts) {
  if (!h) return VMR_EINVAL;
  const char* fn = "vmr_sample_triad_census";
  int rc;
  if ((rc = sampled_counts(h, fn, n_samples, n_trials))) return rc;
  if (!counts) return fail(h, VMR_EINVAL, "vmr_sample_triad_census: counts is NULL");
  if ((rc = expected_begin(h, fn))) return rc;
  const Geo& g = h->g;
  const BitRows b = bit_rows(g);
  SampledOut out[1] = {{counts, (size_t)g.L * VMR_CENSUS_NCLASS * 8, true, "vmr_sample_triad_census: the counts"}};
  size_t C;
  if ((rc = chunk_samples(h, fn, (size_t)n_samples, b.per() + out[0].bytes, 0, &C))) return rc;   // device bytes per sample of a chunk
  Tmp tm(h);
  uint8_t* Y = nullptr;
  u64 *Ao = nullptr, *Ai = nullptr;
  if ((rc = bit_rows_get(tm, b, C, fn, "samples", &Y, &Ao, &Ai))) return rc;
  rc = sampled_chunks(h, tm, (size_t)n_samples, C, seed, n_trials, Y, out, [&](size_t, int c) -> int {
    int rc2;
    if ((rc2 = tri_pack_chunk(h, Y, c, Ao, Ai))) return rc2;
    return census_chunk(h, b, c, Ao, Ai, out[0].as<u64>());
  });
  if (rc) return rc;
  census_finish(counts, (size_t)n_samples * g.L, g.N);
  return VMR_OK;
}

extern "C" int vmr_network_triad_census(vmr_handle h, const uint8_t* Y, int n, uint64_t* counts) {
  if (!h) return VMR_EINVAL;
  const char* fn = "vmr_network_triad_census";
  int rc;
  if (n < 1) return fail(h, VMR_EINVAL, "vmr_network_triad_census: n must be positive");
  if (!Y) return fail(h, VMR_EINVAL, "vmr_network_triad_census: Y is NULL");
  if (!counts) return fail(h, VMR_EINVAL, "vmr_network_triad_census: counts is NULL");
  HIPCHK(h, hipSetDevice(h->device));
  const Geo& g = h->g;
  const BitRows b = bit_rows(g);
  const size_t cb = (size_t)g.L * VMR_CENSUS_NCLASS * 8;
  size_t C;
  if ((rc = chunk_samples(h, fn, (size_t)n, b.per() + cb, 0, &C, "network"))) return rc;
  Tmp tm(h);
  uint8_t* Yd = nullptr;
  u64 *Ao = nullptr, *Ai = nullptr, *cd = nullptr;
  if ((rc = bit_rows_get(tm, b, C, fn, "networks", &Yd, &Ao, &Ai)) || (rc = tm.get(&cd, C * cb, "vmr_network_triad_census: the counts"))) return rc;
  rc = uploaded_chunks(h, b, (size_t)n, C, Y, Yd, Ao, Ai, [&](size_t s0, int c) -> int {
    int rc2;
    HIPCHK(h, hipMemsetAsync(cd, 0, (size_t)c * cb, h->stream));
    if ((rc2 = census_chunk(h, b, c, Ao, Ai, cd))) return rc2;
    HIPCHK(h, hipMemcpyAsync(counts + s0 * g.L * VMR_CENSUS_NCLASS, cd, (size_t)c * cb, hipMemcpyDeviceToHost, h->stream));
    return VMR_OK;
  });
  if (rc) return rc;
  census_finish(counts, (size_t)n * g.L, g.N);
  return VMR_OK;
}
