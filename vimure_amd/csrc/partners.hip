// partners.hip -- shared partners of the posterior's ties on the device: vmr_sample_shared_partners, vmr_network_shared_partners.
//
// The other graph read-outs describe the posterior by dyads, nodes and triples; this one describes it TIE BY TIE.  For A = (Y > 0)
// with the diagonal cleared a mode names a set of ties and, per tie (i, j), its partners k:
//   0 union    unordered pairs i < j tied either way      k tied (either way) to i and to j          Jackson et al.'s support
//   1 mutual   unordered pairs tied both ways             k tied both ways to both                   Krackhardt's Simmelian ties
//   2 path     ordered ties i -> j                        k with i -> k -> j                         the ESP count behind GWESP
// With o and n the words of a node's rows of Aout and Ain, the partners of (i, j) are popc(P_i[w] & Q_j[w]) summed over the W
// words: P = Q = o | n (union), o & n (mutual), and P = o of i, Q = n of j (path).  Neither i nor j passes as its own partner:
// bit i of P_i and bit j of Q_j are diagonal bits and cleared by the packer, and the bits at and above N are zero.  Integers only,
// work proportional to ties x W, any N the handle has.
//
// k_sp_count: one wave per (node i, layer, sample), the neighbour-list walk of k_census (census.hip).  The neighbours of i in the
// mode's tie set are listed a block of SP_BLK words of row i at a time -- j > i only in union and mutual mode, from the block that
// holds bit i on; every out-neighbour in path mode -- then walked 64 / G neighbours per step, G lanes striding the W words of
// the neighbour's row, row i's words in registers when W <= G.  The G popcounts are summed by shuffles; the group's first lane
// adds one to the workgroup's LDS histogram (32-bit integer LDS atomics; a workgroup meets fewer than 4 N ties), counts the tie
// for node j (integer global atomics) and keeps the tie, the support, the partners and the maximum in registers.  Per node the
// wave sums them: into the workgroup's 64-bit totals in LDS and into node i's entries.  At the workgroup's end the non-zero bins
// and the totals leave by 64-bit global atomics, the maximum by an atomic max.  Sums of integers: the same from run to run.
//
// k_sp_pairs: G lanes per (listed pair, sample) test the pair's bit in the mode's tie set and, where it is a tie, take the same
// popcount: three integer atomics per pair for the sampled call, whose accumulators live for the whole call; a store of the
// count, or of -1 where the pair is no tie, for the networks' call.
#include <string>
#include <vector>
#include "sampled_side.h"

namespace {

#define SP_BLK 32       // words of row i whose neighbours are listed at a time
#define SP_LIST (SP_BLK * 64)

// the mode's combination of a word of Aout (o) and of Ain (n): the tie set and P of node i; Q of node j
template <int MODE>
__device__ __forceinline__ u64 sp_p(u64 o, u64 n) { return MODE == VMR_SP_UNION ? (o | n) : MODE == VMR_SP_MUTUAL ? (o & n) : o; }
template <int MODE>
__device__ __forceinline__ u64 sp_q(u64 o, u64 n) { return MODE == VMR_SP_PATH ? n : sp_p<MODE>(o, n); }
// word w of P of the row (ao, ai) and of Q: path mode reads one of the two rows only
template <int MODE>
__device__ __forceinline__ u64 sp_load_p(const u64* __restrict__ ao, const u64* __restrict__ ai, int w) {
  if constexpr (MODE == VMR_SP_PATH) return ao[w];
  else return sp_p<MODE>(ao[w], ai[w]);
}
template <int MODE>
__device__ __forceinline__ u64 sp_load_q(const u64* __restrict__ ao, const u64* __restrict__ ai, int w) {
  if constexpr (MODE == VMR_SP_PATH) return ai[w];
  else return sp_p<MODE>(ao[w], ai[w]);
}
// the sum over the G = 1 << lG lanes of a group, in every one of them (every lane of the wave calls it)
__device__ __forceinline__ unsigned group_sum_u(unsigned v, int G) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    if (o < G) v += (unsigned)__shfl_xor((int)v, o, 64);   // (G is the same in every lane)
  return v;
}

// One wave per (node i = 4 blockIdx.x + wave, layer, sample); G = 1 << lG lanes per neighbour, 64 / G neighbours per step.
// hist[s][l][n_bins], totals[s][l][4], node_ties and node_supported [s][l][N] (or null), all zeroed by the caller.
template <int MODE>
__global__ __launch_bounds__(256) void k_sp_count(const u64* __restrict__ Aout, const u64* __restrict__ Ain, int N, int L, int W, int lG, int n_bins,
                                                  u64* __restrict__ hist, u64* __restrict__ totals, int* __restrict__ node_ties,
                                                  int* __restrict__ node_supported) {
  __shared__ unsigned short list_s[4][SP_LIST];
  __shared__ unsigned hist_s[VMR_SP_MAX_BINS];
  __shared__ u64 tot_s[3];
  __shared__ unsigned max_s;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wv, l = blockIdx.y, s = blockIdx.z;
  const size_t sl = (size_t)s * L + l;
  const int G = 1 << lG, nps = 64 >> lG, sub = lane >> lG, wl = lane & (G - 1);
  unsigned short* list = list_s[wv];
  for (int b = threadIdx.x; b < n_bins; b += 256) hist_s[b] = 0u;
  if (threadIdx.x < 3) tot_s[threadIdx.x] = 0ull;
  if (threadIdx.x == 3) max_s = 0u;
  __syncthreads();
  if (i < N) {   // (the same in every lane of the wave)
    const u64* Ao = Aout + sl * N * W;
    const u64* Ai = Ain + sl * N * W;
    const u64* ao_i = Ao + (size_t)i * W;
    const u64* ai_i = Ai + (size_t)i * W;
    int* nt = node_ties ? node_ties + sl * N : nullptr;
    int* ns = node_supported ? node_supported + sl * N : nullptr;
    const int iw = i >> 6;
    const bool one = W <= G;   // (W a power of two up to 64) a lane meets one word of a row only: row i's stays in a register
    const u64 pi1 = (one && wl < W) ? sp_load_p<MODE>(ao_i, ai_i, wl) : 0ull;
    unsigned r_ties = 0u, r_sup = 0u, r_sum = 0u, r_max = 0u;   // of the neighbours whose group this lane leads (r_sum < N^2)
    const bool ordered = MODE == VMR_SP_PATH;
    for (int wb = ordered ? 0 : (iw & ~(SP_BLK - 1)); wb < W; wb += SP_BLK) {   // (unordered: the blocks below hold no j > i)
      const int w = wb + lane;
      u64 u = 0ull;
      if (lane < SP_BLK && w < W) u = sp_load_p<MODE>(ao_i, ai_i, w);   // P of row i is its tie set too
      if (!ordered) u &= w > iw ? ~0ull : (w == iw ? (~0ull << (i & 63)) << 1 : 0ull);   // the bits of word w that are some j > i
      const unsigned c = (unsigned)__popcll(u);
      unsigned inc = c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
      const int n = __builtin_amdgcn_readfirstlane((int)__shfl(inc, 63, 64));   // neighbours in this block of words, <= SP_LIST
      unsigned off = inc - c;
      wave_sync();   // (the walk of the last block is done with the list)
      while (u) {
        const int bit = __ffsll((long long)u) - 1;
        list[off++] = (unsigned short)(lane * 64 + bit);
        u &= u - 1ull;
      }
      wave_sync();
      for (int t = 0; t < n; t += nps) {
        const int idx = t + sub;
        const bool live = idx < n;
        const int j = live ? wb * 64 + (int)list[idx] : 0;   // < N: the pad bits are zero
        unsigned cnt = 0u;
        if (live) {
          const u64* ao_j = Ao + (size_t)j * W;
          const u64* ai_j = Ai + (size_t)j * W;
          if (one) {
            if (wl < W) cnt = (unsigned)__popcll(pi1 & sp_load_q<MODE>(ao_j, ai_j, wl));
          } else {
            for (int ww = wl; ww < W; ww += G) cnt += (unsigned)__popcll(sp_load_p<MODE>(ao_i, ai_i, ww) & sp_load_q<MODE>(ao_j, ai_j, ww));
          }
        }
        cnt = group_sum_u(cnt, G);
        if (live && wl == 0) {
          atomicAdd(&hist_s[min(cnt, (unsigned)(n_bins - 1))], 1u);
          r_ties += 1u;
          r_sup += cnt ? 1u : 0u;
          r_sum += cnt;
          r_max = max(r_max, cnt);
          if (nt) atomicAdd(nt + j, 1);
          if (ns && cnt) atomicAdd(ns + j, 1);
        }
      }
    }
    r_ties = wave_sum_u(r_ties); r_sup = wave_sum_u(r_sup); r_sum = wave_sum_u(r_sum); r_max = wave_max_u(r_max);
    if (lane == 0 && r_ties) {
      atomicAdd(&tot_s[0], (u64)r_ties);
      if (r_sup) atomicAdd(&tot_s[1], (u64)r_sup);
      if (r_sum) atomicAdd(&tot_s[2], (u64)r_sum);
      if (r_max) atomicMax(&max_s, r_max);
      if (nt) atomicAdd(nt + i, (int)r_ties);
      if (ns && r_sup) atomicAdd(ns + i, (int)r_sup);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < n_bins; b += 256)
    if (hist_s[b]) atomicAdd(hist + sl * n_bins + b, (u64)hist_s[b]);
  if (threadIdx.x < 3 && tot_s[threadIdx.x]) atomicAdd(totals + sl * VMR_SP_NTOTAL + threadIdx.x, tot_s[threadIdx.x]);
  if (threadIdx.x == 3 && max_s) atomicMax(totals + sl * VMR_SP_NTOTAL + 3, (u64)max_s);
}

// G = 1 << lG lanes per (pair p, sample s = blockIdx.y), 256 >> lG pairs per workgroup.  pairs[n_pairs][3] = (layer, i, j).
// NET false: present[p], supported[p], partners[p] accumulate over the samples of the call.  NET true: net[s][p] = the partners
// of the pair in network s, -1 where it is no tie.
template <int MODE, bool NET>
__global__ __launch_bounds__(256) void k_sp_pairs(const u64* __restrict__ Aout, const u64* __restrict__ Ain, int N, int L, int W, int lG,
                                                  const int* __restrict__ pairs, int n_pairs, unsigned* __restrict__ present,
                                                  unsigned* __restrict__ supported, u64* __restrict__ partners, int* __restrict__ net) {
  const int G = 1 << lG, wl = threadIdx.x & (G - 1);
  const long long p = (long long)blockIdx.x * (256 >> lG) + (threadIdx.x >> lG);
  const int s = blockIdx.y;
  const bool live = p < n_pairs;
  bool tie = false;
  unsigned cnt = 0u;
  if (live) {
    const int l = pairs[3 * p], i = pairs[3 * p + 1], j = pairs[3 * p + 2];   // checked on the host: in range, i != j
    const size_t sl = (size_t)s * L + l;
    const u64* ao_i = Aout + (sl * N + i) * W;
    const u64* ai_i = Ain + (sl * N + i) * W;
    const u64* ao_j = Aout + (sl * N + j) * W;
    const u64* ai_j = Ain + (sl * N + j) * W;
    tie = (sp_load_p<MODE>(ao_i, ai_i, j >> 6) >> (j & 63)) & 1ull;
    if (tie)
      for (int ww = wl; ww < W; ww += G) cnt += (unsigned)__popcll(sp_load_p<MODE>(ao_i, ai_i, ww) & sp_load_q<MODE>(ao_j, ai_j, ww));
  }
  cnt = group_sum_u(cnt, G);
  if (live && wl == 0) {
    if (NET) {
      net[(size_t)s * n_pairs + p] = tie ? (int)cnt : -1;
    } else if (tie) {
      atomicAdd(present + p, 1u);
      if (cnt) { atomicAdd(supported + p, 1u); atomicAdd(partners + p, (u64)cnt); }
    }
  }
}

struct SpOut {   // the device buffers of one chunk
  u64 *hist, *totals;
  int *node_ties, *node_supported;
};

template <int MODE>
void sp_launch(vmr_ctx* h, const BitRows& b, int c, const u64* Ao, const u64* Ai, int n_bins, const SpOut& o, const int* pairs, int n_pairs,
               unsigned* present, unsigned* supported, u64* partners, int* net) {
  const Geo& g = h->g;
  hipLaunchKernelGGL(k_sp_count<MODE>, dim3((unsigned)((g.N + 3) / 4), (unsigned)g.L, (unsigned)c), dim3(256), 0, h->stream, Ao, Ai, g.N, g.L, b.W,
                     b.lG, n_bins, o.hist, o.totals, o.node_ties, o.node_supported);
  if (n_pairs > 0) {
    const int ppb = 256 >> b.lG;   // pairs per workgroup
    const dim3 grid((unsigned)((n_pairs + ppb - 1) / ppb), (unsigned)c);
    if (net)
      hipLaunchKernelGGL((k_sp_pairs<MODE, true>), grid, dim3(256), 0, h->stream, Ao, Ai, g.N, g.L, b.W, b.lG, pairs, n_pairs, present, supported,
                         partners, net);
    else
      hipLaunchKernelGGL((k_sp_pairs<MODE, false>), grid, dim3(256), 0, h->stream, Ao, Ai, g.N, g.L, b.W, b.lG, pairs, n_pairs, present, supported,
                         partners, net);
  }
}

// the packed chunk of c samples (or networks), the outputs zeroed -> the counts; pairs on the device, or n_pairs = 0
int sp_chunk(vmr_ctx* h, const BitRows& b, int c, const u64* Ao, const u64* Ai, int mode, int n_bins, const SpOut& o, const int* pairs, int n_pairs,
             unsigned* present, unsigned* supported, u64* partners, int* net) {
  if (mode == VMR_SP_UNION) sp_launch<VMR_SP_UNION>(h, b, c, Ao, Ai, n_bins, o, pairs, n_pairs, present, supported, partners, net);
  else if (mode == VMR_SP_MUTUAL) sp_launch<VMR_SP_MUTUAL>(h, b, c, Ao, Ai, n_bins, o, pairs, n_pairs, present, supported, partners, net);
  else sp_launch<VMR_SP_PATH>(h, b, c, Ao, Ai, n_bins, o, pairs, n_pairs, present, supported, partners, net);
  HIPCHK(h, hipGetLastError());
  return VMR_OK;
}

// what both calls check of their arguments beyond the counts, on the host and before any launch
int sp_args(vmr_ctx* h, const std::string& fn, int mode, int n_bins, const void* hist, const void* totals, const int32_t* pairs, int n_pairs) {
  const Geo& g = h->g;
  if (mode < 0 || mode > VMR_SP_PATH) return fail(h, VMR_EINVAL, (fn + ": mode must be 0 (union), 1 (mutual) or 2 (path)").c_str());
  if (n_bins < 2 || n_bins > VMR_SP_MAX_BINS) return fail(h, VMR_EINVAL, (fn + ": n_bins must be in [2, " + std::to_string(VMR_SP_MAX_BINS) + "]").c_str());
  if (!hist) return fail(h, VMR_EINVAL, (fn + ": hist is NULL").c_str());
  if (!totals) return fail(h, VMR_EINVAL, (fn + ": totals is NULL").c_str());
  if (n_pairs < 0) return fail(h, VMR_EINVAL, (fn + ": n_pairs must not be negative").c_str());
  if (n_pairs > 0 && !pairs) return fail(h, VMR_EINVAL, (fn + ": pairs is NULL with n_pairs > 0").c_str());
  for (int p = 0; p < n_pairs; ++p) {
    const int32_t l = pairs[3 * (size_t)p], i = pairs[3 * (size_t)p + 1], j = pairs[3 * (size_t)p + 2];
    if (l < 0 || l >= g.L || i < 0 || i >= g.N || j < 0 || j >= g.N || i == j) {
      char msg[256];
      snprintf(msg, sizeof msg, "%s: pairs[%d] = (%d, %d, %d) must name a layer below %d and two different nodes below %d", fn.c_str(), p, (int)l,
               (int)i, (int)j, g.L, g.N);
      return fail(h, VMR_EINVAL, msg);
    }
  }
  return VMR_OK;
}

}  // namespace

extern "C" int vmr_sample_shared_partners(vmr_handle h, uint64_t seed, int n_samples, int n_trials, int mode, int n_bins, uint64_t* hist,
                                          uint64_t* totals, int32_t* node_ties, int32_t* node_supported, const int32_t* pairs, int n_pairs,
                                          uint32_t* pair_present, uint32_t* pair_supported, uint64_t* pair_partners) {
  if (!h) return VMR_EINVAL;
  const char* fn = "vmr_sample_shared_partners";
  int rc;
  if ((rc = sampled_counts(h, fn, n_samples, n_trials)) || (rc = sp_args(h, fn, mode, n_bins, hist, totals, pairs, n_pairs))) return rc;
  if (n_pairs > 0 && (!pair_present || !pair_supported || !pair_partners))
    return fail(h, VMR_EINVAL, "vmr_sample_shared_partners: pair_present, pair_supported or pair_partners is NULL with n_pairs > 0");
  if ((rc = expected_begin(h, fn))) return rc;
  const Geo& g = h->g;
  const BitRows b = bit_rows(g);
  const size_t np = (size_t)n_pairs;
  SampledOut out[4] = {{hist, (size_t)g.L * n_bins * 8, true, "vmr_sample_shared_partners: the histograms"},
                       {totals, (size_t)g.L * VMR_SP_NTOTAL * 8, true, "vmr_sample_shared_partners: the totals"},
                       {node_ties, b.LN * 4, true, "vmr_sample_shared_partners: the nodes' ties"},
                       {node_supported, b.LN * 4, true, "vmr_sample_shared_partners: the nodes' supported ties"}};
  size_t per = b.per();
  for (const SampledOut& o : out)
    if (o.host) per += o.bytes;
  size_t C;
  if ((rc = chunk_samples(h, fn, (size_t)n_samples, per, np * (12 + 4 + 4 + 8), &C))) return rc;   // the pairs and their accumulators: per call
  Tmp tm(h);
  uint8_t* Y = nullptr;
  u64 *Ao = nullptr, *Ai = nullptr, *pp = nullptr;
  int* pd = nullptr;
  unsigned *pr = nullptr, *ps = nullptr;
  if ((rc = bit_rows_get(tm, b, C, fn, "samples", &Y, &Ao, &Ai))) return rc;
  if (np) {
    if ((rc = tm.get(&pd, np * 12, "vmr_sample_shared_partners: the pairs")) || (rc = tm.get(&pp, np * 8, "vmr_sample_shared_partners: the pairs' partners")) ||
        (rc = tm.get(&pr, np * 4, "vmr_sample_shared_partners: the pairs' presence")) ||
        (rc = tm.get(&ps, np * 4, "vmr_sample_shared_partners: the pairs' support")))
      return rc;
    HIPCHK(h, hipMemcpyAsync(pd, pairs, np * 12, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(pp, 0, np * 8, h->stream));
    HIPCHK(h, hipMemsetAsync(pr, 0, np * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(ps, 0, np * 4, h->stream));
  }
  rc = sampled_chunks(h, tm, (size_t)n_samples, C, seed, n_trials, Y, out, [&](size_t, int c) -> int {
    int rc2;
    if ((rc2 = tri_pack_chunk(h, Y, c, Ao, Ai))) return rc2;
    const SpOut o = {out[0].as<u64>(), out[1].as<u64>(), out[2].as<int>(), out[3].as<int>()};
    return sp_chunk(h, b, c, Ao, Ai, mode, n_bins, o, pd, n_pairs, pr, ps, pp, nullptr);
  });
  if (rc) return rc;
  if (np) {   // after the last chunk
    HIPCHK(h, hipMemcpyAsync(pair_present, pr, np * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(pair_supported, ps, np * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(pair_partners, pp, np * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return VMR_OK;
}

extern "C" int vmr_network_shared_partners(vmr_handle h, const uint8_t* Y, int n, int mode, int n_bins, uint64_t* hist, uint64_t* totals,
                                           int32_t* node_ties, int32_t* node_supported, const int32_t* pairs, int n_pairs, int32_t* pair_partners) {
  if (!h) return VMR_EINVAL;
  const char* fn = "vmr_network_shared_partners";
  int rc;
  if (n < 1) return fail(h, VMR_EINVAL, "vmr_network_shared_partners: n must be positive");
  if (!Y) return fail(h, VMR_EINVAL, "vmr_network_shared_partners: Y is NULL");
  if ((rc = sp_args(h, fn, mode, n_bins, hist, totals, pairs, n_pairs))) return rc;
  if (n_pairs > 0 && !pair_partners) return fail(h, VMR_EINVAL, "vmr_network_shared_partners: pair_partners is NULL with n_pairs > 0");
  HIPCHK(h, hipSetDevice(h->device));
  const Geo& g = h->g;
  const BitRows b = bit_rows(g);
  const size_t np = (size_t)n_pairs;
  const size_t hb = (size_t)g.L * n_bins * 8, tb = (size_t)g.L * VMR_SP_NTOTAL * 8, nb = b.LN * 4;
  size_t C;
  if ((rc = chunk_samples(h, fn, (size_t)n, b.per() + hb + tb + (node_ties ? nb : 0) + (node_supported ? nb : 0) + np * 4, np * 12, &C, "network")))
    return rc;
  Tmp tm(h);
  uint8_t* Yd = nullptr;
  u64 *Ao = nullptr, *Ai = nullptr;
  SpOut o = {nullptr, nullptr, nullptr, nullptr};
  int *pd = nullptr, *net = nullptr;
  if ((rc = bit_rows_get(tm, b, C, fn, "networks", &Yd, &Ao, &Ai)) || (rc = tm.get(&o.hist, C * hb, "vmr_network_shared_partners: the histograms")) ||
      (rc = tm.get(&o.totals, C * tb, "vmr_network_shared_partners: the totals")))
    return rc;
  if (node_ties && (rc = tm.get(&o.node_ties, C * nb, "vmr_network_shared_partners: the nodes' ties"))) return rc;
  if (node_supported && (rc = tm.get(&o.node_supported, C * nb, "vmr_network_shared_partners: the nodes' supported ties"))) return rc;
  if (np) {
    if ((rc = tm.get(&pd, np * 12, "vmr_network_shared_partners: the pairs")) || (rc = tm.get(&net, C * np * 4, "vmr_network_shared_partners: the pairs' partners")))
      return rc;
    HIPCHK(h, hipMemcpyAsync(pd, pairs, np * 12, hipMemcpyHostToDevice, h->stream));
  }
  return uploaded_chunks(h, b, (size_t)n, C, Y, Yd, Ao, Ai, [&](size_t s0, int c) -> int {
    int rc2;
    HIPCHK(h, hipMemsetAsync(o.hist, 0, (size_t)c * hb, h->stream));
    HIPCHK(h, hipMemsetAsync(o.totals, 0, (size_t)c * tb, h->stream));
    if (o.node_ties) HIPCHK(h, hipMemsetAsync(o.node_ties, 0, (size_t)c * nb, h->stream));
    if (o.node_supported) HIPCHK(h, hipMemsetAsync(o.node_supported, 0, (size_t)c * nb, h->stream));
    if ((rc2 = sp_chunk(h, b, c, Ao, Ai, mode, n_bins, o, pd, n_pairs, nullptr, nullptr, nullptr, net))) return rc2;
    HIPCHK(h, hipMemcpyAsync(hist + s0 * g.L * n_bins, o.hist, (size_t)c * hb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(totals + s0 * g.L * VMR_SP_NTOTAL, o.totals, (size_t)c * tb, hipMemcpyDeviceToHost, h->stream));
    if (o.node_ties) HIPCHK(h, hipMemcpyAsync(node_ties + s0 * b.LN, o.node_ties, (size_t)c * nb, hipMemcpyDeviceToHost, h->stream));
    if (o.node_supported) HIPCHK(h, hipMemcpyAsync(node_supported + s0 * b.LN, o.node_supported, (size_t)c * nb, hipMemcpyDeviceToHost, h->stream));
    if (np) HIPCHK(h, hipMemcpyAsync(pair_partners + s0 * np, net, (size_t)c * np * 4, hipMemcpyDeviceToHost, h->stream));
    return VMR_OK;
  });
}
