// sampled_side.h -- what the units that reduce posterior samples of Y share (netstats.hip, triads.hip, mixing.hip, connectivity.hip,
// centrality.hip, betweenness.hip, cores.hip and the replicates of ppc_rep.hip), on top of read_side.h: the entry checks, the chunk rule, the chunk loop, and on the device the transposed tile.
// Everything here is static or inline.
//
// Sampling in chunks.  Sample s of a call is what vmr_sample(h, seed + s, n_trials) writes (seed + s mod 2^64).  ns_draw_chunk
// (netstats.hip) draws a chunk of c samples from ONE read of rho (8 L N^2 K bytes) into Y[c][L][N][N], one byte per tie in natural
// order, written once; the unit's kernels reduce it to a few integers per sample, which is all that leaves the device.  A chunk
// holds as many samples as fit in half of the free device memory (chunk_samples), NS_CHUNK_MAX at most; its device bytes per
// sample are L N^2 for Y plus the unit's own temporaries and the outputs that are asked for.
//
// The transposed tile.  What needs tie (j, i) next to tie (i, j) -- mutual pairs, in-neighbours -- walks a strip of 64 rows tile by
// tile, four waves per workgroup, wave w on rows 4 it + w with lane = column, and reads the tile (bj, bi) transposed through LDS
// (tile_transposed): both reads of global memory are along rows.
//
// The bit rows.  The units that walk neighbourhoods (triads.hip, connectivity.hip, centrality.hip, betweenness.hip, cores.hip) pack
// a chunk's Y[c][L][N][N] into two bitsets of 64-bit words, W = ceil(N / 64) per row: Aout[c][L][N][W] (row i: the targets of i)
// and Ain[c][L][N][W] (row i: the sources of i, the rows of A^T), A = (Y > 0) with the diagonal bit cleared and the bits at and
// above N zero (tri_pack_chunk, triads.hip).  A row is walked by G = 1 << lG lanes, the largest power of two <= min(W, 64), that
// stride its W words, 64 / G rows side by side.  BitRows holds these numbers, bit_rows_get the three buffers of a chunk;
// uploaded_chunks is the chunk loop of the calls that take the caller's networks in place of samples.
#ifndef VMR_SAMPLED_SIDE_H
#define VMR_SAMPLED_SIDE_H
#include "read_side.h"

// ------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------
#define SS_TILE 64
#define SS_BSTRIDE 68   // bytes per row of the transposed tile in LDS: 17 words, odd, so a wave's column reads spread over the banks

// Bs[c][r] = Ys[j0 + c][i0 + r], c, r in [0, 64), 0 out of range: the tile (rows j0.., columns i0..) of one N x N sample, by the
// 256 threads of the workgroup, whose lane then reads its column's element of row r as Bs[lane * SS_BSTRIDE + r].  The caller
// puts a __syncthreads() before (the last tile's reads are done) and after.
__device__ __forceinline__ void tile_transposed(uint8_t* Bs, const uint8_t* Ys, int i0, int j0, int N) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int it = 0; it < SS_TILE / 4; ++it) {
    const int c = it * 4 + w, jj = j0 + c, ii = i0 + lane;
    Bs[c * SS_BSTRIDE + lane] = (jj < N && ii < N) ? Ys[(size_t)jj * N + ii] : (uint8_t)0;
  }
}

// The second stage of a two-stage sum of doubles, in thread 0: column c of the nb per-workgroup partials part[b][ncol], thread t
// taking b = t, t + 256, .. in ascending order, then block_sum_n (256 threads, every one calls it).  The order is fixed: the result
// is the same on every device.
__device__ __forceinline__ double partials_col_sum(const double* __restrict__ part, int nb, int ncol, int c, double* red) {
  double a = 0.0;
  for (int b = threadIdx.x; b < nb; b += 256) a += part[(size_t)b * ncol + c];
  return block_sum_n(a, red);
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// What every read-out of the posterior starts with (fn: the call's name): a handle that holds a state, its device, and rho
// written where the last sweep left it unwritten.
static inline int expected_begin(vmr_ctx* h, const char* fn) {
  if (!h) return VMR_EINVAL;
  if (!h->have_state) return fail(h, VMR_ESTATE, (std::string("vmr_set_state must be called before ") + fn).c_str());
  HIPCHK(h, hipSetDevice(h->device));
  return ensure_rho_ext(h);
}

// the two counts of a sampled call; noun: what the call names n
static inline int sampled_counts(vmr_ctx* h, const char* fn, int n, int n_trials, const char* noun = "n_samples") {
  if (!h) return VMR_EINVAL;
  if (n < 1) return fail(h, VMR_EINVAL, (std::string(fn) + ": " + noun + " must be positive").c_str());
  if (n_trials < 1) return fail(h, VMR_EINVAL, (std::string(fn) + ": n_trials must be positive").c_str());
  return VMR_OK;
}

// Both, for a call with no checks of its own between them.  (A call that has some -- vmr_sample_mixing, vmr_ppc_replicates --
// runs the two halves around them: the error a caller gets for a bad argument does not depend on the state of the handle.)
static inline int sampled_begin(vmr_ctx* h, const char* fn, int n, int n_trials) {
  const int rc = sampled_counts(h, fn, n, n_trials);
  return rc ? rc : expected_begin(h, fn);
}

// The chunk rule: *C = the samples of a chunk, for n samples of `per` device bytes each beside `fixed` bytes per call -- half of
// the free memory at most, 64 MB left alone in any case, NS_CHUNK_MAX and VMR_NETSTATS_CHUNK at most.  unit: what the call draws.
static inline int chunk_samples(vmr_ctx* h, const char* fn, size_t n, size_t per, size_t fixed, size_t* C, const char* unit = "sample") {
  size_t fr = 0, tot = 0;
  HIPCHK(h, hipMemGetInfo(&fr, &tot));
  const size_t budget = fr / 2 > fixed + (64u << 20) ? fr / 2 - fixed - (64u << 20) : 0;
  *C = std::min<size_t>(std::min<size_t>(n, NS_CHUNK_MAX), budget / per);
  if (h->opt.netstats_chunk > 0) *C = std::min<size_t>(*C, (size_t)h->opt.netstats_chunk);
  if (*C < 1) {
    char msg[256];
    snprintf(msg, sizeof msg, "%s: one %s's temporaries need %.3f GB of device memory, %.3f GB are free", fn, unit, (per + fixed) / 1e9, fr / 1e9);
    return fail(h, VMR_EINVAL, msg);
  }
  return VMR_OK;
}

// The shape of a bit-row chunk on a handle (the layout is in the head of this file), what its kernels are launched with.
struct BitRows {
  int W, lG;           // words per row; log2 of the lanes that stride a row: the largest power of two <= min(W, 64)
  size_t LN, ties;     // L N; bytes of Y per sample
  size_t bits_b;       // bytes of one set of bit rows per sample
  size_t per() const { return ties + 2 * bits_b; }   // device bytes per sample of a chunk: Y, Aout and Ain
};
static inline BitRows bit_rows(const Geo& g) {
  BitRows b;
  b.W = (g.N + 63) / 64;
  b.lG = 0;
  while ((2 << b.lG) <= b.W && b.lG < 6) ++b.lG;
  b.LN = (size_t)g.L * g.N;
  b.ties = b.LN * g.N;
  b.bits_b = b.LN * b.W * 8;
  return b;
}

// Y, Aout and Ain for a chunk of C, from tm; what: "samples" or "networks"
static inline int bit_rows_get(Tmp& tm, const BitRows& b, size_t C, const char* fn, const char* what, uint8_t** Y, u64** Ao, u64** Ai) {
  const std::string f = std::string(fn) + ": the ";
  int rc;
  if ((rc = tm.get(Y, C * b.ties, (f + what).c_str())) || (rc = tm.get(Ao, C * b.bits_b, (f + "out-neighbour bits").c_str())) ||
      (rc = tm.get(Ai, C * b.bits_b, (f + "in-neighbour bits").c_str())))
    return rc;
  return VMR_OK;
}

// The chunk loop over n networks the caller supplies, Y[n][L][N][N] in host memory, in chunks of C: per chunk of c networks from
// network s0 uploads them to Yd, packs them into Ao and Ai, runs run(s0, c) -- the unit's kernels and its copies to the host, on
// the handle's stream; VMR_OK or what ends the call -- and waits for the stream.
template <class Run>
static int uploaded_chunks(vmr_ctx* h, const BitRows& b, size_t n, size_t C, const uint8_t* Y, uint8_t* Yd, u64* Ao, u64* Ai, Run run) {
  int rc;
  for (size_t s0 = 0; s0 < n; s0 += C) {
    const size_t c = std::min<size_t>(C, n - s0);
    HIPCHK(h, hipMemcpyAsync(Yd, Y + s0 * b.ties, c * b.ties, hipMemcpyHostToDevice, h->stream));
    if ((rc = tri_pack_chunk(h, Yd, (int)c, Ao, Ai))) return rc;
    if ((rc = run(s0, (int)c))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return VMR_OK;
}

// f(std::integral_constant<int, KPT>) with KPT = 1, 2, 4 or 8, the smallest that is >= kpt: the nodes a thread of a 256-thread
// workgroup keeps in registers, for the kernels that take them as a template argument (kpt <= 8: N <= 2048)
template <class F>
static inline void with_kpt(int kpt, F f) {
  if (kpt <= 1) f(std::integral_constant<int, 1>{});
  else if (kpt <= 2) f(std::integral_constant<int, 2>{});
  else if (kpt <= 4) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, 8>{});
}

// one output of a sampled call: `bytes` per sample, sample-major
struct SampledOut {
  void* host;         // the caller's array, or null: not asked for
  size_t bytes;
  bool adds;          // the kernels add to it (atomics): zeroed per chunk; else they store every element
  const char* what;   // for Tmp's refusal
  void* dev;          // the chunk's device buffer, set by sampled_chunks: null when host is
  template <class T_>
  T_* as() const { return static_cast<T_*>(dev); }
};

// The chunk loop over n samples in chunks of C.  Allocates the outputs' chunk buffers (out[q].dev, from tm), then per chunk of c
// samples from sample s0: runs before(s0, c), zeroes the outputs the kernels add to, draws Y[c][L][N][N] with seed + s0 (mod 2^64), runs launch(s0, c)
// -- the unit's kernels on the handle's stream -- copies every output that is asked for to host + s0 * bytes and waits for the
// stream.  before and launch return VMR_OK or what ends the call.  before is for what a chunk uploads from host memory:
// queued between the draw and the kernels such copies measured 0.1 ms slower per call (profiles/sampled_side_refactor.md).
template <size_t NO, class Before, class Launch>
static int sampled_chunks(vmr_ctx* h, Tmp& tm, size_t n, size_t C, uint64_t seed, int n_trials, uint8_t* Y, SampledOut (&out)[NO], Before before,
                          Launch launch) {
  int rc;
  for (SampledOut& o : out) {
    o.dev = nullptr;
    if (o.host && (rc = tm.get(&o.dev, C * o.bytes, o.what))) return rc;
  }
  for (size_t s0 = 0; s0 < n; s0 += C) {
    const size_t c = std::min<size_t>(C, n - s0);
    if ((rc = before(s0, (int)c))) return rc;
    for (const SampledOut& o : out)
      if (o.dev && o.adds) HIPCHK(h, hipMemsetAsync(o.dev, 0, c * o.bytes, h->stream));
    if ((rc = ns_draw_chunk(h, Y, (unsigned long long)seed + (unsigned long long)s0, (int)c, n_trials))) return rc;   // (mod 2^64)
    if ((rc = launch(s0, (int)c))) return rc;
    for (const SampledOut& o : out)
      if (o.dev) HIPCHK(h, hipMemcpyAsync(static_cast<char*>(o.host) + s0 * o.bytes, o.dev, c * o.bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return VMR_OK;
}
template <size_t NO, class Launch>
static int sampled_chunks(vmr_ctx* h, Tmp& tm, size_t n, size_t C, uint64_t seed, int n_trials, uint8_t* Y, SampledOut (&out)[NO], Launch launch) {
  return sampled_chunks(h, tm, n, C, seed, n_trials, Y, out, [](size_t, int) -> int { return VMR_OK; }, launch);
}

#endif  // VMR_SAMPLED_SIDE_H
