// create.hip -- everything vmr_create does, once per handle (create.h): packs the dense uint8 tensor X[L,N,N,M] and the mask,
// takes their statistics, turns a sparse tensor into the sorted report lists (sweep_sl.h, sorted_lists.hip) and its mask into
// mask lists, chooses the data format and the LDS shapes of the sweeps (create_tail), and allocates the state, the statistics
// and the scratch.  read_opts here is the one place that reads the environment.  vmr_destroy sits beside the allocations.
// vmr_create_coo (create_coo.hip) shares create_ctx, create_state, sl_finish and create_tail.
#include "create.h"
#include "sweep_tiles.h"

// ------------------------------------------------------------------------------------------
// set-up kernels
// ------------------------------------------------------------------------------------------
__global__ void k_pack_x(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, size_t rows, int M, int Mp) {
  // one 16-byte output chunk per thread
  size_t nchunk = Mp / 16, total = rows * nchunk;
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
    size_t r = q / nchunk; int c = (int)(q - r * nchunk);
    unsigned char b[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) { int m = c * 16 + u; b[u] = (m < M) ? src[r * M + m] : 0; }
    *reinterpret_cast<uint4*>(dst + r * Mp + c * 16) = *reinterpret_cast<uint4*>(b);
  }
}

__global__ void k_pack_r(const uint8_t* __restrict__ src, uint64_t* __restrict__ dst, size_t rows, int M, int W) {
  size_t total = rows * W;
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
    size_t r = q / W; int w = (int)(q - r * W);
    uint64_t bits = 0;
    for (int u = 0; u < 64; ++u) {
      int m = w * 64 + u;
      bool on = (m < M) && (src == nullptr || src[r * M + m] != 0);
      bits |= (uint64_t)on << u;
    }
    dst[q] = bits;
  }
}

// coverage flag per tie + sum(X)
__global__ void k_stats(const uint8_t* __restrict__ X, const uint64_t* __restrict__ Rb, uint8_t* __restrict__ cov,
                        uint8_t* __restrict__ rcls,
                        unsigned long long* sumx, unsigned* xmax, unsigned long long* npartial, size_t rows, int Mp,
                        int W, int M) {
  unsigned long long local = 0, lpart = 0, lempty = 0;
  unsigned lmax = 0;
  for (size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x; r < rows; r += (size_t)gridDim.x * blockDim.x) {
    bool anyx = false, anyr = false;
    const uint4* p = reinterpret_cast<const uint4*>(X + r * Mp);
    for (int c = 0; c < Mp / 16; ++c) {
      uint4 v = p[c];
      if (v.x | v.y | v.z | v.w) {
        anyx = true;
        unsigned d[4] = {v.x, v.y, v.z, v.w};
        for (int u = 0; u < 4; ++u) {
          local += (d[u] & 0xff) + ((d[u] >> 8) & 0xff) + ((d[u] >> 16) & 0xff) + (d[u] >> 24);
          lmax = max(lmax, max(max(d[u] & 0xff, (d[u] >> 8) & 0xff), max((d[u] >> 16) & 0xff, d[u] >> 24)));
        }
      }
    }
    bool full = true;
    for (int w = 0; w < W; ++w) {
      const uint64_t bits = Rb[r * W + w];
      const int rem = M - w * 64;
      const uint64_t fm = rem >= 64 ? ~0ull : ((1ull << rem) - 1ull);
      anyr |= bits != 0;
      full = full && (bits == fm);
    }
    cov[r] = (anyx && anyr) ? 1 : 0;
    rcls[r] = !anyr ? 0 : (full ? 1 : 2);
    if (anyr && !full) ++lpart;
    if (!anyr) ++lempty;
  }
  if (local) atomicAdd(sumx, local);
  if (lpart) atomicAdd(npartial, lpart);
  if (lempty) atomicAdd(npartial + 1, lempty);   // [1]: rows with no reporter at all
  if (lmax) atomicMax(xmax, lmax);
}

// ==========================================================================================
// Report lists (the default data format when X is sparse, which it is: 1.5-5 % of the counts are non-zero)
//
// X is a tensor of COUNTS of which a few per cent are non-zero; every update touches only those, and the only
// thing the mutuality terms need besides a report is the mirrored count X[l,j,i,m].  vmr_create therefore turns
// the dense tensor into one 4-byte entry per non-zero count (layout and limits: sweep_sl.h), sorted by the ties'
// report counts and laid out in steps of 64 ties (sorted_lists.hip); rcls[l][t] = class of the tie's mask row (0 empty,
// 1 all ones, 2 partial; not read when every row is all ones), Qt[l][t] = sum_m R[t,m] X[mirror(t),m] (the ELBO's mirror
// sum, a constant of the data).  A sweep reads 4 B per report + rho/log-prior instead of 1 B per (tie, reporter).  The
// dense tensor is freed once the lists exist.  (Rounds 1-2 kept steps of 64 CONSECUTIVE ties with a scattered rest --
// k_rho_sp, removed in round 3: DESIGN.md section 2.)
// ==========================================================================================
__device__ __forceinline__ unsigned nz_bytes(uint4 v) {
  const unsigned M = 0x7f7f7f7fu;
  unsigned t0 = (((v.x & M) + M) | v.x) & ~M, t1 = (((v.y & M) + M) | v.y) & ~M;
  unsigned t2 = (((v.z & M) + M) | v.z) & ~M, t3 = (((v.w & M) + M) | v.w) & ~M;
  return __popc(t0) + __popc(t1) + __popc(t2) + __popc(t3);
}

// Per tie of one layer (16 lanes per row): rp[t] = its non-zero counts.  The layer total goes to *nnz.
__global__ __launch_bounds__(256) void k_sp_count(const uint8_t* __restrict__ Xl, unsigned* __restrict__ rpl,
                                                  unsigned long long* nnz, Geo g) {
  __shared__ double red[8];
  const int gl = threadIdx.x & 15;
  unsigned long long mine = 0;
  const size_t T = (size_t)g.N * g.N, Tr = (T + 15) / 16 * 16;
  for (size_t t = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 4; t < Tr; t += (size_t)gridDim.x * 16) {
    unsigned c = 0;
    if (t < T) {
      const uint8_t* row = Xl + t * g.Mp;
      for (int ch = gl; ch < g.nchunk; ch += 16) c += nz_bytes(*reinterpret_cast<const uint4*>(row + ch * 16));
    }
    c = group_sum_u(c, 16);
    if (gl == 0 && t < T) { rpl[t] = c; mine += c; }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) rpl[T] = 0u;
  // block total (exact in double: < 2^53)
  double v = block_sum((double)mine, red);
  if (threadIdx.x == 0 && v > 0.0) atomicAdd(nnz, (unsigned long long)v);
}

// in-place exclusive scan of n u32 items in three launches (2048 items per workgroup)
__global__ __launch_bounds__(256) void k_scan_local(unsigned* a, unsigned* bsum, size_t n) {
  __shared__ unsigned sh[256];
  const size_t base = (size_t)blockIdx.x * 2048 + (size_t)threadIdx.x * 8;
  unsigned v[8], s = 0;
#pragma unroll
  for (int u = 0; u < 8; ++u) { unsigned t = (base + u < n) ? a[base + u] : 0u; v[u] = s; s += t; }
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o2 = 1; o2 < 256; o2 <<= 1) {
    unsigned t = (threadIdx.x >= (unsigned)o2) ? sh[threadIdx.x - o2] : 0u;
    __syncthreads();
    sh[threadIdx.x] += t;
    __syncthreads();
  }
  const unsigned excl = sh[threadIdx.x] - s;
#pragma unroll
  for (int u = 0; u < 8; ++u) if (base + u < n) a[base + u] = v[u] + excl;
  if (threadIdx.x == 255) bsum[blockIdx.x] = sh[255];
}
__global__ __launch_bounds__(256) void k_scan_bsum(unsigned* bsum, int nb) {
  __shared__ unsigned sh[256];
  unsigned carry = 0;
  for (int c0 = 0; c0 < nb; c0 += 256) {
    const int i = c0 + threadIdx.x;
    const unsigned s = (i < nb) ? bsum[i] : 0u;
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o2 = 1; o2 < 256; o2 <<= 1) {
      unsigned t = (threadIdx.x >= (unsigned)o2) ? sh[threadIdx.x - o2] : 0u;
      __syncthreads();
      sh[threadIdx.x] += t;
      __syncthreads();
    }
    if (i < nb) bsum[i] = carry + sh[threadIdx.x] - s;
    carry += sh[255];
    __syncthreads();
  }
}
__global__ __launch_bounds__(256) void k_scan_add(unsigned* a, const unsigned* __restrict__ bsum, size_t n) {
  const size_t base = (size_t)blockIdx.x * 2048 + (size_t)threadIdx.x * 8;
  const unsigned add = bsum[blockIdx.x];
#pragma unroll
  for (int u = 0; u < 8; ++u) if (base + u < n) a[base + u] += add;
}
// Write the entries of one layer (16 lanes per tie) and the mirror sums Qt.  rpl is the exclusive scan of the
// per-tie counts: tie t's entries start at rpl[t], reporters ascending.
template <bool MUT>
__global__ __launch_bounds__(256) void k_sp_fill(const uint8_t* __restrict__ Xl, const uint64_t* __restrict__ Rl,
                                                 const unsigned* __restrict__ rpl, unsigned* __restrict__ El, unsigned* __restrict__ El2 /*wide entries: the second words*/,
                                                 unsigned* __restrict__ Qtl, Geo g) {
  const int gl = threadIdx.x & 15;
  const size_t T = (size_t)g.N * g.N, Tr = (T + 15) / 16 * 16;
  for (size_t t = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 4; t < Tr; t += (size_t)gridDim.x * 16) {
    const bool ok = t < T;
    const size_t tc = ok ? t : 0;
    const size_t i = tc / g.N, j = tc - i * g.N, tm = j * g.N + i;
    const uint8_t* row = Xl + tc * g.Mp;
    const uint8_t* mrow = Xl + tm * g.Mp;
    const uint64_t* rr = Rl + tc * g.W;
    const uint64_t* rmr = Rl + tm * g.W;
    size_t pos = rpl[tc];
    unsigned q = 0;
    for (int c0 = 0; c0 < g.nchunk; c0 += 16) {   // uniform over the 16 lanes
      const int ch = c0 + gl;
      uint4 v = make_uint4(0, 0, 0, 0), yv = make_uint4(0, 0, 0, 0);
      if (ok && ch < g.nchunk) {
        v = *reinterpret_cast<const uint4*>(row + ch * 16);
        if (MUT) yv = *reinterpret_cast<const uint4*>(mrow + ch * 16);
      }
      const unsigned xs[4] = {v.x, v.y, v.z, v.w}, ys[4] = {yv.x, yv.y, yv.z, yv.w};
      const unsigned n = nz_bytes(v);
      unsigned incl = n;
#pragma unroll
      for (int o2 = 1; o2 < 16; o2 <<= 1) {
        const unsigned up = __shfl_up(incl, o2, 16);
        if (gl >= o2) incl += up;
      }
      const unsigned tot = __shfl(incl, 15, 16);
      size_t w = pos + incl - n;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        unsigned dw = xs[u];
        while (dw) {
          const int sh = __builtin_ctz(dw) & ~7;
          const unsigned x = (dw >> sh) & 0xffu;
          dw &= ~(0xffu << sh);
          const int m = ch * 16 + u * 4 + (sh >> 3);
          const unsigned inr = (unsigned)((rr[m >> 6] >> (m & 63)) & 1ull);
          unsigned y = 0;
          if (MUT) {
            y = (ys[u] >> sh) & 0xffu;
            if ((rmr[m >> 6] >> (m & 63)) & 1ull) q += x;   // R[mirror,m] X[this,m]
          }
          if (El2) { El[w] = y * (unsigned)g.Mp + (unsigned)m; El2[w] = (x << 1) | inr; ++w; }
          else El[w++] = (y * (unsigned)g.Mp + (unsigned)m) | (inr << 20) | (x << 21);   // (sweep_sl.h)
        }
      }
      pos += tot;
    }
    q = group_sum_u(q, 16);
    if (ok && gl == 0) Qtl[tm] = q;   // every tie is the mirror of exactly one tie
  }
}

// ------------------------------------------------------------------------------------------
// Mask lists: a partial mask row as the list of its reporters (u16), for masks whose partial rows hold few
// reporters (the self-reporter mask of survey data: R[l,i,j,m] = 1 iff m is i or j, two per row).  Reading 4 bytes
// per row instead of W words makes the mask sums A and the per-tie T of such data a few microseconds.
// rq[l][t] (u32, N*N+1 per layer): first reporter of tie t's list, relative to rbase[l]; empty for rows that are
// not partial.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rm_count(const uint64_t* __restrict__ Rl, const uint8_t* __restrict__ cl,
                                                  unsigned* __restrict__ rql, unsigned long long* total, unsigned* maxrow,
                                                  size_t T, int W) {
  __shared__ double red[8];
  unsigned long long mine = 0;
  unsigned mx = 0;
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < T; t += (size_t)gridDim.x * 256) {
    unsigned n = 0;
    if (cl[t] == 2) for (int w = 0; w < W; ++w) n += (unsigned)__popcll(Rl[t * W + w]);
    rql[t] = n;
    mine += n;
    mx = max(mx, n);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) rql[T] = 0u;
  double v = block_sum((double)mine, red);
  if (threadIdx.x == 0 && v > 0.0) atomicAdd(total, (unsigned long long)v);
  if (mx) atomicMax(maxrow, mx);
}
__global__ __launch_bounds__(256) void k_rm_fill(const uint64_t* __restrict__ Rl, const uint8_t* __restrict__ cl,
                                                 const unsigned* __restrict__ rql, unsigned short* __restrict__ Rml, size_t T, int W) {
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < T; t += (size_t)gridDim.x * 256) {
    if (cl[t] != 2) continue;
    size_t q = rql[t];
    for (int w = 0; w < W; ++w) {
      uint64_t bits = Rl[t * W + w];
      while (bits) {
        const int b_ = __builtin_ctzll(bits);
        bits &= bits - 1;
        Rml[q++] = (unsigned short)(w * 64 + b_);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// Geo::farl -- the reports of the levels beyond the LDS ones
// ------------------------------------------------------------------------------------------
// Geo::farl: every tie's reports of the levels beyond the LDS ones (row >= rows_near) are moved to the FRONT of its list -- one wave
// per step, a lane walks its tie's column and swaps a far report with the first near one -- so that only the first nf rounds of a
// step (nf = the most far reports any of its 64 ties has; stored in the high half of sy) ever take the pass' far-level code: left
// where they fall, 2 % of far reports put one into two rounds of three.
// slots read by a statistics pass that skips the rounds of level 0 only: sum over steps of 64 min(R, n1)  (vmr_kernel_bytes)
__global__ __launch_bounds__(256) void k_stat_slots(const unsigned* __restrict__ rsl, const unsigned* __restrict__ syl, size_t NS, unsigned long long* __restrict__ out) {
  unsigned long long v = 0;
  for (size_t s = (size_t)blockIdx.x * 256 + threadIdx.x; s < NS; s += (size_t)gridDim.x * 256) {
    const unsigned R = (rsl[s + 1] - rsl[s]) >> 6, n1 = syl[s] >> 16;
    v += 64ull * (unsigned long long)min(R, n1);
  }
  if (v) atomicAdd(out, v);
}
// x0 != null: also the tie's summed counts of the near reports, by position (SlArgs::x0p).
__global__ __launch_bounds__(256) void k_far_first(unsigned* __restrict__ E, const unsigned* __restrict__ rsl, unsigned* __restrict__ syl, size_t NS, unsigned rows_near,
                                                   unsigned* __restrict__ x0) {
  const int lane = threadIdx.x & 63;
  for (size_t s = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); s < NS; s += (size_t)gridDim.x * 4) {
    const unsigned ea = rsl[s], R = (rsl[s + 1] - ea) >> 6;
    unsigned* col = E + (size_t)ea + lane;
    unsigned f = 0;   // far reports found so far = the slot the next one goes to
    unsigned xs = 0;
    for (unsigned r = 0; r < R; ++r) {
      const unsigned e = col[(size_t)r * 64];
      if (e != 0u && SL_YM(e) >= rows_near) {
        if (f != r) { const unsigned o = col[(size_t)f * 64]; col[(size_t)f * 64] = e; col[(size_t)r * 64] = o; }
        ++f;
      } else xs += SL_X(e);
    }
    if (x0) x0[s * 64 + (unsigned)lane] = xs;
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) f = max(f, (unsigned)__shfl_xor((int)f, o2, 64));
    if (lane == 0) syl[s] = (syl[s] & 0xffffu) | (min(f, 0xffffu) << 16);
  }
}

// One wave per step of the sorted lists: (position, entry) of every report whose mirror count is at least yfar, appended to the
// layer's far list (order immaterial: their sums are float atomics anyway).
__global__ __launch_bounds__(256) void k_far_collect(const unsigned* __restrict__ E, const unsigned* __restrict__ rsl, size_t NS, unsigned rows_near,
                                                     unsigned* __restrict__ far_pos, unsigned* __restrict__ far_ent, unsigned long long* __restrict__ counter) {
  const int lane = threadIdx.x & 63;
  for (size_t s = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); s < NS; s += (size_t)gridDim.x * 4) {
    const unsigned ea = rsl[s], R = (rsl[s + 1] - ea) >> 6;
    for (unsigned r = 0; r < R; ++r) {
      const unsigned e = E[(size_t)ea + r * 64 + lane];
      const bool far = e != 0u && SL_X(e) != 0u && SL_YM(e) >= rows_near;
      const unsigned long long bal = __ballot(far);
      if (bal == 0ull) continue;
      unsigned long long base = 0ull;
      if (lane == 0) base = atomicAdd(counter, (unsigned long long)__popcll(bal));
      base = ((unsigned long long)(unsigned)__shfl((int)(unsigned)(base >> 32), 0, 64) << 32) | (unsigned)__shfl((int)(unsigned)base, 0, 64);
      if (far) {
        const unsigned long long at = base + (unsigned long long)__popcll(bal & ((1ull << lane) - 1ull));
        far_pos[at] = (unsigned)(s * 64 + (unsigned)lane);
        far_ent[at] = e;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// vmr_create (and what vmr_create_coo shares with it: create.h)
// ------------------------------------------------------------------------------------------

static void read_opts(VmrOpts& o) {
  memset(&o, 0, sizeof o);   // (padding too: batch_kind compares records with memcmp)
  auto set = [](const char* n) { return getenv(n) != nullptr; };
  auto num = [](const char* n, int dflt) { const char* e = getenv(n); return e ? atoi(e) : dflt; };
  if (const char* f = getenv("VMR_FORMAT")) o.format = !strcmp(f, "dense") ? 1 : !strcmp(f, "sparse") ? 2 : 0;
  o.deterministic = num("VMR_DETERMINISTIC", 0) != 0;
  o.graph = num("VMR_GRAPH", 0) != 0;
  o.debug = num("VMR_DEBUG", 0);
  o.levels = num("VMR_LEVELS", 64);
  o.two_pass = num("VMR_TWO_PASS", 0);
  o.farl = num("VMR_FARL", 0);
  o.yt = set("VMR_YT") ? std::max(0, num("VMR_YT", 0)) : -1;
  o.hc = set("VMR_HC") ? std::max(0, num("VMR_HC", 0)) : -1;
  o.tpb = num("VMR_TPB", 0);
  o.st_tpb = num("VMR_ST_TPB", 0);
  o.no_level0 = set("VMR_NO_LEVEL0");
  o.no_x0 = set("VMR_NO_X0");
  o.no_lv0r = set("VMR_NO_LV0R");
  o.no_level_sort = set("VMR_NO_LEVEL_SORT");
  o.no_rlists = set("VMR_NO_RLISTS");
  o.no_rm2 = set("VMR_NO_RM2");
  o.no_lp0 = set("VMR_NO_LP0");
  o.no_lpd = set("VMR_NO_LPD");
  o.no_balance = set("VMR_NO_BALANCE");
  o.always_store_rho = set("VMR_ALWAYS_STORE_RHO");
  o.debug_lazy_rho = set("VMR_DEBUG_LAZY_RHO");
  o.gen_hsum = num("VMR_GEN_HSUM", 0);
  o.gen_no_lds_h = set("VMR_GEN_NO_LDS_H");
  o.gen_dbg = num("VMR_GEN_DBG", 0);
  o.netstats_chunk = std::max(0, num("VMR_NETSTATS_CHUNK", 0));
  o.batch_fg = set("VMR_BATCH_FG") ? std::max(1, std::min(FG_G, num("VMR_BATCH_FG", 0))) : 0;
  if (const char* t = getenv("VMR_DEBUG_TIMES")) snprintf(o.debug_times, sizeof o.debug_times, "%s", t);
}

// context, geometry, streams and the small per-dataset arrays
int create_ctx(vmr_ctx** out, hipDeviceProp_t* prop, int device, int L, int N, int M, int K, int mutuality, double eps, bool lists_only) {
  if (L < 1 || N < 1 || M < 1) return fail(nullptr, VMR_EINVAL, "L, N, M must be positive");
  if (K < 2 || K > KGEN_MAX) return fail(nullptr, VMR_EINVAL, "K must be in [2, 256]");
  int ndev = 0;
  CK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(nullptr, VMR_EINVAL, "no such HIP device");
  CK(hipSetDevice(device));
  CK(hipGetDeviceProperties(prop, device));
  vmr_ctx* h = new vmr_ctx();
  *out = h;
  h->device = device;
  Geo& g = h->g;
  g.L = L; g.N = N; g.M = M; g.K = K; g.mut = mutuality ? 1 : 0; g.eps = eps;
  g.gen = K > KMAX ? 1 : 0; g.wide = 0;   // (wide entries: decided once the largest count is known)
  read_opts(h->opt);
  g.dbg = h->opt.debug;
  g.det = h->opt.deterministic ? 1 : 0; g.det_sh = 0; g.det_shr = 0; g.det_sha = 0;   // sorted report lists unless the older step layout is asked for
  std::string err;
  if (choose_geo(g, prop->multiProcessorCount, err, lists_only) != VMR_OK) return fail(nullptr, VMR_EINVAL, err.c_str());
  memset(h->prof_ms, 0, sizeof h->prof_ms); memset(h->prof_n, 0, sizeof h->prof_n);
  CK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  CK(hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
  CK(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
  CK(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
  h->ncu = prop->multiProcessorCount;
  h->use_graphs = h->opt.graph;   // (off by default: see vmr_ctx::graphs)
  const size_t rows = (size_t)L * N * N;
  CK(hipMalloc(&h->cov, rows));
  CK(hipMalloc(&h->rcls, rows));
  CK(hipMalloc(&h->sumx, 8));
  CK(hipMemsetAsync(h->sumx, 0, 8, h->stream));
  CK(hipMalloc(&h->xmax, 4));
  CK(hipMemsetAsync(h->xmax, 0, 4, h->stream));
  CK(hipMalloc(&h->npartial, 16));
  CK(hipMemsetAsync(h->npartial, 0, 16, h->stream));
  return VMR_OK;
}

// variational state and accumulation slots; reads back the data statistics (largest count, mask row classes)
int create_state(vmr_ctx* h, unsigned* xm_out) {
  Geo& g = h->g;
  const size_t rows = (size_t)g.L * g.N * g.N;
  // (64 rows of zeroed slack: the sweep over the sorted lists reads whole 64-tie steps without masks)
  CK(hipMalloc(&h->rho, (rows + 64) * g.K * 8));
  CK(hipMalloc(&h->logpr, (rows + 64) * g.K * 8));
  CK(hipMemsetAsync(h->rho + rows * g.K, 0, (size_t)64 * g.K * 8, h->stream));
  CK(hipMemsetAsync(h->logpr + rows * g.K, 0, (size_t)64 * g.K * 8, h->stream));
  ParOff o = par_off(g.L, g.Mp, g.K);
  h->par_doubles = o.total;
  CK(hipMalloc(&h->par, o.total * 8));
  CK(hipMemsetAsync(h->par, 0, o.total * 8, h->stream));
  const size_t nA = (size_t)g.L * NSLOT * g.W * 64 * g.K * 8;
  CK(hipMalloc(&h->slotA, nA)); CK(hipMemsetAsync(h->slotA, 0, nA, h->stream));
  CK(hipMalloc(&h->slotR, NSLOT * 4 * 8)); CK(hipMemsetAsync(h->slotR, 0, NSLOT * 4 * 8, h->stream));
  g.fuse_full = 1;
  CK(hipMalloc(&h->slotF, (size_t)g.L * NSLOT * g.K * 8));
  CK(hipMemsetAsync(h->slotF, 0, (size_t)g.L * NSLOT * g.K * 8, h->stream));
  CK(hipStreamSynchronize(h->stream));   // the stream is non-blocking: a plain hipMemcpy does not wait for it
  unsigned xm = 0;
  unsigned long long np2[2] = {0, 0};
  CK(hipMemcpy(&xm, h->xmax, 4, hipMemcpyDeviceToHost));
  CK(hipMemcpy(np2, h->npartial, 16, hipMemcpyDeviceToHost));
  h->n_partial = np2[0];
  h->all_full = (np2[0] == 0 && np2[1] == 0) ? 1 : 0;
  g.Y = g.mut ? (int)xm + 1 : 1;   // mirror counts 0..max(X)
  *xm_out = xm;
  return VMR_OK;
}

int scan_u32(vmr_ctx* h, unsigned* a, unsigned* bsum, size_t n) {
  const unsigned nb = (unsigned)((n + 2047) / 2048);
  hipLaunchKernelGGL(k_scan_local, dim3(nb), dim3(256), 0, h->stream, a, bsum, n);
  hipLaunchKernelGGL(k_scan_bsum, dim3(1), dim3(256), 0, h->stream, bsum, (int)nb);
  hipLaunchKernelGGL(k_scan_add, dim3(nb), dim3(256), 0, h->stream, a, bsum, n);
  CK(hipGetLastError());
  return VMR_OK;
}


// mask lists for partial rows that hold few reporters (self-reporter masks: two per row), from the bit-packed words
static int mask_lists_from_words(vmr_ctx* h) {
  Geo& g = h->g;
  const int L = g.L, K = g.K;
  const size_t T = (size_t)g.N * g.N, n = T + 1, rows = (size_t)L * T;
  if (!(h->n_partial > 0) || h->opt.no_rlists) return VMR_OK;
  unsigned long long* tot_dev = nullptr;
  unsigned* max_dev = nullptr;
  unsigned* bsum = nullptr;
  CK(hipMalloc(&h->rq, (size_t)L * n * 4));
  CK(hipMalloc(&tot_dev, (size_t)L * 8));
  CK(hipMalloc(&max_dev, 4));
  CK(hipMalloc(&bsum, (n + 2047) / 2048 * 4));
  CK(hipMemsetAsync(tot_dev, 0, (size_t)L * 8, h->stream));
  CK(hipMemsetAsync(max_dev, 0, 4, h->stream));
  const unsigned rgrid = (unsigned)std::min<size_t>(4096, (T + 255) / 256);
  for (int l = 0; l < L; ++l)
    hipLaunchKernelGGL(k_rm_count, dim3(rgrid), dim3(256), 0, h->stream, h->Rb + (size_t)l * T * g.W,
                       h->rcls + (size_t)l * T, h->rq + (size_t)l * n, tot_dev + l, max_dev, T, g.W);
  CK(hipGetLastError());
  CK(hipStreamSynchronize(h->stream));
  std::vector<unsigned long long> rl_(L), rb_(L);
  unsigned maxrow = 0;
  CK(hipMemcpy(rl_.data(), tot_dev, (size_t)L * 8, hipMemcpyDeviceToHost));
  CK(hipMemcpy(&maxrow, max_dev, 4, hipMemcpyDeviceToHost));
  h->rm_maxrow = maxrow;
  CK(hipFree(tot_dev));
  CK(hipFree(max_dev));
  bool ok32 = true;
  h->n_rm = 0;
  for (int l = 0; l < L; ++l) { rb_[l] = h->n_rm; h->n_rm += rl_[l]; ok32 = ok32 && rl_[l] < 0xffffffffull; }
  // worth it when a list row is at most a quarter of the row's mask words (and rows are short: one lane walks a row) -- and
  // for small networks whatever the bytes: the sweep's pass sums the lists on its way, a launch less per sweep where the
  // launches are what a sweep costs
  const double list_bytes = 2.0 * (double)h->n_rm + 4.0 * (double)rows, word_bytes = (double)h->n_partial * g.W * 8.0;
  if (ok32 && maxrow <= 64 && (list_bytes * 4.0 <= word_bytes || g.N <= 1024) && (size_t)g.Mp * K * 8 <= 160 * 1024) {   // (A[Mp][K] of k_mask_lists lives in LDS)
    for (int l = 0; l < L; ++l) { int rc = scan_u32(h, h->rq + (size_t)l * n, bsum, n); if (rc) return rc; }
    CK(hipMalloc(&h->rbase, (size_t)L * 8));
    CK(hipMemcpyAsync(h->rbase, rb_.data(), (size_t)L * 8, hipMemcpyHostToDevice, h->stream));
    CK(hipMalloc(&h->Rm, ((size_t)h->n_rm + 64) * 2));
    for (int l = 0; l < L; ++l)
      hipLaunchKernelGGL(k_rm_fill, dim3(rgrid), dim3(256), 0, h->stream, h->Rb + (size_t)l * T * g.W,
                         h->rcls + (size_t)l * T, h->rq + (size_t)l * n, h->Rm + rb_[l], T, g.W);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(h->stream));
  } else {
    CK(hipFree(h->rq));
    h->rq = nullptr;
    h->n_rm = 0;
  }
  CK(hipFree(bsum));
  return VMR_OK;
}

// sorted lists: the per-tie arrays the sweeps read, by position (the tie-order originals stay for the mask kernels)
// reports per level (mirror count) of the sorted lists: hist[y], y clamped to 64; empty slots (x = 0, not in R) are skipped
__global__ __launch_bounds__(256) void k_level_hist(const unsigned* __restrict__ E, unsigned long long n, int Mp, unsigned long long* __restrict__ hist) {
  __shared__ unsigned long long sh[65];
  for (int i = threadIdx.x; i < 65; i += 256) sh[i] = 0;
  __syncthreads();
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
    const unsigned e = E[i];
    if (e == 0u) continue;
    const unsigned y = SL_YM(e) / (unsigned)Mp;
    atomicAdd(&sh[y < 64u ? y : 64u], 1ull);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 65; i += 256) if (sh[i]) atomicAdd(&hist[i], sh[i]);
}

// Geo::farl: (position, entry) of the reports of levels >= g.hc, layer by layer (k_far_collect)
static int build_far_lists(vmr_ctx* h) {
  const Geo& g = h->g;
  const size_t T = (size_t)g.N * g.N, NS = (T + 63) / 64;
  unsigned long long* cnt = nullptr;
  unsigned long long* hd = nullptr;
  struct Tmp { unsigned long long*& a; unsigned long long*& b; ~Tmp() { if (a) (void)hipFree(a); if (b) (void)hipFree(b); } } tmp_guard{cnt, hd};   // (freed on every way out)
  CK(hipMalloc(&cnt, 8));
  std::vector<unsigned long long> hist(65, 0);
  CK(hipMalloc(&hd, 65 * 8));
  CK(hipMemsetAsync(hd, 0, 65 * 8, h->stream));
  hipLaunchKernelGGL(k_level_hist, dim3(1024), dim3(256), 0, h->stream, h->E, h->n_slots, g.Mp, hd);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(hist.data(), hd, 65 * 8, hipMemcpyDeviceToHost, h->stream));
  CK(hipStreamSynchronize(h->stream));
  unsigned long long far = 0;
  for (int y = std::min(g.hc, 64); y < 65; ++y) far += hist[y];   // (an upper bound: empty slots of a level count too)
  CK(hipMalloc(&h->far_pos, (size_t)(far + 64) * 4));
  CK(hipMalloc(&h->far_ent, (size_t)(far + 64) * 4));
  h->far_off.assign(g.L + 1, 0ull);
  std::vector<unsigned long long> eb(g.L);
  CK(hipMemcpy(eb.data(), h->ebase, (size_t)g.L * 8, hipMemcpyDeviceToHost));
  for (int l = 0; l < g.L; ++l) {
    hipLaunchKernelGGL(k_far_first, dim3((unsigned)std::min<size_t>(8192, (NS + 3) / 4)), dim3(256), 0, h->stream, h->E + eb[l], h->rs + (size_t)l * (NS + 1),
                       h->sy + (size_t)l * NS, NS, (unsigned)g.hc * (unsigned)g.Mp, (unsigned*)nullptr);
    CK(hipGetLastError());
    { const int rcb = sl_balance_layer(h, l, eb[l], (unsigned)g.hc * (unsigned)g.Mp); if (rcb) return rcb; }   // (before the positions are recorded)
    CK(hipMemsetAsync(cnt, 0, 8, h->stream));
    hipLaunchKernelGGL(k_far_collect, dim3((unsigned)std::min<size_t>(8192, (NS + 3) / 4)), dim3(256), 0, h->stream, h->E + eb[l], h->rs + (size_t)l * (NS + 1), NS,
                       (unsigned)g.hc * (unsigned)g.Mp, h->far_pos + h->far_off[l], h->far_ent + h->far_off[l], cnt);
    CK(hipGetLastError());
    unsigned long long n = 0;
    CK(hipMemcpyAsync(&n, cnt, 8, hipMemcpyDeviceToHost, h->stream));
    CK(hipStreamSynchronize(h->stream));
    h->far_off[l + 1] = h->far_off[l] + n;
    if (h->far_off[l + 1] > far) return fail(nullptr, VMR_EHIP, "far lists: more reports than counted");
  }
  CK(hipMalloc(&h->far_base, (size_t)(g.L + 1) * 8));
  CK(hipMemcpy(h->far_base, h->far_off.data(), (size_t)(g.L + 1) * 8, hipMemcpyHostToDevice));
  return VMR_OK;
}

// the mask lists of at most two reporters, packed by sorted position (SlArgs::rm2)
__global__ __launch_bounds__(256) void k_rm2(const unsigned* __restrict__ perm, const unsigned* __restrict__ rq, const unsigned short* __restrict__ Rm,
                                             const unsigned long long* __restrict__ rbase, unsigned* __restrict__ out, size_t T, size_t NS, int L) {
  const size_t n = (size_t)L * NS * 64;
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (size_t)gridDim.x * 256) {
    const size_t l = q / (NS * 64);
    const unsigned tie = perm[q];
    unsigned w = 0xffffffffu;
    if (tie != 0xffffffffu) {
      const unsigned q0 = rq[l * (T + 1) + tie], q1 = rq[l * (T + 1) + tie + 1];
      const unsigned short* r = Rm + rbase[l];
      const unsigned m0 = q1 > q0 ? r[q0] : 0xffffu, m1 = q1 > q0 + 1 ? r[q0 + 1] : 0xffffu;
      w = m0 | (m1 << 16);
    }
    out[q] = w;
  }
}

int sl_finish(vmr_ctx* h) {
  const Geo& g = h->g;
  const size_t rows = (size_t)g.L * g.N * g.N;
  int rc = VMR_OK;
  if (!h->all_full) {
    CK(hipMalloc(&h->cls_p, rows + 64));   // (64 entries of slack, as rho)
    CK(hipMemsetAsync(h->cls_p + rows, 0, 64, h->stream));
    if ((rc = sl_permute_u8(h, h->rcls, h->cls_p))) return rc;
  }
  if (g.mut && h->Qt) {
    CK(hipMalloc(&h->Qt_p, (rows + 64) * 4));
    CK(hipMemsetAsync(h->Qt_p + rows, 0, 64 * 4, h->stream));
    if ((rc = sl_permute_u32(h, h->Qt, h->Qt_p))) return rc;
    CK(hipStreamSynchronize(h->stream));
    CK(hipFree(h->Qt)); h->Qt = nullptr;   // (only the sweeps read it)
  }
  return VMR_OK;
}

// VMR_DETERMINISTIC=1: the fixed-point scales (Geo::det_sh, det_shr) from the sum of all counts.  xbits: bits of the largest count
// a single add into H can carry -- the sweep kernels convert such a term with the 1.5 * 2^52 trick, which holds |v| 2^sh < 2^51.
static int det_scales(vmr_ctx* h, int xbits, int shr_max) {
  Geo& g = h->g;
  unsigned long long sx = 0;
  CK(hipMemcpyAsync(&sx, h->sumx, 8, hipMemcpyDeviceToHost, h->stream));
  CK(hipStreamSynchronize(h->stream));
  int bits = 1;
  while (bits < 62 && (sx >> bits) != 0ull) ++bits;
  g.det_sh = std::max(0, std::min(51 - xbits, 61 - bits));   // (specialised kernels: counts of 11 bits, so <= 40)
  const unsigned long long eb = 64ull * (sx + (unsigned long long)g.L * g.N * g.N * g.K);
  int rbits = 1;
  while (rbits < 62 && (eb >> rbits) != 0ull) ++rbits;
  // Up to 34 the scale leaves room for eb itself (34: a term converted by the 1.5 * 2^52 trick, ELBO terms up to 2047 * |log eps| < 2^17).
  // eb is no bound on what a partial can hold -- sum over ties of rho T E[lambda] grows with E[theta] -- so a finer scale (shr_max,
  // where the terms are converted exactly) is taken only while 2^63 / 2^det_shr stays above 64 eb = 4096 (sum x + L N^2 K).
  g.det_shr = std::max(std::min(34, std::max(0, 61 - rbits)), std::min(shr_max, 57 - rbits));
  return VMR_OK;
}

// LDS shapes, the statistics / factor tables, scratch; for report lists the count-mode launch (constants C[l][y][m])
int create_tail(vmr_ctx* h, const hipDeviceProp_t& prop) {
  Geo& g = h->g;
  const int L = g.L, K = g.K;
  g.ml = (h->sparse && h->rq) ? 1 : 0;
  // (the self-reporter mask of survey data: lists of two; the general kernels take it on wide handles only, Mp > 8192)
  if (g.ml && (!g.gen || g.Mp > 8192) && h->rm_maxrow <= 2 && !h->opt.no_rm2) {
    const size_t T_ = (size_t)g.N * g.N, NS_ = (T_ + 63) / 64, n_ = (size_t)L * NS_ * 64;
    CK(hipMalloc(&h->rm2, n_ * 4));
    hipLaunchKernelGGL(k_rm2, dim3((unsigned)std::min<size_t>(4096, (n_ + 255) / 256)), dim3(256), 0, h->stream, h->perm, h->rq, h->Rm, h->rbase, h->rm2, T_, NS_, L);
    CK(hipGetLastError());
  }
  if (g.gen) {
    // the general kernels: one copy of H with every category, nothing in LDS, no constants C (sweep_gen.h)
    g.ml = 0; g.hc = 0; g.yt = 0; g.two_pass = 0;
    const double hb = (double)L * g.Y * g.Mp * K * 8.0;
    size_t fr = 0, tot = 0;
    CK(hipMemGetInfo(&fr, &tot));
    if (hb > 0.5 * (double)fr) {
      char msg[256];
      snprintf(msg, sizeof msg, "the statistics table H[L][max count + 1][M][K] would take %.1f GB (largest count %d, M = %d, K = %d): more than half "
               "of the device memory left", hb / 1e9, g.Y - 1, g.M, K);
      return fail(nullptr, VMR_EINVAL, msg);
    }
    CK(hipMalloc(&h->Hg, (size_t)hb));
    CK(hipMemsetAsync(h->Hg, 0, (size_t)hb, h->stream));
    CK(hipMalloc(&h->gen_s1, (size_t)L * (g.Mp + K + 1) * 8));   // (zero between uses: the readers zero what they read)
    CK(hipMemsetAsync(h->gen_s1, 0, (size_t)L * (g.Mp + K + 1) * 8, h->stream));
    CK(hipMalloc(&h->elbo_dev, 8 * 8));
    CK(hipMemsetAsync(h->elbo_dev, 0, 8 * 8, h->stream));
    CK(hipMalloc(&h->nu_acc, (size_t)(3 + L) * 8));
    CK(hipMemsetAsync(h->nu_acc, 0, (size_t)(3 + L) * 8, h->stream));
    CK(hipMalloc(&h->lutg, (size_t)L * g.W * 256 * 8));
    CK(hipMemsetAsync(h->lutg, 0, (size_t)L * g.W * 256 * 8, h->stream));
    if (g.det) {
      // VMR_DETERMINISTIC=1: H, the slots and gen_s1 hold the integer sums themselves (sweep_gen.hip), no shadow; the fixed point
      // of H leaves room for the sum of all counts and for the largest count in one add
      if (!h->sparse) return fail(nullptr, VMR_EINVAL, "VMR_DETERMINISTIC=1 needs the report lists (a sparse tensor)");
      unsigned xm = 0;
      CK(hipMemcpyAsync(&xm, h->xmax, 4, hipMemcpyDeviceToHost, h->stream));
      CK(hipStreamSynchronize(h->stream));
      int xbits = 1;
      while (xbits < 32 && (xm >> xbits) != 0u) ++xbits;
      int rc = det_scales(h, xbits, 34);
      if (rc) return rc;
      // sums of rho: a 64-bit cell (or a lane's sum) holds at most N^2 ties' worth; 2^-50 at most (the conversion trick, rho <= 1).
      // (A fixed 2^-30 moved a K = 12 fit with many nearly empty categories 5e-8 from the default mode.)
      const unsigned long long T_ = (unsigned long long)g.N * g.N;
      int tbits = 1;
      while (tbits < 62 && (T_ >> tbits) != 0ull) ++tbits;
      g.det_sha = std::min(50, 62 - tbits);
      CK(hipMalloc(&h->fr_slots, (size_t)L * FR_G * 2 * 8));
      CK(hipMemsetAsync(h->fr_slots, 0, (size_t)L * FR_G * 2 * 8, h->stream));
    }
    CK(hipStreamSynchronize(h->stream));
    return VMR_OK;
  }
  // LDS levels (mirror counts 0..) of the statistics H and, for report lists, of the factor table F.
  g.hc = g.Y < HC_MAX ? g.Y : HC_MAX;
  g.yt = 0;
  g.two_pass = 0;
  size_t need = 0;
  if (h->sparse) {
    // Sorted lists: the populous levels of F (read) and H (float atomics) in LDS, shared by all waves of a workgroup; no per-wave
    // LDS at all.  One pass per sweep when every level of both fits at >= 16 waves per CU (or the levels beyond hold under 0.1 %
    // of the reports), else the rho pass keeps F and a statistics pass rebuilds H (two passes over the entries).
    const VmrOpts& o = h->opt;
    const int want = std::max(1, std::min(g.Y, o.levels));   // as many levels as fit: with all of them in LDS nothing is "far"
    // a variant's largest workgroup / waves per CU (registers): the statistics-only variant is lighter than the update's
    auto cap_of = [&](bool upd) { return sl_tpb_max(K, false, h->all_full != 0, upd); };
    auto wcu_of = [&](bool upd) { return 4 * sl_wpe(K, false, h->all_full != 0, upd); };
    auto waves = [&](int tpb, int yt, int hc, bool upd, bool hist) {
      const size_t b = sl_smem(g, yt, hc, upd, false, hist);
      if (b > SP_LDS_MAX || tpb > cap_of(upd)) return 0;
      const int nw = tpb / 64, wgs = std::min((int)(SP_LDS_MAX / b), wcu_of(upd) / nw);
      return wgs * nw;
    };
    auto best = [&](bool upd, bool hist, int min_waves, int& lv_out, int& tpb_out) {
      min_waves = std::min(min_waves, wcu_of(upd));
      for (int lv = want; lv >= 1; --lv) {
        int bw = 0, bt = 256;
        for (int tpb : {1024, 768, 512, 256}) { const int w = waves(tpb, upd ? lv : 0, hist ? lv : 0, upd, hist); if (w > bw) { bw = w; bt = tpb; } }
        if (bw >= min_waves) { lv_out = lv; tpb_out = bt; return true; }
      }
      return false;
    };
    int lv1 = 0, t1 = 256, lvr = 0, tr = 256, lvh = 0, th = 256;
    bool want_farl = false;
    bool one = best(true, true, 16, lv1, t1);
    if (one && lv1 < want && g.N > 1024) {   // (small networks: one pass whatever the levels -- a sweep there costs its launches)
      // Not every level fits beside the other table.  A report of a level beyond the LDS ones costs its whole 64-tie round the
      // slow path (the factor formula, a global add), so one pass only pays while such reports are rare: count the reports
      // per level.  (BASELINE config 5 -- M = 1000, K = 3: 3 levels of each fit, 2.5 % of the reports lie beyond, four rounds
      // of five hold one; the two passes keep 6 levels of F and 9 of H.)
      std::vector<unsigned long long> hist(65, 0);
      unsigned long long* hd = nullptr;
      CK(hipMalloc(&hd, 65 * 8));
      CK(hipMemsetAsync(hd, 0, 65 * 8, h->stream));
      hipLaunchKernelGGL(k_level_hist, dim3(1024), dim3(256), 0, h->stream, h->E, h->n_slots, g.Mp, hd);
      CK(hipGetLastError());
      CK(hipMemcpyAsync(hist.data(), hd, 65 * 8, hipMemcpyDeviceToHost, h->stream));
      CK(hipStreamSynchronize(h->stream));
      CK(hipFree(hd));
      unsigned long long tot = 0, far = 0;
      for (int y = 0; y < 65; ++y) { tot += hist[y]; if (y >= lv1) far += hist[y]; }
      if ((double)far > (double)tot / 1024.0) {
        // VMR_FARL=1 (round 4; off by default): still one pass while the far reports are a few per cent -- the pass takes their factors
        // by formula and leaves their statistics to k_far_hist, which adds them from a compact list of exactly those reports, moved
        // to the front of every tie's list (k_far_first).  Measured on a BASELINE config-5 layer: 3.44 ms per sweep against 3.53
        // with two passes, and ELBO sweeps the other way round -- no gain over ten sweeps, so two passes stay.
        // Not in the deterministic mode (its sums are the integer shadows').
        if (g.mut && !g.det && o.farl && (double)far <= 0.125 * (double)tot) want_farl = true;
        else one = false;
      }
    }
    one = one && !o.two_pass;
    if (one) { g.yt = g.hc = lv1; h->sp_tpb = h->st_tpb = t1; g.farl = want_farl ? 1 : 0; }
    else {
      g.two_pass = 1;
      if (!best(true, false, 16, lvr, tr) && !best(true, false, 4, lvr, tr)) { lvr = 0; tr = 256; }
      if (!best(false, true, 16, lvh, th) && !best(false, true, 4, lvh, th)) { lvh = 0; th = 256; }
      g.yt = lvr; g.hc = lvh; h->sp_tpb = tr; h->st_tpb = th;
    }
    {   // small datasets: smaller workgroups, so that the steps spread over every CU
      const long long NS = ((long long)g.N * g.N + 63) / 64;
      for (int* t : {&h->sp_tpb, &h->st_tpb})
        while (*t > 64 && NS * L < (long long)h->ncu * (*t / 64)) *t = std::max(64, (*t / 2) & ~63);   // (768 -> 384 -> 192 -> 64)
    }
    g.yt = std::max(0, std::min(g.Y, o.yt >= 0 ? o.yt : g.yt));
    g.hc = std::max(0, std::min(g.Y, o.hc >= 0 ? o.hc : g.hc));
    if (o.tpb >= 64 && o.tpb <= 1024 && o.tpb % 64 == 0) h->sp_tpb = o.tpb;
    if (o.st_tpb >= 64 && o.st_tpb <= 1024 && o.st_tpb % 64 == 0) h->st_tpb = o.st_tpb;
    for (int v = 0; v < 4; ++v) need = std::max(need, sl_shape(h, v != 3, v == 1 || v == 2, v == 0 || v == 1 || v == 3).smem);
    if (g.two_pass && g.mut && !g.det && g.Y > 1 && !o.no_level0) {
      // Two passes (a wide reporter dimension): the statistics pass is bound by its LDS adds, and at mirror count 0 -- more than half
      // of the reports of a mutual network -- none is needed (SlArgs::h0s): every tie's reports of count >= 1 go first, sy's high half
      // gets the first round of a step that holds level 0 only.
      const size_t T_ = (size_t)g.N * g.N, NS_ = (T_ + 63) / 64;
      std::vector<unsigned long long> eb(L);
      CK(hipMemcpy(eb.data(), h->ebase, (size_t)L * 8, hipMemcpyDeviceToHost));
      if (!o.no_x0) CK(hipMalloc(&h->x0p, (size_t)L * NS_ * 64 * 4));
      for (int l = 0; l < L; ++l)
        hipLaunchKernelGGL(k_far_first, dim3((unsigned)std::min<size_t>(8192, (NS_ + 3) / 4)), dim3(256), 0, h->stream, h->E + eb[l], h->rs + (size_t)l * (NS_ + 1),
                           h->sy + (size_t)l * NS_, NS_, (unsigned)g.Mp, h->x0p ? h->x0p + (size_t)l * NS_ * 64 : nullptr);
      CK(hipGetLastError());
      for (int l = 0; l < L; ++l) { const int rcb = sl_balance_layer(h, l, eb[l], (unsigned)g.Mp); if (rcb) return rcb; }
      if (h->x0p) {
        unsigned long long* ss = nullptr;
        CK(hipMalloc(&ss, 8));
        CK(hipMemsetAsync(ss, 0, 8, h->stream));
        for (int l = 0; l < L; ++l)
          hipLaunchKernelGGL(k_stat_slots, dim3(256), dim3(256), 0, h->stream, h->rs + (size_t)l * (NS_ + 1), h->sy + (size_t)l * NS_, NS_, ss);
        hipError_t es = hipMemcpyAsync(&h->stat_slots, ss, 8, hipMemcpyDeviceToHost, h->stream);
        if (es == hipSuccess) es = hipStreamSynchronize(h->stream);
        (void)hipFree(ss);
        CK(es);
      }
      const size_t n0 = (size_t)L * NSLOT * K;
      CK(hipMalloc(&h->h0s, n0 * 8));
      CK(hipMemsetAsync(h->h0s, 0, n0 * 8, h->stream));
    }
    if (g.farl) {
      // the far lists hold the reports of levels >= g.hc: every variant that adds to H must keep exactly the levels below in LDS
      bool same = g.hc >= 1 && g.hc < g.Y;
      for (int v : {0, 3}) same = same && sl_shape(h, v != 3, false, true).hc == g.hc;
      h->elbo_split = sl_shape(h, true, true, true).hc != g.hc || sl_shape(h, true, true, true).yt != g.yt;   // (the fused ELBO variant also holds the logarithm table)
      if (!same) g.farl = 0;   // (shapes forced through VMR_YT / VMR_HC / VMR_TPB: the pass then adds the far reports itself, global adds)
      else { int rcf = build_far_lists(h); if (rcf) return rcf; }
    }
  } else {
    if (shmem_rho(g, true, false) > 80000) {
      g.two_pass = 1;
      while (g.hc > 0 && shmem_hist(g) > 160000) --g.hc;
    }
    need = std::max(shmem_rho(g, true, true), shmem_hist(g));
  }
  // per-reporter tables live in LDS (dense tiles: E[log theta], the mutuality weights c[m,k], G_theta for the ELBO:
  // (K + 2) * 8 bytes per reporter).  160 KB per workgroup on gfx950.
  if (need > (size_t)prop.sharedMemPerBlock && need > 160 * 1024) {
    char msg[256];
    snprintf(msg, sizeof msg, "M = %d reporters with K = %d%s needs %zu bytes of LDS per workgroup (limit %d): "
             "reduce M or K", g.M, K, g.mut ? " and mutuality" : "", need, 160 * 1024);
    return fail(nullptr, VMR_EINVAL, msg);
  }
  CK(hipMalloc(&h->Hg, (size_t)L * NH * g.Y * g.Mp * K * 8));
  CK(hipMemsetAsync(h->Hg, 0, (size_t)L * NH * g.Y * g.Mp * K * 8, h->stream));
  CK(hipMalloc(&h->elbo_dev, 8 * 8));   // [0..3] results, [4..6] scratch of k_fin_rho
  CK(hipMemsetAsync(h->elbo_dev, 0, 8 * 8, h->stream));
  CK(hipMalloc(&h->nu_acc, (size_t)(3 + L) * 8));   // the nu update inside the pass (SlArgs::nu_acc)
  CK(hipMemsetAsync(h->nu_acc, 0, (size_t)(3 + L) * 8, h->stream));
  // k_fin_gamma: per layer 2 K sums and a ticket; behind them, for the deterministic mode, every workgroup's own 2 K sums
  CK(hipMalloc(&h->fin_g, ((size_t)L * (2 * KMAX + 2) + (size_t)L * FG_G * 2 * KMAX) * 8));
  CK(hipMemsetAsync(h->fin_g, 0, ((size_t)L * (2 * KMAX + 2) + (size_t)L * FG_G * 2 * KMAX) * 8, h->stream));
  if (g.det) {
    // VMR_DETERMINISTIC=1 (sorted report lists only): see SlArgs::det.  The fixed point of the count-weighted sums leaves
    // room for the sum of all counts.
    if (!h->sparse) return fail(nullptr, VMR_EINVAL, "VMR_DETERMINISTIC=1 needs the report lists (a sparse tensor with M <= 8192, counts <= 2047)");
    int rc = det_scales(h, 11, 45);   // (packed entries: counts up to 2047; the ELBO terms are converted exactly, whatever their size)
    if (rc) return rc;
    // sums of rho: a 64-bit cell holds at most N^2 ties' worth, and one conversion a wave's 64 values (64 rho 2^42 < 2^51 up to rho = 4).
    // (A fixed 2^-30 left gamma_rte 1.3e-9 from the reference where most rows of rho are all zero and a category's few tiny values
    // meet a large E[lambda]: tests/test_hip_exp_range.py.)
    const unsigned long long T_ = (unsigned long long)g.N * g.N;
    int tbits = 1;
    while (tbits < 62 && (T_ >> tbits) != 0ull) ++tbits;
    g.det_sha = std::min(42, 62 - tbits);
    const size_t nd = (size_t)L * g.Y * g.Mp * K + (size_t)L * g.W * 64 * K + (size_t)L * K + 5;
    CK(hipMalloc(&h->det_buf, nd * 8));
    CK(hipMemsetAsync(h->det_buf, 0, nd * 8, h->stream));
    CK(hipMalloc(&h->fr_slots, (size_t)L * FR_G * 2 * 8));
    CK(hipMemsetAsync(h->fr_slots, 0, (size_t)L * FR_G * 2 * 8, h->stream));
  }
  CK(hipMalloc(&h->lutg, (size_t)L * g.W * 256 * 8));
  CK(hipMemsetAsync(h->lutg, 0, (size_t)L * g.W * 256 * 8, h->stream));
  if (h->sparse) {
    // the constants C[l][y][m] = sum of the counts per (mirror count, reporter): one statistics launch in count mode
    CK(hipMalloc(&h->Cg, (size_t)L * g.Y * g.Mp * 8));
    int rc = VMR_OK;
    {
      const SlShape sh = sl_shape(h, false, false, true);
      SlArgs a = sl_args(h, sh, 2);
      rc = sl_launch(h, 3, sh, a);
      if (rc == VMR_OK && g.farl) rc = launch_far(h, 1, -1);
    }
    if (rc != VMR_OK) { g_create_err = h->err; return rc; }
    CK(hipGetLastError());
    if ((rc = take_counts(h))) return rc;
  }
  CK(hipStreamSynchronize(h->stream));
  return VMR_OK;
}

static int create_dense(vmr_ctx* h, const hipDeviceProp_t& prop, const uint8_t* X, const uint8_t* R, int data_on_device) {
  Geo& g = h->g;
  const int L = g.L, N = g.N, M = g.M;
  const size_t T = (size_t)N * N, rows = (size_t)L * T, raw = rows * M;
  const size_t slack = (size_t)g.b * N + g.b;   // tile streams may read (never use) rows past the last tie
  CK(hipMalloc(&h->X, (rows + slack) * g.Mp));
  CK(hipMemsetAsync(h->X + rows * g.Mp, 0, slack * g.Mp, h->stream));
  CK(hipMalloc(&h->Rb, (rows + slack) * g.W * 8));
  CK(hipMemsetAsync(h->Rb + rows * g.W, 0, slack * g.W * 8, h->stream));
  {
    uint8_t* tmp = nullptr;
    const uint8_t* src = X;
    if (!data_on_device) { CK(hipMalloc(&tmp, raw)); CK(hipMemcpyAsync(tmp, X, raw, hipMemcpyHostToDevice, h->stream)); src = tmp; }
    hipLaunchKernelGGL(k_pack_x, dim3(4096), dim3(256), 0, h->stream, src, h->X, rows, M, g.Mp);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(h->stream));
    if (tmp) CK(hipFree(tmp));
    tmp = nullptr; src = R;
    if (R && !data_on_device) { CK(hipMalloc(&tmp, raw)); CK(hipMemcpyAsync(tmp, R, raw, hipMemcpyHostToDevice, h->stream)); src = tmp; }
    hipLaunchKernelGGL(k_pack_r, dim3(4096), dim3(256), 0, h->stream, src, h->Rb, rows, M, g.W);
    CK(hipGetLastError());
    hipLaunchKernelGGL(k_stats, dim3(2048), dim3(256), 0, h->stream, h->X, h->Rb, h->cov, h->rcls, h->sumx, h->xmax, h->npartial, rows, g.Mp, g.W, M);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(h->stream));
    if (tmp) CK(hipFree(tmp));
  }
  unsigned xm = 0;
  int rc = create_state(h, &xm);
  if (rc) return rc;
  // ---- data format: report lists unless X is dense enough that 1 B per (tie, reporter) is less to read ----
  const bool force_dense = h->opt.format == 1, force_sparse = h->opt.format == 2;
  // 13-bit reporter field; the sorted lists hold counts <= 2047 and (max count + 1) * Mp <= 2^20 table rows, the step layout counts <= 63
  const bool packed_ok = g.Mp <= 8192 && xm <= SL_XMAX && (size_t)(xm + 1) * g.Mp <= SL_YM_ROWS;
  // beyond KMAX categories there is no dense-tile kernel: the general kernels run on report lists, with wide entries where the
  // packed ones cannot hold the tensor (a uint8 tensor always fits: 256 levels x Mp rows < 2^32)
  const bool need_lists = g.K > KMAX;
  if (need_lists && force_dense) return fail(nullptr, VMR_EINVAL, "VMR_FORMAT=dense: the dense tile kernels hold at most 8 categories");
  // ... and so do tensors the dense tiles cannot hold at all (their per-reporter tables outgrow the LDS: M of several thousand)
  bool dense_fits = true;
  {
    Geo t = g;   // (what create_tail would settle on for the dense tiles)
    t.Y = g.Y; t.hc = t.Y < HC_MAX ? t.Y : HC_MAX;
    if (shmem_rho(t, true, false) > 80000) { t.two_pass = 1; while (t.hc > 0 && shmem_hist(t) > 160000) --t.hc; }
    dense_fits = std::max(shmem_rho(t, true, true), shmem_hist(t)) <= (size_t)160 * 1024;
  }
  const bool can_list = packed_ok || need_lists || force_sparse || !dense_fits;   // (VMR_FORMAT=sparse: wide entries for what the packed ones cannot hold)
  if (!force_dense && can_list) {
    g.wide = packed_ok ? 0 : 1;
    unsigned* rp = nullptr;   // [L][T+1] per-tie entry offsets: only needed to place the entries
    CK(hipMalloc(&rp, (size_t)L * (T + 1) * 4));
    unsigned long long* nnz_dev = nullptr;
    CK(hipMalloc(&nnz_dev, (size_t)L * 8));
    CK(hipMemsetAsync(nnz_dev, 0, (size_t)L * 8, h->stream));
    const unsigned cgrid = (unsigned)std::min<size_t>(8192, (T + 15) / 16);
    for (int l = 0; l < L; ++l)
      hipLaunchKernelGGL(k_sp_count, dim3(cgrid), dim3(256), 0, h->stream, h->X + (size_t)l * T * g.Mp,
                         rp + (size_t)l * (T + 1), nnz_dev + l, g);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(h->stream));
    std::vector<unsigned long long> nl(L);
    CK(hipMemcpy(nl.data(), nnz_dev, (size_t)L * 8, hipMemcpyDeviceToHost));
    CK(hipFree(nnz_dev));
    bool fits = true;
    h->nnz = 0;
    for (int l = 0; l < L; ++l) { h->nnz += nl[l]; fits = fits && nl[l] < 0xffffffffull; }
    const double sparse_bytes = 4.0 * (double)h->nnz + 4.0 * (double)rows, dense_bytes = (double)rows * g.Mp;
    if (need_lists && !fits) { (void)hipFree(rp); return fail(nullptr, VMR_EINVAL, "more than 2^32 reports in one layer"); }
    h->sparse = fits && (force_sparse || need_lists || !dense_fits || sparse_bytes <= 0.5 * dense_bytes);
    if (!h->sparse) g.wide = 0;
    g.gen = (h->sparse && (need_lists || g.wide)) ? 1 : 0;
    if (h->sparse) {
      CK(hipMalloc(&h->Qt, rows * 4));
      CK(hipMemsetAsync(h->Qt, 0, rows * 4, h->stream));
      auto fill_layer = [&](int l, const unsigned* rpl, unsigned* etmp, unsigned* etmp2) {
        if (g.mut)
          hipLaunchKernelGGL(k_sp_fill<true>, dim3(cgrid), dim3(256), 0, h->stream, h->X + (size_t)l * T * g.Mp,
                             h->Rb + (size_t)l * T * g.W, rpl, etmp, etmp2, h->Qt + (size_t)l * T, g);
        else
          hipLaunchKernelGGL(k_sp_fill<false>, dim3(cgrid), dim3(256), 0, h->stream, h->X + (size_t)l * T * g.Mp,
                             h->Rb + (size_t)l * T * g.W, rpl, etmp, etmp2, h->Qt + (size_t)l * T, g);
      };
      {
        const SlFill ff = fill_layer;
        rc = sl_place_entries(h, rp, nl, nullptr, nullptr, &ff);
        if (!rc) rc = sl_finish(h);
      }
      if (!rc) rc = mask_lists_from_words(h);
      if (!rc) { CK(hipFree(h->X)); h->X = nullptr; }   // the lists replace the dense tensor
    }
    CK(hipFree(rp));
    if (rc) return rc;
  } else if (force_sparse) {
    return fail(nullptr, VMR_EINVAL, "VMR_FORMAT=sparse needs M <= 8192, counts <= 2047 and (largest count + 1) * M <= 2^20");
  }
  return create_tail(h, prop);
}

extern "C" int vmr_create(vmr_handle* out, int device, int L, int N, int M, int K, int mutuality, const uint8_t* X,
                          const uint8_t* R, int data_on_device, double eps) {
  if (!out) return fail(nullptr, VMR_EINVAL, "out is NULL");
  *out = nullptr;
  if (L < 1 || N < 1 || M < 1) return fail(nullptr, VMR_EINVAL, "L, N, M must be positive");
  if (K < 2 || K > KGEN_MAX) return fail(nullptr, VMR_EINVAL, "K must be in [2, 256]");
  if (!X) return fail(nullptr, VMR_EINVAL, "X is NULL");
  vmr_ctx* h = nullptr;
  hipDeviceProp_t prop;
  int rc = create_ctx(&h, &prop, device, L, N, M, K, mutuality, eps);
  if (!rc) rc = create_dense(h, prop, X, R, data_on_device);
  if (rc) { if (h) vmr_destroy(h); return rc; }
  *out = h;
  return VMR_OK;
}

extern "C" void vmr_destroy(vmr_handle h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (auto& e : h->evs) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  for (auto& e : h->graphs) (void)hipGraphExecDestroy(e.ex);
  void* ptrs[] = {h->drw, h->x0p, h->h0s, h->far_pos, h->far_ent, h->far_base, h->EX, h->gen_s1, h->rm2, h->det_buf, h->fr_slots, h->nu_acc, h->fin_g, h->perm, h->sy, h->cls_p, h->Qt_p, h->nat, h->rho_snap, h->par_snap, h->rq, h->Rm, h->rbase, h->E, h->rs, h->Cg, h->Qt, h->ebase, h->rcls, h->X, h->Rb, h->cov, h->sumx, h->rho, h->logpr, h->lpd, h->lpb, h->par, h->slotA, h->slotR, h->elbo_dev, h->lutg, h->Hg, h->xmax, h->slotF, h->npartial};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  if (h->stream2) { (void)hipStreamSynchronize(h->stream2); (void)hipStreamDestroy(h->stream2); }
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}
