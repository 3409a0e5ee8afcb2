// create_coo.hip -- vmr_create_coo, once per handle; the steps it shares with vmr_create are create.h's.
#include "create.h"

// ------------------------------------------------------------------------------------------
// vmr_create_coo: coordinate lists (what the reference holds: sptensor subs / vals, model.py:136-171; the reader's output,
// _io.py:132-295) straight to report lists -- no dense [L,N,N,M] tensor anywhere.  A Karnataka village layer is 624
// reports against a 34 MB dense tensor; a layer of BASELINE config 5 is 5 GB of reports against 64 GB.
// Reports and mask entries are sorted by (layer, tie, reporter) (one 64-bit radix sort each); sorted order IS the tie-major
// order k_sp_round consumes, the mirror count and the mask bit of a report are binary searches in the sorted keys, and a
// sparse mask becomes the mask lists directly.
// A key is tie << mb | m, with mb = max(13, ceil(log2 Mp)) bits for the reporter (vmr_ctx::coo_mb): 13 up to Mp = 8192, up to
// 16 at M = 65535 (the mask lists hold 16-bit reporters).
// ------------------------------------------------------------------------------------------
#define COO_KEY(tie, m, mb) (((unsigned long long)(tie) << (mb)) | (unsigned long long)(m))
#define COO_M(key, mb) ((unsigned)((key) & ((1ull << (mb)) - 1ull)))

__global__ void k_coo_keys(const int32_t* __restrict__ sl, const int32_t* __restrict__ si, const int32_t* __restrict__ sj,
                           const int32_t* __restrict__ sm, long long n, int L, int N, int M, int mb, unsigned long long* __restrict__ keys,
                           int* bad) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
    const int l = sl[e], i = si[e], j = sj[e], m = sm[e];
    if (l < 0 || l >= L || i < 0 || i >= N || j < 0 || j >= N || m < 0 || m >= M) { atomicOr(bad, 1); keys[e] = ~0ull; continue; }
    keys[e] = COO_KEY(((unsigned long long)l * N + i) * N + j, m, mb);
  }
}
// index of `key` in the sorted keys, or -1
__device__ __forceinline__ long long coo_find(const unsigned long long* __restrict__ k, long long n, unsigned long long key) {
  long long a = 0, b = n;
  while (a < b) {
    const long long c = a + ((b - a) >> 1);
    if (k[c] < key) a = c + 1; else b = c;
  }
  return (a < n && k[a] == key) ? a : -1;
}
// per-tie counts of the sorted keys (cnt [L][T+1], layer-relative ties); duplicates flagged
__global__ void k_coo_count(const unsigned long long* __restrict__ k, long long n, size_t T, int mb, unsigned* __restrict__ cnt, int* bad) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
    if (e > 0 && k[e] == k[e - 1]) atomicOr(bad, 2);
    const unsigned long long tie = k[e] >> mb, l = tie / T;
    atomicAdd(&cnt[l * (T + 1) + (tie - l * T)], 1u);
  }
}
// per tie: coverage, mask row class, statistics of the partial rows
__global__ void k_coo_class(const unsigned* __restrict__ cx, const unsigned* __restrict__ cr /*null: all ones*/, size_t T, int L, int M,
                            uint8_t* __restrict__ cov, uint8_t* __restrict__ rcls, unsigned long long* npartial, unsigned* maxrow) {
  unsigned long long lpart = 0, lempty = 0;
  unsigned mx = 0;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < (size_t)L * T; q += (size_t)gridDim.x * blockDim.x) {
    const size_t l = q / T, t = q - l * T;
    const unsigned nX = cx[l * (T + 1) + t], nR = cr ? cr[l * (T + 1) + t] : (unsigned)M;
    cov[q] = (nX > 0 && nR > 0) ? 1 : 0;
    const unsigned c = nR == 0 ? 0u : (nR == (unsigned)M ? 1u : 2u);
    rcls[q] = (uint8_t)c;
    if (c == 2u) { ++lpart; mx = max(mx, nR); }
    if (c == 0u) ++lempty;
  }
  if (lpart) atomicAdd(npartial, lpart);
  if (lempty) atomicAdd(npartial + 1, lempty);
  if (mx) atomicMax(maxrow, mx);
}
// the reports' entries in tie-major (= sorted) order, the mirror sums Qt, sum and maximum of the counts
template <bool MUT>
__global__ void k_coo_entries(const unsigned long long* __restrict__ kx, const unsigned* __restrict__ vx, long long nx,
                              const unsigned long long* __restrict__ kr, long long nr /* < 0: all ones */, int N, int Mp, int mb,
                              unsigned* __restrict__ etmp, unsigned* __restrict__ etmp2, unsigned* __restrict__ Qt, unsigned long long* sumx, unsigned* xmax, int* bad) {
  unsigned long long s = 0;
  unsigned mx = 0;
  const unsigned long long T = (unsigned long long)N * N;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < nx; e += (long long)gridDim.x * blockDim.x) {
    const unsigned long long key = kx[e], tie = key >> mb, l = tie / T, t = tie - l * T, i = t / N, j = t - i * N;
    const unsigned m = COO_M(key, mb), x = vx[e];
    if (x == 0u || x > 0x7fffffffu) { atomicOr(bad, 4); continue; }   // (int32 values: zero or negative)
    s += x; mx = max(mx, x);
    const unsigned long long tm = l * T + j * N + i;
    unsigned y = 0;
    if (MUT) {
      const long long f = coo_find(kx, nx, COO_KEY(tm, m, mb));
      y = f >= 0 ? vx[f] : 0u;
      if (nr < 0 || coo_find(kr, nr, COO_KEY(tm, m, mb)) >= 0) atomicAdd(&Qt[tm], x);   // R[mirror, m] X[this, m]
    }
    const unsigned inr = (nr < 0 || coo_find(kr, nr, key) >= 0) ? 1u : 0u;
    // two words per entry (sweep_sl.h, wide entries); k_coo_pack folds them into one where the packed format holds the tensor
    const unsigned long long row = (unsigned long long)y * (unsigned)Mp + m;
    if (row > 0xffffffffull) atomicOr(bad, 8);
    etmp[e] = (unsigned)row;
    etmp2[e] = (x << 1) | inr;
  }
  if (s) atomicAdd(sumx, s);
  if (mx) atomicMax(xmax, mx);
}
__global__ void k_coo_pack(unsigned* __restrict__ etmp, const unsigned* __restrict__ etmp2, long long n) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
    const unsigned w = etmp2[e];
    etmp[e] = etmp[e] | ((w & 1u) << 20) | ((w >> 1) << 21);
  }
}
// first sorted key of every layer (starts[L] = n)
__global__ void k_coo_layer_starts(const unsigned long long* __restrict__ k, long long n, unsigned long long T, int L, int mb, unsigned long long* starts) {
  for (int l = threadIdx.x; l <= L; l += blockDim.x) {
    const unsigned long long k0 = ((unsigned long long)l * T) << mb;
    long long a = 0, b = n;
    while (a < b) { const long long c = a + ((b - a) >> 1); if (k[c] < k0) a = c + 1; else b = c; }
    starts[l] = (unsigned long long)a;
  }
}
// listed counts of the partial rows only
__global__ void k_coo_listed(const unsigned* __restrict__ cr, const uint8_t* __restrict__ rcls, size_t T, int L, unsigned* __restrict__ rq) {
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < (size_t)L * (T + 1); q += (size_t)gridDim.x * blockDim.x) {
    const size_t l = q / (T + 1), t = q - l * (T + 1);
    rq[q] = (t < T && rcls[l * T + t] == 2) ? cr[q] : 0u;
  }
}
// reporters of the partial rows into the mask lists (rq scanned per layer; rbase: layer offsets)
__global__ void k_coo_rm(const unsigned long long* __restrict__ kr, long long nr, size_t T, int mb, const uint8_t* __restrict__ rcls,
                         const unsigned* __restrict__ rq, const unsigned long long* __restrict__ rbase, unsigned short* __restrict__ Rm) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < nr; e += (long long)gridDim.x * blockDim.x) {
    const unsigned long long tie = kr[e] >> mb, l = tie / T, t = tie - l * T;
    if (rcls[tie] != 2) continue;
    long long a = 0, b = e;   // first entry of this tie: lower bound of tie << mb in [0, e]
    const unsigned long long k0 = tie << mb;
    while (a < b) { const long long c = a + ((b - a) >> 1); if (kr[c] < k0) a = c + 1; else b = c; }
    Rm[rbase[l] + rq[l * (T + 1) + t] + (unsigned long long)(e - a)] = (unsigned short)COO_M(kr[e], mb);
  }
}
// a mask whose partial rows are long: bit-packed words as in the dense path
__global__ void k_coo_rbits(const unsigned long long* __restrict__ kr, long long nr, int W, int mb, unsigned long long* __restrict__ Rb) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < nr; e += (long long)gridDim.x * blockDim.x) {
    const unsigned long long tie = kr[e] >> mb;
    const unsigned m = COO_M(kr[e], mb);
    atomicOr(&Rb[tie * W + (m >> 6)], 1ull << (m & 63));
  }
}

// sorted keys (and values) of a coordinate list on the device; *k_out, *v_out are hipMalloc'ed
static int coo_sorted(vmr_ctx* h, long long n, const int32_t* sl, const int32_t* si, const int32_t* sj, const int32_t* sm,
                      const int32_t* sv, int on_device, unsigned long long** k_out, unsigned** v_out, int* bad_dev) {
  const Geo& g = h->g;
  *k_out = nullptr;
  if (v_out) *v_out = nullptr;
  const size_t nn = (size_t)std::max<long long>(n, 1);
  const int32_t* src[5] = {sl, si, sj, sm, sv};
  int32_t* tmp[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  const int ncol = sv ? 5 : 4;
  if (!on_device) {
    for (int c = 0; c < ncol; ++c) {
      CK(hipMalloc(&tmp[c], nn * 4));
      if (n > 0) CK(hipMemcpyAsync(tmp[c], src[c], (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
      src[c] = tmp[c];
    }
  }
  unsigned long long *k0 = nullptr, *k1 = nullptr;
  unsigned* v1 = nullptr;
  CK(hipMalloc(&k0, nn * 8));
  CK(hipMalloc(&k1, nn * 8));
  if (sv) CK(hipMalloc(&v1, nn * 4));
  const unsigned grid = (unsigned)std::min<long long>(4096, (n + 255) / 256 + 1);
  const int mb = h->coo_mb;
  hipLaunchKernelGGL(k_coo_keys, dim3(grid), dim3(256), 0, h->stream, src[0], src[1], src[2], src[3], n, g.L, g.N, g.M, mb, k0, bad_dev);
  CK(hipGetLastError());
  int bits = mb;   // (the sort's bit range: mb reporter bits and ceil(log2(L N^2)) tie bits; create_coo checked it is <= 64)
  { unsigned long long ties = (unsigned long long)g.L * g.N * g.N; while ((1ull << (bits - mb)) < ties && bits < 64) ++bits; }
  size_t tb = 0;
  void* td = nullptr;
  if (n > 0) {
    if (sv) CK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, k0, k1, reinterpret_cast<const unsigned*>(src[4]), v1, (int)n, 0, bits, h->stream));
    else CK(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, k0, k1, (int)n, 0, bits, h->stream));
    CK(hipMalloc(&td, tb ? tb : 8));
    if (sv) CK(hipcub::DeviceRadixSort::SortPairs(td, tb, k0, k1, reinterpret_cast<const unsigned*>(src[4]), v1, (int)n, 0, bits, h->stream));
    else CK(hipcub::DeviceRadixSort::SortKeys(td, tb, k0, k1, (int)n, 0, bits, h->stream));
  }
  CK(hipStreamSynchronize(h->stream));
  if (td) CK(hipFree(td));
  CK(hipFree(k0));
  for (int c = 0; c < ncol; ++c) if (tmp[c]) CK(hipFree(tmp[c]));
  *k_out = k1;
  if (v_out) *v_out = v1;
  return VMR_OK;
}

static int create_coo(vmr_ctx* h, const hipDeviceProp_t& prop, long long nx, const int32_t* xl, const int32_t* xi, const int32_t* xj,
                      const int32_t* xm, const int32_t* xv, long long nr, const int32_t* rl, const int32_t* ri, const int32_t* rj,
                      const int32_t* rm, int on_device) {
  Geo& g = h->g;
  const int L = g.L, N = g.N, M = g.M, K = g.K;
  const size_t T = (size_t)N * N, rows = (size_t)L * T, n1 = (size_t)L * (T + 1);
  const int mb = h->coo_mb;
  if (nx >= 0x7fffffffll || nr >= 0x7fffffffll) return fail(nullptr, VMR_EINVAL, "more than 2^31 coordinates in one call");
  int* bad_dev = nullptr;
  CK(hipMalloc(&bad_dev, 4));
  CK(hipMemsetAsync(bad_dev, 0, 4, h->stream));
  unsigned long long *kx = nullptr, *kr = nullptr;
  unsigned* vx = nullptr;
  int rc = coo_sorted(h, nx, xl, xi, xj, xm, xv, on_device, &kx, &vx, bad_dev);
  if (!rc && nr >= 0) rc = coo_sorted(h, nr, rl, ri, rj, rm, nullptr, on_device, &kr, nullptr, bad_dev);
  unsigned *cx = nullptr, *cr = nullptr, *etmp = nullptr, *etmp2 = nullptr, *maxrow_dev = nullptr;
  auto cleanup = [&]() { void* p[] = {bad_dev, kx, kr, vx, cx, cr, etmp, etmp2, maxrow_dev}; for (void* q : p) if (q) (void)hipFree(q); };
  if (rc) { cleanup(); return rc; }
  {   // subscripts outside the tensor must not reach the kernels below (their keys index the per-tie arrays)
    int bad0 = 0;
    hipError_t e0 = hipMemcpy(&bad0, bad_dev, 4, hipMemcpyDeviceToHost);   // (coo_sorted synchronised the stream)
    if (e0 != hipSuccess) { g_create_err = hipGetErrorString(e0); cleanup(); return VMR_EHIP; }
    if (bad0 & 1) { cleanup(); return fail(nullptr, VMR_EINVAL, "a subscript lies outside (L, N, N, M)"); }
  }
#define CKC(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { g_create_err = std::string(#call) + ": " + hipGetErrorString(e_); (void)hipGetLastError(); cleanup(); return VMR_EHIP; } } while (0)
  CKC(hipMalloc(&cx, n1 * 4));
  CKC(hipMemsetAsync(cx, 0, n1 * 4, h->stream));
  const unsigned gx = (unsigned)std::min<long long>(8192, (nx + 255) / 256 + 1), gr = (unsigned)std::min<long long>(8192, (std::max<long long>(nr, 0) + 255) / 256 + 1);
  hipLaunchKernelGGL(k_coo_count, dim3(gx), dim3(256), 0, h->stream, kx, nx, T, mb, cx, bad_dev);
  if (nr >= 0) {
    CKC(hipMalloc(&cr, n1 * 4));
    CKC(hipMemsetAsync(cr, 0, n1 * 4, h->stream));
    hipLaunchKernelGGL(k_coo_count, dim3(gr), dim3(256), 0, h->stream, kr, nr, T, mb, cr, bad_dev);
  }
  CKC(hipMalloc(&maxrow_dev, 4));
  CKC(hipMemsetAsync(maxrow_dev, 0, 4, h->stream));
  hipLaunchKernelGGL(k_coo_class, dim3((unsigned)std::min<size_t>(4096, (rows + 255) / 256)), dim3(256), 0, h->stream, cx, cr, T, L, M,
                     h->cov, h->rcls, h->npartial, maxrow_dev);
  CKC(hipMalloc(&etmp, ((size_t)nx + 64) * 4));
  CKC(hipMalloc(&etmp2, ((size_t)nx + 64) * 4));
  CKC(hipMalloc(&h->Qt, rows * 4));
  CKC(hipMemsetAsync(h->Qt, 0, rows * 4, h->stream));
  if (g.mut) hipLaunchKernelGGL(k_coo_entries<true>, dim3(gx), dim3(256), 0, h->stream, kx, vx, nx, kr, nr, N, g.Mp, mb, etmp, etmp2, h->Qt, h->sumx, h->xmax, bad_dev);
  else hipLaunchKernelGGL(k_coo_entries<false>, dim3(gx), dim3(256), 0, h->stream, kx, vx, nx, kr, nr, N, g.Mp, mb, etmp, etmp2, h->Qt, h->sumx, h->xmax, bad_dev);
  CKC(hipGetLastError());
  CKC(hipStreamSynchronize(h->stream));
  int bad = 0;
  unsigned maxrow = 0;
  CKC(hipMemcpy(&bad, bad_dev, 4, hipMemcpyDeviceToHost));
  CKC(hipMemcpy(&maxrow, maxrow_dev, 4, hipMemcpyDeviceToHost));
  h->rm_maxrow = maxrow;
  if (bad) {
    cleanup();
    return fail(nullptr, VMR_EINVAL, (bad & 1) ? "a subscript lies outside (L, N, N, M)"
                                   : (bad & 2) ? "duplicate (l, i, j, m) subscripts"
                                   : (bad & 4) ? "counts must be positive (and below 2^31)"
                                               : "(largest count + 1) * M exceeds 2^32 table rows");
  }
  unsigned xmv = 0;
  if ((rc = create_state(h, &xmv))) { cleanup(); return rc; }
  h->sparse = 1;
  h->nnz = (unsigned long long)nx;
  // reports per layer: where each layer starts in the sorted keys
  std::vector<unsigned long long> nl(L, 0);
  {
    unsigned long long* starts = nullptr;
    CKC(hipMalloc(&starts, (size_t)(L + 1) * 8));
    hipLaunchKernelGGL(k_coo_layer_starts, dim3(1), dim3(64), 0, h->stream, kx, nx, (unsigned long long)T, L, mb, starts);
    std::vector<unsigned long long> st(L + 1);
    hipError_t e1 = hipMemcpyAsync(st.data(), starts, (size_t)(L + 1) * 8, hipMemcpyDeviceToHost, h->stream);
    if (e1 == hipSuccess) e1 = hipStreamSynchronize(h->stream);
    (void)hipFree(starts);
    CKC(e1);
    for (int l = 0; l < L; ++l) nl[l] = st[l + 1] - st[l];
  }
  // packed entries (13-bit reporters, 11-bit counts, 2^20 table rows) where they hold the tensor, two words per entry otherwise;
  // the general kernels take over beyond KMAX categories or with wide entries (sweep_gen.h)
  g.wide = (g.Mp <= 8192 && xmv <= SL_XMAX && (size_t)(xmv + 1) * g.Mp <= SL_YM_ROWS) ? 0 : 1;
  g.gen = (K > KMAX || g.wide) ? 1 : 0;
  if ((unsigned long long)xmv * (unsigned long long)M > 0xffffffffull) {
    cleanup();
    return fail(nullptr, VMR_EINVAL, "largest count * M exceeds 2^32 (the per-tie mirror sums are 32-bit)");
  }
  if (!g.wide) {
    hipLaunchKernelGGL(k_coo_pack, dim3(gx), dim3(256), 0, h->stream, etmp, etmp2, (long long)nx);
    CKC(hipGetLastError());
  }
  rc = sl_place_entries(h, cx, nl, etmp, g.wide ? etmp2 : nullptr, nullptr);
  if (!rc) rc = sl_finish(h);
  if (rc) { cleanup(); return rc; }
  // the mask: all ones needs nothing; partial rows become mask lists when they are short, bit-packed words otherwise.  The LDS
  // A[Mp][K] of k_mask_lists and of the K <= 8 sweep bounds the lists of narrow handles; a wide one (Mp > 8192: general kernels
  // only, whose pass walks the lists from global memory) takes them whatever Mp K.
  if (nr >= 0 && h->n_partial > 0) {
    const double list_bytes = 2.0 * (double)nr + 4.0 * (double)rows, word_bytes = (double)h->n_partial * g.W * 8.0;
    const bool lists = !h->opt.no_rlists && maxrow <= 64 && (list_bytes * 4.0 <= word_bytes || g.N <= 1024) &&
                       (g.Mp > 8192 || (size_t)g.Mp * K * 8 <= 160 * 1024);
    {
      size_t fr = 0, tot = 0;
      CKC(hipMemGetInfo(&fr, &tot));
      const double need = lists ? list_bytes + 4.0 * (double)n1 : (double)rows * g.W * 8.0;
      if (need > (double)fr) {
        char msg[320];
        snprintf(msg, sizeof msg, "the mask's partial rows would take %.1f GB as %s (%llu partial rows, longest %u reporters, M = %d): more than the "
                 "device memory left (%.1f GB)", need / 1e9, lists ? "mask lists" : "bit-packed words", (unsigned long long)h->n_partial, maxrow, M, fr / 1e9);
        cleanup();
        return fail(nullptr, VMR_EINVAL, msg);
      }
    }
    if (lists) {
      unsigned* bs = nullptr;
      CKC(hipMalloc(&h->rq, n1 * 4));
      CKC(hipMalloc(&bs, ((T + 1) + 2047) / 2048 * 4));
      hipLaunchKernelGGL(k_coo_listed, dim3((unsigned)std::min<size_t>(4096, (n1 + 255) / 256)), dim3(256), 0, h->stream, cr, h->rcls, T, L, h->rq);
      std::vector<unsigned long long> rb_(L);
      h->n_rm = 0;
      for (int l = 0; l < L; ++l) {
        if ((rc = scan_u32(h, h->rq + (size_t)l * (T + 1), bs, T + 1))) { (void)hipFree(bs); cleanup(); return rc; }
        unsigned tot = 0;
        CKC(hipStreamSynchronize(h->stream));
        CKC(hipMemcpy(&tot, h->rq + (size_t)l * (T + 1) + T, 4, hipMemcpyDeviceToHost));
        rb_[l] = h->n_rm; h->n_rm += tot;
      }
      CKC(hipFree(bs));
      CKC(hipMalloc(&h->rbase, (size_t)L * 8));
      CKC(hipMemcpy(h->rbase, rb_.data(), (size_t)L * 8, hipMemcpyHostToDevice));
      CKC(hipMalloc(&h->Rm, ((size_t)h->n_rm + 64) * 2));
      hipLaunchKernelGGL(k_coo_rm, dim3(gr), dim3(256), 0, h->stream, kr, nr, T, mb, h->rcls, h->rq, h->rbase, h->Rm);
      CKC(hipGetLastError());
    } else {
      CKC(hipMalloc(&h->Rb, rows * g.W * 8));
      CKC(hipMemsetAsync(h->Rb, 0, rows * g.W * 8, h->stream));
      hipLaunchKernelGGL(k_coo_rbits, dim3(gr), dim3(256), 0, h->stream, kr, nr, g.W, mb, reinterpret_cast<unsigned long long*>(h->Rb));
      CKC(hipGetLastError());
    }
  }
  CKC(hipStreamSynchronize(h->stream));
#undef CKC
  cleanup();
  return create_tail(h, prop);
}

extern "C" int vmr_create_coo(vmr_handle* out, int device, int L, int N, int M, int K, int mutuality, int64_t nx, const int32_t* xl,
                              const int32_t* xi, const int32_t* xj, const int32_t* xm, const int32_t* xv, int64_t nr, const int32_t* rl,
                              const int32_t* ri, const int32_t* rj, const int32_t* rm, int data_on_device, double eps) {
  if (!out) return fail(nullptr, VMR_EINVAL, "out is NULL");
  *out = nullptr;
  if (nx < 0 || (nx > 0 && (!xl || !xi || !xj || !xm || !xv))) return fail(nullptr, VMR_EINVAL, "X coordinate arrays missing");
  if (nr > 0 && (!rl || !ri || !rj || !rm)) return fail(nullptr, VMR_EINVAL, "R coordinate arrays missing");
  // limits of the coordinate route, before anything is allocated
  if (L < 1 || N < 1 || M < 1) return fail(nullptr, VMR_EINVAL, "L, N, M must be positive");
  if (M > 65535) return fail(nullptr, VMR_EINVAL, "M exceeds 65535 (M_COO_MAX): the mask lists hold 16-bit reporter indices");
  int mb = 13;   // reporter bits of a sort key (COO_KEY): 13 up to Mp = 8192, as before wider reporter dimensions were taken
  while ((1 << mb) < (M + 15) / 16 * 16) ++mb;
  if ((((unsigned __int128)L * (unsigned)N * (unsigned)N) << mb) >> 64)
    return fail(nullptr, VMR_EINVAL, "L * N^2 * 2^ceil(log2 M) must stay below 2^64 (the 64-bit sort keys of the coordinates)");
  vmr_ctx* h = nullptr;
  hipDeviceProp_t prop;
  int rc = create_ctx(&h, &prop, device, L, N, M, K, mutuality, eps, true);
  if (!rc) h->coo_mb = mb;
  if (!rc) rc = create_coo(h, prop, nx, xl, xi, xj, xm, xv, nr, rl, ri, rj, rm, data_on_device);
  if (rc) { if (h) vmr_destroy(h); return rc; }
  *out = h;
  return VMR_OK;
}
