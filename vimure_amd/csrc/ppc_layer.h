// ppc_layer.h -- what the posterior predictive kernels share (ppc.hip: expected reports and their AUC; ppc_rep.hip: replicated and
// observed discrepancy statistics): one layer of a handle as a kernel sees it, the lookup of a count in either data format, the
// temporaries of a call, and the per-layer preparation that builds the tie-major index of the report lists (defined in ppc.hip).
#ifndef VMR_PPC_LAYER_H
#define VMR_PPC_LAYER_H
#include "vmr_internal.h"

// one layer of a handle, as the kernels see it
struct PpcLayer {
  int l, N, M, Mp, K, W, mut, mb;
  size_t T;
  const uint8_t* X;                 // dense tiles: [T][Mp] of the layer, else null
  const uint64_t* Rb;               // [T][W] mask words of the layer, or null
  const uint8_t* cls;               // [T] class of the mask row: 0 empty, 1 all ones, 2 partial
  const unsigned* rq;               // mask lists: [T + 1] first listed reporter of a row (relative to Rm), or null
  const unsigned short* Rm;
  const unsigned long long* ik;     // report lists: tie-major index, keys tie << mb | m (sorted) ...
  const unsigned* iv;               // ... values x << 1 | R ...
  const unsigned* ip;               // ... row starts [T + 1]
  const unsigned* inv;              // tie -> sorted position (rho by position), or null (rho by tie)
  const double* rho;                // [T][K] of the layer
  const double* gth;                // G_theta [Mp] of the layer, G_lambda [K], G_nu (the current parameters, vmr_get_geometric)
  const double* gla;
  const double* gnu;
};

// count X[t, m] of the layer: the dense row, or the tie's row of the index
__device__ __forceinline__ unsigned ppc_x(const PpcLayer& p, size_t t, unsigned m) {
  if (p.X) return p.X[t * p.Mp + m];
  unsigned a = p.ip[t], b = p.ip[t + 1];
  const unsigned long long key = ((unsigned long long)t << p.mb) | m;
  while (a < b) {
    const unsigned c = a + ((b - a) >> 1);
    if (p.ik[c] < key) a = c + 1; else b = c;
  }
  return (a < p.ip[t + 1] && p.ik[a] == key) ? (p.iv[a] >> 1) : 0u;
}

// Per-reporter integer bins (ppc_rep.hip, reporter_table.hip) and a tie's mask row as a walk sees it.
#define PR_HIST_M 2048   // by_reporter in LDS up to this many reporters (32 KB)

// a tie's mask row: c 0 empty, 1 all ones, 2 partial -- then mask words (lst null) or a sorted reporter list
struct MaskRow {
  int c;
  unsigned n;
  const uint64_t* w;
  const unsigned short* lst;
};

__device__ __forceinline__ MaskRow mask_row(const uint8_t* cls, const uint64_t* Rb, const unsigned* rq, const unsigned short* Rm, int W, size_t t) {
  MaskRow r;
  r.c = cls[t]; r.n = 0; r.w = nullptr; r.lst = nullptr;
  if (r.c == 2) {
    if (rq) { const unsigned a = rq[t]; r.lst = Rm + a; r.n = rq[t + 1] - a; }
    else r.w = Rb + t * (size_t)W;
  }
  return r;
}

__device__ __forceinline__ bool row_has(const MaskRow& r, unsigned m) {
  if (r.c == 1) return true;
  if (r.c != 2) return false;
  if (!r.lst) return (r.w[m >> 6] >> (m & 63)) & 1ull;
  unsigned a = 0, b = r.n;
  while (a < b) { const unsigned c = a + ((b - a) >> 1); if ((unsigned)r.lst[c] < m) a = c + 1; else b = c; }
  return a < r.n && (unsigned)r.lst[a] == m;
}

// temporaries of one call: freed on every exit path; an allocation that does not fit in the free device memory is refused
struct Tmp {
  vmr_ctx* h;
  std::vector<void*> ptrs;
  explicit Tmp(vmr_ctx* h_) : h(h_) {}
  ~Tmp() { for (void* q : ptrs) (void)hipFree(q); }
  Tmp(const Tmp&) = delete;
  Tmp& operator=(const Tmp&) = delete;
  template <class T_>
  int get(T_** out, size_t bytes, const char* what) {
    *out = nullptr;
    size_t fr = 0, tot = 0;
    HIPCHK(h, hipMemGetInfo(&fr, &tot));
    if (bytes + (64u << 20) > fr) {
      char msg[256];
      snprintf(msg, sizeof msg, "%s needs %.2f GB of device memory, %.2f GB are free", what, bytes / 1e9, fr / 1e9);
      return fail(h, VMR_EINVAL, msg);
    }
    void* q = nullptr;
    HIPCHK(h, hipMalloc(&q, bytes ? bytes : 8));
    ptrs.push_back(q);
    *out = reinterpret_cast<T_*>(q);
    return VMR_OK;
  }
  void release(void* q) {
    for (auto& e : ptrs) if (e == q) { (void)hipFree(e); e = nullptr; }
  }
};

// One layer prepared for the walks: the index (report lists), tie -> position, the support offsets off [T + 1] and, with
// positives, poff [T + 1].  Its temporaries live in `tmp`; release() gives the layer's memory back before the next one.
struct LayerPrep {
  PpcLayer p;
  unsigned long long *off = nullptr, *poff = nullptr;
  unsigned long long nsup = 0, npos = 0;
  std::vector<void*> mine;
};


// The mask of layer l (classes, words, lists) and the geometry, into p (zeroed first); the rest of p is ppc_prep_layer's.
int ppc_layer_mask(vmr_ctx* h, int l, PpcLayer& p);

// positives: the counts are needed (the index of report-list handles is built) and poff is filled; walk: rho is read by tie (the
// tie -> position table) and, with mutuality, the mirror counts; index: build the index of a report-list handle in any case;
// offsets = false: no support offsets (off stays null, nsup 0) for a caller that walks ties, not the support (edge_table.hip);
// mirror = false: a walk whose mirror counts come from its caller (heldout.hip): mutuality alone builds no index for them.
int ppc_prep_layer(vmr_ctx* h, Tmp& tm, int l, bool positives, bool walk, LayerPrep& lp, bool index = false, bool offsets = true,
                   bool mirror = true);
void ppc_release_layer(Tmp& tm, LayerPrep& lp);

#endif  // VMR_PPC_LAYER_H
