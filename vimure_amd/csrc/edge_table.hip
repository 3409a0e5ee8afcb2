// edge_table.hip -- the inferred network as an edge table, built where rho lives: vmr_edge_table_size, vmr_edge_table
// (the reference driver's vimure_model_edgelist.csv, notebooks/python/experiments/karnataka.py:200-318, for any K and any mask).
//
// A row per tie (l,i,j) that someone reported (n_rep > 0) and / or that the read-out infers (y > 0), in lexicographic order, with
// the posterior probability of a tie, the report baselines and the same figures of the mirror tie (l,j,i).  One layer at a time:
//   k_et_tie   a group of G lanes per tie reduces the tie's reports -- report lists: the tie's row of the tie-major index of ppc.hip;
//              dense tiles: the Mp-byte row in 16-byte loads -- to n_rep and total (shuffles inside the group), its first lane reads
//              the tie's rho row once for y, and writes a 16-byte record (total, n_rep, y, row flag);
//   scan       exclusive sum of the row flags (hipcub, read out of the records): a row's place in the table, 4 B per tie;
//   k_et_rows  a lane per tie; a flagged tie gathers its mirror's record at j N + i, reads its rho row again for prob and mean, looks
//              its ego's and alter's own reports up (ppc_x), sizes its mask row, and writes the structure-of-arrays outputs.
// Only rows take the second kernel's extra reads: a few per cent of the ties.  No sum crosses lanes in floating point and nothing is
// an atomic: the table is bit-identical from run to run.
#include "read_side.h"

namespace {

// a tie's record: sum of its counts, number of reporters with a count, y in bits 0..7 and the row flag in bit 8
struct EtRec {
  unsigned long long total;
  unsigned n_rep;
  unsigned yf;
};
#define ET_FLAG 0x100u

struct EtFlag {
  __host__ __device__ __forceinline__ unsigned operator()(const EtRec& r) const { return (r.yf >> 8) & 1u; }
};

// the outputs of one layer, already offset to the layer's first row; any pointer may be null
struct EtOut {
  int32_t *sl, *si, *sj;
  uint8_t* y;
  double *prob, *mean;
  uint32_t* n_rep;
  uint64_t* total;
  uint32_t *n_mask, *ego, *alter;
  uint8_t* y_T;
  uint32_t* n_rep_T;
  uint64_t* total_T;
};
#define ET_NOUT 14
static const size_t et_width[ET_NOUT] = {4, 4, 4, 1, 8, 8, 4, 8, 4, 4, 4, 1, 4, 8};

// per tie: the reports reduced, the read-out, the record.  rec has T + 1 entries; entry T is zero (the scan then ends in the row count)
__global__ __launch_bounds__(256) void k_et_tie(PpcLayer p, int G, int method, double threshold, int select, EtRec* __restrict__ rec) {
  const int lane = threadIdx.x & 63, gl = lane & (G - 1);
  const size_t gpb = 256 / G, ngr = (size_t)gridDim.x * gpb;
  for (size_t t = (size_t)blockIdx.x * gpb + threadIdx.x / G; t <= p.T; t += ngr) {   // (uniform over the group)
    if (t == p.T) {
      if (gl == 0) { EtRec z; z.total = 0ull; z.n_rep = 0u; z.yf = 0u; rec[t] = z; }
      continue;
    }
    unsigned cnt = 0;
    unsigned long long tot = 0;
    if (p.X) {
      const uint8_t* row = p.X + t * (size_t)p.Mp;   // (rows are Mp = 16 n bytes, the array 256-byte aligned)
      for (int c0 = gl * 16; c0 < p.Mp; c0 += G * 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(row + c0);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const unsigned b = (c0 + q < p.M) ? ((w[q >> 2] >> ((q & 3) * 8)) & 0xffu) : 0u;
          cnt += b != 0u;
          tot += b;
        }
      }
    } else {
      const unsigned e1 = p.ip[t + 1];
      for (unsigned e = p.ip[t] + (unsigned)gl; e < e1; e += (unsigned)G) {
        const unsigned x = p.iv[e] >> 1;
        cnt += x != 0u;
        tot += x;
      }
    }
    for (int o = G >> 1; o > 0; o >>= 1) {
      cnt += __shfl_xor(cnt, o, 64);
      tot += (unsigned long long)__shfl_xor((long long)tot, o, 64);
    }
    if (gl == 0) {
      const unsigned y = rho_row_readout(tie_rho(p, t), p.K, method, threshold);
      const bool row = ((select & VMR_EDGE_REPORTED) && cnt > 0u) || ((select & VMR_EDGE_INFERRED) && y > 0u);
      EtRec r;
      r.total = tot; r.n_rep = cnt; r.yf = y | (row ? ET_FLAG : 0u);
      rec[t] = r;
    }
  }
}

// the rows, in order: a flagged tie writes row off[t]
__global__ __launch_bounds__(256) void k_et_rows(PpcLayer p, const EtRec* __restrict__ rec, const unsigned* __restrict__ off, unsigned nrows,
                                                 EtOut o, int* __restrict__ bad) {
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < p.T; t += (size_t)gridDim.x * 256) {
    const EtRec r = rec[t];
    if (!(r.yf & ET_FLAG)) continue;
    const unsigned at = off[t];
    if (at >= nrows) { atomicOr(bad, 2); continue; }   // (the scan and the flags disagree: never written out of bounds)
    const size_t i = t / p.N, j = t - i * p.N, tm = j * p.N + i;
    const EtRec rm = rec[tm];
    if (o.sl) o.sl[at] = p.l;
    if (o.si) o.si[at] = (int32_t)i;
    if (o.sj) o.sj[at] = (int32_t)j;
    if (o.y) o.y[at] = (uint8_t)(r.yf & 0xffu);
    if (o.n_rep) o.n_rep[at] = r.n_rep;
    if (o.total) o.total[at] = r.total;
    if (o.y_T) o.y_T[at] = (uint8_t)(rm.yf & 0xffu);
    if (o.n_rep_T) o.n_rep_T[at] = rm.n_rep;
    if (o.total_T) o.total_T[at] = rm.total;
    if (o.prob || o.mean) {
      // prob: the adds of vmr_expected_stats (k ascending); mean: every product and sum rounded on its own, k ascending
      double pr, mn;
      rho_row_prob_mean(tie_rho(p, t), p.K, pr, mn);
      if (o.prob) o.prob[at] = pr;
      if (o.mean) o.mean[at] = mn;
    }
    if (o.n_mask) o.n_mask[at] = mask_row_size(p, t, p.cls[t]);
    if (o.ego) o.ego[at] = (i < (size_t)p.M && r.n_rep) ? ppc_x(p, t, (unsigned)i) : 0u;
    if (o.alter) o.alter[at] = (j < (size_t)p.M && r.n_rep) ? ppc_x(p, t, (unsigned)j) : 0u;
  }
}

static int et_check(vmr_ctx* h, int method, int select, int layer, const char* fn) {
  if (!h->have_state) return fail(h, VMR_ESTATE, (std::string("vmr_set_state must be called before ") + fn).c_str());
  if (method != VMR_READ_RHO_MAX && method != VMR_READ_THRESHOLD)
    return fail(h, VMR_EINVAL, (std::string(fn) + ": the method must be VMR_READ_RHO_MAX or VMR_READ_THRESHOLD (a table of categories)").c_str());
  if (select < 1 || select > (VMR_EDGE_REPORTED | VMR_EDGE_INFERRED))
    return fail(h, VMR_EINVAL, (std::string(fn) + ": select must be VMR_EDGE_REPORTED, VMR_EDGE_INFERRED or both").c_str());
  if (layer >= h->g.L) return fail(h, VMR_EINVAL, (std::string(fn) + ": layer out of range").c_str());
  if ((size_t)h->g.N * h->g.N >= 0x7fffffffull) return fail(h, VMR_EINVAL, (std::string(fn) + ": 2^31 ties or more in one layer").c_str());
  HIPCHK(h, hipSetDevice(h->device));
  return ensure_rho_ext(h);
}

// One layer's records and row offsets (both T + 1 long, temporaries of tm), the layer prepared in lp; *nrows = its rows.
static int et_layer(vmr_ctx* h, Tmp& tm, int l, int method, double threshold, int select, LayerPrep& lp, EtRec** rec_out, unsigned** off_out,
                    unsigned* nrows) {
  const size_t T = (size_t)h->g.N * h->g.N;
  int rc;
  if ((rc = ppc_prep_layer(h, tm, l, false, true, lp, true, false))) return rc;
  EtRec* rec = nullptr;
  unsigned* off = nullptr;
  void* ts = nullptr;
  size_t tb = 0;
  if ((rc = tm.get(&rec, (T + 1) * sizeof(EtRec), "the ties' records")) || (rc = tm.get(&off, (T + 1) * 4, "the rows' offsets"))) return rc;
  *rec_out = rec; *off_out = off;
  // lanes per tie: no more than the row gives work to -- dense tiles one lane per 16-byte chunk, report lists index_lanes
  const int G = h->sparse ? index_lanes(h) : pow2_lanes((size_t)h->g.Mp / 16);
  hipLaunchKernelGGL(k_et_tie, dim3(grid_for((T + 1) * G, 256, 65536)), dim3(256), 0, h->stream, lp.p, G, method, threshold, select, rec);
  HIPCHK(h, hipGetLastError());
  hipcub::TransformInputIterator<unsigned, EtFlag, const EtRec*> flags(rec, EtFlag());
  HIPCHK(h, hipcub::DeviceScan::ExclusiveSum(nullptr, tb, flags, off, (int)(T + 1), h->stream));
  if ((rc = tm.get(&ts, tb, "the rows' scan"))) return rc;
  HIPCHK(h, hipcub::DeviceScan::ExclusiveSum(ts, tb, flags, off, (int)(T + 1), h->stream));
  HIPCHK(h, hipMemcpyAsync(nrows, off + T, 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  tm.release(ts);
  return VMR_OK;
}

static void et_release(Tmp& tm, LayerPrep& lp, EtRec* rec, unsigned* off) {
  if (rec) tm.release(rec);
  if (off) tm.release(off);
  ppc_release_layer(tm, lp);
}

}  // namespace

extern "C" int vmr_edge_table_size(vmr_handle h, int method, double threshold, int select, int layer, uint64_t* n) {
  if (!h || !n) return VMR_EINVAL;
  int rc = et_check(h, method, select, layer, "vmr_edge_table_size");
  if (rc) return rc;
  Tmp tm(h);
  unsigned long long tot = 0;
  for (int l = (layer < 0 ? 0 : layer); l < (layer < 0 ? h->g.L : layer + 1); ++l) {
    LayerPrep lp;
    EtRec* rec = nullptr;
    unsigned *off = nullptr, nrows = 0;
    if ((rc = et_layer(h, tm, l, method, threshold, select, lp, &rec, &off, &nrows))) return rc;
    tot += nrows;
    et_release(tm, lp, rec, off);
  }
  *n = tot;
  return VMR_OK;
}

extern "C" int vmr_edge_table(vmr_handle h, int method, double threshold, int select, int layer, uint64_t n, int32_t* sl, int32_t* si,
                              int32_t* sj, uint8_t* y, double* prob, double* mean, uint32_t* n_rep, uint64_t* total, uint32_t* n_mask,
                              uint32_t* ego, uint32_t* alter, uint8_t* y_T, uint32_t* n_rep_T, uint64_t* total_T, int out_on_device) {
  if (!h) return VMR_EINVAL;
  int rc = et_check(h, method, select, layer, "vmr_edge_table");
  if (rc) return rc;
  uint64_t need = 0;
  if ((rc = vmr_edge_table_size(h, method, threshold, select, layer, &need))) return rc;
  if (n < need) {
    char msg[160];
    snprintf(msg, sizeof msg, "vmr_edge_table: the outputs hold %llu rows, the table has %llu", (unsigned long long)n, (unsigned long long)need);
    return fail(h, VMR_EINVAL, msg);
  }
  void* user[ET_NOUT] = {sl, si, sj, y, prob, mean, n_rep, total, n_mask, ego, alter, y_T, n_rep_T, total_T};
  Tmp tm(h);
  int* bad = nullptr;
  if ((rc = tm.get(&bad, 4, "a flag"))) return rc;
  HIPCHK(h, hipMemsetAsync(bad, 0, 4, h->stream));
  const size_t T = (size_t)h->g.N * h->g.N;
  unsigned long long base = 0;   // row of the layer's first
  for (int l = (layer < 0 ? 0 : layer); l < (layer < 0 ? h->g.L : layer + 1); ++l) {
    LayerPrep lp;
    EtRec* rec = nullptr;
    unsigned *off = nullptr, nrows = 0;
    if ((rc = et_layer(h, tm, l, method, threshold, select, lp, &rec, &off, &nrows))) return rc;
    if (base + nrows > need) return fail(h, VMR_EHIP, "vmr_edge_table: the row count changed between the passes");
    if (nrows) {
      void* dst[ET_NOUT];
      void* stage[ET_NOUT];
      for (int q = 0; q < ET_NOUT; ++q) {
        dst[q] = nullptr; stage[q] = nullptr;
        if (!user[q]) continue;
        if (out_on_device) dst[q] = static_cast<char*>(user[q]) + base * et_width[q];
        else {
          char* st = nullptr;
          if ((rc = tm.get(&st, (size_t)nrows * et_width[q], "the staging of the table"))) return rc;
          dst[q] = stage[q] = st;
        }
      }
      EtOut o;
      o.sl = (int32_t*)dst[0]; o.si = (int32_t*)dst[1]; o.sj = (int32_t*)dst[2]; o.y = (uint8_t*)dst[3];
      o.prob = (double*)dst[4]; o.mean = (double*)dst[5]; o.n_rep = (uint32_t*)dst[6]; o.total = (uint64_t*)dst[7];
      o.n_mask = (uint32_t*)dst[8]; o.ego = (uint32_t*)dst[9]; o.alter = (uint32_t*)dst[10]; o.y_T = (uint8_t*)dst[11];
      o.n_rep_T = (uint32_t*)dst[12]; o.total_T = (uint64_t*)dst[13];
      hipLaunchKernelGGL(k_et_rows, dim3(grid_for(T, 256, 16384)), dim3(256), 0, h->stream, lp.p, (const EtRec*)rec, (const unsigned*)off, nrows, o, bad);
      HIPCHK(h, hipGetLastError());
      if (!out_on_device)
        for (int q = 0; q < ET_NOUT; ++q)
          if (user[q]) HIPCHK(h, hipMemcpyAsync(static_cast<char*>(user[q]) + base * et_width[q], stage[q], (size_t)nrows * et_width[q], hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
      for (int q = 0; q < ET_NOUT; ++q) if (stage[q]) tm.release(stage[q]);
    }
    base += nrows;
    et_release(tm, lp, rec, off);
  }
  int b = 0;
  HIPCHK(h, hipMemcpy(&b, bad, 4, hipMemcpyDeviceToHost));
  if (b) return fail(h, VMR_EHIP, "vmr_edge_table: the rows' scan and the row flags disagree");
  return VMR_OK;
}
