// connectivity.hip -- connectivity of the posterior on the device: vmr_sample_connectivity.
//
// vmr_sample_stats stops at dyads, vmr_sample_triads at triads; whether the inferred network hangs together, how large its giant
// component is and who reaches whom in how many steps is what measurement error distorts most -- one missed bridge splits a
// component, one invented tie shortens thousands of geodesics.  vmr_sample_connectivity draws S posterior samples of Y in chunks
// (sampled_side.h: sample s is what vmr_sample(h, seed + s, n_trials) writes) and returns per sample and layer, for A = (Y > 0)
// with the diagonal cleared and U = A | A^T: the weak and strong components, the reachable ordered pairs, the sum, the histogram
// and the maximum of their distances and, per node, its component labels, how many nodes it reaches and is reached by, and the
// sums of those distances (include/vimure_hip.h has the definitions).  Everything is an integer.
//
// Layout.  The chunk's samples are packed into bit rows (sampled_side.h has the layout).
// k_conn_closure: one workgroup (4 waves) per (source block b of 64 nodes, layer, sample).  A closure is a breadth-first search
// from the block's 64 sources at once: node v carries a 64-bit word seen[v] whose bit q says that source 64 b + q has reached v.
// Three arrays of 64 W words live in LDS: seen, the frontier and the next frontier (24 N bytes: N <= VMR_CONN_NMAX = 2048 is
// 48 KiB, three workgroups to a CU).  A level has two steps:
//   expand   a wave takes 64 consecutive nodes, one per lane, and ballots the non-empty frontier words; a block of nodes without
//            any costs one LDS read.  Else G lanes (the largest power of two <= min(W, 64)) stride the W words of the row of each
//            frontier node u and OR frontier[u] into next[v] for every set bit v with an LDS atomic; the words of CONN_FLY rows
//            are loaded before the first is used, the step waits on the latency of these gathers from L2;
//   update   thread t owns nodes t, t + 256, ..: new = next[v] & ~seen[v] joins seen[v] and becomes the frontier; popc(new) at
//            level d is the number of the block's sources at distance d from v.
// and the closure ends with the first level that adds nothing.  Three closures: over Aout | Ain (seen[v] is then v's weak
// component within the block: the label is the smallest 64 b + ctz(seen[v]) over the blocks, an integer atomic min), over Aout
// (popc(new) at level d summed over v: the block's share of dist_hist[d - 1], reach_pairs and dist_sum, the last level that added
// something its share of the diameter; per v its share of node_reach_in and, times d, of node_dist_in) and over Ain, the reversed
// graph (the same per v for node_reach_out and node_dist_out).  The forward seen words stay in registers (8 per thread) across
// the backward closure: seen_fwd[v] & seen_bwd[v] is the mutual-reachability word, which labels the strong components as above.
// The per-node shares are kept in registers over a closure and added once at its end.
// k_conn_finish: one workgroup per (layer, sample) tallies the component sizes from the two label arrays in LDS and stores
// components, giant and pairs of both kinds and the isolates (the weak components of one node).
// All sums are sums of integers, maxima and minima of integers: the same from run to run in any order, and for any chunking.
#include "conn_expand.h"

namespace {

#define CONN_KPT (VMR_CONN_NMAX / CONN_TPB)   // nodes a thread owns at most

// One closure over the rows A (| B with `both`) from the sources of block b; see the head of the file.  seen, fr, nx: 64 W words of
// LDS each.  Returns the last level that added anything (in every thread).  nr[k], nd[k]: over the levels d, popc(new) and
// d popc(new) of node threadIdx.x + 256 k.  With `totals`, hist_s[min(d, 64) - 1] (LDS, zeroed by the caller) receives the level's
// new (source, node) pairs, and reach / dsum this thread's share of their number and of their distances.
__device__ __forceinline__ int conn_closure(const u64* __restrict__ A, const u64* __restrict__ B, bool both, bool totals, int N, int W, int lG,
                                            int b, u64* seen, u64* fr, u64* nx, unsigned* hist_s, u64& reach, u64& dsum,
                                            unsigned (&nr)[CONN_KPT], unsigned (&nd)[CONN_KPT]) {
  const int tid = threadIdx.x, lane = tid & 63;
  __syncthreads();   // (the caller is done with the three arrays)
  for (int v = tid; v < W * 64; v += CONN_TPB) {
    const u64 bit = (v >> 6) == b && v < N ? 1ull << (v & 63) : 0ull;
    seen[v] = bit; fr[v] = bit; nx[v] = 0ull;
  }
#pragma unroll
  for (int k = 0; k < CONN_KPT; ++k) { nr[k] = 0u; nd[k] = 0u; }
  __syncthreads();
  int last = 0;
  for (int d = 1;; ++d) {
    if (both) conn_expand<true>(A, B, N, W, lG, fr, nx);
    else conn_expand<false>(A, B, N, W, lG, fr, nx);
    __syncthreads();
    unsigned lvl = 0u;
#pragma unroll
    for (int k = 0; k < CONN_KPT; ++k) {
      const int v = tid + k * CONN_TPB;
      if (v < W * 64) {
        const u64 nw = nx[v] & ~seen[v];
        if (nw) seen[v] |= nw;
        nx[v] = nw;
        fr[v] = 0ull;
        const unsigned c = (unsigned)__popcll(nw);
        lvl += c; nr[k] += c; nd[k] += c * (unsigned)d;
      }
    }
    { u64* t = fr; fr = nx; nx = t; }
    if (totals) {
      reach += lvl; dsum += (u64)lvl * (u64)d;
      const unsigned ws = (unsigned)wave_sum_ull(lvl);
      if (lane == 0 && ws) atomicAdd(&hist_s[(d < VMR_CONN_NDIST ? d : VMR_CONN_NDIST) - 1], ws);
    }
    if (!__syncthreads_or(lvl != 0u)) break;
    last = d;
  }
  return last;
}

// label[v] = min(label[v], cand); the plain read first spares most of the atomics (a stale read only costs one)
__device__ __forceinline__ void conn_label(int32_t* label, int cand) {
  if (cand < *(volatile int32_t*)label) atomicMin(label, cand);
}

// Grid (W source blocks, L, samples of the chunk); dynamic LDS: 3 x 64 W words.  counts[s][l]: 7 reach_pairs, 8 dist_sum,
// 9 diameter are added to / raised here (zeroed per chunk).  nodes: the six node arrays of the chunk, `plane` elements each, in
// the order of the call's arguments: the two label arrays hold a value >= N on entry, the reach and distance arrays zeros, and
// are added to with want_nodes only.  hist may be null.
__global__ __launch_bounds__(CONN_TPB) void k_conn_closure(const u64* __restrict__ Aout, const u64* __restrict__ Ain, int N, int L, int W, int lG,
                                                           u64* __restrict__ counts, u64* __restrict__ hist, int32_t* __restrict__ nodes,
                                                           size_t plane, bool want_nodes) {
  extern __shared__ u64 conn_lds[];
  __shared__ unsigned hist_s[VMR_CONN_NDIST];
  __shared__ u64 red[CONN_TPB / 64];
  const int tid = threadIdx.x;
  const int b = blockIdx.x, l = blockIdx.y, s = blockIdx.z;
  const size_t sl = (size_t)s * L + l;
  const u64* Ao = Aout + sl * N * W;
  const u64* Ai = Ain + sl * N * W;
  u64 *seen = conn_lds, *fa = conn_lds + (size_t)W * 64, *fb = conn_lds + (size_t)W * 128;
  unsigned nr[CONN_KPT], nd[CONN_KPT];
  u64 reach = 0ull, dsum = 0ull;
  if (tid < VMR_CONN_NDIST) hist_s[tid] = 0u;

  u64 keep[CONN_KPT];
  // three closures: 0 over U = Aout | Ain, which is symmetric: seen[v] holds the sources of v's weak component; 1 forward, bit q of
  // seen[v]: source 64 b + q reaches v; 2 backward, over the reversed graph, bit q of seen[v]: v reaches source 64 b + q
  for (int pass = 0; pass < 3; ++pass) {
    const int last = conn_closure(pass == 2 ? Ai : Ao, pass == 2 ? Ao : Ai, pass == 0, pass == 1, N, W, lG, b, seen, fa, fb, hist_s, reach, dsum,
                                  nr, nd);
    if (pass == 1) {
      const u64 treach = block_sum_ull(reach, red);
      const u64 tdsum = block_sum_ull(dsum, red);
      if (tid == 0 && treach) {
        u64* c = counts + sl * VMR_CONN_NSTAT;
        atomicAdd(c + 7, treach);
        atomicAdd(c + 8, tdsum);
        atomicMax(c + 9, (u64)last);
      }
      if (hist && tid < VMR_CONN_NDIST && hist_s[tid]) atomicAdd(hist + sl * VMR_CONN_NDIST + tid, (u64)hist_s[tid]);
    }
    int32_t* mine = nodes + sl * N + (pass == 0 ? 0 : plane);   // the pass' labels; its reach is 2 (backward) or 3 planes on, its
    const size_t pr = (pass == 1 ? 2 : 1) * plane;             // distances 2 more
#pragma unroll
    for (int k = 0; k < CONN_KPT; ++k) {
      const int v = tid + k * CONN_TPB;
      if (v < N) {
        const u64 sv = seen[v];
        if (pass == 1) keep[k] = sv;
        else {   // the component's sources in this block: everything seen over U, what reaches v and is reached by it over A
          const u64 m = pass == 0 ? sv : keep[k] & sv;
          if (m) conn_label(mine + v, b * 64 + __ffsll((long long)m) - 1);
        }
        if (pass != 0 && want_nodes && nr[k]) {
          atomicAdd(mine + pr + v, (int)nr[k]);
          atomicAdd(mine + pr + 2 * plane + v, (int)nd[k]);
        }
      }
    }
  }
}

// Grid (L, samples of the chunk).  The labels are the smallest index of the node's component: size[label]++ in LDS, then every
// label that was used is one component.  Stores counts[s][l][0..6].
__global__ __launch_bounds__(CONN_TPB) void k_conn_finish(const int32_t* __restrict__ comp_w, const int32_t* __restrict__ comp_s, int N, int L,
                                                          u64* __restrict__ counts) {
  __shared__ int size_w[VMR_CONN_NMAX], size_s[VMR_CONN_NMAX];
  __shared__ u64 tot[7];
  const int tid = threadIdx.x, l = blockIdx.x, s = blockIdx.y;
  const size_t sl = (size_t)s * L + l;
  const int32_t* cw = comp_w + sl * N;
  const int32_t* cs = comp_s + sl * N;
  for (int v = tid; v < N; v += CONN_TPB) { size_w[v] = 0; size_s[v] = 0; }
  if (tid < 7) tot[tid] = 0ull;
  __syncthreads();
  for (int v = tid; v < N; v += CONN_TPB) {
    const int a = cw[v], c = cs[v];
    if ((unsigned)a < (unsigned)N) atomicAdd(&size_w[a], 1);
    if ((unsigned)c < (unsigned)N) atomicAdd(&size_s[c], 1);
  }
  __syncthreads();
  u64 nw = 0, gw = 0, pw = 0, iso = 0, ns = 0, gs = 0, ps = 0;
  for (int v = tid; v < N; v += CONN_TPB) {
    const u64 a = (u64)size_w[v], c = (u64)size_s[v];
    if (a) { ++nw; gw = a > gw ? a : gw; pw += a * (a - 1ull); iso += a == 1ull; }
    if (c) { ++ns; gs = c > gs ? c : gs; ps += c * (c - 1ull); }
  }
  if (nw) { atomicAdd(&tot[0], nw); atomicMax(&tot[1], gw); }
  if (pw) atomicAdd(&tot[2], pw);
  if (iso) atomicAdd(&tot[3], iso);
  if (ns) { atomicAdd(&tot[4], ns); atomicMax(&tot[5], gs); }
  if (ps) atomicAdd(&tot[6], ps);
  __syncthreads();
  if (tid < 7) counts[sl * VMR_CONN_NSTAT + tid] = tot[tid];
}

}  // namespace

extern "C" int vmr_sample_connectivity(vmr_handle h, uint64_t seed, int n_samples, int n_trials, uint64_t* counts, uint64_t* dist_hist,
                                       int32_t* node_comp_w, int32_t* node_comp_s, int32_t* node_reach_out, int32_t* node_reach_in,
                                       int32_t* node_dist_out, int32_t* node_dist_in) {
  if (!h) return VMR_EINVAL;
  if (!counts) return fail(h, VMR_EINVAL, "vmr_sample_connectivity: counts is NULL");
  int rc;
  if ((rc = sampled_counts(h, "vmr_sample_connectivity", n_samples, n_trials))) return rc;
  const Geo& g = h->g;
  if (g.N > VMR_CONN_NMAX) {
    char msg[256];
    snprintf(msg, sizeof msg, "vmr_sample_connectivity: the closure keeps 24 N bytes in LDS: N <= %d, the handle has N = %d", VMR_CONN_NMAX, g.N);
    return fail(h, VMR_EINVAL, msg);
  }
  if ((rc = expected_begin(h, "vmr_sample_connectivity"))) return rc;
  const BitRows b = bit_rows(g);
  const int W = b.W;
  const size_t node_b = b.LN * 4;
  SampledOut out[2] = {{counts, (size_t)g.L * VMR_CONN_NSTAT * 8, true, "vmr_sample_connectivity: the counts"},
                       {dist_hist, (size_t)g.L * VMR_CONN_NDIST * 8, true, "vmr_sample_connectivity: the distance histogram"}};
  int32_t* const node_host[6] = {node_comp_w, node_comp_s, node_reach_out, node_reach_in, node_dist_out, node_dist_in};
  const bool want_nodes = node_reach_out || node_reach_in || node_dist_out || node_dist_in;
  // device bytes per sample of a chunk: Y, the bit rows, the six node arrays (the labels are needed in any case), the outputs
  const size_t per = b.per() + 6 * node_b + out[0].bytes + (dist_hist ? out[1].bytes : 0);
  size_t C;
  if ((rc = chunk_samples(h, "vmr_sample_connectivity", (size_t)n_samples, per, 0, &C))) return rc;
  Tmp tm(h);
  uint8_t* Y = nullptr;
  u64 *Ao = nullptr, *Ai = nullptr;
  int32_t* nodes = nullptr;
  if ((rc = bit_rows_get(tm, b, C, "vmr_sample_connectivity", "samples", &Y, &Ao, &Ai)) ||
      (rc = tm.get(&nodes, 6 * C * node_b, "vmr_sample_connectivity: the node arrays")))
    return rc;
  const size_t smem = (size_t)W * 64 * 3 * 8;
  const size_t plane = C * (size_t)g.L * g.N;   // elements of one node array of a chunk
  return sampled_chunks(h, tm, (size_t)n_samples, C, seed, n_trials, Y, out, [&](size_t s0, int c) -> int {
    int rc2;
    if ((rc2 = tri_pack_chunk(h, Y, c, Ao, Ai))) return rc2;
    HIPCHK(h, hipMemsetAsync(nodes, 0x7f, 2 * plane * 4, h->stream));   // (0x7f7f7f7f: above every node index)
    if (want_nodes) HIPCHK(h, hipMemsetAsync(nodes + 2 * plane, 0, 4 * plane * 4, h->stream));
    hipLaunchKernelGGL(k_conn_closure, dim3((unsigned)W, (unsigned)g.L, (unsigned)c), dim3(CONN_TPB), smem, h->stream, Ao, Ai, g.N, g.L, W, b.lG,
                       out[0].as<u64>(), out[1].as<u64>(), nodes, plane, want_nodes);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_conn_finish, dim3((unsigned)g.L, (unsigned)c), dim3(CONN_TPB), 0, h->stream, nodes, nodes + plane, g.N, g.L, out[0].as<u64>());
    HIPCHK(h, hipGetLastError());
    for (int q = 0; q < 6; ++q)
      if (node_host[q])
        HIPCHK(h, hipMemcpyAsync(node_host[q] + s0 * g.L * g.N, nodes + q * plane, (size_t)c * node_b, hipMemcpyDeviceToHost, h->stream));
    return VMR_OK;
  });
}
