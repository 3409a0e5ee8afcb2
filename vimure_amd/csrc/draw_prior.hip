// draw_prior.hip -- the initial rho prior of a realisation on the device (vmr_draw_pr_rho), bit for bit what the reference's
// `_set_rho_prior` (latentnetworks/vimure src/python/vimure/model.py:470-482, 509-559) draws for a RandomState:
//
//     pr_rho = 1 + 0.01 * prng.rand(L, N, N, K)          (MT19937, genrand_res53 doubles, C order)
//     pr_rho[..., 0] += bias0
//     (undirected: pr_rho = (pr_rho + pr_rho.transpose(0, 2, 1, 3)) / 2)
//     pr_rho /= pr_rho.sum(axis=-1)[..., None]
//     pr_rho[coverage == 0] = one-hot(0)
//
// The host walks the generator without producing numbers (vmr_host_mt_states, host_init.c) and hands over the (key[624], pos) state
// at the first word of every block of whole ties.  One workgroup per block then refills, tempers and converts the words itself:
// no L N^2 K host array and no upload of one.
//
// Rounding, as NumPy's:
//   - no contraction (the pragma below): `1 + 0.01 u` rounds twice, the bias and the sums once per addition;
//   - the divisions are IEEE divides (hipcc's f64 `/`: v_div_scale / v_div_fmas / v_div_fixup, not v_rcp_f64 + Newton);
//   - the sum over the K categories is NumPy's pairwise_sum, in its order (checked bit for bit against NumPy 2.2 for K = 2..256):
//       n < 8:        left to right (from 0.0);
//       8 <= n <= 128: eight accumulators r[j] = a[j], r[j] += a[i + j] over the whole groups of 8, then
//                      ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the remaining elements left to right;
//       n > 128:      split at n2 = n/2 - (n/2) % 8 and add the two halves' pairwise sums.
#include "vmr_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int MT_N = 624, MT_M = 397;
constexpr int DP_TPB = 256;       // threads per block workgroup (>= 227: one thread per word of a refill phase)
constexpr int DP_WORDS = 4096;    // generator words staged in LDS per chunk of whole ties (K <= 256: at least 8 ties)

static_assert(DP_TPB >= MT_N - MT_M + 1, "a refill phase is one word per thread");

__device__ __forceinline__ uint32_t mt_word(uint32_t ki, uint32_t ki1, uint32_t km) {   // key[i] of the next state
  const uint32_t y = (ki & 0x80000000u) | (ki1 & 0x7fffffffu);
  return km ^ (y >> 1) ^ ((0u - (y & 1u)) & 0x9908b0dfu);
}

__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}

// The MT19937 refill of key[624] (LDS) in place.  The sequential loop reads key[i + 1] before it is rewritten and key[i + 397]
// (i < 227) or key[i - 227] (i >= 227) after, so three phases with every word's inputs read before any is written:
// [0, 227) from the old key; [227, 454) from phase 1's words; [454, 623) from phase 2's, together with word 623 (old key[623],
// new key[0] and key[396]).  Every thread of the workgroup calls it (barriers).
__device__ void mt_refill(uint32_t* key) {
  const int t = threadIdx.x;
  const int n1 = MT_N - MT_M;   // 227
  uint32_t v = 0;
  if (t < n1) v = mt_word(key[t], key[t + 1], key[t + MT_M]);
  __syncthreads();
  if (t < n1) key[t] = v;
  __syncthreads();
  if (t < n1) v = mt_word(key[n1 + t], key[n1 + t + 1], key[t]);
  __syncthreads();
  if (t < n1) key[n1 + t] = v;
  __syncthreads();
  const int n3 = MT_N - 1 - 2 * n1;   // 169
  if (t < n3) v = mt_word(key[2 * n1 + t], key[2 * n1 + t + 1], key[n1 + t]);
  else if (t == n3) v = mt_word(key[MT_N - 1], key[0], key[MT_M - 1]);
  __syncthreads();
  if (t < n3) key[2 * n1 + t] = v;
  else if (t == n3) key[MT_N - 1] = v;
  __syncthreads();
}

// NumPy's pairwise_sum of a(o), .., a(o + n - 1) (see the head of this file).  D bounds the splits: n <= 256 needs 2.
template <class F>
__device__ __forceinline__ double pw_leaf(const F& a, int o, int n) {
  if (n < 8) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += a(o + i);
    return s;
  }
  double r0 = a(o), r1 = a(o + 1), r2 = a(o + 2), r3 = a(o + 3), r4 = a(o + 4), r5 = a(o + 5), r6 = a(o + 6), r7 = a(o + 7);
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
    r0 += a(o + i); r1 += a(o + i + 1); r2 += a(o + i + 2); r3 += a(o + i + 3);
    r4 += a(o + i + 4); r5 += a(o + i + 5); r6 += a(o + i + 6); r7 += a(o + i + 7);
  }
  double s = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < n; ++i) s += a(o + i);
  return s;
}

template <int D, class F>
__device__ double pw_sum(const F& a, int o, int n) {
  if constexpr (D == 0) {
    return pw_leaf(a, o, n);
  } else {
    if (n <= 128) return pw_leaf(a, o, n);
    int n2 = n / 2;
    n2 -= n2 % 8;
    return pw_sum<D - 1>(a, o, n2) + pw_sum<D - 1>(a, o + n2, n - n2);
  }
}
static_assert(KGEN_MAX <= 256, "pw_sum<3> splits often enough for 256 terms");

// One workgroup per block b: ties [cuts[b], cuts[b + 1]) from the generator state (keys[b], pos[b]) at the block's first word.
// Chunks of whole ties: 2K words each are tempered into w (a tie's words, even a double's two, may straddle a refill), turned into
// doubles in d, normalised per tie (NORM; the undirected prior is symmetrised first, by k_sym_pr_rho) and written in natural order.
template <bool NORM>
__global__ __launch_bounds__(DP_TPB) void k_draw_pr_rho(const int64_t* __restrict__ cuts, const uint32_t* __restrict__ keys,
                                                        const int32_t* __restrict__ pos, int K, double bias0,
                                                        const uint8_t* __restrict__ cov, double* __restrict__ out) {
  __shared__ uint32_t mt[MT_N];
  __shared__ uint32_t w[DP_WORDS];
  __shared__ double d[DP_WORDS / 2];
  const int t = threadIdx.x;
  const int64_t t0 = cuts[blockIdx.x], t1 = cuts[blockIdx.x + 1];
  for (int i = t; i < MT_N; i += DP_TPB) mt[i] = keys[(size_t)blockIdx.x * MT_N + i];
  int p = pos[blockIdx.x];   // (uniform: every thread follows the same generator position)
  __syncthreads();
  const int ct = (DP_WORDS / 2) / K;
  for (int64_t c0 = t0; c0 < t1; c0 += ct) {
    const int nt = (int)min((int64_t)ct, t1 - c0), nd = nt * K, nw = 2 * nd;
    for (int f = 0; f < nw;) {
      if (p >= MT_N) {
        __syncthreads();   // (the words of the old key have been read)
        mt_refill(mt);
        p = 0;
      }
      const int m = min(MT_N - p, nw - f);
      for (int i = t; i < m; i += DP_TPB) w[f + i] = mt_temper(mt[p + i]);
      p += m;
      f += m;
    }
    __syncthreads();
    for (int i = t; i < nd; i += DP_TPB) {   // genrand_res53, then 1 + 0.01 u (+ bias0 on category 0)
      const double u = ((double)(w[2 * i] >> 5) * 67108864.0 + (double)(w[2 * i + 1] >> 6)) / 9007199254740992.0;
      double v = 1.0 + 0.01 * u;
      if (i % K == 0) v = v + bias0;
      d[i] = v;
    }
    __syncthreads();
    if (NORM) {
      for (int q = t; q < nt; q += DP_TPB) {
        double* v = d + q * K;
        if (cov[c0 + q]) {
          const double s = pw_sum<3>([v](int k) { return v[k]; }, 0, K);
          for (int k = 0; k < K; ++k) v[k] = v[k] / s;
        } else {
          v[0] = 1.0;
          for (int k = 1; k < K; ++k) v[k] = 0.0;
        }
      }
      __syncthreads();
    }
    double* o = out + c0 * K;
    for (int i = t; i < nd; i += DP_TPB) o[i] = d[i];
    __syncthreads();   // (w and d are the next chunk's)
  }
}

// Undirected: p[l,i,j,:] and p[l,j,i,:] <- (p[l,i,j,:] + p[l,j,i,:]) / 2 (equal: addition commutes), normalised, one-hot where
// each tie's own coverage is 0.  One thread per pair i <= j, in place; the diagonal stays (p + p) / 2 = p.
__global__ __launch_bounds__(256) void k_sym_pr_rho(double* __restrict__ p, const uint8_t* __restrict__ cov, int L, int N, int K) {
  const size_t NN = (size_t)N * N, n = (size_t)L * NN;
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < n; q += (size_t)gridDim.x * blockDim.x) {
    const size_t l = q / NN, r = q - l * NN;
    const size_t i = r / N, j = r - i * N;
    if (j < i) continue;
    const size_t qt = l * NN + j * N + i;
    double* a = p + q * K;
    double* b = p + qt * K;
    auto sym = [a, b](int k) { return (a[k] + b[k]) / 2.0; };
    const double s = pw_sum<3>(sym, 0, K);
    const bool ca = cov[q] != 0, cb = cov[qt] != 0;
    for (int k = 0; k < K; ++k) {
      const double x = sym(k) / s, oh = k == 0 ? 1.0 : 0.0;
      a[k] = ca ? x : oh;
      b[k] = cb ? x : oh;
    }
  }
}

}  // namespace

// Queue the draw on the handle's stream: nblk blocks (device arrays cuts[nblk + 1], keys[nblk][624], pos[nblk], validated by the
// caller) into out [L][N][N][K] (device).
int draw_pr_rho_launch(vmr_ctx* h, int nblk, const int64_t* cuts, const uint32_t* keys, const int32_t* pos, double bias0,
                       int undirected, double* out) {
  const Geo& g = h->g;
  if (undirected) {
    hipLaunchKernelGGL(k_draw_pr_rho<false>, dim3(nblk), dim3(DP_TPB), 0, h->stream, cuts, keys, pos, g.K, bias0, h->cov, out);
    HIPCHK(h, hipGetLastError());
    const size_t n = (size_t)g.L * g.N * g.N;
    const unsigned grid = (unsigned)std::min<size_t>(8192, (n + 255) / 256);
    hipLaunchKernelGGL(k_sym_pr_rho, dim3(grid), dim3(256), 0, h->stream, out, h->cov, g.L, g.N, g.K);
  } else {
    hipLaunchKernelGGL(k_draw_pr_rho<true>, dim3(nblk), dim3(DP_TPB), 0, h->stream, cuts, keys, pos, g.K, bias0, h->cov, out);
  }
  HIPCHK(h, hipGetLastError());
  return VMR_OK;
}
