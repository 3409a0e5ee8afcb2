"""The device random draws restated in NumPy, from the contracts in the comments of include/vimure_hip.h, csrc/sample_draw.h,
csrc/report_draw.h and csrc/generate.hip: Philox4x32-10, the categorical trial of vmr_sample, the report stream, the Poisson
draw (sequential inversion below 30, Hoermann's transformed rejection PTRS from 30 up) and the pair draw of vmr_generate_x /
vmr_generate_y / vmr_ppc_replicates.  Vectorised over ties and over (pair, reporter); nothing here imports vimure_amd.

Integer arithmetic (Philox) and the sampler's uniform and running sum are exact, so `sample_ref` must equal the device bit for
bit.  The Poisson draw goes through exp / log / lgamma and expressions a compiler may contract into FMAs, which may differ from
the device in the last few ulps.  A draw can differ only where one of the comparisons on its path is that close, so every
Poisson draw comes with a MARGIN: the smallest |lhs - rhs| / max(1, |lhs|, |rhs|) over

    u > cdf at every visited step of the inversion;   V <= vr, us >= 0.07, us < 0.013, V > us;
    the argument of floor against the nearest integer;   the final log-domain acceptance test;
    the branch test rate < 30;   the coin u < 0.5.

A draw is DECIDABLE when its margin is at least `MARGIN` = 1e-10: the operands are at most about 1e3 and carry a few ulps
(about 1e-13 absolute), which leaves three orders; about 4e-9 of all draws fall below it.  (The margin of a comparison is taken
wherever the comparison could lie on the path, also where short-circuit evaluation skips it: never too large.)"""
import numpy as np
from scipy.special import gammaln

MARGIN = 1e-10
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
_TWO26 = 67108864.0
_TWOM53 = 1.0 / 9007199254740992.0
Y_KEY = 0x9E3779B97F4A7C15          # vmr_generate_y keys its stream with seed ^ Y_KEY ...
Y_REPORTER = 0xFFFF                 # ... and the reporter word 0xffff


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al. 2011) on uint64 arrays that hold 32-bit words; returns the four output words."""
    c0, c1, c2, c3, k0, k1 = (_u64(v) & _M32 for v in (c0, c1, c2, c3, k0, k1))
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for r in range(10):
        if r:
            k0, k1 = (k0 + w0) & _M32, (k1 + w1) & _M32          # the key is bumped between rounds
        p0, p1 = m0 * c0, m1 * c2                                # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32
    return c0, c1, c2, c3


def _split(seed):
    seed = int(seed) % 2 ** 64
    return np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)


# ---------------------------------------------------------------------------------------------- vmr_sample
def sample_uniform(wa, wb):
    """The sampler's uniform in [0, 1) from two Philox words: 27 + 26 bits, exact in float64."""
    wa, wb = _u64(wa), _u64(wb)
    return ((wa >> np.uint64(5)).astype(np.float64) * _TWO26 + (wb >> np.uint64(6)).astype(np.float64)) * _TWOM53


def sample_uniforms(n_ties, seed, n_trials):
    """u [n_trials, n_ties]: counter (tie low, tie high, trial pair, 0), key (seed low, seed high); trial 2p takes words 0 and 1 of
    call p, trial 2p + 1 words 2 and 3."""
    t = np.arange(n_ties, dtype=np.uint64)
    k0, k1 = _split(seed)
    u = np.empty((n_trials, n_ties))
    for p in range((n_trials + 1) // 2):
        w = philox4x32_10(t & _M32, t >> _S32, np.uint64(p), np.uint64(0), k0, k1)
        u[2 * p] = sample_uniform(w[0], w[1])
        if 2 * p + 1 < n_trials:
            u[2 * p + 1] = sample_uniform(w[2], w[3])
    return u


def sample_ref(rho, seed, n_trials):
    """What vmr_sample(h, seed, n_trials) writes for rho [L, N, N, K]: uint8 [L, N, N].  A trial selects the first k with
    u < rho_0 + .. + rho_k (a sequential running sum in float64; the last category catches the rest); the tie's value is the most
    frequent category of its trials, first maximum."""
    rho = np.asarray(rho, dtype=np.float64)
    L, N, _, K = rho.shape
    r = rho.reshape(-1, K)
    T = r.shape[0]
    u = sample_uniforms(T, seed, n_trials)
    cnt = np.zeros((T, K), dtype=np.int64)
    rows = np.arange(T)
    for n in range(n_trials):
        sel = np.full(T, K - 1, dtype=np.int64)
        found = np.zeros(T, dtype=bool)
        acc = np.zeros(T)
        for k in range(K - 1):
            acc = acc + r[:, k]
            hit = ~found & (u[n] < acc)
            sel[hit] = k
            found |= hit
        cnt[rows, sel] += 1
    return np.argmax(cnt, axis=1).astype(np.uint8).reshape(L, N, N)          # (argmax: the first maximum)


# ---------------------------------------------------------------------------------------------- the report stream
def report_uniform(a, b):
    """The report stream's uniform from two Philox words: ((a >> 5) 2^26 + (b >> 6) + 0.5) 2^-53.  The + 0.5 rounds (to even) once
    the integer reaches 2^52, so the range is [2^-54, 1.0]: all-ones words give exactly 1.0."""
    a, b = _u64(a), _u64(b)
    return ((a >> np.uint64(5)).astype(np.float64) * _TWO26 + (b >> np.uint64(6)).astype(np.float64) + 0.5) * _TWOM53


class ReportStream:
    """The uniforms of many (layer, pair, reporter) lanes: counter (pair low, pair high, m ^ (l << 20), call number), key (seed low,
    seed high); a call's words are consumed 3, 2 then 1, 0.  `uniform(idx)` advances the lanes idx only."""

    def __init__(self, seed, l, pair, m):
        self.k0, self.k1 = _split(seed)
        pair = _u64(pair)
        self.c0, self.c1 = pair & _M32, pair >> _S32
        self.c2 = (_u64(m) ^ (_u64(l) << np.uint64(20))) & _M32
        n = self.c0.shape[0]
        self.n = np.zeros(n, dtype=np.uint64)
        self.have = np.zeros(n, dtype=np.int64)
        self.w = np.zeros((4, n), dtype=np.uint64)

    def uniform(self, idx=None):
        idx = np.arange(self.have.shape[0]) if idx is None else np.asarray(idx)
        sub = idx[self.have[idx] < 2]
        if sub.size:
            self.w[:, sub] = philox4x32_10(self.c0[sub], self.c1[sub], self.c2[sub], self.n[sub], self.k0, self.k1)
            self.n[sub] += np.uint64(1)
            self.have[sub] = 4
        h = self.have[idx]
        a, b = self.w[h - 1, idx], self.w[h - 2, idx]
        self.have[idx] = h - 2
        return report_uniform(a, b)


def report_uniforms(seed, l, pair, m, count):
    """The first `count` uniforms of the lanes (l, pair, m): float64 [count, lanes]."""
    l, pair, m = np.broadcast_arrays(_u64(l), _u64(pair), _u64(m))
    s = ReportStream(seed, l.ravel(), pair.ravel(), m.ravel())
    return np.stack([s.uniform() for _ in range(count)])


# ---------------------------------------------------------------------------------------------- Poisson
def _rel(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    return np.abs(a - b) / np.maximum(1.0, np.maximum(np.abs(a), np.abs(b)))


def _inversion(rate, u):
    """Sequential search: k = 0, p = cdf = exp(-rate); while u > cdf (and k < 1000): k += 1, p *= rate / k, cdf += p."""
    n = rate.shape[0]
    k = np.zeros(n, dtype=np.int64)
    p = np.exp(-rate)
    cdf = p.copy()
    mg = np.full(n, np.inf)
    act = np.arange(n)
    while act.size:
        mg[act] = np.minimum(mg[act], _rel(u[act], cdf[act]))
        act = act[(u[act] > cdf[act]) & (k[act] < 1000)]
        k[act] += 1
        p[act] = p[act] * (rate[act] / k[act].astype(np.float64))
        cdf[act] = cdf[act] + p[act]
    return k, mg


def _ptrs(rate, stream, idx):
    """Hoermann's PTRS (1993), as NumPy's legacy generator has it for rate >= 10, with at most 64 trials."""
    n = rate.shape[0]
    slam, loglam = np.sqrt(rate), np.log(rate)
    b = 0.931 + 2.53 * slam
    a = -0.059 + 0.02483 * b
    invalpha = 1.1239 + 1.1328 / (b - 3.4)
    vr = 0.9277 - 3.6224 / (b - 2.0)
    k = np.floor(rate + 0.5).astype(np.int64)                   # what 64 failed trials leave (not reached in practice)
    mg = np.full(n, np.inf)
    act = np.arange(n)
    for _ in range(64):
        if not act.size:
            break
        U = stream.uniform(idx[act]) - 0.5
        V = stream.uniform(idx[act])
        us = 0.5 - np.abs(U)
        ra, aa, ba = rate[act], a[act], b[act]
        x = (2.0 * aa / us + ba) * U + ra + 0.43
        kf = np.floor(x)
        m = np.minimum(mg[act], np.minimum(_rel(x, np.rint(x)), _rel(us, 0.07)))
        big = us >= 0.07
        m = np.where(big, np.minimum(m, _rel(V, vr[act])), m)
        squeeze = big & (V <= vr[act])
        m = np.where(squeeze, m, np.minimum(m, _rel(us, 0.013)))
        small = ~squeeze & (us < 0.013)
        m = np.where(small, np.minimum(m, _rel(V, us)), m)
        again = ~squeeze & ((kf < 0.0) | (small & (V > us)))
        test = ~squeeze & ~again
        kq = np.where(test, kf, 0.0)
        lhs = np.log(V) + np.log(invalpha[act]) - np.log(aa / (us * us) + ba)
        rhs = -ra + kq * loglam[act] - gammaln(kq + 1.0)
        m = np.where(test, np.minimum(m, _rel(lhs, rhs)), m)
        done = squeeze | (test & (lhs <= rhs))
        mg[act] = m
        k[act[done]] = kf[done].astype(np.int64)
        act = act[~done]
    return k, mg


def poisson_ref(rate, stream, idx=None):
    """Poisson(rate) for the lanes idx of `stream` (rate aligned with idx): (draw int64, margin float64).  rate <= 0: 0, no
    uniform is consumed."""
    rate = np.asarray(rate, dtype=np.float64)
    idx = np.arange(rate.shape[0]) if idx is None else np.asarray(idx)
    k = np.zeros(rate.shape[0], dtype=np.int64)
    mg = np.full(rate.shape[0], np.inf)
    pos = rate > 0.0
    mg[pos] = _rel(rate[pos], 30.0)
    lo = np.flatnonzero(pos & (rate < 30.0))
    hi = np.flatnonzero(pos & ~(rate < 30.0))
    if lo.size:
        kk, mm = _inversion(rate[lo], stream.uniform(idx[lo]))
        k[lo], mg[lo] = kk, np.minimum(mg[lo], mm)
    if hi.size:
        kk, mm = _ptrs(rate[hi], stream, idx[hi])
        k[hi], mg[hi] = kk, np.minimum(mg[hi], mm)
    return k, mg


# ---------------------------------------------------------------------------------------------- the pair, X, Y
def pair_ref(la, lb, th, eta, stream):
    """The reports (x_ij, x_ji) of every lane of `stream`, unclamped, and the lane's margin.  a = la th, b = lb th; a fair coin
    (u < 0.5: i -> j first) picks the direction drawn first ~ Poisson((own + eta mirror) / (1 - eta^2)); the other
    ~ Poisson(own + eta first)."""
    a, b = la * th, lb * th
    inv = 1.0 / (1.0 - eta * eta)
    u = stream.uniform()
    ij = u < 0.5
    mg = _rel(u, 0.5)
    first, m1 = poisson_ref(np.where(ij, (a + eta * b) * inv, (b + eta * a) * inv), stream)
    second, m2 = poisson_ref(np.where(ij, b, a) + eta * first.astype(np.float64), stream)
    return np.where(ij, first, second), np.where(ij, second, first), np.minimum(mg, np.minimum(m1, m2))


def generate_x_ref(lam, theta, eta, seed, self_reporter=False):
    """What vmr_generate_x draws from lam [L, N, N] (float64), theta [L, M], eta, seed -- before its clamp at 255: X int64
    [L, N, N, M] and the margins [L, N, N, M] (of a pair's draw at both directions; inf where nothing is drawn).  The diagonal
    holds no report; self_reporter: only the reporters m = i and m = j of a pair are drawn (M == N), the rest stays zero."""
    lam, theta = np.asarray(lam, dtype=np.float64), np.asarray(theta, dtype=np.float64)
    L, N, _ = lam.shape
    M = theta.shape[1]
    iu, ju = np.triu_indices(N, 1)
    P = iu.shape[0]
    X = np.zeros((L, N, N, M), dtype=np.int64)
    mg = np.full((L, N, N, M), np.inf)
    if P == 0:
        return X, mg
    if self_reporter:
        assert M == N
        l = np.repeat(np.arange(L), 2 * P)
        i, j = np.tile(np.repeat(iu, 2), L), np.tile(np.repeat(ju, 2), L)
        m = np.where(np.tile(np.arange(2), L * P) == 0, i, j)
    else:
        l = np.repeat(np.arange(L), P * M)
        i, j = np.tile(np.repeat(iu, M), L), np.tile(np.repeat(ju, M), L)
        m = np.tile(np.arange(M), L * P)
    s = ReportStream(seed, l, i * N + j, m)
    xij, xji, g = pair_ref(lam[l, i, j], lam[l, j, i], theta[l, m], float(eta), s)
    X[l, i, j, m], X[l, j, i, m] = xij, xji
    mg[l, i, j, m], mg[l, j, i, m] = g, g
    return X, mg


def lam_of_y(Y, lambda_diff=None):
    """lambda of a tie from the ground truth: 0.01 where Y = 0, else Y, or 0.01 + lambda_diff when that is given and positive."""
    Y = np.asarray(Y)
    on = (0.01 + lambda_diff) if (lambda_diff is not None and lambda_diff > 0.0) else Y.astype(np.float64)
    return np.where(Y == 0, 0.01, on)


def generate_y_ref(w, grp, K, seed, L):
    """What vmr_generate_y writes: Y[l, i, j] ~ Poisson(w[grp_i, grp_j]) clipped to K - 1, zero diagonal: (uint8 [L, N, N], margins
    [L, N, N]).  The stream of the ordered tie t = i N + j of layer l, keyed by seed ^ Y_KEY, reporter word 0xffff."""
    w, grp = np.asarray(w, dtype=np.float64), np.asarray(grp)
    N = grp.shape[0]
    i, j = np.nonzero(~np.eye(N, dtype=bool))
    P = i.shape[0]
    l = np.repeat(np.arange(L), P)
    i, j = np.tile(i, L), np.tile(j, L)
    s = ReportStream((int(seed) % 2 ** 64) ^ Y_KEY, l, i * N + j, np.full(L * P, Y_REPORTER))
    y, g = poisson_ref(w[grp[i], grp[j]], s)
    Y = np.zeros((L, N, N), dtype=np.uint8)
    mg = np.full((L, N, N), np.inf)
    Y[l, i, j] = np.minimum(y, K - 1)
    mg[l, i, j] = g
    return Y, mg


def ppc_replicates_ref(rho, R, theta, lam, eta, seed_y, seed_x, n_trials=1):
    """What vmr_ppc_replicates returns for a handle with rho [L, N, N, K] and mask R (None: all ones): counts int64 [n_rep, L, 6],
    by_reporter int64 [n_rep, L, M, 2], the smallest margin, the largest count drawn inside the support of R.  Replicate r: Y = sample_ref(rho, seed_y + r),
    the tie's lambda is lam[r, l, Y], X = generate_x_ref(.., theta[r], eta[r], seed_x + r) UNCLAMPED, reduced over the support of
    R by ppc_rep_util.stats_np."""
    from tests.ppc_rep_util import stats_np
    theta, lam, eta = np.asarray(theta, dtype=np.float64), np.asarray(lam, dtype=np.float64), np.atleast_1d(eta)
    L = rho.shape[0]
    cs, bs, lo, top = [], [], np.inf, 0
    for r in range(eta.shape[0]):
        Y = sample_ref(rho, (int(seed_y) + r) % 2 ** 64, n_trials)
        lam_t = lam[r][np.arange(L)[:, None, None], Y]
        X, mg = generate_x_ref(lam_t, theta[r], float(eta[r]), (int(seed_x) + r) % 2 ** 64)
        c, b = stats_np(X, R)
        cs.append(c)
        bs.append(b)
        lo, top = min(lo, float(mg.min())), max(top, int((X if R is None else np.where(np.asarray(R) != 0, X, 0)).max()))
    return np.stack(cs), np.stack(bs), lo, top
