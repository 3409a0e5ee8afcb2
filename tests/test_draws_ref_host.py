"""Host: the NumPy restatement of the device draws (tests/draws_ref.py) held to outside truth -- the Random123 known-answer
vectors of Philox4x32-10, the end points of the two uniforms, the exact Poisson distribution (chi-square against
scipy.stats.poisson on both branches), the pair's mean and coin -- and the CASES that tests/test_hip_draws_exact.py runs on
the GPU, built here so that this file can assert, without a GPU, that none of them holds an undecidable draw (a draw whose
margin is below draws_ref.MARGIN, see there): with that condition met the GPU tests compare every element with no allowance.
A seed that produced an undecidable draw would be changed here, on the CPU, never after a look at device output."""
import functools

import numpy as np
import pytest
from scipy import stats

from tests import draws_ref as dr

# ================================================================================================ the cases of the GPU file
SAMPLE_L, SAMPLE_N = 3, 23
SAMPLE_KS_REG, SAMPLE_KS_GEN = (2, 3, 8), (9, 12, 70, 256)       # trial counts in registers (K <= 8) / in LDS
SAMPLE_TRIALS = (1, 2, 3, 7)
SAMPLE_SEEDS = (7, 2 ** 32 + 5, 2 ** 64 - 1)                      # (the second one sets the key's high word)
CRAFT_SEED = 7                                                    # the hand-made rows below are made for this seed


def engine_data(L, N, M, seed=0):
    """A small X for a handle whose rho is then set: 5 % of the entries hold a report."""
    g = np.random.RandomState(seed)
    return ((g.rand(L, N, N, M) < 0.05) * g.randint(1, 4, (L, N, N, M))).astype(np.uint8)


def engine_state(L, M, K, rho):
    """(gamma, phi, nu, rho) for set_state: only rho matters to the draws."""
    return np.full((L, M), 2.0), np.full((L, M), 1.5), np.full((L, K), 3.0), np.full((L, K), 2.0), 3.0, 2.5, rho


@functools.lru_cache(maxsize=None)
def sample_case(K):
    """rho [3, 23, 23, K] and the ties of its hand-made rows.  Random rows, and by tie index (t in [L,N,N] order):
      one-hot rows; rows with exact zeros in the middle; rows that sum to 1 - 1e-12 (the last category catches the rest);
      boundary rows, for trial 0 of CRAFT_SEED with the host's u_t: rho_0 = u_t exactly must select category 1 (u < sum is
      false at equality), rho_0 = nextafter(u_t, 1) must select category 0; for K >= 3 the same at the last boundary: zeros,
      then rho_{K-2} = u_t | nextafter(u_t, 1), the rest in K - 1;
      mode ties, K >= 3, for n_trials = 2 of CRAFT_SEED: (0, x, 1 - x, 0..) with x between the tie's two uniforms, so one trial
      selects 1 and the other 2: the first maximum, 1, wins."""
    L, N = SAMPLE_L, SAMPLE_N
    T = L * N * N
    g = np.random.RandomState(100 + K)
    rho = g.gamma(0.7, 1.0, (T, K)) + 1e-3
    rho /= rho.sum(-1, keepdims=True)
    u = dr.sample_uniforms(T, CRAFT_SEED, 2)
    marks = {"at": [], "above": [], "last_at": [], "last_above": [], "mode": []}
    for q in range(min(K, 12)):                                  # one-hot
        rho[10 + q] = 0.0
        rho[10 + q, (q * 7) % K if K > 12 else q] = 1.0
    rho[30, -1], rho[30, :-1] = 1.0, 0.0                         # one-hot in the last category
    if K >= 3:
        for t in range(40, 60):                                  # exact zeros in the middle
            rho[t, 1:K - 1:2 if K > 3 else 1] = 0.0
            rho[t] /= rho[t].sum()
    rho[70:90] *= (1.0 - 1e-12)                                  # rows that sum to 1 - 1e-12
    rest = g.gamma(1.0, 1.0, (T, K)) + 0.05                      # how a boundary row spreads what rho_0 leaves
    for n, t in enumerate(list(range(100, 112)) + list(range(N * N + 3, N * N + 15)) + list(range(2 * N * N + 500, 2 * N * N + 512))):
        ut = u[0, t]
        assert 0.0 < ut < 1.0
        kind = ("at", "above", "last_at", "last_above")[n % 4 if K >= 3 else n % 2]
        edge = ut if kind.endswith("at") else np.nextafter(ut, 1.0)
        if kind in ("at", "above"):
            rho[t, 0] = edge
            rho[t, 1:] = rest[t, 1:] / rest[t, 1:].sum() * (1.0 - edge)
        else:
            rho[t] = 0.0
            rho[t, K - 2], rho[t, K - 1] = edge, 1.0 - edge
        marks[kind].append(t)
    if K >= 3:
        for t in list(range(200, 215)) + list(range(N * N + 200, N * N + 215)):
            assert u[0, t] != u[1, t]
            rho[t] = 0.0
            rho[t, 1] = 0.5 * (u[0, t] + u[1, t])
            rho[t, 2] = 1.0 - rho[t, 1]
            marks["mode"].append(t)
    return np.ascontiguousarray(rho.reshape(L, N, N, K)), {k: np.array(v, dtype=np.int64) for k, v in marks.items()}


@functools.lru_cache(maxsize=None)
def sample_want(K, n_trials, seed):
    return dr.sample_ref(sample_case(K)[0], seed, n_trials)


@functools.lru_cache(maxsize=None)
def sample_big_case():
    """L = 1, N = 1030, K = 2: 1 060 900 ties, more than the 4096 x 256 threads k_sample launches: its grid-stride loop takes a
    second trip."""
    N = 1030
    p = np.random.RandomState(31).rand(1, N, N)
    return np.ascontiguousarray(np.stack([p, 1.0 - p], axis=-1))


@functools.lru_cache(maxsize=None)
def sample_big_want(n_trials, seed):
    return dr.sample_ref(sample_big_case(), seed, n_trials)


def hash_name(name):
    return sum((k + 1) * ord(c) for k, c in enumerate(name))


@functools.lru_cache(maxsize=None)
def sample_gen_big_case():
    """L = 1, N = 520, K = 9: 270 400 ties, more than the 4096 x 64 threads k_sample_gen launches: its grid-stride loop takes a
    second trip, on which a thread's LDS count column is used again."""
    N, K = 520, 9
    rho = np.random.RandomState(32).gamma(0.7, 1.0, (1, N, N, K)) + 1e-3
    return np.ascontiguousarray(rho / rho.sum(-1, keepdims=True))


@functools.lru_cache(maxsize=None)
def sample_gen_big_want(n_trials, seed):
    return dr.sample_ref(sample_gen_big_case(), seed, n_trials)


def _gx(lam, theta, eta, seed, self_reporter=False, Y=None, lambda_diff=None):
    return dict(lam=lam, theta=theta, eta=eta, seed=seed, self_reporter=self_reporter, Y=Y, lambda_diff=lambda_diff)


GENERATE_X_CASES = ("base_eta0", "base_eta0.3", "base_eta0.9", "stride", "clamp", "self_reporter", "from_y", "from_y_diff", "second_trip")


@functools.lru_cache(maxsize=None)
def generate_x_case(name):
    """The arguments of vmr_generate_x (lam float64 [L, N, N] or Y uint8 with lambda_diff; theta [L, M]; eta; seed)."""
    g = np.random.RandomState(hash_name(name))
    if name.startswith("base_eta"):
        # a = lam theta from 0.005 to 210 on the 70 reporters of one tie row: the first-draw rates (a + eta b) / (1 - eta^2)
        # span 0.005 to about 200 and straddle 30 across the reporters (lam scaled by 1 - eta: with a = b the first rate is a)
        eta = float(name[len("base_eta"):])
        L, N, M = 3, 23, 70
        lam = g.choice([0.01, 0.3, 1.5, 3.0, 10.0], size=(L, N, N)) * (1.0 - eta)
        theta = np.exp(np.linspace(np.log(0.5), np.log(21.0), M))[None, :] * (1.0 + 0.05 * g.rand(L, M))
        return _gx(lam, theta, eta, 2 ** 40 + 17)
    if name == "stride":                                         # M = 300: the reporter stride of 256 threads, m > 255
        L, N, M = 2, 9, 300
        return _gx(g.choice([0.01, 1.0, 4.0], size=(L, N, N)), 0.2 + 9.0 * g.rand(L, M), 0.3, 5)
    if name == "clamp":                                          # counts on both sides of 255: first rates from 170 to 490
        L, N, M = 1, 9, 20
        return _gx(np.full((L, N, N), 100.0), 1.2 + 2.2 * g.rand(L, M), 0.3, 6)
    if name == "self_reporter":
        L, N, M = 3, 23, 23
        return _gx(g.choice([0.01, 1.0, 12.0], size=(L, N, N)), 0.5 + 4.0 * g.rand(L, M), 0.3, 2 ** 64 - 3, self_reporter=True)
    if name in ("from_y", "from_y_diff"):
        L, N, M = 2, 23, 70
        Y = g.randint(0, 4, (L, N, N)).astype(np.uint8) * (g.rand(L, N, N) < 0.5)
        return _gx(None, 0.5 + 14.0 * g.rand(L, M), 0.3, 8, Y=Y.astype(np.uint8), lambda_diff=0.7 if name == "from_y_diff" else None)
    if name == "second_trip":                                    # 1 060 900 ties > 2^20 workgroups: k_gen_x's block-stride loop goes round
        L, N, M = 1, 1030, 2
        return _gx(0.01 + 0.5 * g.rand(L, N, N), 0.5 + g.rand(L, M), 0.3, 9)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def generate_x_want(name):
    """(X int64 unclamped, smallest margin) of the case."""
    c = generate_x_case(name)
    lam = c["lam"] if c["lam"] is not None else dr.lam_of_y(c["Y"], c["lambda_diff"])
    X, mg = dr.generate_x_ref(lam, c["theta"], c["eta"], c["seed"], c["self_reporter"])
    return X, float(mg.min())


GENERATE_Y_KS = (2, 4, 64)                                      # (64: the PTRS draws of w = 45 are not clipped away)
GENERATE_Y_SEEDS = (11, 2 ** 63 + 2 ** 31 + 1)


@functools.lru_cache(maxsize=None)
def generate_y_case():
    """L = 2, N = 37, C = 3; w holds 0, 0.02, 0.8, 5 (inversion) and 45 (PTRS)."""
    w = np.array([[5.0, 0.02, 0.0], [0.8, 45.0, 0.02], [0.0, 0.8, 5.0]])
    return dict(L=2, N=37, C=3, w=w, grp=(np.arange(37) * 3 // 37).astype(np.int32))


@functools.lru_cache(maxsize=None)
def generate_y_want(K, seed):
    c = generate_y_case()
    Y, mg = dr.generate_y_ref(c["w"], c["grp"], K, seed, c["L"])
    return Y, float(mg.min())


PPC_SEED_Y, PPC_SEED_X = 1234, 2 ** 33 + 98765
PPC_CASES = ("K2", "K3", "K12", "coo_self", "high")


@functools.lru_cache(maxsize=None)
def ppc_case(name):
    """A handle (X, R, K, rho; coo: built by from_coo) and the replicates' parameters (theta [3, L, M], lam [3, L, K], eta [3]).
    Base: L = 2, N = 23, M = 70, Bernoulli(0.3) mask with rows forced empty and full; coo_self: N = M = 23 with the self-reporter
    mask; high: lambda high enough that replicate counts pass 255."""
    g = np.random.RandomState(hash_name("ppc" + name))
    K = {"K2": 2, "K3": 3, "K12": 12, "coo_self": 2, "high": 2}[name]
    L, N = 2, 23
    M = N if name == "coo_self" else 70
    X = engine_data(L, N, M, seed=K)
    if name == "coo_self":
        R = np.zeros((L, N, N, M), np.uint8)
        idx = np.arange(N)
        R[:, idx, :, idx] = 1
        R[:, :, idx, idx] = 1
        X = X * R
    else:
        R = (g.rand(L, N, N, M) < 0.3).astype(np.uint8)
        R[0, 3, :5], R[1, 7, 10:13], R[0, 20, 22] = 0, 0, 0
        R[0, 4, :4], R[1, 22, 0], R[1, 0, 22], R[0, 9, 9] = 1, 1, 1, 1
    rho = g.rand(L, N, N, K)
    rho[..., 0] *= 3.0
    rho /= rho.sum(-1, keepdims=True)
    n_rep = 3
    theta = 0.5 + 1.5 * g.rand(n_rep, L, M)
    if name == "high":
        lam = np.broadcast_to(np.array([0.01, 120.0]), (n_rep, L, K)).copy()
        theta += 1.5
    else:
        lam = np.linspace(0.01, 1.5, K)[None, None, :] * (0.8 + 0.4 * g.rand(n_rep, L, 1))
        lam[1, 1] = lam[1, 1, ::-1]                              # the table is per replicate and per layer
    eta = np.array([0.3, 0.0, 0.6])
    return dict(K=K, X=X, R=R, rho=np.ascontiguousarray(rho), coo=name == "coo_self", theta=theta, lam=lam, eta=eta)


@functools.lru_cache(maxsize=None)
def ppc_want(name, n_trials):
    """(counts, by_reporter, smallest margin, largest count drawn)"""
    c = ppc_case(name)
    return dr.ppc_replicates_ref(c["rho"], c["R"], c["theta"], c["lam"], c["eta"], PPC_SEED_Y, PPC_SEED_X, n_trials)


PPC_RUNS = [(n, t) for n in PPC_CASES for t in ((1, 3) if n.startswith("K") else (1,))]


# ================================================================================================ Philox
KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answer_vectors():
    """Random123's kat_vectors for philox4x32-10, one by one and as one vectorised call."""
    for ctr, key, want in KAT:
        got = dr.philox4x32_10(*ctr, *key)
        assert tuple(int(w) for w in got) == want, [hex(int(w)) for w in got]
    cols = [np.array([k[0][q] for k in KAT], dtype=np.uint64) for q in range(4)] + [np.array([k[1][q] for k in KAT], dtype=np.uint64) for q in range(2)]
    got = np.stack(dr.philox4x32_10(*cols), axis=1)
    assert got.dtype == np.uint64 and np.array_equal(got, np.array([k[2] for k in KAT], dtype=np.uint64))


# ================================================================================================ uniforms, streams
def test_uniform_end_points():
    """The sampler's u lies in [0, 1 - 2^-53].  The report uniform is 2^-54 for all-zero words; for all-ones words the integer is
    2^53 - 1, and 2^53 - 1 + 0.5 rounds to 2^53, so u = 1.0 exactly: the range is [2^-54, 1], not the open (0, 1) -- at
    probability 2^-53, recorded in report_draw.h and left as it is (log(V) = 0 and us = 0 there)."""
    ones = 0xFFFFFFFF
    assert dr.sample_uniform(0, 0) == 0.0 and dr.sample_uniform(ones, ones) == 1.0 - 2.0 ** -53
    assert dr.sample_uniform(1 << 5, 0) == 2.0 ** -27 and dr.sample_uniform(0, 1 << 6) == 2.0 ** -53
    assert dr.sample_uniform(31, 63) == 0.0                      # the low 5 and 6 bits are dropped
    assert dr.report_uniform(0, 0) == 2.0 ** -54
    assert dr.report_uniform(ones, ones) == 1.0
    assert dr.report_uniform(ones, ones - 64) == 1.0 - 2.0 ** -52      # 2^53 - 2 + 0.5 ties to even: 2^53 - 2
    assert dr.report_uniform(((1 << 26) - 1) << 5, ones) == 0.5 - 2.0 ** -54      # 2^52 - 1: the last integer whose + 0.5 is exact
    assert dr.report_uniform(1 << 31, 0) == 0.5                  # 2^52 + 0.5 ties to even: the coin's u < 0.5 is false here


def test_stream_counters_and_word_order():
    seed = 2 ** 40 + 3
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    # the sampler: counter (tie low, tie high, trial pair, 0); trial 2p words 0, 1; trial 2p + 1 words 2, 3
    u = dr.sample_uniforms(5, seed, 3)
    for t in range(5):
        w0, w1 = dr.philox4x32_10(t, 0, 0, 0, k0, k1), dr.philox4x32_10(t, 0, 1, 0, k0, k1)
        assert u[0, t] == dr.sample_uniform(w0[0], w0[1]) and u[1, t] == dr.sample_uniform(w0[2], w0[3])
        assert u[2, t] == dr.sample_uniform(w1[0], w1[1])
    # the report stream: counter (pair low, pair high, m ^ (l << 20), call); words 3, 2 then 1, 0
    l, pair, m = 2, 2 ** 33 + 7, 261
    got = dr.report_uniforms(seed, l, pair, m, 5)[:, 0]
    for call in range(3):
        w = dr.philox4x32_10(pair & 0xFFFFFFFF, pair >> 32, m ^ (l << 20), call, k0, k1)
        assert got[2 * call] == dr.report_uniform(w[3], w[2])
        if 2 * call + 1 < 5:
            assert got[2 * call + 1] == dr.report_uniform(w[1], w[0])
    assert np.array_equal(dr.report_uniforms(seed, 1, 9, 0, 2), dr.report_uniforms(seed, 0, 9, 1 << 20, 2))
    assert not np.array_equal(dr.report_uniforms(seed, 1, 9, 0, 2), dr.report_uniforms(seed, 0, 9, 0, 2))
    # lanes advance on their own
    s = dr.ReportStream(seed, np.zeros(3, int), np.arange(3), np.zeros(3, int))
    a = s.uniform(np.array([0, 2]))
    b = s.uniform()
    full = dr.report_uniforms(seed, 0, np.arange(3), 0, 2)
    assert np.array_equal(a, full[0, [0, 2]]) and np.array_equal(b, [full[1, 0], full[0, 1], full[1, 2]])


def test_sample_ref_against_a_scalar_loop():
    g = np.random.RandomState(3)
    L, N, K = 2, 5, 4
    rho = g.rand(L, N, N, K)
    rho /= rho.sum(-1, keepdims=True)
    rho[0, 0, 1] = (0.0, 1.0, 0.0, 0.0)
    for n_trials in (1, 2, 5):
        u = dr.sample_uniforms(L * N * N, 9, n_trials)
        want = np.zeros(L * N * N, np.uint8)
        for t, r in enumerate(rho.reshape(-1, K)):
            cnt = [0] * K
            for n in range(n_trials):
                acc, sel = 0.0, K - 1
                for k in range(K):
                    acc += r[k]
                    if u[n, t] < acc:
                        sel = k
                        break
                cnt[sel] += 1
            want[t] = cnt.index(max(cnt))
        got = dr.sample_ref(rho, 9, n_trials)
        assert got.dtype == np.uint8 and np.array_equal(got.ravel(), want) and got[0, 0, 1] == 1


def test_sample_cases_hold_their_hand_made_rows():
    """The boundary rows select what the contract `first k with u < running sum` says, on the host; the mode ties give 1."""
    for K in SAMPLE_KS_REG + SAMPLE_KS_GEN:
        rho, marks = sample_case(K)
        assert np.all(rho >= 0.0) and np.abs(rho.sum(-1) - 1.0).max() < 1e-9
        y1 = sample_want(K, 1, CRAFT_SEED).ravel()
        assert np.all(y1[marks["at"]] == 1) and np.all(y1[marks["above"]] == 0)
        assert len(marks["at"]) >= 9 and len(marks["above"]) >= 9
        if K >= 3:
            assert np.all(y1[marks["last_at"]] == K - 1) and np.all(y1[marks["last_above"]] == K - 2)
            y2 = sample_want(K, 2, CRAFT_SEED).ravel()
            assert np.all(y2[marks["mode"]] == 1) and len(marks["mode"]) == 30
            assert set(np.unique(y1[marks["mode"]])) == {1, 2}       # (either trial order occurs)
        assert len({sample_want(K, 1, s).tobytes() for s in SAMPLE_SEEDS}) == 3


# ================================================================================================ Poisson, pair
def _draw(rate, n, seed):
    s = dr.ReportStream(seed, np.zeros(n, int), np.arange(n), np.zeros(n, int))
    return dr.poisson_ref(np.full(n, rate), s)


@pytest.mark.parametrize("rate", [0.01, 0.7, 3.7, 29.9, 30.0, 41.5, 400.0])
def test_poisson_ref_against_the_exact_distribution(rate):
    """30 000 draws per rate, both branches (inversion below 30, PTRS from 30 up): chi-square against scipy.stats.poisson over
    the bins with expected count >= 5 (tails pooled), p > 1e-4; the mean within 4.5 standard errors."""
    n = 30000
    k, mg = _draw(rate, n, 12345)
    assert k.min() >= 0 and (mg.min() >= dr.MARGIN or rate == 30.0)      # (rate == 30 exactly: the branch test has no margin)
    z = (k.mean() - rate) / np.sqrt(rate / n)
    lo, hi = int(stats.poisson.ppf(1e-9, rate)), int(stats.poisson.isf(1e-9, rate)) + 1
    ks = np.arange(lo, hi + 1)
    e = n * stats.poisson.pmf(ks, rate)
    while e[0] < 5.0 and len(ks) > 2:                            # pool the lower tail into its neighbour
        e, ks = np.concatenate([[e[0] + e[1]], e[2:]]), ks[1:]
    while e[-1] < 5.0 and len(ks) > 2:
        e, ks = np.concatenate([e[:-2], [e[-2] + e[-1]]]), ks[:-1]
    e[0] += n * stats.poisson.cdf(lo - 1, rate)                  # (what lies outside [lo, hi]: about 1e-9 each)
    e[-1] += n * stats.poisson.sf(hi, rate)
    o = np.bincount(np.clip(k, ks[0], ks[-1]) - ks[0], minlength=len(ks)).astype(np.float64)
    chi2 = ((o - e) ** 2 / e).sum()
    p = stats.chi2.sf(chi2, len(ks) - 1)
    print("rate %g: mean z %.2f, chi2 %.1f on %d bins, p %.4f" % (rate, z, chi2, len(ks), p))
    assert abs(z) < 4.5, z
    assert p > 1e-4, (chi2, len(ks), p)


def test_poisson_ref_edges():
    s = dr.ReportStream(1, np.zeros(4, int), np.arange(4), np.zeros(4, int))
    k, mg = dr.poisson_ref(np.array([0.0, -1.0, np.nan, 1e-300]), s)
    assert np.array_equal(k, [0, 0, 0, 0]) and np.all(mg[:3] == np.inf)
    assert np.array_equal(s.n, [0, 0, 0, 1])                     # a rate <= 0 consumes nothing
    # the margin flags a comparison at equality: u = cdf(0) = exp(-rate)
    u = dr.report_uniforms(1, 0, 5, 0, 1)[0, 0]
    s = dr.ReportStream(1, [0], [5], [0])
    k, mg = dr.poisson_ref(np.array([-np.log(u)]), s)
    assert mg[0] < 1e-15 and k[0] in (0, 1)


@pytest.mark.parametrize("a,b,eta", [(1.3, 0.4, 0.3), (40.0, 5.0, 0.5), (0.02, 0.0, 0.9)])
def test_pair_ref_mean_and_coin(a, b, eta):
    """E[x_ij] = (a + eta b) / (1 - eta^2) in either order of the draw; the coin is fair."""
    n = 20000
    s = dr.ReportStream(77, np.zeros(n, int), np.arange(n), np.full(n, 3))
    xij, xji, mg = dr.pair_ref(np.full(n, a), np.full(n, b), 1.0, eta, s)
    assert mg.shape == (n,) and mg.min() >= 0.0                  # (5 + 0.5 * 50 is a second rate of exactly 30: margin 0)
    for x, m in ((xij, (a + eta * b) / (1.0 - eta * eta)), (xji, (b + eta * a) / (1.0 - eta * eta))):
        se = x.std(ddof=1) / np.sqrt(n)
        assert abs(x.mean() - m) <= 5.0 * se, (x.mean(), m, se)
    heads = (dr.report_uniforms(77, 0, np.arange(n), 3, 1)[0] < 0.5).mean()
    assert abs(heads - 0.5) <= 4.5 * 0.5 / np.sqrt(n), heads


def test_generate_refs_shapes_and_scope():
    X, mg = generate_x_want("self_reporter")
    L, N, M = X.shape[0], X.shape[1], X.shape[3]
    i, j, m = np.arange(N)[:, None, None], np.arange(N)[None, :, None], np.arange(M)[None, None, :]
    scope = ((m == i) | (m == j)) & (i != j)
    assert X.dtype == np.int64 and not X[:, ~scope].any() and X[:, scope].any()
    X, mg = generate_x_want("clamp")
    assert X.max() > 255 and not X[:, np.arange(9), np.arange(9)].any()
    assert (X > 255).mean() > 0.2 and ((X > 0) & (X < 255)).mean() > 0.15 and (X == 255).any()      # both sides of the clamp, and 255 itself
    Y, mg = generate_y_want(4, GENERATE_Y_SEEDS[0])
    assert Y.dtype == np.uint8 and Y.max() == 3 and not Y[:, np.arange(37), np.arange(37)].any()
    assert generate_y_want(2, GENERATE_Y_SEEDS[0])[0].max() == 1
    y64 = generate_y_want(64, GENERATE_Y_SEEDS[0])[0]
    assert 45 < y64.max() < 63 and len(np.unique(y64[y64 > 20])) > 20      # the PTRS draws show
    assert generate_x_case("self_reporter")["theta"].shape == (L, M)


# ================================================================================================ the condition of the GPU file
@pytest.mark.parametrize("name", GENERATE_X_CASES)
def test_no_undecidable_draw_generate_x(name):
    X, lo = generate_x_want(name)
    print("%s: %d entries, smallest margin %.3e, largest count %d" % (name, X.size, lo, X.max()))
    assert lo >= dr.MARGIN, lo


def test_base_cases_take_both_branches_on_one_tie_row():
    for eta in ("0", "0.3", "0.9"):
        c = generate_x_case("base_eta" + eta)
        a = c["lam"][..., None] * c["theta"][:, None, None, :]
        first = (a + c["eta"] * a.transpose(0, 2, 1, 3)) / (1.0 - c["eta"] ** 2)
        assert first.min() < 0.006 and 150.0 < first.max() < 1000.0
        assert ((first.min(-1) < 30.0) & (first.max(-1) >= 30.0)).mean() > 0.2     # rows that straddle the branch test


@pytest.mark.parametrize("K", GENERATE_Y_KS)
def test_no_undecidable_draw_generate_y(K):
    for seed in GENERATE_Y_SEEDS:
        Y, lo = generate_y_want(K, seed)
        assert lo >= dr.MARGIN, (seed, lo)


@pytest.mark.parametrize("name,n_trials", PPC_RUNS)
def test_no_undecidable_draw_ppc(name, n_trials):
    counts, by_rep, lo, top = ppc_want(name, n_trials)
    assert lo >= dr.MARGIN, lo
    assert counts.shape == (3, 2, 6) and counts[..., 0].min() > 0
    assert (top > 255) == (name == "high"), top                  # (top: the largest count inside the support of R)
