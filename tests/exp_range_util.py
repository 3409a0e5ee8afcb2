"""Cases in which the rho update's raw exponentials leave the range of a double -- TEST INFRASTRUCTURE.

The reference takes exp(a_k) with no max-subtraction and normalises only where the sum is positive (model.py:807-811): a tie
whose exponentials all underflow keeps an all-zero row, a tie with an overflowing one becomes inf/inf = NaN.  `build_case` makes
the smallest network (L = 2, N = 48, M = 64, uint8 counts) in which the ties of single waves fall on both sides of those edges,
and `bands` classifies every tie from a_k recomputed here in extended precision, so that a GPU test can apply to each row the
tolerance that its band allows and a host test can show that no row sits so close to an edge that last-bit differences between
two exp implementations would decide its band.

Layer 0 is mild (every |a_k| < 700); layer 1 carries the extreme state and the large counts."""
import numpy as np
from scipy.special import psi

L, N, M = 2, 48, 64
EPS = 1e-12
PRI = (0.1, 0.1, 10.0, 10.0, 0.5, 1.0)              # the project's usual priors (sub-steps)
PRI_STRONG = (2e4, 0.1, 1e6, 10.0, 0.5, 1.0)        # whole sweeps: theta and lambda stay where the first sweep put them
U_MIN = 2.0 ** -1074                                # one unit of the subnormal range
DBL_MIN = 2.0 ** -1022
LN_ZERO = float(np.log(np.longdouble(2.0)) * -1075)   # exp(a) rounds to 0 below: -745.1332...
LN_MAX = float(np.log(np.longdouble(np.finfo(np.float64).max)))   # exp(a) overflows above: 709.7827...
ONES_SPREAD = 1.3                                   # max_k / min_k of E[lambda_k] in layer 1 under the all-ones mask stays below
IRREGULAR = 1e-14                                   # the kernels' |1 - sum(rho)| threshold of an "irregular" tie
SAFE, LITERAL, SUBNORMAL, ZERO, NAN = range(5)
BAND_NAMES = ("safe", "literal", "subnormal", "zero", "nan")

# (K, mask, seed) of every committed case: tests/test_exp_range_host.py holds each of them to the conditions the GPU tests rely on.
CASES = [(K, mask, 1) for K in (2, 3, 5, 8, 9, 16) for mask in ("partial", "ones")]
SWEEP_CASES = [(K, "partial", seed) for K in (2, 3) for seed in (1, 2, 3)]   # (seeds 2, 3: the other units of the lockstep loop)


def make_data(mask, seed, large=True, clustered=True):
    """X, R.

    clustered (the sub-step cases): a twentieth of the ties is reported on, each by its own share of 30-90 % of the reporters
    with counts 1-3 (3 % of the entries), another twentieth by one or two reporters, and about half of the reports are mirrored
    with counts 1-2 (levels >= 1); 5 % of the entries are non-zero in all.  This is NOT the recipe of the issue this file was
    written for, which spreads 4 % non-zero entries evenly: under the all-ones mask every tie then has two or three reports and
    more than 5 % of them end with a subnormal sum.  With the reports clustered, the ties with no or few reports stay below the
    range (all-zero rows that do carry reports: their deficits count), those with many are lifted back into it, and the mirror
    ties with their fewer reports are the ones that end near its lower edge.

    clustered=False (the whole-sweep cases): the issue's recipe, 4 % of the entries non-zero wherever they fall -- no tie has so
    many reports that a sweep from the strong priors overflows.

    large: layer 1 also gets counts of 100-255 -- 0.2 % of its entries one by one, and a dozen ties with 2 to 24 of them, from
    back-in-range to overflow under either mask.

    mask "partial": per tie n_t uniform in 0..M and exactly n_t random reporters; "ones": every reporter on every tie."""
    g = np.random.RandomState(1000 + seed)
    share = (g.rand(L, N, N) < 0.05) * g.uniform(0.3, 0.9, size=(L, N, N))
    share = np.where(g.rand(L, N, N) < 0.05, 0.02, share) if clustered else np.full((L, N, N), 0.04)
    X = ((g.rand(L, N, N, M) < share[..., None]) * g.randint(1, 4, size=(L, N, N, M))).astype(np.uint8)
    mir = (np.transpose(X, (0, 2, 1, 3)) > 0) & (g.rand(L, N, N, M) < 0.5)
    X = np.maximum(X, mir * g.randint(1, 3, size=(L, N, N, M))).astype(np.uint8)
    if large:
        big = g.rand(N, N, M) < 0.002
        X[1][big] = g.randint(100, 256, size=int(big.sum()))
        for n_big in (2, 3, 4, 5, 6, 8, 10, 12, 14, 16, 20, 24):
            i, j = g.randint(0, N, 2)
            ms = g.choice(M, n_big, replace=False)
            X[1, i, j, ms] = g.randint(100, 256, size=n_big)
    if mask == "ones":
        R = np.ones((L, N, N, M), np.uint8)
    else:   # n_t uniform in 0..M, exactly n_t random reporters
        n_t = g.randint(0, M + 1, size=(L, N, N))
        R = (np.argsort(g.rand(L, N, N, M), axis=-1) < n_t[..., None]).astype(np.uint8)
    return X, R


def make_prior_rows(K, seed, unnormalised=False):
    g = np.random.RandomState(2000 + seed)
    pr = g.rand(L, N, N, K) + 0.05
    pr /= pr.sum(-1, keepdims=True)
    if unnormalised:   # a user-supplied prior: a tenth of the rows short of 1, a few all zero
        short = g.rand(L, N, N) < 0.1
        pr[short] *= g.uniform(0.2, 0.9, size=(int(short.sum()), 1))
        pr[g.rand(L, N, N) < 0.005] = 0.0
    return pr


def substep_state(K, mask, seed, unnormalised=False):
    """(gamma_shp, gamma_rte, phi_shp, phi_rte, nu_shp, nu_rte, pr_rho): layer 0 with E[theta] in 0.5..1.5, layer 1 with
    E[theta] in 8..24 under a partial mask (T E[lambda] spans 0..3000 across the ties of a wave) and, under the all-ones mask
    where T is one number per layer, scaled so that T min_k E[lambda_k] = 752: ties without reports underflow by a few units.
    E[lambda_k] lies in 1..2; in layer 1 under the all-ones mask in 1..ONES_SPREAD, because T (max_k - min_k) E[lambda_k] is what
    the reports of a tie have to lift every category back by for the tie to be safe, and 64 counts of 1-3 lift by a few hundred."""
    g = np.random.RandomState(3000 + seed)
    gamma_rte = 0.5 + g.rand(L, M)
    ratio = np.stack([0.5 + g.rand(M), 8.0 + 16.0 * g.rand(M)])
    phi_rte = 1.0 + g.rand(L, K)
    spread = g.rand(L, K)
    if mask == "ones":
        spread[1] *= ONES_SPREAD - 1.0
    phi_shp = phi_rte * (1.0 + spread)
    if mask == "ones":
        ratio[1] *= 752.0 / (ratio[1].sum() * (phi_shp[1] / phi_rte[1]).min())
    gamma_shp = ratio * gamma_rte
    return (gamma_shp, gamma_rte, phi_shp, phi_rte, 0.7, 5.0, make_prior_rows(K, seed, unnormalised))


def build_case(K, mask, seed, kind="finite"):
    """kind: "finite" (counts 1-3 only), "overflow" (the large counts too), "prior" (finite, un-normalised prior rows) -- the
    sub-step cases, with the usual priors -- or "sweep": evenly spread small counts and the same state under the strong priors.
    Returns (X, R, priors, state)."""
    X, R = make_data(mask, seed, large=(kind == "overflow"), clustered=(kind != "sweep"))
    if kind == "sweep":
        return X, R, PRI_STRONG, substep_state(K, mask, seed)
    return X, R, PRI, substep_state(K, mask, seed, unnormalised=(kind == "prior"))


def coo_oracle(X, R, K, priors, state, mutuality=True):
    from oracle import cavi_coo
    sx = np.nonzero(X)
    return cavi_coo.CooRef((sx, X[sx]), None if R is None else np.nonzero(R), X.shape, K, mutuality, priors, *state)


def log_rho(X, R, state, mutuality=True, magnitude=False):
    """a_k = log(pr_k + eps) + U_k - T E[lambda_k] per tie, [L,N,N,K] in np.longdouble, from the state alone (reference
    model.py:795-806; the formulas of test_config5_layer_at_stated_size).  magnitude=True: also max_k (|log(pr_k + eps)| + sum of
    the |terms| of U_k + T E[lambda_k]) per tie in float64, above every partial sum that an evaluation of a_k in doubles meets."""
    ld = np.longdouble
    gs, gr, ps, pr_, ns, nr, pr = state
    K = ps.shape[1]
    lth, lla = (psi(gs) - np.log(gr)).astype(ld), (psi(ps) - np.log(pr_)).astype(ld)
    Eth, Ela = (gs / gr).astype(ld), (ps / pr_).astype(ld)
    gnu = ld(np.exp(psi(ns) - np.log(nr))) if mutuality else ld(0)
    T = np.einsum("lijm,lm->lij", R.astype(ld), Eth)
    a = np.log(pr + EPS).astype(ld) - T[..., None] * Ela[:, None, None, :]
    mag = np.abs(np.log(pr + EPS)).astype(ld) + T[..., None] * Ela[:, None, None, :]
    x = X.astype(ld)
    z2 = gnu * np.transpose(x, (0, 2, 1, 3))
    for k in range(K):
        z1 = np.broadcast_to((np.exp(lth) * np.exp(lla[:, k])[:, None])[:, None, None, :], x.shape)
        den = z1 + z2
        den = np.where(den == 0, ld(1), den)
        terms = x * (lth[:, None, None, :] + lla[:, k][:, None, None, None]) * (z1 / den)
        a[..., k] += terms.sum(axis=-1)
        mag[..., k] += np.abs(terms).sum(axis=-1)
    return (a, mag.max(axis=-1).astype(np.float64)) if magnitude else a


def bands(a):
    """a [.., K] -> (band [..] int, rho [.., K] float64, S [..] float64): what exp and the reference's conditional divide make of
    every tie.  A row whose sum is normal while single terms are subnormal counts as literal: those terms are below the absolute
    tolerance."""
    a64 = np.asarray(a, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        ex = np.exp(a64)
        S = ex.sum(axis=-1)
        rho = np.where((S > 0)[..., None], ex / np.where(S > 0, S, 1.0)[..., None], ex)
    band = np.where((np.abs(a64) >= 700).any(axis=-1), LITERAL, SAFE)
    band[(S > 0) & (S < DBL_MIN)] = SUBNORMAL
    band[S == 0] = ZERO
    band[~np.isfinite(S)] = NAN
    return band, rho, S


def edge_distances(a, rho):
    """How close any tie comes to a decision that last bits could flip: (|max_k a_k - ln 2^-1075|, |a_k - ln DBL_MAX|,
    |log10(|1 - sum rho| / 1e-14)| over rows with a finite non-zero residue), each the minimum over ties."""
    a64 = np.asarray(a, dtype=np.float64)
    d_zero = np.abs(a64.max(axis=-1) - LN_ZERO).min()
    d_max = np.abs(a64 - LN_MAX).min()
    with np.errstate(invalid="ignore", divide="ignore"):
        res = np.abs(1.0 - rho.sum(axis=-1))
        dec = np.abs(np.log10(res[np.isfinite(res) & (res > 0)] / IRREGULAR))
    return float(d_zero), float(d_max), float(dec.min()) if dec.size else np.inf


def subnormal_bound(rho_ref, S, K):
    """|rho_k - rho_ref_k| allowed on a row whose sum S is subnormal: each library's exp is within one unit u = 2^-1074 of the
    true value there, so two libraries differ by up to 2u per exponential; d(e_k / S) <= 2u / S + e_k K 2u / S^2."""
    return 2.0 * U_MIN * (1.0 + K * rho_ref) / S[..., None]


ARG_C = 8.0             # roundings of half an ulp that an evaluation of a_k is allowed to have gathered: sqrt(M) for M = 64
ARG_FROM = 2.0 ** 43    # in units u: the sum S beyond which 2u / S is less than one ulp of a_k (2^-52 * 745 = 1.7e-13)


def argument_bound(rho_ref, S, mag):
    """What a difference between two evaluations of the ARGUMENTS allows on a row with a subnormal sum S > 2^43 u, on top of
    `subnormal_bound` (which holds for two exp of the same argument): zero at or below 2^43 u.

    a_k is a sum of the M terms of T, the reports' terms of U_k and log pr_k, in doubles, each addition rounding by up to half an
    ulp of a partial sum, that is 2^-53 mag.  Two implementations add in another order (the device with fused multiply-adds,
    the C oracle over coordinate lists), so their a_k differ by a random walk of those roundings: about sqrt(M) / 2 half-ulps
    each, the worst case being M.  ARG_C = sqrt(M) = 8 half-ulps of EACH side are allowed, d = 2 ARG_C 2^-53 mag = ARG_C 2^-52 mag
    (1.4e-12 at mag = 800).  rho_k = e_k / S then moves by rho_k (d_k - sum_j rho_j d_j), at most 2 d rho_k.  Below 2^43 u the
    term is less than the exp bound and is left out: the committed cases meet the exp bound alone on every row."""
    d = ARG_C * 2.0 ** -52 * mag
    return np.where(S > ARG_FROM * U_MIN, 2.0 * d, 0.0)[..., None] * np.abs(rho_ref)


def assert_rho(rho, rho_ref, band, S, K, rtol=1e-9, atol=1e-13, what="", mag=None):
    """rho against the oracle's, band by band: rtol + atol on safe and literal rows, exact zeros, equal NaN masks, the
    subnormal-sum bound 2u (1 + K rho) / S on rows with a subnormal sum.  mag (log_rho's magnitude, per tie): `argument_bound` on
    top of that -- for randomly drawn cases; every committed case is held to the subnormal-sum bound alone."""
    assert np.array_equal(np.isnan(rho), np.isnan(rho_ref)), f"{what}: NaN masks differ"
    z = band == ZERO
    assert not rho[z].any(), f"{what}: {int(rho[z].any(axis=-1).sum())} zero rows are not exactly zero"
    n = band == NAN
    fin = ~np.isnan(rho_ref[n])
    assert np.array_equal(rho[n][fin], rho_ref[n][fin]), f"{what}: finite entries of NaN rows"
    r = (band == SAFE) | (band == LITERAL)
    np.testing.assert_allclose(rho[r], rho_ref[r], rtol=rtol, atol=atol, err_msg=f"{what}: safe and literal rows")
    s = band == SUBNORMAL
    if s.any():
        err, bound = np.abs(rho[s] - rho_ref[s]), subnormal_bound(rho_ref[s], S[s], K)
        if mag is not None:
            bound = bound + argument_bound(rho_ref[s], S[s], mag[s])
        worst = (err / bound).max()
        assert worst <= 1.0, f"{what}: subnormal-sum rows off by {worst:.3g} x the bound 2u(1 + K rho)/S" + (" + arguments" if mag is not None else "")


def without_deficits(rho):
    """rho with category 0 rebuilt as if every row summed to 1: what an engine that dropped the deficits D would use."""
    out = rho.copy()
    out[..., 0] = 1.0 - rho[..., 1:].sum(axis=-1)
    return out
