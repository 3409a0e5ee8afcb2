"""Host: the conditions that keep tests/test_hip_exp_range.py honest, shown on the reference side alone (CPU oracles, no GPU).

For every committed case of tests/exp_range_util.py: the util's a_k and bands reproduce the oracle's rho with its zero and NaN
patterns; layer 1 populates every band while layer 0 stays safe; no tie sits where last bits decide whether a row is zero, NaN or
irregular, so no tie is excluded from any comparison; and dropping the deficits of irregular rows would move gamma, phi and nu by
more than 1000 times the tolerance the GPU tests apply."""
import numpy as np
import pytest

from oracle import vimure_oracle as vo
from tests import exp_range_util as u

GPU_RTOL = 1e-9   # tests/test_hip_exp_range.py on gamma, phi, nu


def _case(K, mask, seed, kind):
    X, R, pri, st = u.build_case(K, mask, seed, kind)
    a = u.log_rho(X, R, st)
    band, rho, S = u.bands(a)
    c = u.coo_oracle(X, R, K, pri, st)
    c.update_rho()
    return X, R, pri, st, a, band, rho, S, c


def _counts(band):
    return [[int((band[l] == b).sum()) for b in range(5)] for l in range(u.L)]


@pytest.mark.parametrize("kind", ["finite", "overflow", "prior"])
@pytest.mark.parametrize("K,mask,seed", u.CASES)
def test_bands_match_the_oracle_and_are_populated(K, mask, seed, kind):
    X, R, pri, st, a, band, rho, S, c = _case(K, mask, seed, kind)
    cnt = _counts(band)
    print(f"bands K={K} {mask} seed={seed} {kind}: " + "; ".join(
        f"layer {l}: " + ", ".join(f"{n} {cnt[l][b]}" for b, n in enumerate(u.BAND_NAMES)) for l in range(u.L)))
    assert X.shape == (u.L, u.N, u.N, u.M) and X.dtype == np.uint8
    # the util's rho is the oracle's: 1e-12 relative; the oracle sums a_k of size 3000 in doubles, which moves the tiniest
    # entries of a row by more than that, all of them below the absolute 1e-20
    u.assert_rho(rho, c.rho, band, S, K, rtol=1e-12, atol=1e-20, what="util against oracle")
    assert np.array_equal(rho == 0, c.rho == 0)
    # populations
    ties = u.N * u.N
    assert cnt[0][u.SAFE] == ties, "layer 0 is all safe"
    n_safe, n_lit, n_sub, n_zero, n_nan = cnt[1]
    assert n_zero >= 0.10 * ties and n_sub >= 5 and n_lit >= 1 and n_safe >= 1
    assert n_sub <= 0.05 * ties
    assert (n_nan >= 1) if kind == "overflow" else (n_nan == 0)
    # a sum that overflows without a single overflowing term would be a zero row with a positive sum: none
    assert not ((band == u.NAN) & ~np.isnan(rho).any(axis=-1)).any()
    # nothing within reach of last bits: no tie is excluded from any comparison
    d_zero, d_max, dec = u.edge_distances(a, rho)
    assert d_zero > 1e-6 and d_max > 1e-6 and dec > 1.0, (d_zero, d_max, dec)
    # the same for the oracle's own rows: irregular or not is decided the same way on both sides
    with np.errstate(invalid="ignore"):
        res = np.abs(1.0 - c.rho.sum(axis=-1))
    res = res[np.isfinite(res)]
    assert not ((res > u.IRREGULAR / 10) & (res < u.IRREGULAR * 10)).any()
    if kind != "prior":   # every regular row of layer 1 sums to 1
        fin = np.isfinite(c.rho.sum(axis=-1)) & (band != u.ZERO) & (band != u.SUBNORMAL)
        assert np.abs(1.0 - c.rho.sum(axis=-1)[fin]).max() < 5e-16 * 2


@pytest.mark.parametrize("K,mask,seed", u.CASES)
def test_dropped_deficits_would_show(K, mask, seed):
    """gamma_shp, phi_shp and nu_shp of the NumPy oracle with H_0 = C - sum_{k>0} H_k (the deficits ignored) against the true
    ones: more than 1000 x the GPU tests' tolerance apart."""
    X, R, pri, st, a, band, rho, S, c = _case(K, mask, seed, "finite")
    pb = vo.Problem(X, R, K, True, vo.make_priors(u.L, u.M, K, theta_prior=pri[0:2], lambda_prior=pri[2:4], eta_prior=pri[4:6]))
    out = []
    for r in (c.rho, u.without_deficits(c.rho)):
        s = vo.State(*(np.array(v, dtype=float) for v in st[:4]), st[4], st[5], r.copy(), st[6], np.log(st[6] + u.EPS))
        vo.update_nu(pb, s)
        vo.update_gamma(pb, s)
        vo.update_phi(pb, s)
        out.append((s.gamma_shp, s.phi_shp, np.float64(s.nu_shp)))
    for name, true, wrong in zip(("gamma_shp", "phi_shp", "nu_shp"), *out):
        rel = np.max(np.abs(wrong - true) / np.abs(true))
        print(f"K={K} {mask}: {name} moves by {rel:.3g} relative without the deficits")
        assert rel > 1000 * GPU_RTOL, (name, rel)
    # and the oracle pair agrees on the true values (the C oracle is the GPU tests' reference)
    c.update_nu()
    c.update_gamma()
    c.update_phi()
    np.testing.assert_allclose(c.gamma_shp, out[0][0], rtol=1e-12)
    np.testing.assert_allclose(c.phi_shp, out[0][1], rtol=1e-12)
    np.testing.assert_allclose(c.nu_shp, out[0][2], rtol=1e-12)


@pytest.mark.parametrize("K,mask,seed", u.SWEEP_CASES)
def test_strong_priors_keep_zero_rows_over_three_sweeps(K, mask, seed):
    """The whole-sweep recipe: with the strong priors gamma and phi stay where the first sweep put them, so a share of rows is
    still all zero after sweeps 1, 2 and 3, the state and the ELBO finite throughout; with the usual priors none is left."""
    X, R, pri, st = u.build_case(K, mask, seed, "sweep")
    c = u.coo_oracle(X, R, K, pri, st)
    shares = []
    for it in range(3):
        c.cavi_step()
        e = c.elbo()
        assert np.isfinite(e) and np.isfinite(c.rho).all() and np.isfinite(c.gamma_shp).all() and np.isfinite(c.phi_rte).all()
        shares.append(float((c.rho == 0).all(axis=-1).mean()))
    print(f"K={K} {mask}: all-zero rows after sweeps 1, 2, 3: " + ", ".join(f"{100 * s:.0f} %" for s in shares))
    assert min(shares) >= 0.10, shares


@pytest.mark.parametrize("K,mask,seed", u.SWEEP_CASES)
def test_third_sweep_update_by_update_is_the_sweep(K, mask, seed):
    """The GPU test classifies the ties of the third sweep's rho update from the oracle's state after that sweep's gamma and phi:
    the four updates one by one are the sweep, the bands reproduce its rho, and no tie lies where the 1e-9 the two
    states may differ by could move it across an edge (a tie near an edge has |a_k| of 700-odd: 1e-6; the nearest is 1e-3 away)."""
    X, R, pri, st = u.build_case(K, mask, seed, "sweep")
    whole, parts = u.coo_oracle(X, R, K, pri, st), u.coo_oracle(X, R, K, pri, st)
    for _ in range(3):
        whole.cavi_step()
    parts.cavi_step()
    parts.cavi_step()
    parts.update_gamma()
    parts.update_phi()
    mid = (parts.gamma_shp.copy(), parts.gamma_rte.copy(), parts.phi_shp.copy(), parts.phi_rte.copy(), parts.nu_shp, st[5], st[6])
    a = u.log_rho(X, R, mid)
    band, rho, S = u.bands(a)
    parts.update_rho()
    parts.update_nu()
    # (two runs of the oracle differ in last bits: its threads add their partial sums in the order they finish)
    for n in ("gamma_shp", "gamma_rte", "phi_shp", "phi_rte", "nu_shp"):
        np.testing.assert_allclose(getattr(parts, n), getattr(whole, n), rtol=1e-12, err_msg=n)
    assert abs(parts.elbo() - whole.elbo()) <= 1e-12 * abs(whole.elbo())
    assert np.array_equal(parts.rho == 0, whole.rho == 0)
    u.assert_rho(rho, whole.rho, band, S, K, rtol=1e-12, atol=1e-20, what="util against oracle, third sweep")
    d_zero, d_max, dec = u.edge_distances(a, rho)
    print(f"K={K} {mask} third sweep: " + ", ".join(f"{n} {int((band == b).sum())}" for b, n in enumerate(u.BAND_NAMES)) + f"; edge {d_zero:.3g}")
    assert d_zero > 1e-3 and d_max > 1e-3 and dec > 1.0
    assert (band == u.NAN).sum() == 0 and (band == u.ZERO).mean() > 0.9 and ((band == u.SAFE) | (band == u.LITERAL)).sum() >= 50


@pytest.mark.parametrize("K,seed,scale", [(9, 50566, 1.04), (2, 11, 0.96), (5, 12, 0.97), (16, 13, 0.955)])
def test_argument_term_covers_the_oracle_pair(K, seed, scale):
    """Randomly drawn all-ones cases (tools/fuzz_parity.py scales layer 1 by 0.95..1.1) put rows at sums S > 2^43 u, where
    2u / S is less than an ulp of a_k and two evaluations of the arguments in another order are further apart than two exp of
    one argument: there the fuzz family adds `argument_bound`.  Shown here without a device: the util (a_k in extended precision,
    rounded once) against the C oracle (a_k summed in doubles) stays within the composite bound on such rows, and the share of
    the exp bound alone that the pair uses is printed."""
    X, R, pri, st = u.build_case(K, "ones", seed, "finite")
    st = (st[0] * np.array([1.0, scale])[:, None],) + tuple(st[1:])
    a, mag = u.log_rho(X, R, st, magnitude=True)
    band, rho, S = u.bands(a)
    c = u.coo_oracle(X, R, K, pri, st)
    c.update_rho()
    high = (band == u.SUBNORMAL) & (S > u.ARG_FROM * u.U_MIN)
    assert high.sum() >= 5, int(high.sum())
    err = np.abs(rho[high] - c.rho[high])
    exp_b, arg_b = u.subnormal_bound(c.rho[high], S[high], K), u.argument_bound(c.rho[high], S[high], mag[high])
    print(f"K={K} seed={seed}: {int(high.sum())} rows beyond 2^43 u, pair at {(err / exp_b).max():.3g} of the exp bound, "
          f"{(err / (exp_b + arg_b)).max():.3g} of the composite one, argument term {(arg_b / np.maximum(c.rho[high], 1e-300)).max():.3g} rho")
    assert (err <= exp_b + arg_b).all()
    assert (arg_b <= 1e-11 * np.abs(c.rho[high])).all()   # the term is a few ulp of the argument, nowhere near the general 1e-9


@pytest.mark.parametrize("kind", ["finite", "overflow"])
def test_bands_without_mutuality(kind):
    X, R, pri, st = u.build_case(3, "partial", 1, kind)
    st = st[:4] + (1e-6, 1.0) + st[6:]
    a = u.log_rho(X, R, st, mutuality=False)
    band, rho, S = u.bands(a)
    c = u.coo_oracle(X, R, 3, pri, st, mutuality=False)
    c.update_rho()
    u.assert_rho(rho, c.rho, band, S, 3, rtol=1e-12, atol=1e-20, what="util against oracle, mutuality off")
    assert np.array_equal(rho == 0, c.rho == 0)
    n = [int((band[1] == b).sum()) for b in range(5)]
    assert n[u.ZERO] >= 230 and n[u.SUBNORMAL] >= 5 and n[u.SAFE] >= 1 and n[u.LITERAL] >= 1 and (n[u.NAN] >= 1) == (kind == "overflow")
    d_zero, d_max, dec = u.edge_distances(a, rho)
    assert d_zero > 1e-6 and d_max > 1e-6 and dec > 1.0
