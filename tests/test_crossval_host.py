"""CPU: the host side of the held-out log-likelihood and of k-fold cross-validation (vimure_amd/crossval.py).  The NumPy
restatement of vmr_heldout_loglik against a brute-force mixture of scipy.stats.poisson.logpmf, its zero-rate and -inf rules, the
fold assignment, and the dense and coordinate forms of the training mask, the counts and the mirror counts."""
import math

import numpy as np
import pytest

from vimure_amd.crossval import (assign_folds, counts_at, heldout_loglik_np, in_mask, mirror_counts, support, train_mask)
from vimure_amd.tensor import SparseTensor


def _tiny(seed=0, L=2, N=5, M=3, K=3, n=40):
    g = np.random.RandomState(seed)
    rho = g.rand(L, N, N, K)
    rho /= rho.sum(-1, keepdims=True)
    theta, lam = g.gamma(2.0, 0.5, (L, M)) + 0.05, g.gamma(2.0, 1.0, (L, K)) + 0.05
    subs = (np.sort(g.randint(0, L, n)), g.randint(0, N, n), g.randint(0, N, n), g.randint(0, M, n))
    x, xt = g.randint(0, 6, n), g.randint(0, 4, n)
    return rho, subs, x, xt, theta, lam


def test_restatement_matches_a_brute_force_poisson_mixture():
    from scipy.stats import poisson
    rho, subs, x, xt, theta, lam = _tiny()
    eta = 0.3
    logp, mean, sums, counts = heldout_loglik_np(rho, subs, x, xt, theta, lam, eta)
    for e, (l, i, j, m) in enumerate(zip(*subs)):
        mu = theta[l, m] * lam[l] + eta * xt[e]
        want = math.log(float(np.sum(rho[l, i, j] * np.exp(poisson.logpmf(x[e], mu)))))
        assert abs(logp[e] - want) <= 1e-12 * (1.0 + abs(want)), (e, logp[e], want)
        assert abs(mean[e] - float(np.dot(rho[l, i, j], mu))) <= 1e-14 * mean[e]
    for l in range(2):
        w = subs[0] == l
        assert counts[l].tolist() == [w.sum(), (w & (x > 0)).sum(), 0, w.sum()]           # R None: every entry is in the mask
        assert np.allclose(sums[l], [logp[w].sum(), ((x[w] - mean[w]) ** 2).sum(), x[w].sum(), mean[w].sum()], rtol=1e-13)
    # without mirrored counts the rate is theta lambda alone
    lp0, mn0, _, _ = heldout_loglik_np(rho, subs, x, None, theta, lam, eta)
    lp1, mn1, _, _ = heldout_loglik_np(rho, subs, x, np.zeros_like(x), theta, lam, 0.0)
    assert np.array_equal(lp0, lp1) and np.array_equal(mn0, mn1)


def test_a_one_hot_row_gives_exactly_one_poisson_logpmf():
    from scipy.special import gammaln
    from scipy.stats import poisson
    rho, subs, x, xt, theta, lam = _tiny(1)
    for k in range(3):
        rho[:] = 0.0
        rho[..., k] = 1.0
        logp, mean, _, _ = heldout_loglik_np(rho, subs, x, xt, theta, lam, 0.25)
        mu = theta[subs[0], subs[3]] * lam[subs[0], k] + 0.25 * xt
        assert np.array_equal(mean, mu)
        want = x * np.log(mu) - mu - gammaln(x + 1.0)
        assert np.array_equal(logp, want)                                                    # log(1) = 0 and exp(0) = 1: nothing is added
        assert np.allclose(logp, poisson.logpmf(x, mu), rtol=1e-13, atol=1e-13)


def test_zero_rates_and_the_minus_infinity_rule():
    L, N, M, K = 1, 3, 2, 3
    rho = np.zeros((L, N, N, K))
    rho[0, 0, 1] = [0.5, 0.0, 0.5]          # a zero in the middle
    rho[0, 1, 2] = [0.25, 0.25, 0.5]
    rho[0, 2, 2] = [1.0, 0.0, 0.0]
    theta = np.array([[1.5, 0.0]])           # reporter 1 never reports: every rate 0 without mutuality
    lam = np.array([[0.0, 1.0, 2.0]])        # category 0: rate 0
    subs = (np.zeros(6, int), np.array([0, 0, 1, 2, 2, 1]), np.array([1, 1, 2, 2, 2, 2]), np.array([0, 0, 0, 0, 0, 1]))
    x = np.array([0, 2, 0, 0, 3, 1])
    logp, mean, sums, counts = heldout_loglik_np(rho, subs, x, None, theta, lam, 0.0)
    # entry 0: x = 0; category 0 (rate 0) contributes log 0.5, category 1 (rho 0) nothing, category 2 log 0.5 - 3
    assert np.isclose(logp[0], math.log(0.5 + 0.5 * math.exp(-3.0)), rtol=1e-15)
    # entry 1: x = 2; category 0 has rate 0 against x > 0: nothing; only category 2 is left
    assert np.isclose(logp[1], math.log(0.5) + 2 * math.log(3.0) - 3.0 - math.lgamma(3.0), rtol=1e-15)
    assert np.isclose(logp[2], math.log(0.25 + 0.25 * math.exp(-1.5) + 0.5 * math.exp(-3.0)), rtol=1e-15)
    assert logp[3] == 0.0                                                # one-hot on the zero-rate category, x = 0: log 1
    assert logp[4] == -np.inf and logp[5] == -np.inf                     # ... x > 0: no category contributes; theta = 0 likewise
    assert mean[3] == 0.0 and mean[5] == 0.0
    assert counts[0].tolist() == [6, 3, 2, 6]
    assert np.isclose(sums[0, 0], logp[:4].sum(), rtol=1e-15)            # the -inf entries are left out of the sum ...
    assert np.isclose(sums[0, 1], ((x - mean) ** 2).sum(), rtol=1e-15)   # ... and of nothing else
    # with a mirrored count the rate is eta xt > 0 and the entry has a density again
    lp, _, _, c = heldout_loglik_np(rho, subs, x, np.full(6, 2), theta, lam, 0.5)
    assert np.isfinite(lp).all() and c[0, 2] == 0
    assert np.isclose(lp[5], math.log(1.0) - 1.0, rtol=1e-15)            # Poisson(1; 1) on every category, rho sums to 1


def test_the_in_mask_count_takes_R_in_either_form():
    rho, subs, x, xt, theta, lam = _tiny(2)
    R = (np.random.RandomState(5).rand(2, 5, 5, 3) < 0.5).astype(np.uint8)
    _, _, _, c_dense = heldout_loglik_np(rho, subs, x, xt, theta, lam, 0.1, R=R)
    _, _, _, c_coo = heldout_loglik_np(rho, subs, x, xt, theta, lam, 0.1, R=SparseTensor.fromarray(R))
    assert np.array_equal(c_dense, c_coo)
    assert c_dense[:, 3].sum() == int(R[subs].sum()) and 0 < c_dense[:, 3].sum() < len(x)
    assert np.array_equal(in_mask(R, subs), R[subs] != 0)


def _self_reporter(N=6, L=2, seed=3):
    from vimure_amd.synthetic import self_reporter_mask
    g = np.random.RandomState(seed)
    R = np.asarray(self_reporter_mask(L, N, N)).astype(np.uint8)
    X = ((g.rand(L, N, N, N) < 0.4) * g.randint(1, 4, (L, N, N, N))).astype(np.uint8) * R
    return X, R


@pytest.mark.parametrize("unit", ["pair", "entry"])
def test_assign_folds_partitions_the_support(unit):
    X, R = _self_reporter()
    sup = support(X, R)
    assert np.array_equal(np.stack(sup), np.stack(np.nonzero(R)))                           # lexicographic
    f = assign_folds(sup, 4, seed=7, unit=unit, shape=X.shape)
    assert f.shape == sup[0].shape and set(f.tolist()) == {0, 1, 2, 3}                      # a partition, no fold empty
    assert np.array_equal(f, assign_folds(sup, 4, seed=7, unit=unit, shape=X.shape))        # the same seed, the same folds
    assert not np.array_equal(f, assign_folds(sup, 4, seed=8, unit=unit, shape=X.shape))
    l, i, j, m = sup
    fold_of = {(a, b, c, d): q for a, b, c, d, q in zip(l.tolist(), i.tolist(), j.tolist(), m.tolist(), f.tolist())}
    together = [fold_of[(a, c, b, d)] == q for (a, b, c, d), q in fold_of.items() if (a, c, b, d) in fold_of]
    assert len(together) > 0
    if unit == "pair":
        assert all(together)                                                                # both directions of a pair together
    else:
        assert not all(together)
    if unit == "entry":                                                                     # dealt round-robin
        assert np.bincount(f).max() - np.bincount(f).min() <= 1
    with pytest.raises(ValueError):
        assign_folds(tuple(s[:3] for s in sup), 4, seed=0, unit="entry")
    with pytest.raises(ValueError):
        assign_folds(sup, 4, unit="tie")


def test_support_without_R_and_its_limit():
    X = np.zeros((2, 3, 3, 2), np.uint8)
    sup = support(X, None)
    assert len(sup[0]) == 36 and np.array_equal(np.stack(sup), np.stack(np.nonzero(np.ones(X.shape))))
    with pytest.raises(ValueError, match="folds"):
        support(X, None, max_support=35)
    big = SparseTensor((np.zeros(1, int),) * 4, np.ones(1), shape=(4, 3000, 3000, 3000))
    with pytest.raises(ValueError, match="explicit `folds` sample"):
        support(big, None)                                                                   # 1.08e11 elements: refused before anything is built
    R = (np.random.RandomState(0).rand(*X.shape) < 0.5).astype(np.uint8)
    with pytest.raises(ValueError, match="max_support"):
        support(X, R, max_support=int(R.sum()) - 1)
    g = np.random.RandomState(1)
    Rc = SparseTensor.fromarray(R)
    p = g.permutation(len(Rc.vals))
    Rc = SparseTensor(tuple(s[p] for s in Rc.subs), Rc.vals[p], shape=R.shape)              # a container in any order
    assert np.array_equal(np.stack(support(X, Rc)), np.stack(np.nonzero(R)))


def test_train_mask_counts_and_mirror_counts_agree_between_the_forms():
    X, R = _self_reporter(N=7)
    Xc, Rc = SparseTensor.fromarray(X), SparseTensor.fromarray(R)
    sup = support(X, R)
    f = assign_folds(sup, 3, seed=1, shape=X.shape)
    out = tuple(s[f == 1] for s in sup)
    R_before = R.copy()
    Rd = train_mask(X, R, out)
    assert Rd.dtype == np.uint8 and Rd.shape == R.shape and not Rd[out].any() and Rd.sum() == R.sum() - len(out[0])
    assert np.array_equal(R, R_before)                                                       # (the caller's mask is not written)
    Rs = train_mask(Xc, Rc, out)
    assert hasattr(Rs, "subs") and np.array_equal(Rs.toarray() != 0, Rd != 0)
    assert np.array_equal(train_mask(X, Rc, out), Rd)
    # without R: all ones minus the held-out entries
    R1 = train_mask(X, None, out)
    assert R1.sum() == X.size - len(out[0]) and not R1[out].any()
    assert np.array_equal(train_mask(Xc, None, out).toarray() != 0, R1 != 0)
    # counts and mirror counts: the full data, whatever the mask
    assert np.array_equal(counts_at(X, sup), X[sup]) and np.array_equal(counts_at(Xc, sup), X[sup])
    want = X[sup[0], sup[2], sup[1], sup[3]]
    assert np.array_equal(mirror_counts(X, sup), want) and np.array_equal(mirror_counts(Xc, sup), want)
    assert want.any() and (want == 0).any()
    empty = SparseTensor(tuple(np.zeros(0, int) for _ in range(4)), np.zeros(0), shape=X.shape)
    assert not mirror_counts(empty, sup).any()


def test_the_drivers_own_keywords_are_refused_before_anything_runs():
    from vimure_amd.crossval import compare_models, cross_validate
    X, R = _self_reporter()
    for kw in (dict(keep_engine=False), dict(engine=None)):
        with pytest.raises(ValueError, match="set by the driver"):
            cross_validate(X, R, n_folds=2, **kw)
    for cand in (dict(seed=3), dict(R=None), dict(keep_engine=True), dict(K=2, folds=None)):
        with pytest.raises(ValueError, match="candidate 1"):
            compare_models(X, R, [dict(K=2), cand], n_folds=2)
    with pytest.raises(ValueError, match="estimate"):
        cross_validate(X, R, estimate="mode")
