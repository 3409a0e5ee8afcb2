"""Shared by tests/test_hip_heldout.py and tests/test_hip_crossval.py: the bounds that hold vmr_heldout_loglik to its NumPy
restatement (`crossval.heldout_loglik_np`).

  mean   |got - want| <= (2 K + 2) 2^-52 mean                      (derived: K products, K adds)
  logp   |got - want| <= C_LOGP 2^-52 T, T = max over the contributing categories of |x log mu_k| + mu_k + |log rho_k|, plus
         lgamma(x + 1) + 1: the size of the terms that cancel
  sums   n 2^-52 sum |v| plus the per-entry bounds, whatever the tree

C_LOGP is four times the worst |got - want| / (2^-52 T) measured on an MI355X over the cases of tests/test_hip_heldout.py and
tests/test_hip_crossval.py against the restatement, whose own error is a few ulp of T: worst 1.167 (K = 3, the masked M = 70 case),
so 4.67 -- and never above 64.  A dropped or wrong term is an error of order T, 2^52 times the bound: the constant hides nothing."""
import math

import numpy as np

U = 2.0 ** -52
C_LOGP = 4.67   # 4 x the measured worst 1.167


def term_size(rho, subs, x, xt, theta, lam, eta):
    """T [n] of the entries (see the module docstring)."""
    l, i, j, m = subs
    x = np.asarray(x, dtype=np.int64)
    xt = np.zeros_like(x) if xt is None else np.asarray(xt, dtype=np.int64)
    r = rho[l, i, j]
    mu = theta[l, m][:, None] * lam[l] + (eta * xt)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.abs(x[:, None] * np.log(mu)) + mu + np.abs(np.log(r))
    t = np.where((r > 0) & ~((mu == 0) & (x[:, None] > 0)) & np.isfinite(t), t, 0.0)
    return t.max(axis=1) + np.array([math.lgamma(v + 1.0) for v in x]) + 1.0


def compare_entries(got, want, T, K, what=""):
    """got: the engine's dict; want: the restatement's (logp, mean, sums, counts).  Counts exact; logp and mean within their
    bounds.  Prints every figure before it asserts."""
    logp, mean, _, counts = want
    assert np.array_equal(got["counts"], counts), (what, got["counts"], counts)
    if got["logp"] is None:
        return
    glp, gmn = np.asarray(got["logp"]), np.asarray(got["mean"])
    inf = logp == -np.inf
    assert np.array_equal(glp == -np.inf, inf) and not np.isnan(glp).any() and not np.isnan(logp).any()
    e_mean = np.abs(gmn - mean)
    ratio = np.abs(glp[~inf] - logp[~inf]) / (U * T[~inf])
    print(f"{what}: logp worst ratio |got - want| / (2^-52 T) = {ratio.max(initial=0.0):.4f}; mean worst / (2^-52 mean) = "
          f"{(e_mean / (U * np.maximum(mean, 1e-300))).max(initial=0.0):.3f} (bound {2 * K + 2})")
    assert (e_mean <= (2 * K + 2) * U * mean).all(), float((e_mean - (2 * K + 2) * U * mean).max())
    assert (ratio <= C_LOGP).all(), float(ratio.max())


def compare_sums(got_sums, want, subs, x, T, K, what=""):
    """The layer sums [L, 4] within n 2^-52 sum |v| (any summation order of n terms) plus the entries' own bounds."""
    logp, mean, sums, _ = want
    x = np.asarray(x, dtype=np.float64)
    for l in range(sums.shape[0]):
        w = subs[0] == l
        n = int(w.sum())
        fin = w & np.isfinite(logp)
        b_lp, b_mn = C_LOGP * U * T, (2 * K + 2) * U * mean
        d = np.abs(x - mean)
        bound = np.array([n * U * np.abs(logp[fin]).sum() + b_lp[fin].sum(),
                          n * U * (d[w] ** 2).sum() + (2.0 * d[w] * b_mn[w] + b_mn[w] ** 2 + 2 * U * d[w] ** 2).sum(),
                          n * U * x[w].sum(), n * U * mean[w].sum() + b_mn[w].sum()])
        err = np.abs(got_sums[l] - sums[l])
        print(f"{what} layer {l}: n {n}, |sums - want| {err}, bound {bound}")
        assert (err <= bound).all(), (what, l, err, bound)
