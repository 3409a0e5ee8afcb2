"""Posterior predictive checks: the host side of `VimureModel.posterior_predictive_check`.

`draw_parameters` draws the parameters of every replicate from the Gamma posteriors of a fit (the draw of
`PosteriorSyntheticNetwork.build_X`, reference synthetic.py:964-1177); the device draws the replicates over the support of R
and reduces them (`CaviEngine.ppc_replicates`, `CaviEngine.ppc_observed`); `PredictiveCheck` holds the integers that come back
and turns them into posterior predictive p-values.
"""
import numpy as np

from ._lib import PPC_STAT_NAMES
from .netstats import _ratio

MAX_ETA_REDRAWS = 1000


def draw_parameters(gamma_shp, gamma_rte, phi_shp, phi_rte, nu_shp, nu_rte, n_rep, seed, params="draw"):
    """(theta [n_rep, L, M], lam [n_rep, L, K], eta [n_rep], redraws) of n_rep replicates.
    params="draw": from Gamma(shape, 1 / rate) with `np.random.RandomState(seed)`, per replicate in the order theta, lambda, eta
    (`build_X`'s order).  The generator needs eta in [0, 1): a draw >= 1 is drawn again from the same generator, at most
    MAX_ETA_REDRAWS times per replicate (then ValueError); `redraws` counts them.  params="mean": the posterior means shape / rate
    for every replicate (a mean eta >= 1 is a ValueError).  A zero rate raises `build_X`'s ValueError."""
    gamma_shp, gamma_rte = np.asarray(gamma_shp, dtype=np.float64), np.asarray(gamma_rte, dtype=np.float64)
    phi_shp, phi_rte = np.asarray(phi_shp, dtype=np.float64), np.asarray(phi_rte, dtype=np.float64)
    for nm, arr in (("theta_rte", gamma_rte), ("lambda_rte", phi_rte), ("mutuality_rte", nu_rte)):
        if np.any(np.asarray(arr) == 0):
            raise ValueError(f"{nm} has some zero entries!")
    n_rep = int(n_rep)
    if n_rep < 1:
        raise ValueError("n_rep must be positive")
    (L, M), K = gamma_shp.shape, phi_shp.shape[1]
    if params == "mean":
        eta = float(nu_shp) / float(nu_rte)
        if not 0.0 <= eta < 1.0:
            raise ValueError("The mutuality parameter has to be in [0, 1)!")
        return (np.broadcast_to(gamma_shp / gamma_rte, (n_rep, L, M)).copy(), np.broadcast_to(phi_shp / phi_rte, (n_rep, L, K)).copy(),
                np.full(n_rep, eta), 0)
    if params != "draw":
        raise ValueError("params must be 'draw' or 'mean'")
    prng = np.random.RandomState(seed)
    theta, lam, eta = np.empty((n_rep, L, M)), np.empty((n_rep, L, K)), np.empty(n_rep)
    redraws = 0
    for r in range(n_rep):
        theta[r] = prng.gamma(shape=gamma_shp, scale=1.0 / gamma_rte, size=(L, M))
        lam[r] = prng.gamma(shape=phi_shp, scale=1.0 / phi_rte, size=(L, K))
        e = prng.gamma(shape=nu_shp, scale=1.0 / nu_rte, size=1)[0]
        tries = 0
        while not e < 1.0:
            if tries == MAX_ETA_REDRAWS:
                raise ValueError("the posterior of the mutuality puts (almost) all its mass on eta >= 1: %d redraws of replicate %d "
                                 "gave none in [0, 1)" % (MAX_ETA_REDRAWS, r))
            e = prng.gamma(shape=nu_shp, scale=1.0 / nu_rte, size=1)[0]
            tries += 1
        redraws += tries
        eta[r] = e
    return theta, lam, eta, redraws


def _p_value(obs, rep):
    """(#{rep > obs} + #{rep = obs} / 2) / n_rep along the first axis of rep."""
    rep = np.asarray(rep)
    obs = np.asarray(obs)[None]
    return ((rep > obs).sum(axis=0) + 0.5 * (rep == obs).sum(axis=0)) / float(rep.shape[0])


class PredictiveCheck:
    """observed int64 [L, 6] and replicated int64 [n_rep, L, 6]: per layer, over the support S of R (x: the count at a support
    element) -- `STATISTICS`, in this order:
      n_pos #{x > 0}, total sum x, sumsq sum x^2, mutual #{x_ijm > 0 and x_jim > 0, both in S, i != j} (ordered),
      ties_reported #{(i,j): some m with x > 0}, ties_agreed #{(i,j): at least two m with x > 0}.
    observed_by_reporter [L, M, 2], replicated_by_reporter [n_rep, L, M, 2]: (n_pos, total) of every reporter, or None.
    support [L]: |S| per layer (for `dispersion`), or None.  seed_y, seed_x, n_trials: replicate r drew its Y with seed_y + r
    and its reports with seed_x + r.  theta, lam, eta: the parameters of the replicates; eta_redraws: eta draws >= 1 that
    were drawn again."""
    STATISTICS = tuple(PPC_STAT_NAMES)

    def __init__(self, observed, replicated, observed_by_reporter=None, replicated_by_reporter=None, support=None, seed_y=None,
                 seed_x=None, n_trials=1, theta=None, lam=None, eta=None, eta_redraws=0, params=None):
        self.observed = np.asarray(observed, dtype=np.int64)
        self.replicated = np.asarray(replicated, dtype=np.int64)
        ns = len(self.STATISTICS)
        if self.observed.ndim != 2 or self.observed.shape[1] != ns or self.replicated.ndim != 3 or self.replicated.shape[1:] != self.observed.shape:
            raise ValueError(f"observed [L, {ns}] and replicated [n_rep, L, {ns}] expected")
        self.n_rep, self.L = self.replicated.shape[0], self.observed.shape[0]
        self.observed_by_reporter = None if observed_by_reporter is None else np.asarray(observed_by_reporter, dtype=np.int64)
        self.replicated_by_reporter = None if replicated_by_reporter is None else np.asarray(replicated_by_reporter, dtype=np.int64)
        self.support = None if support is None else np.asarray(support, dtype=np.int64).reshape(self.L)
        self.seed_y, self.seed_x, self.n_trials = seed_y, seed_x, int(n_trials)
        self.theta, self.lam, self.eta, self.eta_redraws, self.params = theta, lam, eta, int(eta_redraws), params

    def statistic(self, name):
        """(observed [L], replicated [n_rep, L]) of a raw statistic."""
        k = self.STATISTICS.index(name)
        return self.observed[:, k], self.replicated[:, :, k]

    def p_values(self):
        """Posterior predictive p-values [L, 6]: (#{rep > obs} + #{rep = obs} / 2) / n_rep per layer and statistic."""
        return _p_value(self.observed, self.replicated)

    def p_values_by_reporter(self):
        """The same for the per-reporter (n_pos, total): [L, M, 2], or None."""
        if self.observed_by_reporter is None:
            return None
        return _p_value(self.observed_by_reporter, self.replicated_by_reporter)

    # -- derived ratios: (observed [L], replicated [n_rep, L]), NaN where undefined
    @property
    def report_reciprocity(self):
        """mutual / n_pos: the share of positive reports whose mirror report (same reporter) is positive too."""
        return _ratio(self.observed[:, 3], self.observed[:, 0]), _ratio(self.replicated[:, :, 3], self.replicated[:, :, 0])

    @property
    def dispersion(self):
        """(sumsq / |S|) / (total / |S|)^2 - 1 - 1 / (total / |S|): the excess of the second moment over a Poisson's with the
        same mean.  NaN where total is 0 (no mean to compare with); None without `support`."""
        if self.support is None:
            return None

        def one(c, n):
            n = np.broadcast_to(n, c.shape[:-1]).astype(np.float64)
            mean = _ratio(c[..., 1], n)
            return _ratio(_ratio(c[..., 2], n), mean * mean) - 1.0 - _ratio(1.0, mean)
        return one(self.observed, self.support), one(self.replicated, self.support[None, :])

    def summary(self, q=(0.025, 0.5, 0.975), derived=False):
        """DataFrame with one row per (statistic, layer): observed, the replicates' quantiles q, the p-value.  derived=True adds
        the rows of `report_reciprocity` and `dispersion` (NaN replicates left out of their quantiles and p-values)."""
        import pandas as pd
        q = tuple(float(x) for x in q)
        pv = self.p_values()
        rows = []
        for k, name in enumerate(self.STATISTICS):
            for l in range(self.L):
                row = {"statistic": name, "layer": l, "observed": float(self.observed[l, k])}
                row.update({"q%g" % x: float(y) for x, y in zip(q, np.quantile(self.replicated[:, l, k].astype(np.float64), q))})
                row["p_value"] = float(pv[l, k])
                rows.append(row)
        if derived:
            for name in ("report_reciprocity", "dispersion"):
                pair = getattr(self, name)
                if pair is None:
                    continue
                for l in range(self.L):
                    o, v = pair[0][l], pair[1][:, l]
                    v = v[~np.isnan(v)]
                    row = {"statistic": name, "layer": l, "observed": float(o)}
                    qs = np.quantile(v, q) if v.size else np.full(len(q), np.nan)
                    row.update({"q%g" % x: float(y) for x, y in zip(q, qs)})
                    row["p_value"] = float(_p_value(o, v)) if v.size and not np.isnan(o) else np.nan
                    rows.append(row)
        return pd.DataFrame(rows, columns=["statistic", "layer", "observed"] + ["q%g" % x for x in q] + ["p_value"])
