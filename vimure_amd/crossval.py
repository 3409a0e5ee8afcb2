"""Held-out report log-likelihood and k-fold cross-validation -- the host side of `CaviEngine.heldout_loglik`.

Everything else the package says about a fit looks at the data the model was fitted to; the ELBOs of different K are not
comparable.  Is K = 3 better than K = 2, does mutuality help, which prior is better: the standard answer is the predictive
probability of reports the fit never saw.  Holding reports out is what the reporter mask already does -- an entry (l,i,j,m) with
R = 0 is outside the model: its count is discarded and it adds nothing to the rates -- and vmr_heldout_loglik
(include/vimure_hip.h) scores such entries under the fitted posterior where rho lives.

`heldout_loglik_np` restates that entry point in NumPy, the yardstick of the device pass.  `support`, `assign_folds`,
`train_mask`, `counts_at` and `mirror_counts` cut a dataset into folds, for dense arrays and coordinate containers alike;
`cross_validate` fits every fold and scores its held-out list, `compare_models` runs the same folds for several candidates.
"""
import warnings
from dataclasses import dataclass, field

import numpy as np

from .tensor import SparseTensor, is_sparse_like

SUM_NAMES = ("logp", "sq_err", "total", "exp_total")
COUNT_NAMES = ("n", "n_pos", "n_inf", "n_in_mask")
ESTIMATES = ("mean", "geometric")
UNITS = ("pair", "entry")
MAX_SUPPORT = 2 ** 28
_DRIVER_KEYS = ("seed", "R", "keep_engine", "engine")   # what cross_validate passes to every fold's fit itself


# ------------------------------------------------------------------------------------------------ the restatement
def _gammaln(v):
    try:
        from scipy.special import gammaln
        return gammaln(v)
    except ImportError:
        import math
        return np.array([math.lgamma(float(q)) for q in np.asarray(v).reshape(-1)]).reshape(np.shape(v))


def _subs(subs):
    if len(subs) != 4:
        raise ValueError("subs must be the 4 index arrays (l, i, j, m)")
    out = tuple(np.asarray(s, dtype=np.int64).reshape(-1) for s in subs)
    if any(len(s) != len(out[0]) for s in out):
        raise ValueError("subs: arrays of one length expected")
    return out


def _key(subs, shape):
    return np.ravel_multi_index(tuple(np.asarray(s, dtype=np.int64) for s in subs), tuple(int(v) for v in shape))


def in_mask(R, subs, shape=None):
    """bool [n]: R != 0 at every (l, i, j, m) of subs.  R: a dense array, a coordinate container, or None (all ones)."""
    subs = _subs(subs)
    if R is None:
        return np.ones(len(subs[0]), bool)
    if is_sparse_like(R):
        shape = tuple(int(v) for v in R.shape)
        keys = np.sort(_key(R.subs, shape))
        q = _key(subs, shape)
        at = np.minimum(np.searchsorted(keys, q), max(len(keys) - 1, 0))
        return (keys[at] == q) if len(keys) else np.zeros(len(q), bool)
    return np.asarray(R)[subs] != 0


def heldout_loglik_np(rho, subs, x, xt, theta, lam, eta, R=None):
    """vmr_heldout_loglik in NumPy, from its definitions.  rho [L,N,N,K]; subs the 4 index arrays (l, i, j, m) of the entries; x the
    held-out counts; xt the mirrored counts (None: 0); theta [L,M], lam [L,K], eta.  Per entry, mu_k = theta[l,m] lam[l,k] + eta xt,
    mean = sum_k rho_k mu_k (k ascending, every product and sum rounded on its own) and logp = log sum_k rho_k Poisson(x; mu_k) as
    a log-sum-exp over the categories with rho_k > 0 of b_k = x log(mu_k) - mu_k + log(rho_k), lgamma(x + 1) subtracted once;
    mu_k = 0 and x = 0 contributes log(rho_k), mu_k = 0 and x > 0 nothing; no contribution at all: -inf.
    Returns (logp [n], mean [n], sums float64 [L,4], counts int64 [L,4]): per layer the sum of the finite logp, of (x - mean)^2,
    of x and of mean (added in extended precision), and the number of entries, of entries with x > 0, of entries with logp =
    -inf, and of entries inside the mask R (dense, coordinate container or None = all ones)."""
    rho = np.asarray(rho, dtype=np.float64)
    L, K = rho.shape[0], rho.shape[-1]
    l, i, j, m = _subs(subs)
    x = np.asarray(x, dtype=np.int64).reshape(-1)
    xt = np.zeros(len(x), np.int64) if xt is None else np.asarray(xt, dtype=np.int64).reshape(-1)
    theta, lam = np.asarray(theta, dtype=np.float64), np.asarray(lam, dtype=np.float64)
    if x.min(initial=0) < 0 or xt.min(initial=0) < 0:
        raise ValueError("counts must be >= 0")
    xd = x.astype(np.float64)
    r = rho[l, i, j]                                                              # [n, K]
    mu = theta[l, m][:, None] * lam[l] + (float(eta) * xt.astype(np.float64))[:, None]
    mean = np.zeros(len(x))
    for k in range(K):
        mean = mean + r[:, k] * mu[:, k]
    with np.errstate(divide="ignore", invalid="ignore"):
        b = xd[:, None] * np.log(mu) - mu + np.log(r)
        b = np.where(mu == 0.0, np.where(xd[:, None] > 0, -np.inf, np.log(r)), b)
        b = np.where(r > 0.0, b, -np.inf)
        mx = b.max(axis=1)
        s = np.zeros(len(x))
        for k in range(K):
            s = s + np.where(b[:, k] > -np.inf, np.exp(b[:, k] - mx), 0.0)
        logp = np.where(mx == -np.inf, -np.inf, mx + np.log(s) - _gammaln(xd + 1.0))
    logp = np.where(np.isnan(b).any(axis=1), np.nan, logp)
    inm = in_mask(R, (l, i, j, m))
    sums, counts = np.zeros((L, 4)), np.zeros((L, 4), np.int64)
    ld = np.longdouble
    for q in range(L):
        w = l == q
        fin = w & np.isfinite(logp)
        sums[q] = [np.sum(logp[fin], dtype=ld), np.sum((xd[w] - mean[w]) ** 2, dtype=ld), np.sum(xd[w], dtype=ld),
                   np.sum(mean[w], dtype=ld)]
        counts[q] = [w.sum(), (w & (x > 0)).sum(), (w & (logp == -np.inf)).sum(), (w & inm).sum()]
    return logp, mean, sums, counts


# ------------------------------------------------------------------------------------------------ cutting a dataset into folds
def _shape_of(X):
    shape = tuple(int(v) for v in X.shape)
    if len(shape) != 4 or shape[1] != shape[2]:
        raise ValueError("X must have shape (L, N, N, M)")
    return shape


def support(X, R=None, max_support=MAX_SUPPORT):
    """The coordinate list of the support, lexicographic: the 4 int64 index arrays (l, i, j, m) of np.nonzero(R), of R.subs for a
    coordinate container, or of every (l, i, j, m) of X's shape without R.  Beyond max_support elements it is refused: pass an
    explicit `folds` sample to `cross_validate` instead."""
    shape = _shape_of(X)
    if R is None:
        n = int(np.prod([float(v) for v in shape]))
    elif is_sparse_like(R):
        n = len(R.subs[0])
    else:
        n = int(np.count_nonzero(np.asarray(R)))
    if n > max_support:
        raise ValueError(f"the support holds {n} elements, more than max_support = {max_support}: pass an explicit `folds` sample "
                         "(an array over a support of your own, -1 where an element is never held out)")
    if R is None:
        return tuple(a.reshape(-1).astype(np.int64) for a in np.indices(shape))
    if is_sparse_like(R):
        if tuple(int(v) for v in R.shape) != shape:
            raise ValueError("Dimensions of reporter mask (R) do not match L x N x N x M")
        keys = np.unique(_key(R.subs, shape))
        return tuple(a.astype(np.int64) for a in np.unravel_index(keys, shape))
    R = np.asarray(R)
    if R.shape != shape:
        raise ValueError("Dimensions of reporter mask (R) do not match L x N x N x M")
    return tuple(a.astype(np.int64) for a in np.nonzero(R))


def assign_folds(subs, n_folds, seed=0, unit="pair", shape=None):
    """The fold in [0, n_folds) of every support element.  unit="pair": the unit is (l, min(i,j), max(i,j), m), so both directions
    of a reporter's pair are held out together -- with mutuality an entry's rate reads its mirror, and under "pair" no training
    entry ever conditions on a held-out count.  unit="entry": every element stands on its own; a held-out count then still enters
    the fit as the mirror count of its partner's rate (and its own rate is scored given a partner the fit has seen): with
    mutuality the held-out density leaks information and reads too well.  The assignment is a RandomState(seed) permutation of
    the units, dealt round-robin: every fold is non-empty (fewer units than folds: ValueError)."""
    if unit not in UNITS:
        raise ValueError("unit must be \"pair\" or \"entry\"")
    l, i, j, m = _subs(subs)
    n_folds = int(n_folds)
    if n_folds < 2:
        raise ValueError("n_folds must be at least 2")
    if shape is None:
        nn = int(max(i.max(initial=0), j.max(initial=0))) + 1
        shape = (int(l.max(initial=0)) + 1, nn, nn, int(m.max(initial=0)) + 1)
    a, b = (np.minimum(i, j), np.maximum(i, j)) if unit == "pair" else (i, j)
    units, inv = np.unique(_key((l, a, b, m), shape), return_inverse=True)
    if len(units) < n_folds:
        raise ValueError(f"{len(units)} units cannot fill {n_folds} folds")
    of_unit = np.empty(len(units), np.int64)
    of_unit[np.random.RandomState(seed).permutation(len(units))] = np.arange(len(units)) % n_folds
    return of_unit[inv.reshape(-1)]


def train_mask(X, R, subs_out):
    """R with the held-out entries removed, in the form `fit` takes beside X: a dense uint8 array for a dense X, a coordinate
    container for a coordinate X (without R its support is every (l, i, j, m): `support`'s limit applies).  X itself is passed to
    `fit` unchanged: the mask is what discards the held-out counts."""
    shape = _shape_of(X)
    out = _subs(subs_out)
    if not is_sparse_like(X):
        if R is None:
            Rt = np.ones(shape, np.uint8)
        elif is_sparse_like(R):
            Rt = np.zeros(shape, np.uint8)
            Rt[tuple(np.asarray(s, dtype=np.int64) for s in R.subs)] = 1
        else:
            Rt = (np.asarray(R) != 0).astype(np.uint8)
        Rt[out] = 0
        return Rt
    sup = _key(support(X, R), shape)                     # sorted, unique
    keep = sup[~np.isin(sup, _key(out, shape))]
    return SparseTensor(tuple(np.unravel_index(keep, shape)), np.ones(len(keep), np.uint8), shape=shape)


def counts_at(X, subs):
    """X[l,i,j,m] at every entry of subs, int64.  A dense X is indexed; a coordinate container is looked up by sorted key (no
    dense array is built)."""
    shape = _shape_of(X)
    subs = _subs(subs)
    if not is_sparse_like(X):
        if type(X).__module__.startswith("torch"):
            import torch
            return X[tuple(torch.as_tensor(s, device=X.device) for s in subs)].cpu().numpy().astype(np.int64)
        return np.asarray(X)[subs].astype(np.int64)
    keys = _key(X.subs, shape)
    order = np.argsort(keys, kind="stable")
    keys, vals = keys[order], np.asarray(X.vals).astype(np.int64)[order]
    q = _key(subs, shape)
    if len(keys) == 0:
        return np.zeros(len(q), np.int64)
    at = np.minimum(np.searchsorted(keys, q), len(keys) - 1)
    return np.where(keys[at] == q, vals[at], 0)


def mirror_counts(X, subs):
    """X[l,j,i,m] of the FULL data at every entry (l, i, j, m) of subs: the count an entry's rate conditions on with mutuality."""
    l, i, j, m = _subs(subs)
    return counts_at(X, (l, j, i, m))


# ------------------------------------------------------------------------------------------------ the driver
def plug_in_tables(model, eng, estimate="mean"):
    """(theta [L,M], lam [L,K], eta) a fitted model scores held-out reports with.  "mean": the posterior means gamma_shp / gamma_rte,
    phi_shp / phi_rte, nu_shp / nu_rte of the best realisation; "geometric": g_theta, g_lambda, g_nu of the engine's
    vmr_get_geometric, the quantities `calculate_mean_poisson` uses.  Mutuality off: eta = 0."""
    if estimate not in ESTIMATES:
        raise ValueError("estimate must be \"mean\" or \"geometric\"")
    if estimate == "mean":
        theta = np.asarray(model.gamma_shp_f, dtype=np.float64) / np.asarray(model.gamma_rte_f, dtype=np.float64)
        lam = np.asarray(model.phi_shp_f, dtype=np.float64) / np.asarray(model.phi_rte_f, dtype=np.float64)
        eta = float(model.nu_shp_f) / float(model.nu_rte_f)
    else:
        theta, lam, eta, _ = eng.get_geometric()
    return theta, lam, (float(eta) if model.mutuality else 0.0)


def _per_entry(sums, counts):
    """(mean log predictive density over the entries with finite logp, MSE over all entries) of [.., L, 4] sums and counts."""
    s, c = np.asarray(sums, dtype=np.float64), np.asarray(counts, dtype=np.float64)
    n_fin = (c[..., 0] - c[..., 2]).sum(axis=-1)
    n = c[..., 0].sum(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return s[..., 0].sum(axis=-1) / n_fin, s[..., 1].sum(axis=-1) / n


def _mean_se(v):
    v = np.asarray(v, dtype=np.float64)
    se = float(np.std(v, ddof=1) / np.sqrt(len(v))) if len(v) > 1 else float("nan")
    return float(np.mean(v)), se


@dataclass
class CVResult:
    """What `cross_validate` returns.  sums float64 [F, L, 4] (`SUM_NAMES`) and counts int64 [F, L, 4] (`COUNT_NAMES`) of every
    fold's held-out list per layer, in_sums / in_counts the same for a same-sized random sample of the fold's training support;
    lpd [F] the held-out mean log predictive density per entry (over the entries with a finite logp: `n_inf` counts the others),
    in_lpd [F] the in-sample one, mse / in_mse [F] the mean squared error of the expected report; lpd_mean, lpd_se (and in_, mse_)
    the mean over the folds and its standard error; folds the fold of every element of `subs` (-1: never held out)."""
    K: int
    mutuality: bool
    estimate: str
    unit: str
    seed: int
    subs: tuple
    folds: np.ndarray
    sums: np.ndarray
    counts: np.ndarray
    in_sums: np.ndarray
    in_counts: np.ndarray
    elbo: np.ndarray
    config: dict = field(default_factory=dict)

    @property
    def n_folds(self):
        return int(self.sums.shape[0])

    @property
    def lpd(self):
        return _per_entry(self.sums, self.counts)[0]

    @property
    def mse(self):
        return _per_entry(self.sums, self.counts)[1]

    @property
    def in_lpd(self):
        return _per_entry(self.in_sums, self.in_counts)[0]

    @property
    def in_mse(self):
        return _per_entry(self.in_sums, self.in_counts)[1]

    @property
    def n_inf(self):
        return self.counts[..., 2].sum(axis=-1)

    lpd_mean = property(lambda self: _mean_se(self.lpd)[0])
    lpd_se = property(lambda self: _mean_se(self.lpd)[1])
    in_lpd_mean = property(lambda self: _mean_se(self.in_lpd)[0])
    in_lpd_se = property(lambda self: _mean_se(self.in_lpd)[1])
    mse_mean = property(lambda self: _mean_se(self.mse)[0])
    mse_se = property(lambda self: _mean_se(self.mse)[1])

    def frame(self):
        """One row per (fold, layer): the counts, the sums, and the per-entry figures of that cell, held-out and in-sample."""
        import pandas as pd
        rows = []
        F, L = self.sums.shape[:2]
        for f in range(F):
            for l in range(L):
                row = {"fold": f, "layer": l}
                for tag, s, c in (("", self.sums, self.counts), ("in_", self.in_sums, self.in_counts)):
                    row.update({tag + n: int(c[f, l, q]) for q, n in enumerate(COUNT_NAMES)})
                    row.update({tag + n: float(s[f, l, q]) for q, n in enumerate(SUM_NAMES)})
                    lpd, mse = _per_entry(s[f, l][None], c[f, l][None])
                    row[tag + "lpd"], row[tag + "mse"] = float(lpd), float(mse)
                rows.append(row)
        return pd.DataFrame(rows)

    def summary(self):
        return {"K": self.K, "mutuality": self.mutuality, "n_folds": self.n_folds, "lpd": self.lpd_mean, "lpd_se": self.lpd_se,
                "in_lpd": self.in_lpd_mean, "mse": self.mse_mean, "mse_se": self.mse_se, "n_inf": int(self.n_inf.sum())}


def _fold_lists(sup, folds, n_folds):
    folds = np.asarray(folds, dtype=np.int64).reshape(-1)
    if len(folds) != len(sup[0]):
        raise ValueError(f"folds has {len(folds)} elements, the support {len(sup[0])}")
    if folds.min(initial=0) < -1:
        raise ValueError("folds: -1 (never held out) or a fold number expected")
    F = int(folds.max(initial=-1)) + 1 if n_folds is None else int(n_folds)
    if F < 2 or any(not (folds == f).any() for f in range(F)):
        raise ValueError("folds: at least two folds, none of them empty, expected")
    return folds, F


def cross_validate(X, R=None, K=2, mutuality=True, n_folds=5, seed=0, folds=None, estimate="mean", unit="pair", subs=None,
                   on_fold=None, **fit_kwargs):
    """k-fold cross-validation of one model on the reports of X.  The support (`support(X, R)`) is cut into folds
    (`assign_folds`; or `folds`, an array over the support with -1 = never held out -- with `subs`, a support of the caller's own,
    which is how the support of a large all-ones problem is sampled); for each fold: `VimureModel(mutuality=mutuality).fit(X,
    R=train_mask(..), K=K, seed=seed, keep_engine=True, **fit_kwargs)`, the held-out list scored on the device under the fit's
    plug-in tables (`plug_in_tables(estimate)`, the mirrored counts from the full X), a same-sized random sample of the training
    support scored the same way for the in-sample figure, and the engine closed.  Every fold's in-mask count must be 0.  The fits
    run one after another.  `seed`, `R`, `keep_engine` and `engine` are the driver's and refused among fit_kwargs.  on_fold(f, model, subs_out, x_out, xt_out, (theta, lam, eta)) is called while fold f's model still
    holds its engine (to keep a read-out of it, say); the model is not kept.  Returns a `CVResult`."""
    from .model import VimureModel
    if estimate not in ESTIMATES:
        raise ValueError("estimate must be \"mean\" or \"geometric\"")
    taken = sorted(k for k in fit_kwargs if k in _DRIVER_KEYS)
    if taken:
        raise ValueError(f"{', '.join(taken)}: set by the driver for every fold (seed= seeds the fits too), not a keyword of the fits")
    shape = _shape_of(X)
    sup = support(X, R) if subs is None else _subs(subs)
    if subs is not None and folds is None:
        raise ValueError("subs= is taken with folds= only")
    if folds is None:
        folds = assign_folds(sup, n_folds, seed, unit, shape)
        F = int(n_folds)
    else:
        folds, F = _fold_lists(sup, folds, None)
    folds = np.asarray(folds, dtype=np.int64)
    key = _key(sup, shape)
    if len(key) > 1 and not (key[1:] > key[:-1]).all():   # the lists go to the device sorted: the fast case, and el in order
        order = np.argsort(key, kind="stable")
        sup, folds = tuple(s[order] for s in sup), folds[order]
    x_all = counts_at(X, sup)
    xt_all = mirror_counts(X, sup) if mutuality else None
    L = shape[0]
    sums, counts = np.zeros((F, L, 4)), np.zeros((F, L, 4), np.int64)
    in_sums, in_counts = np.zeros((F, L, 4)), np.zeros((F, L, 4), np.int64)
    elbo = np.zeros(F)
    for f in range(F):
        out = np.flatnonzero(folds == f)
        rest = np.flatnonzero(folds != f)
        subs_out = tuple(s[out] for s in sup)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            model = VimureModel(mutuality=mutuality)
            model.fit(X, R=train_mask(X, R, subs_out), K=K, seed=seed, keep_engine=True, **fit_kwargs)
        eng = model._engine
        try:
            theta, lam, eta = plug_in_tables(model, eng, estimate)
            res = eng.heldout_loglik(subs_out, x_all[out], None if xt_all is None else xt_all[out], theta=theta, lam=lam, eta=eta,
                                     per_entry=False)
            if res["counts"][:, 3].any():
                raise RuntimeError(f"fold {f}: {int(res['counts'][:, 3].sum())} held-out entries lie inside the training mask")
            sums[f], counts[f] = res["sums"], res["counts"]
            if len(rest):
                pick = np.sort(np.random.RandomState(int(seed) + 1 + f).choice(rest, size=min(len(out), len(rest)), replace=False))
                ins = eng.heldout_loglik(tuple(s[pick] for s in sup), x_all[pick], None if xt_all is None else xt_all[pick],
                                         theta=theta, lam=lam, eta=eta, per_entry=False)
                in_sums[f], in_counts[f] = ins["sums"], ins["counts"]
            elbo[f] = float(model.maxL)
            if on_fold is not None:
                on_fold(f, model, subs_out, x_all[out], None if xt_all is None else xt_all[out], (theta, lam, eta))
        finally:
            model.close()
    cfg = dict(fit_kwargs)
    return CVResult(K=int(K), mutuality=bool(mutuality), estimate=estimate, unit=unit, seed=int(seed), subs=sup, folds=folds,
                    sums=sums, counts=counts, in_sums=in_sums, in_counts=in_counts, elbo=elbo, config=cfg)


@dataclass
class ModelComparison:
    """What `compare_models` returns: `table`, one row per candidate sorted by held-out density (best first) with the paired
    per-fold difference to the best candidate (`d_lpd`, its standard error `d_lpd_se`; 0 and NaN for the best itself), and
    `results`, the candidates' `CVResult`s in the order given."""
    table: object
    results: list


def compare_models(X, R, candidates, n_folds=5, seed=0, folds=None, estimate="mean", unit="pair", subs=None, **fit_kwargs):
    """The same folds for every candidate: a dict with `K`, `mutuality` (defaults 2, True) and any keyword of `fit` (priors ...)
    over the common `fit_kwargs` -- except `seed`, `R`, `keep_engine` and `engine`, which the driver sets for every fold
    (ValueError).  Returns a `ModelComparison`."""
    import pandas as pd
    candidates = [dict(c) for c in candidates]
    if not candidates:
        raise ValueError("no candidates")
    for q, c in enumerate(candidates):   # (a candidate may not move the folds, the seed or the driver's own fit keywords)
        taken = sorted(k for k in c if k in _DRIVER_KEYS + ("n_folds", "folds", "estimate", "unit", "subs", "on_fold"))
        if taken:
            raise ValueError(f"candidate {q}: {', '.join(taken)} is the driver's, the same for every candidate (seed=, n_folds=, folds= ... are compare_models' own arguments)")
    if folds is None:
        subs = support(X, R)
        folds = assign_folds(subs, n_folds, seed, unit, _shape_of(X))
    elif subs is None:
        subs = support(X, R)
    results = []
    for c in candidates:
        kw = dict(fit_kwargs)
        kw.update(c)
        K, mut = kw.pop("K", 2), kw.pop("mutuality", True)
        results.append(cross_validate(X, R, K=K, mutuality=mut, seed=seed, folds=folds, estimate=estimate, unit=unit, subs=subs, **kw))
    best = int(np.argmax([r.lpd_mean for r in results]))
    rows = []
    for q, (c, r) in enumerate(zip(candidates, results)):
        d = r.lpd - results[best].lpd
        row = {"candidate": q}
        row.update({k: (v if np.isscalar(v) else repr(v)) for k, v in c.items()})
        row.update(r.summary())
        row["d_lpd"], row["d_lpd_se"] = (0.0, float("nan")) if q == best else _mean_se(d)
        rows.append(row)
    table = pd.DataFrame(rows).sort_values("lpd", ascending=False, kind="stable").reset_index(drop=True)
    return ModelComparison(table=table, results=results)
