"""Reporter influence: whose word does an inferred tie rest on -- the host side of `CaviEngine.reporter_influence` and
`VimureModel.reporter_influence`.

In a self-reporter survey each tie has two possible reporters, and the network the analyst gets is only as robust as the ties that
survive when one reporter's word is dropped.  The CAVI update of a tie's row of rho is additive over the reporters of its mask,
log rho_k = logpr_k + sum_m c_mk + const, so dividing reporter m's factor out of the fitted row gives the row the update would
have produced with R[l,i,j,m] = 0: the leave-one-reporter-out posterior, in closed form.  vmr_reporter_influence
(include/vimure_hip.h) evaluates it at every element of the support where rho lives and returns per-reporter integer counts, two
fixed-point sums, a histogram of the shift and only the rows worth reading.

What the numbers are: the parameters are held fixed and one reporter's factor is removed from one tie.  They are an exact refit
of that row only when rho is the update's fixed point for the tables given.

`influence_np` restates the entry point in NumPy -- the authoritative statement of the order of the operations, and for small
inputs the yardstick of the device pass.  `ReporterInfluence` holds a result; `min_tv_for_top` and `top_rows` are the top-n
selection of `VimureModel.reporter_influence`.
"""
import math

import numpy as np

from .crossval import counts_at, mirror_counts, support

SELECT = {"none": 0, "lost": 1, "gained": 2, "both": 3}
METHODS = {"rho_max": 0, "threshold": 2}
COLUMNS = ("l", "i", "j", "m", "x", "xt", "prob", "prob_loo", "tv")
COUNT_NAMES = ("n_scope", "lost", "gained", "flagged")
SUM_NAMES = ("tv", "shift")
GRID_EDGES = 4096          # the edge grid of the top-n selection: k / 4096, k = 0 .. 4095 (every edge is exact in binary)


class InfluenceArgumentError(ValueError):
    """An argument `influence_np` refuses, as vmr_reporter_influence does: a selection outside none / lost / gained / both, a NaN
    or negative min_tv, a method that gives no categories, a table entry out of range, edges that decrease, a layer out of range."""


def select_code(select):
    """0 (none), 1 (lost), 2 (gained) or 3 (both) of a name or of the code itself."""
    if isinstance(select, str):
        if select not in SELECT:
            raise InfluenceArgumentError("select must be \"lost\", \"gained\", \"both\" or \"none\"")
        return SELECT[select]
    if select not in (0, 1, 2, 3):
        raise InfluenceArgumentError("select must be \"lost\", \"gained\", \"both\" or \"none\" (0..3)")
    return int(select)


def method_code(method):
    """0 (the first maximum) or 2 (rho_1 >= threshold) of "rho_max" / "threshold" or of the code itself."""
    if isinstance(method, str):
        if method not in METHODS:
            raise InfluenceArgumentError("'method' should be one of \"rho_max\", \"threshold\".")
        return METHODS[method]
    if method not in (0, 2):
        raise InfluenceArgumentError("the method must be rho_max (0) or threshold (2): a readout of categories")
    return int(method)


def grid_edges():
    """The fixed edge grid of the top-n selection over [0, 1]: 0, 1/4096, 2/4096, .. (4096 edges)."""
    return np.arange(GRID_EDGES, dtype=np.float64) / float(GRID_EDGES)


def sum_quantum(N):
    """The fixed point of vmr_reporter_influence's sums: every term is rounded to a multiple of 2^-(61 - b), b = ceil(log2 N^2); a
    reporter's sum of n terms is within n q / 2 of the exact sum of its terms."""
    T, b = int(N) * int(N), 0
    while b < 63 and (1 << b) < T:
        b += 1
    return 2.0 ** -(61 - b)


def _exp_table(a):
    """exp of a small table, entry by entry through the C library (what the entry point does on the host)."""
    a = np.asarray(a, dtype=np.float64)
    return np.array([math.exp(v) for v in a.reshape(-1)], dtype=np.float64).reshape(a.shape)


def loo_rows(r, x, xt, e_th, elog_th, g_th, e_la, elog_la, g_la, g_nu):
    """The leave-one-out rows q [n, K] of n elements: r [n, K] their ties' rows of rho, x, xt [n] the counts, e_th, elog_th, g_th
    [n] the reporter's table entries, e_la, elog_la, g_la [n, K] the layer's, g_nu the scalar.  Every product, quotient and sum is
    rounded on its own, in the order vmr_reporter_influence states."""
    r = np.asarray(r, dtype=np.float64)
    xd, xtd = np.asarray(x, dtype=np.float64), np.asarray(xt, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        z1 = g_th[:, None] * g_la
        den = z1 + (g_nu * xtd)[:, None]
        den[den == 0.0] = 1.0
        w1 = z1 / den
        xw = xd[:, None] * w1
        c = (elog_th[:, None] + elog_la) * xw - e_th[:, None] * e_la
        d = -c
        pos = r > 0.0
        mx = np.where(pos, d, -np.inf).max(axis=1)
        u = np.where(pos, r * np.exp(np.where(pos, d - mx[:, None], 0.0)), 0.0)
        S = np.zeros(len(r))
        for k in range(r.shape[1]):                           # k ascending
            S = S + u[:, k]
        q = np.where(pos, u / S[:, None], 0.0)
    return q


def _readout(q, method, threshold):
    """The byte vmr_readout gives a row: the first maximum, or q_1 >= threshold."""
    if method == 2:
        with np.errstate(invalid="ignore"):
            return (q[:, 1] >= threshold).astype(np.int64)
    return np.argmax(q, axis=1).astype(np.int64)


def influence_np(rho, X, R, e_theta, elog_theta, e_lambda, elog_lambda, g_nu, mutuality=True, method="rho_max", threshold=0.0,
                 select="both", min_tv=np.inf, layer=None, edges=None):
    """vmr_reporter_influence in NumPy, from its definitions.  rho [L,N,N,K]; X [L,N,N,M] the counts (dense or a coordinate
    container), R the mask (dense, a coordinate container, or None: every (l, i, j, m)); e_theta, elog_theta [L,M], e_lambda,
    elog_lambda [L,K] and g_nu the tables.  Over the support of R in lexicographic order (of `layer` alone when it is given).
    Returns the dict of `CaviEngine.reporter_influence`: counts int64 [L',M,4] (n_scope, lost, gained, flagged), sums float64
    [L',M,2] (sum tv, sum (prob_loo - prob); plain double sums, NOT quantised), hist int64 [L', n_edges + 1, 2] (exactly c edges <=
    tv; class 0: x > 0, 1: x = 0; None without edges), the flagged rows l, i, j, m, x, xt, prob, prob_loo, tv, their "lost" and
    "gained" marks and their leave-one-out rows "q" [n, K]."""
    sel, code = select_code(select), method_code(method)
    min_tv, threshold, g_nu = float(min_tv), float(threshold), float(g_nu)
    if not min_tv >= 0.0:
        raise InfluenceArgumentError("min_tv must lie in [0, +inf]")
    rho = np.asarray(rho, dtype=np.float64)
    L, K = int(rho.shape[0]), int(rho.shape[3])
    e_theta, elog_theta = np.asarray(e_theta, dtype=np.float64), np.asarray(elog_theta, dtype=np.float64)
    e_lambda, elog_lambda = np.asarray(e_lambda, dtype=np.float64), np.asarray(elog_lambda, dtype=np.float64)
    M = int(e_theta.shape[1])
    if e_theta.shape != (L, M) or elog_theta.shape != (L, M) or e_lambda.shape != (L, K) or elog_lambda.shape != (L, K):
        raise InfluenceArgumentError(f"the tables must be [L, M] = {(L, M)} and [L, K] = {(L, K)}")
    for name, a, nonneg in (("e_theta", e_theta, True), ("e_lambda", e_lambda, True), ("elog_theta", elog_theta, False),
                            ("elog_lambda", elog_lambda, False), ("g_nu", np.array([g_nu]), True)):
        if not np.isfinite(a).all() or (nonneg and (a < 0).any()):
            raise InfluenceArgumentError(f"{name} must be finite" + (" and non-negative" if nonneg else ""))
    if layer is not None and not 0 <= int(layer) < L:
        raise InfluenceArgumentError(f"layer {layer} out of range [0, {L})")
    ed = None
    if edges is not None:
        ed = np.ascontiguousarray(np.atleast_1d(edges), dtype=np.float64)
        if not np.isfinite(ed).all() or (np.diff(ed) < 0).any() or len(ed) > GRID_EDGES:
            raise InfluenceArgumentError("the edges must be finite, non-decreasing and at most 4096")
    sup = support(X, R)
    x = counts_at(X, sup)
    xt = mirror_counts(X, sup) if mutuality else np.zeros(len(x), np.int64)
    l, i, j, m = sup
    layers = np.arange(L)
    if layer is not None:
        w = l == int(layer)
        l, i, j, m, x, xt = l[w], i[w], j[w], m[w], x[w], xt[w]
        layers = np.array([int(layer)])
    l0, Lq = int(layers[0]), len(layers)
    g_theta, g_lambda = _exp_table(elog_theta), _exp_table(elog_lambda)
    r = rho[l, i, j]
    q = loo_rows(r, x, xt, e_theta[l, m], elog_theta[l, m], g_theta[l, m], e_lambda[l], elog_lambda[l], g_lambda[l],
                 g_nu if mutuality else 0.0)
    n = len(l)
    prob, prob_loo, t = np.zeros(n), np.zeros(n), np.zeros(n)
    with np.errstate(invalid="ignore"):
        for k in range(1, K):                                 # k ascending
            prob = prob + r[:, k]
            prob_loo = prob_loo + q[:, k]
        for k in range(K):
            t = t + np.abs(q[:, k] - r[:, k])
        tv = 0.5 * t
        if np.isnan(prob).any() or np.isnan(prob_loo).any() or np.isnan(tv).any():
            raise ValueError("reporter_influence: a leave-one-out value is NaN")
        y, y_loo = _readout(r, code, threshold), _readout(q, code, threshold)
        lost, gained = (y > 0) & (y_loo == 0), (y == 0) & (y_loo > 0)
        flag = (lost & bool(sel & 1)) | (gained & bool(sel & 2)) | (tv >= min_tv)
    counts = np.zeros((Lq, M, 4), np.int64)
    for c, w in enumerate((np.ones(n, bool), lost, gained, flag)):
        np.add.at(counts[:, :, c], (l[w] - l0, m[w]), 1)
    sums = np.zeros((Lq, M, 2), np.float64)
    np.add.at(sums[:, :, 0], (l - l0, m), tv)
    np.add.at(sums[:, :, 1], (l - l0, m), prob_loo - prob)
    hist = None
    if ed is not None:
        cbin = np.searchsorted(ed, tv, side="right")          # #{tau : edges[tau] <= tv}
        hist = np.zeros((Lq, len(ed) + 1, 2), np.int64)
        np.add.at(hist, (l - l0, cbin, (x == 0).astype(np.int64)), 1)
    out = {"counts": counts, "sums": sums, "hist": hist, "edges": ed, "layers": layers, "method": code, "threshold": threshold,
           "select": sel, "min_tv": min_tv, "lost": lost[flag], "gained": gained[flag], "q": q[flag]}
    for name, col in zip(COLUMNS, (l, i, j, m, x, xt, prob, prob_loo, tv)):
        out[name] = col[flag]
    return out


def min_tv_for_top(hist, edges, top, max_rows=None):
    """(min_tv, n): the largest edge with at least `top` elements at or above it and their number, from a histogram hist
    [L', n_edges + 1, 2] of tv over `edges` (an element sits in bin #{tau : edges[tau] <= tv}).  No such edge: (0.0, every
    element) -- a total variation is not negative.  n above max_rows: a ValueError that names n."""
    hist, edges = np.asarray(hist, dtype=np.int64), np.asarray(edges, dtype=np.float64)
    top = int(top)
    if top < 1:
        raise ValueError("top must be at least 1")
    per_bin = hist.sum(axis=(0, 2))
    at_or_above = np.cumsum(per_bin[::-1])[::-1][1:]           # [tau]: elements with tv >= edges[tau]
    ok = np.flatnonzero(at_or_above >= top)
    thr, n = (float(edges[ok[-1]]), int(at_or_above[ok[-1]])) if len(ok) else (0.0, int(per_bin.sum()))
    if max_rows is not None and n > int(max_rows):
        raise ValueError(f"{n} elements have a shift of at least {thr}, the level that holds the top {top}: more than max_rows = "
                         f"{int(max_rows)}; raise max_rows or ask for fewer")
    return thr, n


def top_rows(rows, top):
    """The `top` rows with the largest tv: sorted by (-tv, l, i, j, m), cut.  rows: a dict with the columns of `COLUMNS` (and
    "lost", "gained" when it has them); returns the same columns."""
    names = [c for c in COLUMNS + ("lost", "gained") if rows.get(c) is not None]
    cols = {c: np.asarray(rows[c]) for c in names}
    order = np.lexsort((cols["m"], cols["j"], cols["i"], cols["l"], -cols["tv"]))[:int(top)]
    return {c: v[order] for c, v in cols.items()}


def _host(a):
    return np.asarray(a.cpu().numpy() if type(a).__module__.startswith("torch") else a)


class ReporterInfluence:
    """What `reporter_influence` returns, held together: per layer and reporter the counts (`COUNT_NAMES`: the elements of the
    reporter's scope, those whose removal loses an inferred tie, those whose removal gains one, the flagged ones) and the sums
    (`SUM_NAMES`: of the total variation between the row and its leave-one-out row, and of the shift prob_loo - prob), the
    histogram of tv over `edges`, and the flagged rows.  result: the dict of `CaviEngine.reporter_influence` or `influence_np`.
    The parameters are held fixed and one reporter's factor is removed from one tie: an exact refit of that row only when rho is
    the update's fixed point."""

    def __init__(self, result, top=None):
        self.counts = np.asarray(result["counts"], dtype=np.int64)
        self.sums = np.asarray(result["sums"], dtype=np.float64)
        self.hist = None if result.get("hist") is None else np.asarray(result["hist"], dtype=np.int64)
        self.edges = None if result.get("edges") is None else np.asarray(result["edges"], dtype=np.float64)
        self.layers = np.asarray(result.get("layers", np.arange(len(self.counts))), dtype=np.int64)
        self.method, self.threshold = result.get("method"), result.get("threshold")
        self.select, self.min_tv = result.get("select"), result.get("min_tv")
        self.top = top
        self._rows = None
        if result.get("l") is not None:
            self._rows = {c: _host(result[c]) for c in COLUMNS + ("lost", "gained") if result.get(c) is not None}

    def __len__(self):
        return 0 if self._rows is None else int(len(self._rows["l"]))

    def frame(self):
        """One row per (layer, reporter): n_scope, lost, gained, flagged, and the means of tv and of the shift over the scope."""
        import pandas as pd
        Lq, M = self.counts.shape[:2]
        c, s = self.counts.reshape(Lq * M, -1), self.sums.reshape(Lq * M, -1)
        with np.errstate(divide="ignore", invalid="ignore"):
            mean_tv, mean_shift = s[:, 0] / c[:, 0], s[:, 1] / c[:, 0]
        return pd.DataFrame({"layer": np.repeat(self.layers, M), "reporter": np.tile(np.arange(M), Lq), "n_scope": c[:, 0],
                             "lost": c[:, 1], "gained": c[:, 2], "flagged": c[:, 3], "mean_tv": mean_tv, "mean_shift": mean_shift})

    def rows(self):
        """One row per flagged element, in the order of the table: layer, source, target, reporter, x, x_mirror, prob, prob_loo,
        shift = prob_loo - prob, tv, and lost / gained where the result holds the marks."""
        import pandas as pd
        if self._rows is None:
            raise ValueError("no rows were asked for (rows=False)")
        r = self._rows
        prob, loo = np.asarray(r["prob"], np.float64), np.asarray(r["prob_loo"], np.float64)
        d = {"layer": np.asarray(r["l"], np.int64), "source": np.asarray(r["i"], np.int64), "target": np.asarray(r["j"], np.int64),
             "reporter": np.asarray(r["m"], np.int64), "x": np.asarray(r["x"], np.int64), "x_mirror": np.asarray(r["xt"], np.int64),
             "prob": prob, "prob_loo": loo, "shift": loo - prob, "tv": np.asarray(r["tv"], np.float64)}
        for c in ("lost", "gained"):
            if c in r:
                d[c] = np.asarray(r[c], bool)
        return pd.DataFrame(d)

    def fragile_ties(self):
        """The rows with `lost` set: inferred ties that rest on one reporter's word."""
        f = self.rows()
        if "lost" not in f:
            raise ValueError("the result holds no lost / gained marks (flips=False)")
        return f[f["lost"]].reset_index(drop=True)

    def summary(self):
        return {"n": int(self.counts[:, :, 0].sum()), "lost": int(self.counts[:, :, 1].sum()), "gained": int(self.counts[:, :, 2].sum()),
                "flagged": int(self.counts[:, :, 3].sum()), "min_tv": self.min_tv, "rows": len(self)}
