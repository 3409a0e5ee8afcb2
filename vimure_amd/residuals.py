"""Surprising reports: every report of the support scored under the posterior -- the host side of `CaviEngine.report_scores` and
`VimureModel.surprising_reports`.

After a fit the first question of a survey analyst is which individual reports the model disbelieves, and which omissions:
which (l, i, j, m) inside the reporter mask hold a count, or a zero, that is improbable under the posterior.  That list is what
gets checked against the questionnaires; it is the per-report counterpart of `reporters.ReporterTable`.  vmr_report_scores
(include/vimure_hip.h) walks the support where rho lives, evaluates the likelihood of `heldout_loglik` at every element, and
returns integer histograms of the surprise -log p, the exact in-sample log predictive density, and the flagged rows only.

`report_scores_np` restates that entry point in NumPy on top of `crossval.support`, `counts_at`, `mirror_counts` and
`heldout_loglik_np` -- for small inputs, the yardstick of the device pass.  `ReportScores` holds a result; `threshold_for_top` and
`top_rows` are the top-n selection of `surprising_reports`: a threshold read off a histogram over a fixed grid, then a sort of the
rows at or above it.
"""
import numpy as np

from .crossval import counts_at, heldout_loglik_np, mirror_counts, support

SELECT = {"reports": 1, "omissions": 2, "both": 3}
COLUMNS = ("l", "i", "j", "m", "x", "xt", "logp", "mean")
SUM_NAMES = ("logp", "sq_err", "total", "exp_total")
COUNT_NAMES = ("n", "n_reports", "n_inf", "n_flagged")
GRID_EDGES = 4096          # the edge grid of the top-n selection: GRID_EDGES edges, GRID_STEP nat apart, from 0
GRID_STEP = 1.0 / 64.0


def select_code(select):
    """1 (reports: x > 0), 2 (omissions: x = 0) or 3 (both) of a name or of the code itself."""
    if isinstance(select, str):
        if select not in SELECT:
            raise ValueError("select must be \"reports\", \"omissions\" or \"both\"")
        return SELECT[select]
    if select not in (1, 2, 3):
        raise ValueError("select must be \"reports\", \"omissions\" or \"both\" (1, 2 or 3)")
    return int(select)


def grid_edges():
    """The fixed edge grid of the top-n selection: 0, 1/64, 2/64, .. (4096 edges; every edge is exact in binary)."""
    return np.arange(GRID_EDGES, dtype=np.float64) * GRID_STEP


def report_scores_np(rho, X, R, theta, lam, eta, threshold, select="both", edges=None, mutuality=True):
    """vmr_report_scores in NumPy, from its definitions.  rho [L,N,N,K]; X [L,N,N,M] the counts (dense or a coordinate container),
    R the mask (dense, a coordinate container, or None: every (l, i, j, m)); theta [L,M], lam [L,K], eta the tables.  Over the
    support of R in lexicographic order: x = X[l,i,j,m], xt = X[l,j,i,m] with mutuality else 0, (logp, mean) of
    `heldout_loglik_np`, surprise s = -logp; an element is a report when x > 0, else an omission, and flagged when its class is in
    `select` and s >= threshold.  Returns the dict of `CaviEngine.report_scores` for all layers: counts int64 [L,4] (elements,
    reports, elements with logp = -inf, flagged), sums float64 [L,4] (as `heldout_loglik_np`), hist int64 [L, n_edges + 1, 2] over
    ALL elements (hist[l, c, b]: exactly c edges <= s; b = 0 reports, 1 omissions; None without edges), by_reporter int64
    [L,M,2], and the flagged rows l, i, j, m, x, xt, logp, mean."""
    sel = select_code(select)
    threshold = float(threshold)
    if np.isnan(threshold) or threshold == -np.inf:
        raise ValueError("the threshold must be finite or +inf")
    rho = np.asarray(rho, dtype=np.float64)
    L, M = int(rho.shape[0]), int(np.shape(theta)[1])
    sup = support(X, R)
    x = counts_at(X, sup)
    xt = mirror_counts(X, sup) if mutuality else np.zeros(len(x), np.int64)
    logp, mean, sums, counts = heldout_loglik_np(rho, sup, x, xt, theta, lam, eta, R=R)
    l, i, j, m = sup
    with np.errstate(invalid="ignore"):
        s = -logp
        cls = (x == 0).astype(np.int64)                       # 0 a report, 1 an omission
        chosen = np.where(cls == 0, (sel & 1) != 0, (sel & 2) != 0)
        flag = chosen & (s >= threshold)
    counts = counts.copy()
    counts[:, 3] = np.bincount(l[flag], minlength=L)
    hist, ed = None, None
    if edges is not None:
        ed = np.ascontiguousarray(np.atleast_1d(edges), dtype=np.float64)
        if not np.isfinite(ed).all() or (np.diff(ed) < 0).any():
            raise ValueError("the edges must be finite and non-decreasing")
        c = np.searchsorted(ed, s, side="right")              # #{tau : edges[tau] <= s}
        hist = np.zeros((L, len(ed) + 1, 2), np.int64)
        np.add.at(hist, (l, c, cls), 1)
    rep = np.zeros((L, M, 2), np.int64)
    np.add.at(rep, (l[flag], m[flag], cls[flag]), 1)
    out = {"counts": counts, "sums": sums, "hist": hist, "edges": ed, "by_reporter": rep, "layers": np.arange(L),
           "threshold": threshold, "select": sel}
    for name, col in zip(COLUMNS, (l, i, j, m, x, xt, logp, mean)):
        out[name] = col[flag]
    return out


def threshold_for_top(hist, edges, top, select="both", max_rows=None):
    """(threshold, n): the largest edge with at least `top` selected elements at or above it and their number, from a histogram
    hist [L', n_edges + 1, 2] over `edges` (`report_scores`' convention: an element with surprise s sits in bin #{tau : edges[tau]
    <= s}).  No such edge: (0.0, every selected element) -- a surprise is not negative beyond its rounding.  n above max_rows: a ValueError that
    names n (the level that holds the top rows holds too many to fetch)."""
    sel = select_code(select)
    hist, edges = np.asarray(hist, dtype=np.int64), np.asarray(edges, dtype=np.float64)
    top = int(top)
    if top < 1:
        raise ValueError("top must be at least 1")
    per_bin = np.zeros(hist.shape[1], np.int64)
    for b in (0, 1):
        if sel & (1 << b):
            per_bin += hist[:, :, b].sum(axis=0)
    at_or_above = np.cumsum(per_bin[::-1])[::-1][1:]           # [tau]: elements with s >= edges[tau], i.e. in a bin above tau
    ok = np.flatnonzero(at_or_above >= top)
    thr, n = (float(edges[ok[-1]]), int(at_or_above[ok[-1]])) if len(ok) else (0.0, int(per_bin.sum()))
    if max_rows is not None and n > int(max_rows):
        raise ValueError(f"{n} elements have a surprise of at least {thr}, the level that holds the top {top}: more than max_rows = "
                         f"{int(max_rows)}; raise max_rows or ask for fewer")
    return thr, n


def top_rows(rows, top):
    """The `top` most surprising of a table's rows: sorted by (-surprise, l, i, j, m), cut.  rows: a dict with the columns of
    `COLUMNS` (NumPy arrays of one length); returns the same columns."""
    cols = {c: np.asarray(rows[c]) for c in COLUMNS}
    with np.errstate(invalid="ignore"):
        order = np.lexsort((cols["m"], cols["j"], cols["i"], cols["l"], cols["logp"]))   # -surprise = logp, ascending
    order = order[:int(top)]
    return {c: v[order] for c, v in cols.items()}


class ReportScores:
    """What `report_scores` returns, held together: per layer the counts (`COUNT_NAMES`: elements, reports, elements with logp =
    -inf, flagged), the sums (`SUM_NAMES`), the histogram of the surprise over `edges` (all elements, by class), the flagged
    elements of every reporter, and the flagged rows.  result: the dict of `CaviEngine.report_scores` or `report_scores_np`."""

    def __init__(self, result, estimate=None, top=None):
        self.counts = np.asarray(result["counts"], dtype=np.int64)
        self.sums = np.asarray(result["sums"], dtype=np.float64)
        self.hist = None if result.get("hist") is None else np.asarray(result["hist"], dtype=np.int64)
        self.edges = None if result.get("edges") is None else np.asarray(result["edges"], dtype=np.float64)
        self.by_reporter = None if result.get("by_reporter") is None else np.asarray(result["by_reporter"], dtype=np.int64)
        self.layers = np.asarray(result.get("layers", np.arange(len(self.counts))), dtype=np.int64)
        self.threshold = result.get("threshold")
        self.select = result.get("select")
        self.estimate, self.top = estimate, top
        self.rows = None
        if result.get("l") is not None:
            self.rows = {c: np.asarray(result[c].cpu().numpy() if type(result[c]).__module__.startswith("torch") else result[c])
                         for c in COLUMNS}

    @property
    def lppd(self):
        """[L'] the in-sample log predictive density of every layer: the sum of logp over its elements with a finite logp."""
        return self.sums[:, 0]

    @property
    def lppd_per_element(self):
        """[L'] `lppd` over the number of elements with a finite logp (`counts[:, 2]` counts the others)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.sums[:, 0] / (self.counts[:, 0] - self.counts[:, 2])

    @property
    def n_flagged(self):
        return int(self.counts[:, 3].sum())

    def __len__(self):
        return 0 if self.rows is None else int(len(self.rows["l"]))

    def frame(self):
        """One row per flagged element, in the order of the rows: layer, source, target, reporter, x, x_mirror, logp, surprise =
        -logp, expected (the mean of the mixture) and residual = x - expected."""
        import pandas as pd
        if self.rows is None:
            raise ValueError("no rows were asked for (rows=False)")
        r = self.rows
        x, expected = np.asarray(r["x"], np.int64), np.asarray(r["mean"], np.float64)
        logp = np.asarray(r["logp"], np.float64)
        return pd.DataFrame({"layer": np.asarray(r["l"], np.int64), "source": np.asarray(r["i"], np.int64),
                             "target": np.asarray(r["j"], np.int64), "reporter": np.asarray(r["m"], np.int64), "x": x,
                             "x_mirror": np.asarray(r["xt"], np.int64), "logp": logp, "surprise": -logp, "expected": expected,
                             "residual": x - expected})

    def reporters(self):
        """One row per (layer, reporter): the flagged reports and omissions of the reporter and their sum."""
        import pandas as pd
        if self.by_reporter is None:
            raise ValueError("the reporters' counts were not asked for (by_reporter=False)")
        Lq, M = self.by_reporter.shape[:2]
        b = self.by_reporter.reshape(Lq * M, 2)
        return pd.DataFrame({"layer": np.repeat(self.layers, M), "reporter": np.tile(np.arange(M), Lq), "flagged_reports": b[:, 0],
                             "flagged_omissions": b[:, 1], "flagged": b.sum(axis=1)})

    def summary(self):
        return {"n": int(self.counts[:, 0].sum()), "n_reports": int(self.counts[:, 1].sum()), "n_inf": int(self.counts[:, 2].sum()),
                "n_flagged": self.n_flagged, "lppd": float(self.lppd.sum()), "threshold": self.threshold, "rows": len(self)}
