"""The reporter table: each reporter's reports against the posterior -- the host side of `VimureModel.reporter_table`.

VIMuRe exists to say which reporters are reliable; after theta, three things are asked of every reporter: how many of their
reports fall on ties the model believes in, how many inferred ties within their scope they left out, and how their report total
compares with what the model expects of them.  `reporter_table_np` restates vmr_reporter_table (include/vimure_hip.h) from dense
arrays, element by element -- the yardstick of the device pass; `ReporterTable` holds the two arrays either of them returns and
derives the columns a user reads; `sum_quanta` restates the fixed point the device accumulates its sums in.
"""
import math

import numpy as np

from .netstats import _ratio

COUNT_NAMES = ("n_scope", "n_rep", "total", "n_inferred", "hits", "mutual", "n_out")
SUM_NAMES = ("exp_ties", "exp_hits", "exp_total")
METHODS = ("rho_max", "threshold")


def tie_readout_np(rho, method="rho_max", threshold=None):
    """(y, prob), each [L,N,N]: the byte `CaviEngine.readout(method, threshold)` gives a tie -- the first maximum of rho, or
    rho_1 >= threshold -- and prob = sum_{k>=1} rho_k added in ascending k (np.sum adds in another order)."""
    rho = np.asarray(rho, dtype=np.float64)
    if method not in METHODS:
        raise ValueError("method must be \"rho_max\" or \"threshold\"")
    if method == "threshold":
        if threshold is None:
            raise ValueError("method=\"threshold\" needs a threshold")
        y = (rho[..., 1] >= float(threshold)).astype(np.int64)
    else:
        y = np.argmax(rho, axis=-1).astype(np.int64)
    prob = np.zeros(rho.shape[:-1])
    for k in range(1, rho.shape[-1]):
        prob = prob + rho[..., k]
    return y, prob


def mean_poisson_np(X, rho, g_theta, g_lambda, g_nu, mutuality):
    """The dense [L,N,N,M] array of vmr_mean_poisson's values, R ignored: sum_k rho_k (G_theta[l,m] G_lambda[l,k] + G_nu X^T),
    k ascending, X^T = X[l,j,i,m] with mutuality, else 0."""
    X, rho = np.asarray(X), np.asarray(rho, dtype=np.float64)
    g_theta, g_lambda = np.asarray(g_theta, dtype=np.float64), np.asarray(g_lambda, dtype=np.float64)
    XT = np.transpose(X, (0, 2, 1, 3)).astype(np.float64) if mutuality else np.zeros(X.shape)
    nx = float(g_nu) * XT
    mp = np.zeros(X.shape)
    for k in range(rho.shape[-1]):
        mp = mp + rho[..., k][..., None] * (g_theta[:, None, None, :] * g_lambda[:, k][:, None, None, None] + nx)
    return mp


def _msum(a, mask):
    """sum of a over mask along (i, j), per (l, m), accumulated in extended precision: the yardstick's own error stays far below
    one ulp of the result."""
    return np.sum(np.where(mask, a, 0.0), axis=(1, 2), dtype=np.longdouble).astype(np.float64)


def reporter_table_np(X, R, rho, g_theta, g_lambda, g_nu, mutuality, method="rho_max", threshold=None):
    """vmr_reporter_table in NumPy, from its definitions.  X [L,N,N,M] counts, R the same shape or None (every reporter on every
    tie, the diagonal included), rho [L,N,N,K], g_theta [L,M], g_lambda [L,K], g_nu.  Returns {"counts": int64 [L,M,7]
    (`COUNT_NAMES`), "sums": float64 [L,M,3] (`SUM_NAMES`)}."""
    X = np.asarray(X)
    rho = np.asarray(rho, dtype=np.float64)
    if X.ndim != 4 or X.shape[1] != X.shape[2]:
        raise ValueError("X must have shape (L, N, N, M)")
    if rho.ndim != 4 or rho.shape[:3] != X.shape[:3] or rho.shape[3] < 2:
        raise ValueError("rho must have shape (L, N, N, K)")
    if R is not None and np.asarray(R).shape != X.shape:
        raise ValueError("Dimensions of reporter mask (R) do not match L x N x N x M")
    L, N, _, M = X.shape
    S = np.ones(X.shape, bool) if R is None else np.asarray(R) != 0
    y, prob = tie_readout_np(rho, method, threshold)
    mp = mean_poisson_np(X, rho, g_theta, g_lambda, g_nu, mutuality)
    xi = X.astype(np.int64)
    pos = xi > 0
    inf = (y > 0)[..., None]
    offdiag = ~np.eye(N, dtype=bool)[None, :, :, None]
    ST, posT = np.transpose(S, (0, 2, 1, 3)), np.transpose(pos, (0, 2, 1, 3))
    counts = np.zeros((L, M, len(COUNT_NAMES)), np.int64)
    counts[..., 0] = S.sum(axis=(1, 2))
    counts[..., 1] = (S & pos).sum(axis=(1, 2))
    counts[..., 2] = np.where(S, xi, 0).sum(axis=(1, 2))
    counts[..., 3] = (S & inf).sum(axis=(1, 2))
    counts[..., 4] = (S & pos & inf).sum(axis=(1, 2))
    counts[..., 5] = (S & pos & ST & posT & offdiag).sum(axis=(1, 2))
    counts[..., 6] = (~S & pos).sum(axis=(1, 2))
    sums = np.zeros((L, M, len(SUM_NAMES)))
    pb = np.broadcast_to(prob[..., None], X.shape)
    sums[..., 0] = _msum(pb, S)
    sums[..., 1] = _msum(pb, S & pos)
    sums[..., 2] = _msum(mp, S)
    if np.isnan(sums).any():
        raise ValueError("reporter_table: a sum is NaN")
    return {"counts": counts, "sums": sums}


def sum_quanta(N, g_theta, g_lambda, g_nu, sum_x, mutuality=True):
    """The fixed point of vmr_reporter_table's sums, as include/vimure_hip.h states it: float64 [L, M, 3], the quantum q a term
    of each sum is rounded to.  With b = ceil(log2 N^2), max G_lambda < 2^e_l and sum X < 2^e_x:  exp_ties and exp_hits
    2^-(61 - b);  exp_total g_theta[l,m] 2^-(61 - b - e_l) + g_nu 2^-(61 - e_x) (the second part with mutuality only).  A sum of
    n terms is within n q / 2 of the exact sum of its terms."""
    g_theta, g_lambda = np.asarray(g_theta, dtype=np.float64), np.asarray(g_lambda, dtype=np.float64)
    T = int(N) * int(N)
    b = 0
    while (1 << b) < T:
        b += 1
    gmax = float(g_lambda.max())
    e_l = max(math.frexp(gmax)[1], -900) if gmax > 0 else -900
    e_x = math.frexp(float(sum_x) + 1.0)[1]
    q = np.zeros(g_theta.shape + (3,))
    q[..., 0] = q[..., 1] = math.ldexp(1.0, -(61 - b))
    q[..., 2] = g_theta * math.ldexp(1.0, -(61 - b - e_l)) + (float(g_nu) * math.ldexp(1.0, -(61 - e_x)) if mutuality else 0.0)
    return q


class ReporterTable:
    """What `reporter_table` returns, per layer l and reporter m (see vmr_reporter_table).  With S_m the ties reporter m may
    report on (R != 0), x their count on a tie, y > 0 an inferred tie and prob its posterior probability:
      n_scope #S_m; n_rep #{S_m : x > 0}; total sum x; n_inferred #{S_m : y > 0}; hits #{S_m : x > 0, y > 0}; mutual: reciprocated
      reports (ordered); n_out: reports outside S_m, which the mask discards; exp_ties sum prob; exp_hits sum_{x > 0} prob;
      exp_total the sum of the expected reports (`calculate_mean_poisson`'s values) over S_m.
    Derived, float64 [L, M], NaN where a denominator is 0:
      false_reports = n_rep - hits   (reports on ties the model does not infer)
      omissions     = n_inferred - hits   (inferred ties within scope left unreported)
      precision = hits / n_rep;  recall = hits / n_inferred;  residual = total - exp_total;  ratio = total / exp_total
    result: the dict of `CaviEngine.reporter_table` or `reporter_table_np`.  layers: the layer index of every row of the arrays
    (default 0..L-1).  theta, theta_mean, theta_interval ([L, M, 2]): what `VimureModel.reporter_table` puts beside the table."""

    def __init__(self, result, layers=None, theta=None, theta_mean=None, theta_interval=None, method="rho_max", threshold=None):
        self.counts = np.asarray(result["counts"], dtype=np.int64)
        self.sums = np.asarray(result["sums"], dtype=np.float64)
        if self.counts.ndim != 3 or self.counts.shape[2] != len(COUNT_NAMES) or self.sums.shape != self.counts.shape[:2] + (len(SUM_NAMES),):
            raise ValueError("counts [L, M, 7] and sums [L, M, 3] expected")
        self.layers = np.arange(self.counts.shape[0]) if layers is None else np.asarray(layers, dtype=np.int64)
        self.theta = None if theta is None else np.asarray(theta, dtype=np.float64)
        self.theta_mean = None if theta_mean is None else np.asarray(theta_mean, dtype=np.float64)
        self.theta_interval = None if theta_interval is None else np.asarray(theta_interval, dtype=np.float64)
        self.method, self.threshold = method, threshold

    def __getattr__(self, name):
        if name in COUNT_NAMES:
            return self.counts[..., COUNT_NAMES.index(name)]
        if name in SUM_NAMES:
            return self.sums[..., SUM_NAMES.index(name)]
        raise AttributeError(name)

    @property
    def false_reports(self):
        return self.n_rep - self.hits

    @property
    def omissions(self):
        return self.n_inferred - self.hits

    @property
    def precision(self):
        return _ratio(self.hits, self.n_rep)

    @property
    def recall(self):
        return _ratio(self.hits, self.n_inferred)

    @property
    def residual(self):
        return self.total - self.exp_total

    @property
    def ratio(self):
        return _ratio(self.total, self.exp_total)

    def frame(self):
        """A pandas DataFrame, one row per (layer, reporter): the counts, the sums, the derived columns and, when given, theta."""
        import pandas as pd
        Lq, M = self.counts.shape[:2]
        cols = {"layer": np.repeat(self.layers, M), "reporter": np.tile(np.arange(M), Lq)}
        for n in COUNT_NAMES + SUM_NAMES + ("false_reports", "omissions", "precision", "recall", "residual", "ratio"):
            cols[n] = np.asarray(getattr(self, n)).reshape(-1)
        for n in ("theta", "theta_mean"):
            if getattr(self, n) is not None:
                cols[n] = getattr(self, n).reshape(-1)
        if self.theta_interval is not None:
            cols["theta_lo"], cols["theta_hi"] = self.theta_interval[..., 0].reshape(-1), self.theta_interval[..., 1].reshape(-1)
        return pd.DataFrame(cols)
