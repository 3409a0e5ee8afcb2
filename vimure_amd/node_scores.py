"""What the results that score every node over the posterior samples share (`centrality.CentralityStats`,
`betweenness.BetweennessStats`, `cores.CoreStats`): the per-node sums of the device's node-score fold and what is derived from
them, `top()`, `frame()`, `statistics()` and `summary()`; and the row of `summary()` every sampled result uses.
"""
import numpy as np


def quantile_row(v, q):
    """mean, std (population) and the quantiles q of the samples v, NaN samples left out: {"mean", "std", "q<x>", ..}."""
    v = np.asarray(v, dtype=np.float64)
    v = v[~np.isnan(v)]
    row = {"mean": v.mean() if v.size else np.nan, "std": v.std() if v.size else np.nan}
    qs = np.quantile(v, q) if v.size else np.full(len(q), np.nan)
    row.update({"q%g" % x: float(y) for x, y in zip(q, qs)})
    return row


class NodeScoreStats:
    """A score of every node over S posterior samples, from the sums the device folds: node_sum, node_sumsq (float64 [L, N]),
    node_rank_sum, node_top (int64 [L, N]) and from them mean, sd (population, clipped at 0), expected_rank and top_prob; values
    [S, L, N] when the counts hold them, else None.  A subclass names its per-sample statistics in `stat_keys` ([S, L] arrays of
    `counts`, set as attributes in the order `statistics()` gives them; the first gives S and L) and passes `top()` and `frame()`
    what is its own."""

    stat_keys = ()
    stat_dtype = np.float64

    def __init__(self, N, counts, top_k, seed, n_trials):
        self.N, self.top_k = int(N), int(top_k)
        self.seed, self.n_trials = seed, int(n_trials)
        self.node_sum = np.asarray(counts["node_sum"], dtype=np.float64)
        self.node_sumsq = np.asarray(counts["node_sumsq"], dtype=np.float64)
        self.node_rank_sum = np.asarray(counts["node_rank_sum"], dtype=np.int64)
        self.node_top = np.asarray(counts["node_top"], dtype=np.int64)
        for k in self.stat_keys:
            setattr(self, k, np.asarray(counts[k], dtype=self.stat_dtype))
        self.S, self.L = getattr(self, self.stat_keys[0]).shape
        v = counts.get("values")
        self.values = None if v is None else np.asarray(v)
        S = float(self.S)
        self.mean = self.node_sum / S
        self.sd = np.sqrt(np.maximum(self.node_sumsq / S - self.mean * self.mean, 0.0))
        self.expected_rank = self.node_rank_sum / S
        self.top_prob = self.node_top / S

    def top(self, n=10, layer=0, key="top_prob"):
        """The n nodes of layer `layer` with the highest `key` (an [L, N] attribute), ties broken by the higher mean (then by the
        smaller index)."""
        l = int(layer)
        order = np.lexsort((np.arange(self.N), -self.mean[l], -getattr(self, key)[l]))
        return order[:max(int(n), 0)]

    def frame(self, node_names=None, columns=("mean", "sd", "expected_rank", "top_prob"), extra=None):
        """One row per (layer, node): `columns` and, when it was computed (is not None), the attribute `extra`.  node_names: N
        names in node order for a `name` column."""
        import pandas as pd
        if node_names is not None and len(node_names) != self.N:
            raise ValueError(f"node_names has {len(node_names)} entries, the network {self.N} nodes")
        cols = {"layer": np.repeat(np.arange(self.L), self.N), "node": np.tile(np.arange(self.N), self.L)}
        if node_names is not None:
            cols["name"] = list(node_names) * self.L
        for k in columns:
            cols[k] = getattr(self, k).reshape(-1)
        if extra is not None and getattr(self, extra) is not None:
            cols[extra] = getattr(self, extra).reshape(-1)
        return pd.DataFrame(cols)

    def statistics(self):
        """name -> [S, L] array of every per-sample statistic this result holds."""
        return {k: getattr(self, k) for k in self.stat_keys}

    def summary(self, q=(0.025, 0.5, 0.975)):
        """DataFrame with one row per (layer, statistic): mean, std (population) and the quantiles q over the samples."""
        import pandas as pd
        q = tuple(float(x) for x in q)
        rows = []
        for l in range(self.L):
            for name, arr in self.statistics().items():
                row = {"layer": l, "statistic": name}
                row.update(quantile_row(arr[:, l], q))
                rows.append(row)
        return pd.DataFrame(rows, columns=["layer", "statistic", "mean", "std"] + ["q%g" % x for x in q])
