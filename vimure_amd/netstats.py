"""Result of `VimureModel.posterior_network_stats`: the counts the device returns per posterior sample and layer
(`CaviEngine.sample_stats`), the analytic expectations (`CaviEngine.expected_stats`), and what is derived from them on the host.
"""
import numpy as np

_EXPECTED_KEYS = ("edges", "weight", "mutual", "edges_var")


def _ratio(a, b):
    """a / b elementwise in float64, NaN where b is 0."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.full(np.broadcast(a, b).shape, np.nan)
    np.divide(a, b, out=out, where=b != 0)
    return out


class NetworkStats:
    """Per sample s and layer l (arrays [S, L]; sample s is the draw of seed + s):
      edges, weight, mutual, tp   the raw integer counts over all (i, j), the diagonal included (tp: zeros without Y_true)
      reciprocity                 mutual / weight (`utils.calculate_overall_reciprocity` of the sample; NaN where weight is 0)
      density                     edges / N^2
      precision, recall, f1       with Y_true: tp / edges, tp / ref_edges, 2 tp / (edges + ref_edges); NaN where undefined
      deg_out, deg_in             int32 [S, L, N] when asked for
    ref_edges [L]: (Y_true > 0).sum() per layer.  expected: dict of float64 [L] arrays -- `edges`, `weight`, `mutual`,
    `edges_var` (`CaviEngine.expected_stats`) and `expected_reciprocity` = mutual / edges."""

    def __init__(self, N, counts, expected=None, ref_edges=None, seed=None, n_trials=1):
        self.N = int(N)
        self.seed, self.n_trials = seed, int(n_trials)
        for k in ("edges", "weight", "mutual", "tp"):
            setattr(self, k, np.asarray(counts[k], dtype=np.int64))
        self.deg_out, self.deg_in = counts.get("deg_out"), counts.get("deg_in")
        self.S, self.L = self.edges.shape
        self.reciprocity = _ratio(self.mutual, self.weight)
        self.density = self.edges / float(self.N * self.N)
        self.ref_edges = None
        self.precision = self.recall = self.f1 = None
        if ref_edges is not None:
            self.ref_edges = np.asarray(ref_edges, dtype=np.int64).reshape(self.L)
            self.precision = _ratio(self.tp, self.edges)
            self.recall = _ratio(self.tp, np.broadcast_to(self.ref_edges, self.tp.shape))
            self.f1 = _ratio(2 * self.tp, self.edges + self.ref_edges[None, :])
        self.expected = None
        if expected is not None:
            self.expected = {k: np.asarray(expected[k], dtype=np.float64) for k in _EXPECTED_KEYS}
            self.expected["expected_reciprocity"] = _ratio(self.expected["mutual"], self.expected["edges"])

    def statistics(self):
        """name -> [S, L] array of every per-sample statistic this result holds."""
        out = {k: getattr(self, k) for k in ("edges", "weight", "mutual", "reciprocity", "density")}
        if self.ref_edges is not None:
            out.update({k: getattr(self, k) for k in ("tp", "precision", "recall", "f1")})
        return out

    def summary(self, q=(0.025, 0.5, 0.975)):
        """DataFrame with one row per (layer, statistic): mean, std (population) and the quantiles q over the samples (NaN
        samples left out)."""
        import pandas as pd
        q = tuple(float(x) for x in q)
        rows = []
        for l in range(self.L):
            for name, arr in self.statistics().items():
                v = np.asarray(arr[:, l], dtype=np.float64)
                v = v[~np.isnan(v)]
                row = {"layer": l, "statistic": name, "mean": v.mean() if v.size else np.nan, "std": v.std() if v.size else np.nan}
                qs = np.quantile(v, q) if v.size else np.full(len(q), np.nan)
                row.update({"q%g" % x: float(y) for x, y in zip(q, qs)})
                rows.append(row)
        return pd.DataFrame(rows, columns=["layer", "statistic", "mean", "std"] + ["q%g" % x for x in q])
