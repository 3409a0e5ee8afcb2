"""Result of `VimureModel.posterior_network_stats`: the counts the device returns per posterior sample and layer
(`CaviEngine.sample_stats`, and `CaviEngine.sample_triads` when triads were asked for), the analytic expectations
(`CaviEngine.expected_stats`, `CaviEngine.expected_triads`), and what is derived from them on the host.
"""
import numpy as np

_EXPECTED_KEYS = ("edges", "weight", "mutual", "edges_var")
TRIAD_KEYS = ("transitive", "cyclic", "two_paths", "triangles_u", "wedges_u", "edges_u")
_TRIAD_RATIOS = ("transitivity_directed", "cyclicity", "transitivity")


def _ratio(a, b):
    """a / b elementwise in float64, NaN where b is 0."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.full(np.broadcast(a, b).shape, np.nan)
    np.divide(a, b, out=out, where=b != 0)
    return out


def _nanmean_last(a):
    """Mean over the last axis leaving NaN out; NaN where every entry is NaN (no warning)."""
    ok = ~np.isnan(a)
    return _ratio(np.where(ok, a, 0.0).sum(-1), ok.sum(-1))


class NetworkStats:
    """Per sample s and layer l (arrays [S, L]; sample s is the draw of seed + s):
      edges, weight, mutual, tp   the raw integer counts over all (i, j), the diagonal included (tp: zeros without Y_true)
      reciprocity                 mutual / weight (`utils.calculate_overall_reciprocity` of the sample; NaN where weight is 0)
      density                     edges / N^2
      precision, recall, f1       with Y_true: tp / edges, tp / ref_edges, 2 tp / (edges + ref_edges); NaN where undefined
      deg_out, deg_in             int32 [S, L, N] when asked for
    ref_edges [L]: (Y_true > 0).sum() per layer.  expected: dict of float64 [L] arrays -- `edges`, `weight`, `mutual`,
    `edges_var` (`CaviEngine.expected_stats`) and `expected_reciprocity` = mutual / edges.

    With triads (`CaviEngine.sample_triads`: A = (Y > 0) without its diagonal, U = A | A.T; None otherwise):
      transitive, cyclic, two_paths, triangles_u, wedges_u, edges_u   the integer counts
      transitivity_directed       transitive / two_paths
      cyclicity                   cyclic / two_paths
      transitivity                3 triangles_u / wedges_u        (NaN where the denominator is 0)
      node_tri, node_deg          int32 [S, L, N] when asked for: triangles of U through a node, its degree d in U
      local_clustering            [S, L, N] 2 node_tri / (d (d - 1)), NaN where d < 2; avg_clustering [S, L] its mean over the
                                  nodes where it is defined
    and `expected` gains `exp_<count>` (`CaviEngine.expected_triads`): expectations of the counts -- a ratio of them is not the
    expectation of the ratio."""

    def __init__(self, N, counts, expected=None, ref_edges=None, seed=None, n_trials=1, triads=None, expected_triads=None):
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
        for k in TRIAD_KEYS + _TRIAD_RATIOS + ("node_tri", "node_deg", "local_clustering", "avg_clustering"):
            setattr(self, k, None)
        self.has_triads = triads is not None
        if self.has_triads:
            for k in TRIAD_KEYS:
                setattr(self, k, np.asarray(triads[k], dtype=np.int64))
            self.transitivity_directed = _ratio(self.transitive, self.two_paths)
            self.cyclicity = _ratio(self.cyclic, self.two_paths)
            self.transitivity = _ratio(3 * self.triangles_u, self.wedges_u)
            self.node_tri, self.node_deg = triads.get("node_tri"), triads.get("node_deg")
            if self.node_tri is not None and self.node_deg is not None:
                d = np.asarray(self.node_deg, dtype=np.int64)
                self.local_clustering = _ratio(2 * np.asarray(self.node_tri, dtype=np.int64), d * (d - 1))
                self.avg_clustering = _nanmean_last(self.local_clustering)
            if expected_triads is not None:
                if self.expected is None:
                    self.expected = {}
                for k in TRIAD_KEYS:
                    self.expected["exp_" + k] = np.asarray(expected_triads[k], dtype=np.float64)

    def statistics(self):
        """name -> [S, L] array of every per-sample statistic this result holds."""
        out = {k: getattr(self, k) for k in ("edges", "weight", "mutual", "reciprocity", "density")}
        if self.ref_edges is not None:
            out.update({k: getattr(self, k) for k in ("tp", "precision", "recall", "f1")})
        if self.has_triads:
            out.update({k: getattr(self, k) for k in TRIAD_KEYS + _TRIAD_RATIOS})
            if self.avg_clustering is not None:
                out["avg_clustering"] = self.avg_clustering
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
