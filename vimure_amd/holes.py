"""Result of `VimureModel.posterior_structural_holes`: the per-node sums the device returns over the posterior samples
(`CaviEngine.sample_structural_holes`) and what is derived from them on the host.
"""
import numpy as np

from .node_scores import NodeScoreStats

HOLES_KEYS = ("node_sum", "node_sumsq", "node_rank_sum", "node_top", "node_defined", "n_defined", "effective_size_sum", "constraint_sum")
MEASURES = ("effective_size", "constraint")   # the order of the leading axis of the device's accumulators


class HolesMeasure(NodeScoreStats):
    """One of the two measures over S posterior samples, per layer l; arrays [L, N]:
      mean, sd          over the samples in which the node is DEFINED (has a tie): node_sum / node_defined and the (population)
                        standard deviation with the same counts, clipped at 0; NaN where the node is isolated in every sample
      expected_rank     the mean over all samples of the node's rank among the defined nodes (0: the first broker -- the largest
                        effective size, the smallest constraint; an undefined node ranks behind every defined one)
      top_prob          the share of all samples with rank < top_k
      defined_prob      node_defined / S
    values [S, L, N] (NaN where undefined) when they were asked for, else None; `top()`, `frame()` as `NodeScoreStats` has them."""

    stat_keys = ("n_defined",)

    def __init__(self, N, counts, top_k, seed, n_trials):
        super().__init__(N, counts, top_k, seed, n_trials)
        self.node_defined = np.asarray(counts["node_defined"], dtype=np.int64)
        nd = np.where(self.node_defined > 0, self.node_defined, 1).astype(np.float64)
        some = self.node_defined > 0
        self.mean = np.where(some, self.node_sum / nd, np.nan)
        self.sd = np.where(some, np.sqrt(np.maximum(self.node_sumsq / nd - (self.node_sum / nd) ** 2, 0.0)), np.nan)
        self.defined_prob = self.node_defined / float(self.S)

    def top(self, n=10, layer=0, key="top_prob"):
        """The n nodes of layer `layer` with the highest `key`, ties broken by the smaller expected rank (then by the smaller
        index)."""
        l = int(layer)
        order = np.lexsort((np.arange(self.N), self.expected_rank[l], -getattr(self, key)[l]))
        return order[:max(int(n), 0)]

    def frame(self, node_names=None):
        """One row per (layer, node): mean, sd, expected_rank, top_prob, defined_prob."""
        return super().frame(node_names, columns=("mean", "sd", "expected_rank", "top_prob", "defined_prob"))


class StructuralHoles:
    """Burt's structural holes of every node over S posterior samples (sample s is the draw of seed + s), per layer, for A = (Y >
    0) without its diagonal and U = A | A.T.  mode "union": the weights z = U (`networkx.effective_size` / `constraint` of the
    undirected graph); "weighted": z = A + A.T (networkx on the DiGraph, but defined for every node with a tie).
      effective_size, constraint   two `HolesMeasure` views: mean, sd, expected_rank, top_prob, defined_prob, values, top(), frame()
      defined_prob                 float64 [L, N]: the share of the samples in which the node has a tie
      n_defined, effective_size_sum, constraint_sum   float64 [S, L]: per sample the defined nodes and the two sums over them
      inferred                     the measures of the point estimate `get_inferred_model()` (`CaviEngine.network_structural_holes`),
                                   a dict of [L, N] arrays, or None
      degree, strength, redundancy   [S, L, N] when values were asked for, else None
      efficiency()                 ES / d of every sample [S, L, N] when values were asked for, else None
      brokers(n, layer)            the n nodes most often among the top_k least constrained
      frame(node_names)            one row per (layer, node), both measures side by side;  summary(): mean, std and quantiles of the
                                   three per-sample numbers per layer."""

    def __init__(self, N, counts, mode="union", top_k=10, inferred=None, seed=None, n_trials=1):
        self.N, self.mode, self.top_k = int(N), mode, int(top_k)
        self.seed, self.n_trials = seed, int(n_trials)
        views = []
        for q, name in enumerate(MEASURES):
            part = {k: np.asarray(counts[k])[q] for k in ("node_sum", "node_sumsq", "node_rank_sum", "node_top")}
            part.update(node_defined=counts["node_defined"], n_defined=counts["n_defined"], values=counts.get(name))
            views.append(HolesMeasure(N, part, top_k, seed, n_trials))
        self.effective_size, self.constraint = views
        self.S, self.L = self.effective_size.S, self.effective_size.L
        self.node_defined = self.effective_size.node_defined
        self.defined_prob = self.effective_size.defined_prob
        for k in ("n_defined", "effective_size_sum", "constraint_sum"):
            setattr(self, k, np.asarray(counts[k], dtype=np.float64))
        for k in ("degree", "strength", "redundancy"):
            setattr(self, k, None if counts.get(k) is None else np.asarray(counts[k]))
        self.inferred = inferred

    def efficiency(self):
        """ES / d of every sample, float64 [S, L, N] (NaN where the node is isolated), or None without values."""
        if self.effective_size.values is None or self.degree is None:
            return None
        d = self.degree.astype(np.float64)
        return np.where(d > 0, self.effective_size.values / np.where(d > 0, d, 1.0), np.nan)

    def brokers(self, n=10, layer=0):
        """The n nodes of layer `layer` most often among the top_k least constrained, ties broken by the smaller expected rank."""
        return self.constraint.top(n, layer)

    def statistics(self):
        """name -> [S, L] array of the three per-sample statistics."""
        return {k: getattr(self, k) for k in ("n_defined", "effective_size_sum", "constraint_sum")}

    def frame(self, node_names=None):
        """One row per (layer, node): defined_prob, then mean, sd, expected_rank and top_prob of each measure under its name's
        prefix and, when it was computed, the point estimate's two measures."""
        f = self.effective_size.frame(node_names)[["layer", "node"] + (["name"] if node_names is not None else []) + ["defined_prob"]]
        for name, view in zip(MEASURES, (self.effective_size, self.constraint)):
            for k in ("mean", "sd", "expected_rank", "top_prob"):
                f[name + "_" + k] = getattr(view, k).reshape(-1)
            if self.inferred is not None:
                f[name + "_inferred"] = np.asarray(self.inferred[name]).reshape(-1)
        return f

    def summary(self, q=(0.025, 0.5, 0.975)):
        """DataFrame with one row per (layer, statistic): mean, std (population) and the quantiles q over the samples."""
        import pandas as pd
        from .node_scores import quantile_row
        q = tuple(float(x) for x in q)
        rows = []
        for l in range(self.L):
            for name, arr in self.statistics().items():
                row = {"layer": l, "statistic": name}
                row.update(quantile_row(arr[:, l], q))
                rows.append(row)
        return pd.DataFrame(rows, columns=["layer", "statistic", "mean", "std"] + ["q%g" % x for x in q])
