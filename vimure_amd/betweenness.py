"""Result of `VimureModel.posterior_betweenness`: the per-node sums the device returns over the posterior samples
(`CaviEngine.sample_betweenness`) and what is derived from them on the host.
"""
import numpy as np

from .node_scores import NodeScoreStats

BTW_KEYS = ("node_sum", "node_sumsq", "node_rank_sum", "node_top", "total", "max")


class BetweennessStats(NodeScoreStats):
    """Betweenness centrality b[v] = sum over s != v != t of the share of the shortest s -> t paths through v (unnormalised,
    endpoints excluded: `networkx.betweenness_centrality(normalized=False)`) of every node over S posterior samples (sample s is
    the draw of seed + s), per layer l, for A = (Y > 0) without its diagonal searched as it is ("directed") or as A | A.T
    ("union", every unordered pair once).  Arrays [L, N]:
      mean, sd          the mean and the (population) standard deviation of b over the samples; sd is clipped at 0
      expected_rank     the mean over the samples of rank[v] = #{u : b[u] > b[v]} (0: the first broker)
      top_prob          the share of the samples in which the node is among the top_k: rank < top_k
      inferred          the betweenness of the point estimate `get_inferred_model()` returns (`CaviEngine.network_betweenness`),
                        or None.  Not a mean-network plug-in -- shortest paths of a network of probabilities mean nothing -- and
                        not the posterior mean of b: one invented tie reroutes thousands of paths
    and [S, L]: total (sum_v b[v]) and max (max_v b[v]) of every sample; values [S, L, N] when asked for, else None.
      normalized()      (mean, sd, inferred) divided by (N - 1)(N - 2) for "directed" and by half of that for "union"
      top(n, layer)     the n nodes of highest top_prob, ties broken by mean
      frame(node_names) one row per (layer, node);  summary(): mean, std and quantiles of total and max per layer."""

    stat_keys = ("total", "max")

    def __init__(self, N, counts, direction="directed", top_k=10, inferred=None, seed=None, n_trials=1):
        super().__init__(N, counts, top_k, seed, n_trials)
        self.direction = direction
        self.inferred = None if inferred is None else np.asarray(inferred, dtype=np.float64)

    @property
    def scale(self):
        """The number of pairs a node can lie between: (N - 1)(N - 2) ordered ("directed"), half of it unordered ("union")."""
        pairs = float((self.N - 1) * (self.N - 2))
        return pairs if self.direction in ("directed", 0) else pairs / 2.0

    def normalized(self):
        """dict: mean, sd and inferred (None when it was not computed) divided by `scale`, so that 1 is a node every shortest
        path between others passes through; NaN when N < 3."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return {"mean": self.mean / self.scale, "sd": self.sd / self.scale,
                    "inferred": None if self.inferred is None else self.inferred / self.scale}

    def frame(self, node_names=None):
        """One row per (layer, node): mean, sd, expected_rank, top_prob and, when it was computed, inferred.  node_names: N names
        in node order for a `name` column."""
        return super().frame(node_names, extra="inferred")
