"""Result of `VimureModel.posterior_betweenness`: the per-node sums the device returns over the posterior samples
(`CaviEngine.sample_betweenness`) and what is derived from them on the host.
"""
import numpy as np

from .connectivity import ConnectivityStats

BTW_KEYS = ("node_sum", "node_sumsq", "node_rank_sum", "node_top", "total", "max")


class BetweennessStats:
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

    def __init__(self, N, counts, direction="directed", top_k=10, inferred=None, seed=None, n_trials=1):
        self.N = int(N)
        self.direction, self.top_k = direction, int(top_k)
        self.seed, self.n_trials = seed, int(n_trials)
        self.node_sum = np.asarray(counts["node_sum"], dtype=np.float64)
        self.node_sumsq = np.asarray(counts["node_sumsq"], dtype=np.float64)
        self.node_rank_sum = np.asarray(counts["node_rank_sum"], dtype=np.int64)
        self.node_top = np.asarray(counts["node_top"], dtype=np.int64)
        self.total = np.asarray(counts["total"], dtype=np.float64)
        self.max = np.asarray(counts["max"], dtype=np.float64)
        self.S, self.L = self.total.shape
        v = counts.get("values")
        self.values = None if v is None else np.asarray(v)
        S = float(self.S)
        self.mean = self.node_sum / S
        self.sd = np.sqrt(np.maximum(self.node_sumsq / S - self.mean * self.mean, 0.0))
        self.expected_rank = self.node_rank_sum / S
        self.top_prob = self.node_top / S
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

    def top(self, n=10, layer=0):
        """The n nodes of layer `layer` with the highest top_prob, ties broken by the higher mean (then by the smaller index)."""
        l = int(layer)
        order = np.lexsort((np.arange(self.N), -self.mean[l], -self.top_prob[l]))
        return order[:max(int(n), 0)]

    def frame(self, node_names=None):
        """One row per (layer, node): mean, sd, expected_rank, top_prob and, when it was computed, inferred.  node_names: N names
        in node order for a `name` column."""
        import pandas as pd
        if node_names is not None and len(node_names) != self.N:
            raise ValueError(f"node_names has {len(node_names)} entries, the network {self.N} nodes")
        cols = {"layer": np.repeat(np.arange(self.L), self.N), "node": np.tile(np.arange(self.N), self.L)}
        if node_names is not None:
            cols["name"] = list(node_names) * self.L
        for k in ("mean", "sd", "expected_rank", "top_prob"):
            cols[k] = getattr(self, k).reshape(-1)
        if self.inferred is not None:
            cols["inferred"] = self.inferred.reshape(-1)
        return pd.DataFrame(cols)

    def statistics(self):
        """name -> [S, L] array of every per-sample statistic this result holds."""
        return {"total": self.total, "max": self.max}

    def summary(self, q=(0.025, 0.5, 0.975)):
        """DataFrame with one row per (layer, statistic): mean, std (population) and the quantiles q over the samples."""
        import pandas as pd
        q = tuple(float(x) for x in q)
        rows = []
        for l in range(self.L):
            for name, arr in self.statistics().items():
                row = {"layer": l, "statistic": name}
                row.update(ConnectivityStats._row(arr[:, l], q))
                rows.append(row)
        return pd.DataFrame(rows, columns=["layer", "statistic", "mean", "std"] + ["q%g" % x for x in q])
