"""Result of `VimureModel.posterior_centrality`: the per-node sums the device returns over the posterior samples
(`CaviEngine.sample_centrality`) and what is derived from them on the host.
"""
import numpy as np

from .connectivity import ConnectivityStats

CENT_KEYS = ("node_sum", "node_sumsq", "node_rank_sum", "node_top", "total", "max")


def default_q(N, expected_edges):
    """The passing probability `posterior_centrality` takes when none is given, per layer: min(1, N / expected edges), the
    reciprocal of the expected mean degree -- the value at which a walk's expected offspring is one.  A choice of scale, not the
    1 / lambda_1 of the diffusion-centrality literature (the largest eigenvalue of a sampled network varies from sample to sample
    and is not computed here).  A layer without expected edges takes 1."""
    e = np.asarray(expected_edges, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(e > 0, float(N) / e, 1.0)
    return np.minimum(1.0, q)


class CentralityStats:
    """Diffusion centrality c = sum_{t=1..T} (q M)^t 1 of every node over S posterior samples (sample s is the draw of seed + s),
    per layer l, for A = (Y > 0) without its diagonal and M = A ("out"), A.T ("in") or A | A.T ("union").  Arrays [L, N]:
      mean, sd          the mean and the (population) standard deviation of c over the samples; sd is clipped at 0
      expected_rank     the mean over the samples of rank[v] = #{u : c[u] > c[v]} (0: the most central node)
      top_prob          the share of the samples in which the node is among the top_k: rank < top_k
      plug_in           the centrality of the posterior mean network (`CaviEngine.mean_centrality`), or None: for "out" and "in"
                        with T <= 2 the expectation of c, otherwise only a plug-in
    and [S, L]: total (sum_v c[v]) and max (max_v c[v]) of every sample; values [S, L, N] when asked for, else None.
      top(n, layer)     the n nodes of highest top_prob, ties broken by mean
      frame(node_names) one row per (layer, node);  summary(): mean, std and quantiles of total and max per layer."""

    def __init__(self, N, counts, q, T, direction="out", top_k=10, plug_in=None, seed=None, n_trials=1):
        self.N = int(N)
        self.q = np.atleast_1d(np.asarray(q, dtype=np.float64))
        self.T, self.direction, self.top_k = int(T), direction, int(top_k)
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
        self.plug_in = None if plug_in is None else np.asarray(plug_in, dtype=np.float64)

    def top(self, n=10, layer=0):
        """The n nodes of layer `layer` with the highest top_prob, ties broken by the higher mean (then by the smaller index)."""
        l = int(layer)
        order = np.lexsort((np.arange(self.N), -self.mean[l], -self.top_prob[l]))
        return order[:max(int(n), 0)]

    def frame(self, node_names=None):
        """One row per (layer, node): mean, sd, expected_rank, top_prob and, when it was computed, plug_in.  node_names: N names
        in node order for a `name` column."""
        import pandas as pd
        if node_names is not None and len(node_names) != self.N:
            raise ValueError(f"node_names has {len(node_names)} entries, the network {self.N} nodes")
        cols = {"layer": np.repeat(np.arange(self.L), self.N), "node": np.tile(np.arange(self.N), self.L)}
        if node_names is not None:
            cols["name"] = list(node_names) * self.L
        for k in ("mean", "sd", "expected_rank", "top_prob"):
            cols[k] = getattr(self, k).reshape(-1)
        if self.plug_in is not None:
            cols["plug_in"] = self.plug_in.reshape(-1)
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
