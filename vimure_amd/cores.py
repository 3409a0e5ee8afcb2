"""Result of `VimureModel.posterior_cores`: the per-node sums the device returns over the posterior samples
(`CaviEngine.sample_cores`) and what is derived from them on the host.
"""
import numpy as np

from .connectivity import ConnectivityStats

CORE_KEYS = ("node_sum", "node_sumsq", "node_rank_sum", "node_top", "node_main", "node_atleast", "degeneracy", "main_core_size",
             "core_sum", "kcore_size")


class CoreStats:
    """The k-core decomposition of every node over S posterior samples (sample s is the draw of seed + s), per layer l, for A =
    (Y > 0) without its diagonal: core[v] is the largest k such that v lies in a node set whose every node has degree >= k inside
    the set, the degree taken as `mode` says ("union": distinct neighbours in A | A.T, `networkx.core_number` of the undirected
    graph; "total": in plus out, `networkx.core_number` of the DiGraph; "in"; "out").  Arrays [L, N]:
      mean, sd          the mean and the (population) standard deviation of core over the samples; sd is clipped at 0
      expected_rank     the mean over the samples of rank[v] = #{u : core[u] > core[v]} (0: the main core; a shell shares a rank)
      top_prob          the share of the samples with rank < top_k -- whole shells enter together, so more than top_k nodes can
      main_core_prob    the share of the samples in which the node attains the sample's degeneracy
      kcore_prob        the share of the samples in which core >= k_min: the node is in the k_min-core
      inferred          the coreness of the point estimate `get_inferred_model()` returns (`CaviEngine.network_cores`), or None
    and [S, L]: degeneracy (max_v core), main_core_size (the nodes that attain it), kcore_size (#{v : core >= k_min}) and core_sum
    (sum_v core) of every sample; values uint16 [S, L, N] when asked for, else None.
      top(n, layer)            the n nodes of highest main_core_prob, ties broken by mean
      core_members(prob)       bool [L, N]: kcore_prob >= prob, the nodes the posterior puts in the k_min-core
      frame(node_names)        one row per (layer, node);  summary(): mean, std and quantiles of the per-sample numbers per layer."""

    def __init__(self, N, counts, mode="union", k_min=0, top_k=10, inferred=None, seed=None, n_trials=1):
        self.N = int(N)
        self.mode, self.k_min, self.top_k = mode, int(k_min), int(top_k)
        self.seed, self.n_trials = seed, int(n_trials)
        self.node_sum = np.asarray(counts["node_sum"], dtype=np.float64)
        self.node_sumsq = np.asarray(counts["node_sumsq"], dtype=np.float64)
        for k in CORE_KEYS[2:]:
            setattr(self, k, np.asarray(counts[k], dtype=np.int64))
        self.S, self.L = self.degeneracy.shape
        v = counts.get("values")
        self.values = None if v is None else np.asarray(v)
        S = float(self.S)
        self.mean = self.node_sum / S
        self.sd = np.sqrt(np.maximum(self.node_sumsq / S - self.mean * self.mean, 0.0))
        self.expected_rank = self.node_rank_sum / S
        self.top_prob = self.node_top / S
        self.main_core_prob = self.node_main / S
        self.kcore_prob = self.node_atleast / S
        self.inferred = None if inferred is None else np.asarray(inferred, dtype=np.int64)

    def top(self, n=10, layer=0):
        """The n nodes of layer `layer` with the highest main_core_prob, ties broken by the higher mean (then by the smaller
        index)."""
        l = int(layer)
        order = np.lexsort((np.arange(self.N), -self.mean[l], -self.main_core_prob[l]))
        return order[:max(int(n), 0)]

    def core_members(self, prob=0.5):
        """bool [L, N]: the nodes whose coreness is >= k_min in at least the share `prob` of the samples."""
        return self.kcore_prob >= float(prob)

    def frame(self, node_names=None):
        """One row per (layer, node): mean, sd, expected_rank, top_prob, main_core_prob, kcore_prob and, when it was computed,
        inferred.  node_names: N names in node order for a `name` column."""
        import pandas as pd
        if node_names is not None and len(node_names) != self.N:
            raise ValueError(f"node_names has {len(node_names)} entries, the network {self.N} nodes")
        cols = {"layer": np.repeat(np.arange(self.L), self.N), "node": np.tile(np.arange(self.N), self.L)}
        if node_names is not None:
            cols["name"] = list(node_names) * self.L
        for k in ("mean", "sd", "expected_rank", "top_prob", "main_core_prob", "kcore_prob"):
            cols[k] = getattr(self, k).reshape(-1)
        if self.inferred is not None:
            cols["inferred"] = self.inferred.reshape(-1)
        return pd.DataFrame(cols)

    def statistics(self):
        """name -> [S, L] array of every per-sample statistic this result holds."""
        return {"degeneracy": self.degeneracy, "main_core_size": self.main_core_size, "kcore_size": self.kcore_size,
                "core_sum": self.core_sum}

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
