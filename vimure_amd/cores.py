"""Result of `VimureModel.posterior_cores`: the per-node sums the device returns over the posterior samples
(`CaviEngine.sample_cores`) and what is derived from them on the host.
"""
import numpy as np

from .node_scores import NodeScoreStats

CORE_KEYS = ("node_sum", "node_sumsq", "node_rank_sum", "node_top", "node_main", "node_atleast", "degeneracy", "main_core_size",
             "core_sum", "kcore_size")


class CoreStats(NodeScoreStats):
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

    stat_keys = ("degeneracy", "main_core_size", "kcore_size", "core_sum")
    stat_dtype = np.int64

    def __init__(self, N, counts, mode="union", k_min=0, top_k=10, inferred=None, seed=None, n_trials=1):
        super().__init__(N, counts, top_k, seed, n_trials)
        self.mode, self.k_min = mode, int(k_min)
        self.node_main = np.asarray(counts["node_main"], dtype=np.int64)
        self.node_atleast = np.asarray(counts["node_atleast"], dtype=np.int64)
        self.main_core_prob = self.node_main / float(self.S)
        self.kcore_prob = self.node_atleast / float(self.S)
        self.inferred = None if inferred is None else np.asarray(inferred, dtype=np.int64)

    def top(self, n=10, layer=0):
        """The n nodes of layer `layer` with the highest main_core_prob, ties broken by the higher mean (then by the smaller
        index)."""
        return super().top(n, layer, key="main_core_prob")

    def core_members(self, prob=0.5):
        """bool [L, N]: the nodes whose coreness is >= k_min in at least the share `prob` of the samples."""
        return self.kcore_prob >= float(prob)

    def frame(self, node_names=None):
        """One row per (layer, node): mean, sd, expected_rank, top_prob, main_core_prob, kcore_prob and, when it was computed,
        inferred.  node_names: N names in node order for a `name` column."""
        return super().frame(node_names, columns=("mean", "sd", "expected_rank", "top_prob", "main_core_prob", "kcore_prob"), extra="inferred")
