"""Result of `VimureModel.posterior_cutpoints`: the per-node sums the device returns over the posterior samples
(`CaviEngine.sample_cutpoints`) and what is derived from them on the host.
"""
import numpy as np

from .node_scores import NodeScoreStats

CUT_KEYS = ("node_sum", "node_sumsq", "node_rank_sum", "node_top", "node_cut", "node_branch_sum", "node_bridge_sum", "n_cut", "n_bridges",
            "max_pairs_cut", "connected_pairs")
CUT_VALUES = ("pairs_cut", "branches", "bridges")


class CutpointStats(NodeScoreStats):
    """Who holds the network together, over S posterior samples (sample s is the draw of seed + s), per layer l, for A = (Y > 0)
    without its diagonal and the undirected graph G = A | A.T (`mode` "union") or A & A.T ("mutual").  The branches of node v are
    the components of v's component once v is taken out, of sizes s_1..s_b; v is a cut point iff b >= 2; pairs_cut[v] = sum_{i<j}
    s_i s_j is the number of pairs of other nodes that lose every path with v (Borgatti's key-player fragmentation, as a count);
    bridges[v] the ties of v that are the only connection between two parts.  Arrays [L, N]:
      cut_prob          the share of the samples in which the node is a cut point
      mean, sd          the mean and the (population) standard deviation of pairs_cut over the samples; sd is clipped at 0
      expected_rank     the mean over the samples of rank[v] = #{u : pairs_cut[u] > pairs_cut[v]} (all non-cut nodes share a rank)
      top_prob          the share of the samples with rank < top_k -- the non-cut nodes enter together, so more than top_k nodes can
      mean_branches, mean_bridges   the means of branches and of bridges over the samples
      inferred          {"pairs_cut", "branches", "bridges"} of the point estimate `get_inferred_model()`
                        (`CaviEngine.network_cutpoints`), or None
    and [S, L]: n_cut (the cut points), n_bridges (the bridges), max_pairs_cut and connected_pairs (the connected unordered pairs
    of G) of every sample; pairs_cut uint32, branches, bridges uint16 [S, L, N] when asked for, else None.
      fragmentation()          float64 [S, L, N]: pairs_cut over the sample's connected pairs (needs the values)
      quantiles(q)             {statistic: [len(q), L]} of the per-sample counts
      top(n, layer)            the n nodes of highest cut_prob, ties broken by mean
      key_players(min_prob)    bool [L, N]: cut_prob >= min_prob
      frame(node_names)        one row per (layer, node);  summary(): mean, std and quantiles of the per-sample numbers per layer."""

    stat_keys = ("n_cut", "n_bridges", "max_pairs_cut", "connected_pairs")
    stat_dtype = np.int64

    def __init__(self, N, counts, mode="union", top_k=10, inferred=None, seed=None, n_trials=1):
        super().__init__(N, counts, top_k, seed, n_trials)
        self.mode = mode
        self.node_cut = np.asarray(counts["node_cut"], dtype=np.int64)
        self.node_branch_sum = np.asarray(counts["node_branch_sum"], dtype=np.int64)
        self.node_bridge_sum = np.asarray(counts["node_bridge_sum"], dtype=np.int64)
        S = float(self.S)
        self.cut_prob = self.node_cut / S
        self.mean_branches = self.node_branch_sum / S
        self.mean_bridges = self.node_bridge_sum / S
        for k in CUT_VALUES:
            setattr(self, k, None if counts.get(k) is None else np.asarray(counts[k]))
        self.values = self.pairs_cut
        self.inferred = None if inferred is None else {k: np.asarray(inferred[k], dtype=np.int64) for k in CUT_VALUES}
        self.inferred_pairs_cut = None if inferred is None else self.inferred["pairs_cut"]

    def fragmentation(self):
        """float64 [S, L, N]: pairs_cut over the sample's connected pairs -- the share of the pairs connected in G that the
        removal of the node disconnects, the pairs the node itself is part of left out of the numerator; 0 where the sample has
        no connected pair.  Needs values=True."""
        if self.pairs_cut is None:
            raise ValueError("fragmentation() needs the per-sample values: posterior_cutpoints(..., values=True)")
        den = self.connected_pairs[:, :, None].astype(np.float64)
        return np.divide(self.pairs_cut.astype(np.float64), den, out=np.zeros(self.pairs_cut.shape, np.float64), where=den > 0)

    def quantiles(self, q=(0.025, 0.5, 0.975)):
        """{statistic: float64 [len(q), L]}: the quantiles q over the samples of every per-sample count."""
        q = tuple(float(x) for x in q)
        return {k: np.quantile(arr.astype(np.float64), q, axis=0) for k, arr in self.statistics().items()}

    def top(self, n=10, layer=0):
        """The n nodes of layer `layer` with the highest cut_prob, ties broken by the higher mean pairs_cut (then by the smaller
        index)."""
        return super().top(n, layer, key="cut_prob")

    def key_players(self, min_prob=0.5):
        """bool [L, N]: the nodes that are cut points in at least the share `min_prob` of the samples."""
        return self.cut_prob >= float(min_prob)

    def frame(self, node_names=None):
        """One row per (layer, node): cut_prob, mean, sd, expected_rank, top_prob, mean_branches, mean_bridges and, when it was
        computed, inferred_pairs_cut.  node_names: N names in node order for a `name` column."""
        return super().frame(node_names, columns=("cut_prob", "mean", "sd", "expected_rank", "top_prob", "mean_branches", "mean_bridges"),
                             extra="inferred_pairs_cut")
