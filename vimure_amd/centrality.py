"""Result of `VimureModel.posterior_centrality`: the per-node sums the device returns over the posterior samples
(`CaviEngine.sample_centrality`) and what is derived from them on the host.
"""
import numpy as np

from .node_scores import NodeScoreStats

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


class CentralityStats(NodeScoreStats):
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

    stat_keys = ("total", "max")

    def __init__(self, N, counts, q, T, direction="out", top_k=10, plug_in=None, seed=None, n_trials=1):
        super().__init__(N, counts, top_k, seed, n_trials)
        self.q = np.atleast_1d(np.asarray(q, dtype=np.float64))
        self.T, self.direction = int(T), direction
        self.plug_in = None if plug_in is None else np.asarray(plug_in, dtype=np.float64)

    def frame(self, node_names=None):
        """One row per (layer, node): mean, sd, expected_rank, top_prob and, when it was computed, plug_in.  node_names: N names
        in node order for a `name` column."""
        return super().frame(node_names, extra="plug_in")
