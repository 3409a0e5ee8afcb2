"""Result of `VimureModel.posterior_connectivity`: the integers the device returns per posterior sample and layer
(`CaviEngine.sample_connectivity`) and what is derived from them on the host.
"""
import numpy as np

from .netstats import _ratio
from .node_scores import quantile_row

CONN_KEYS = ("components_w", "giant_w", "pairs_w", "isolates", "components_s", "giant_s", "pairs_s", "reach_pairs", "dist_sum",
             "diameter")
NODE_KEYS = ("node_comp_w", "node_comp_s", "node_reach_out", "node_reach_in", "node_dist_out", "node_dist_in")
_DERIVED = ("giant_fraction_w", "giant_fraction_s", "connectedness", "reach_fraction", "avg_path_length", "global_efficiency")


class ConnectivityStats:
    """Per sample s and layer l (arrays [S, L]; sample s is the draw of seed + s), for A = (Y > 0) without its diagonal,
    U = A | A.T and d(i, j) the length of a shortest directed path in A:
      components_w, giant_w, pairs_w, isolates   weak components (those of U), the largest one's size, the ordered pairs of
                                  distinct nodes in one component, the nodes without a neighbour
      components_s, giant_s, pairs_s   the same of the strong components (classes of mutual reachability)
      reach_pairs, dist_sum, diameter   #{i != j : d(i, j) finite}, the sum of those distances, their maximum (0: no tie)
      dist_hist                   int64 [S, L, 64] when asked for: bin d - 1 the ordered pairs at distance d, the last bin every
                                  distance >= 64
      giant_fraction_w, giant_fraction_s   giant / N
      connectedness               pairs_w / (N (N - 1))
      reach_fraction              reach_pairs / (N (N - 1))
      avg_path_length             dist_sum / reach_pairs, NaN where nothing is reachable
      global_efficiency           sum_d dist_hist[d - 1] / d / (N (N - 1)): the mean of 1 / d(i, j) over all ordered pairs, an
                                  unreachable pair counting 0; NaN where the last bin is not empty (distances it does not
                                  resolve), None without dist_hist
    (the ratios over N (N - 1) are NaN for N = 1.)  With the node arrays (int32 [S, L, N]; None otherwise):
      node_comp_w, node_comp_s    the smallest node index of the node's weak / strong component
      node_reach_out, node_reach_in   nodes it reaches / that reach it
      node_dist_out, node_dist_in     the sums of those distances
      closeness_out, closeness_in     [S, L, N] Wasserman-Faust closeness (r / (N - 1)) (r / dist) with r the reach and dist the
                                  distance sum of the direction; 0 where r = 0
      same_component(i, j, strong=False)   the share of samples, per layer, in which i and j share a component."""

    def __init__(self, N, counts, seed=None, n_trials=1):
        self.N = int(N)
        self.seed, self.n_trials = seed, int(n_trials)
        for k in CONN_KEYS:
            setattr(self, k, np.asarray(counts[k], dtype=np.int64))
        self.S, self.L = self.components_w.shape
        dh = counts.get("dist_hist")
        self.dist_hist = None if dh is None else np.asarray(dh, dtype=np.int64)
        pairs = float(self.N) * (self.N - 1)
        self.giant_fraction_w = self.giant_w / float(self.N)
        self.giant_fraction_s = self.giant_s / float(self.N)
        self.connectedness = _ratio(self.pairs_w, pairs)
        self.reach_fraction = _ratio(self.reach_pairs, pairs)
        self.avg_path_length = _ratio(self.dist_sum, self.reach_pairs)
        self.global_efficiency = None
        if self.dist_hist is not None:
            nb = self.dist_hist.shape[-1]
            eff = _ratio((self.dist_hist[..., :nb - 1] / np.arange(1, nb, dtype=np.float64)).sum(-1), pairs)
            self.global_efficiency = np.where(self.dist_hist[..., nb - 1] > 0, np.nan, eff)
        for k in NODE_KEYS:
            v = counts.get(k)
            setattr(self, k, None if v is None else np.asarray(v))
        self.has_nodes = all(getattr(self, k) is not None for k in NODE_KEYS)
        self.closeness_out = self.closeness_in = None
        if self.has_nodes:
            self.closeness_out = self._closeness(self.node_reach_out, self.node_dist_out)
            self.closeness_in = self._closeness(self.node_reach_in, self.node_dist_in)

    def _closeness(self, reach, dist):
        r = np.asarray(reach, dtype=np.float64)
        c = _ratio(r * r, (self.N - 1.0) * np.asarray(dist, dtype=np.float64))
        return np.where(r > 0, c, 0.0)

    def same_component(self, i, j, strong=False):
        """float64 [L]: the share of the samples in which nodes i and j lie in one weak (strong=True: strong) component."""
        lab = self.node_comp_s if strong else self.node_comp_w
        if lab is None:
            raise ValueError("the node arrays were not asked for: posterior_connectivity(nodes=True)")
        return (lab[:, :, int(i)] == lab[:, :, int(j)]).mean(axis=0)

    def statistics(self):
        """name -> [S, L] array of every per-sample statistic this result holds."""
        out = {k: getattr(self, k) for k in CONN_KEYS + _DERIVED}
        if self.global_efficiency is None:
            del out["global_efficiency"]
        return out

    def summary(self, q=(0.025, 0.5, 0.975)):
        """DataFrame with one row per (layer, statistic): mean, std (population) and the quantiles q over the samples (NaN
        samples left out)."""
        import pandas as pd
        q = tuple(float(x) for x in q)
        rows = []
        for l in range(self.L):
            for name, arr in self.statistics().items():
                row = {"layer": l, "statistic": name}
                row.update(quantile_row(arr[:, l], q))
                rows.append(row)
        return pd.DataFrame(rows, columns=["layer", "statistic", "mean", "std"] + ["q%g" % x for x in q])

    def frame(self, q=(0.025, 0.5, 0.975)):
        """The distribution of the distances as a long table: one row per (layer, distance d) up to the largest distance any
        sample of the layer holds -- the last bin's row stands for every distance >= 64 -- with the mean, std and quantiles q over
        the samples of the number of ordered pairs at that distance."""
        import pandas as pd
        if self.dist_hist is None:
            raise ValueError("the distance histogram was not asked for")
        q = tuple(float(x) for x in q)
        rows = []
        for l in range(self.L):
            used = np.nonzero(self.dist_hist[:, l].any(axis=0))[0]
            for b in range(int(used.max()) + 1 if used.size else 0):
                row = {"layer": l, "distance": b + 1}
                row.update(quantile_row(self.dist_hist[:, l, b], q))
                rows.append(row)
        return pd.DataFrame(rows, columns=["layer", "distance", "mean", "std"] + ["q%g" % x for x in q])
