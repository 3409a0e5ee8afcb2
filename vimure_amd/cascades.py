"""Results of `VimureModel.posterior_cascades`: what the device returns of the independent-cascade model over the posterior
samples (`CaviEngine.sample_outreach`, `CaviEngine.sample_seed_outreach`) and what is derived from it on the host.
"""
import numpy as np

from .node_scores import NodeScoreStats, quantile_row

CASCADE_KEYS = ("node_sum", "node_sumsq", "node_rank_sum", "node_top", "total", "max")


def resolve_seed_sets(seeds, N, node_names=None):
    """(labels, sets) of the seed sets `seeds` = {label: nodes}: every node given by its name (node_names: the name of node
    0 .. N - 1) or, where it is no node's name, by its index in [0, N); what is neither is a ValueError.  A set may be empty."""
    if not hasattr(seeds, "items"):
        raise ValueError("seeds must map a label to the nodes of its seed set")
    where = {} if node_names is None else {n: i for i, n in enumerate(node_names)}
    labels, sets = [], []
    for label, nodes in seeds.items():
        if isinstance(nodes, (str, bytes)) or not hasattr(nodes, "__iter__"):
            nodes = [nodes]
        idx = []
        for v in nodes:
            if v in where:
                idx.append(where[v])
            elif isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 0 <= int(v) < N:
                idx.append(int(v))
            else:
                raise ValueError(f"seed set {label!r} names {v!r}, which is not a node of the model")
        labels.append(label)
        sets.append(sorted(set(idx)))
    if not sets:
        raise ValueError("seeds holds no seed set")
    return labels, sets


class CascadeStats(NodeScoreStats):
    """The outreach of every node as a single seed under the independent-cascade model over S posterior samples (sample s is the
    draw of seed + s) and n_cascades cascades of each: every tie of A = (Y > 0) without its diagonal passes the information on
    with probability q_l, the spread follows A ("out"), A.T ("in") or A | A.T ("union"), and the outreach is the number of other
    nodes informed after T periods.  The node score of a sample is its mean over the cascades.  Arrays [L, N]:
      mean, sd          the mean and the (population) standard deviation of the score over the samples; sd is clipped at 0
      expected_rank     the mean over the samples of rank[v] = #{u : score[u] > score[v]} (0: the best entry point)
      top_prob          the share of the samples in which the node is among the top_k entry points
      inferred          the outreach of the point estimate `get_inferred_model()` SUMMED over its n_cascades cascades, int64
                        (`CaviEngine.network_outreach`, cascades keyed by cascade_seed), or None; inferred_score = inferred /
                        n_cascades is on the scale of mean
    and [S, L]: total (sum_v of the outreach summed over the cascades) and max (its maximum over the nodes) of every sample;
    values uint32 [S, L, N], the outreach summed over the cascades, when asked for, else None.
      top(n, layer)            the n nodes of highest top_prob, ties broken by mean
      frame(node_names)        one row per (layer, node);  summary(): mean, std and quantiles of the per-sample numbers per layer."""

    stat_keys = ("total", "max")
    stat_dtype = np.int64

    def __init__(self, N, counts, q, T, direction="out", n_cascades=16, top_k=10, inferred=None, seed=None, cascade_seed=None, n_trials=1):
        super().__init__(N, counts, top_k, seed, n_trials)
        self.q, self.T, self.direction = np.asarray(q, dtype=np.float64), int(T), direction
        self.n_cascades, self.cascade_seed = int(n_cascades), cascade_seed
        self.inferred = None if inferred is None else np.asarray(inferred, dtype=np.int64)
        self.inferred_score = None if inferred is None else self.inferred / float(self.n_cascades)

    def frame(self, node_names=None):
        """One row per (layer, node): mean, sd, expected_rank, top_prob and, when it was computed, inferred_score.  node_names: N
        names in node order for a `name` column."""
        return super().frame(node_names, extra="inferred_score")


class SeedOutreach:
    """The outreach of seed sets under the independent-cascade model of `CascadeStats` over S posterior samples and n_cascades
    cascades of each.  result: the dict of `CaviEngine.sample_seed_outreach` -- values uint32 [S, L, n_sets] (the nodes outside
    the set informed after T periods, summed over the cascades), curve int64 [L, n_sets, 64] or absent, node_hits int64
    [L, n_sets, N] or absent.  labels: the sets' names; sets: their node indices.  Arrays [L, n_sets]:
      mean, sd          the mean and the (population) standard deviation over the samples of the outreach per cascade
    quantiles(q) [len(q), L, n_sets]; curve() [L, n_sets, 64], the cumulative share of the set's total outreach reached by
    period t (NaN for a set that reaches nobody); reach_prob() [L, n_sets, N], the share of the (sample, cascade) pairs in which
    the node is informed after T periods (1 for the seeds); frame() one row per (layer, set); summary() mean, std and quantiles."""

    def __init__(self, N, result, labels, sets, q, T, direction="out", n_cascades=16, seed=None, cascade_seed=None, n_trials=1):
        self.N, self.labels, self.sets = int(N), list(labels), [list(s) for s in sets]
        self.q, self.T, self.direction = np.asarray(q, dtype=np.float64), int(T), direction
        self.n_cascades, self.seed, self.cascade_seed, self.n_trials = int(n_cascades), seed, cascade_seed, int(n_trials)
        self.values = np.asarray(result["values"])
        self.S, self.L, self.n_sets = self.values.shape
        self.curve_counts = result.get("curve")
        self.node_hits = result.get("node_hits")
        self.per_cascade = self.values.astype(np.float64) / float(self.n_cascades)
        self.mean = self.per_cascade.mean(axis=0)
        self.sd = self.per_cascade.std(axis=0)

    def quantiles(self, q=(0.025, 0.5, 0.975)):
        """The quantiles q over the samples of the outreach per cascade: float64 [len(q), L, n_sets]."""
        return np.quantile(self.per_cascade, tuple(float(x) for x in q), axis=0)

    def curve(self):
        """float64 [L, n_sets, 64]: the share of the set's total outreach reached by period t = bin + 1 (the last bin: by T), NaN
        for a set that reaches nobody.  Needs the call's curve."""
        if self.curve_counts is None:
            raise ValueError("the curve was not asked for")
        c = np.cumsum(np.asarray(self.curve_counts, dtype=np.float64), axis=-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(c[..., -1:] > 0, c / c[..., -1:], np.nan)

    def reach_prob(self):
        """float64 [L, n_sets, N]: the share of the (sample, cascade) pairs in which the node is informed after T periods.  Needs
        the call's node_hits."""
        if self.node_hits is None:
            raise ValueError("node_hits was not asked for")
        return np.asarray(self.node_hits, dtype=np.float64) / float(self.S * self.n_cascades)

    def frame(self):
        """One row per (layer, set): its label, size, and the mean and sd of its outreach per cascade."""
        import pandas as pd
        size = [len(s) for s in self.sets]
        return pd.DataFrame({"layer": np.repeat(np.arange(self.L), self.n_sets), "set": self.labels * self.L, "size": size * self.L,
                             "mean": self.mean.reshape(-1), "sd": self.sd.reshape(-1)})

    def summary(self, q=(0.025, 0.5, 0.975)):
        """DataFrame with one row per (layer, set): mean, std (population) and the quantiles q over the samples."""
        import pandas as pd
        q = tuple(float(x) for x in q)
        rows = []
        for l in range(self.L):
            for b, name in enumerate(self.labels):
                row = {"layer": l, "set": name}
                row.update(quantile_row(self.per_cascade[:, l, b], q))
                rows.append(row)
        return pd.DataFrame(rows, columns=["layer", "set", "mean", "std"] + ["q%g" % x for x in q])
