"""Result of `VimureModel.posterior_shared_partners`: the shared partners of the ties of every posterior sample, as the device
returns them (`CaviEngine.sample_shared_partners`), and what is derived from them on the host: the support of Jackson,
Rodriguez-Barraquer and Tan, the local bridges, the mean embeddedness, the GWESP statistic of the edgewise-shared-partner
distribution, and the listed ties one by one.
"""
import numpy as np

from ._lib import SP_MODES, SP_TOTALS
from .node_scores import quantile_row


def _ratio(a, b):
    """a / b in float64, NaN where b is 0."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.divide(a, b, out=np.full(np.broadcast(a, b).shape, np.nan), where=b > 0)


def gwesp_of(hist, decay):
    """float64, the shape of hist[..., 0]: the geometrically weighted edgewise shared partners of a histogram hist[..., b] of ties
    with b partners, e^decay sum_b (1 - (1 - e^-decay)^b) hist_b (Hunter 2007).  decay = 0 counts the supported ties; as decay
    grows the statistic approaches the partners summed over the ties."""
    decay = float(decay)
    if decay < 0:
        raise ValueError(f"decay must not be negative, got {decay}")
    b = np.arange(np.shape(hist)[-1], dtype=np.float64)
    if decay == 0:
        w = (b > 0).astype(np.float64)
    else:   # 1 - (1 - x)^b without the cancellation at small x = e^-decay
        w = np.exp(decay) * -np.expm1(b * np.log1p(-np.exp(-decay)))
    return np.asarray(hist, dtype=np.float64) @ w


class SharedPartners:
    """The shared partners of the ties of S posterior samples (sample s is the draw of seed + s), per layer, for A = (Y > 0)
    without its diagonal and one of the modes `SP_MODES`: "union" (unordered pairs tied either way; a partner is tied to both
    ends), "mutual" (pairs tied both ways; a partner is tied both ways to both: Simmelian ties) or "path" (ordered ties i -> j; a
    partner k has i -> k -> j).
      hist                   int64 [S, L, n_bins]: the ties with exactly b partners; the last bin holds b >= n_bins - 1
      totals                 int64 [S, L, 4]: `SP_TOTALS` -- ties, supported ties, partners summed over the ties, the largest count
      support()              float64 [S, L]: supported ties / ties; NaN where a sample has no tie
      mean_partners()        float64 [S, L]: partners per tie (the mean embeddedness); NaN where there is no tie
      local_bridges()        int64 [S, L]: the ties with no partner
      statistics()           name -> [S, L]; `mean`, `sd` name -> [L] over the samples (NaN samples left out); quantiles(q)
      gwesp(decay)           float64 [S, L] from the histogram; refused when the pooled last bin is not empty
      node_ties, node_supported   int32 [S, L, N] or None; node_support() float64 [L, N]
      inferred               the dict of `CaviEngine.network_shared_partners` on the point estimate, or None
      pairs                  int64 [P, 3] (layer, i, j) or None, with pair_present, pair_supported, pair_partners int64 [P] and
                             inferred_partners int64 [P] (-1: not a tie of the point estimate)
      ties_frame(), bridges(min_prob), frame(), summary()   DataFrames."""

    def __init__(self, N, mode, hist, totals, node_ties=None, node_supported=None, pairs=None, pair_present=None, pair_supported=None,
                 pair_partners=None, inferred=None, seed=None, n_trials=1):
        if mode not in SP_MODES:
            raise ValueError(f"mode must be one of {SP_MODES}, got {mode!r}")
        self.N, self.mode = int(N), mode
        self.hist = np.asarray(hist, dtype=np.int64)
        self.totals = np.asarray(totals, dtype=np.int64)
        if self.hist.ndim != 3 or self.totals.shape != self.hist.shape[:2] + (len(SP_TOTALS),):
            raise ValueError(f"hist has shape {self.hist.shape} and totals {self.totals.shape}, expected (S, L, n_bins) and (S, L, {len(SP_TOTALS)})")
        self.S, self.L, self.n_bins = self.hist.shape
        self.seed, self.n_trials = seed, int(n_trials)
        self.node_ties = None if node_ties is None else np.asarray(node_ties)
        self.node_supported = None if node_supported is None else np.asarray(node_supported)
        self.inferred = inferred
        self.pairs = None if pairs is None else np.asarray(pairs, dtype=np.int64).reshape(-1, 3)
        if self.pairs is not None:
            self.pair_present, self.pair_supported, self.pair_partners = (np.asarray(a, dtype=np.int64) for a in (pair_present, pair_supported, pair_partners))
            if not (self.pair_present.shape == self.pair_supported.shape == self.pair_partners.shape == (len(self.pairs),)):
                raise ValueError("the pair arrays must hold one number per listed pair")
        ip = None if inferred is None else inferred.get("pair_partners")
        self.inferred_partners = None if ip is None else np.asarray(ip, dtype=np.int64)
        stats = self.statistics()
        with np.errstate(invalid="ignore"):
            self.mean = {k: np.array([quantile_row(v[:, l], ())["mean"] for l in range(self.L)]) for k, v in stats.items()}
            self.sd = {k: np.array([quantile_row(v[:, l], ())["std"] for l in range(self.L)]) for k, v in stats.items()}

    # ------------------------------------------------------------------ per sample and layer
    def total(self, name):
        """int64 [S, L]: one of `SP_TOTALS` by name."""
        return self.totals[..., SP_TOTALS.index(name)]

    def support(self):
        """float64 [S, L]: the share of ties whose two ends have a partner in common; NaN where a sample has no tie."""
        return _ratio(self.total("supported"), self.total("ties"))

    def mean_partners(self):
        """float64 [S, L]: partners per tie; NaN where a sample has no tie."""
        return _ratio(self.total("partners"), self.total("ties"))

    def local_bridges(self):
        """int64 [S, L]: the ties whose ends have no partner in common."""
        return self.total("ties") - self.total("supported")

    def gwesp(self, decay):
        """float64 [S, L]: e^decay sum_b (1 - (1 - e^-decay)^b) hist_b.  The last bin pools every count >= n_bins - 1; when a tie of
        any sample fell into it the statistic cannot be had from this histogram and the call raises, naming the n_bins to ask for."""
        if self.hist[..., -1].any():
            need = int(self.total("max_partners").max()) + 2
            raise ValueError(f"the last bin of the histogram (n_bins = {self.n_bins}) pools ties with {self.n_bins - 1} or more partners; "
                             f"ask for n_bins >= {need}" + ("" if need <= 1024 else ", beyond the 1024 the device offers: no exact GWESP for these samples"))
        return gwesp_of(self.hist, decay)

    def statistics(self):
        """name -> [S, L]: ties, supported, local_bridges, partners, max_partners, support, mean_partners."""
        out = {"ties": self.total("ties"), "supported": self.total("supported"), "local_bridges": self.local_bridges(),
               "partners": self.total("partners"), "max_partners": self.total("max_partners"), "support": self.support(),
               "mean_partners": self.mean_partners()}
        return out

    def quantiles(self, q=(0.025, 0.5, 0.975)):
        """name -> float64 [len(q), L]: the quantiles q of every statistic over the samples (NaN samples left out)."""
        q = tuple(float(x) for x in q)
        return {k: np.array([[quantile_row(v[:, l], q)["q%g" % x] for l in range(self.L)] for x in q]).reshape(len(q), self.L)
                for k, v in self.statistics().items()}

    # ------------------------------------------------------------------ nodes
    def node_support(self):
        """float64 [L, N]: over all samples, the share of a node's counted ties that have a partner; NaN for a node never tied."""
        if self.node_ties is None:
            raise ValueError("the node arrays were not asked for: nodes=True")
        return _ratio(self.node_supported.sum(axis=0, dtype=np.int64), self.node_ties.sum(axis=0, dtype=np.int64))

    # ------------------------------------------------------------------ listed ties
    def ties_frame(self):
        """One row per listed tie: layer, i, j, P(present) over the samples, P(supported | present), E[partners | present] (NaN
        where the tie is in no sample) and, when the point estimate was reduced, its count there (`inferred_partners`, -1: no
        tie)."""
        import pandas as pd
        if self.pairs is None:
            raise ValueError("no ties were listed: ties='inferred' or an array of (layer, i, j)")
        cols = {"layer": self.pairs[:, 0], "i": self.pairs[:, 1], "j": self.pairs[:, 2], "p_present": self.pair_present / float(self.S),
                "p_supported": _ratio(self.pair_supported, self.pair_present), "mean_partners": _ratio(self.pair_partners, self.pair_present)}
        if self.inferred_partners is not None:
            cols["inferred_partners"] = self.inferred_partners
        return pd.DataFrame(cols)

    def bridges(self, min_prob=0.5):
        """The rows of `ties_frame()` the posterior calls bridges: present in at least min_prob of the samples and, where present,
        more often without a partner than with one; ordered by P(present), descending."""
        t = self.ties_frame()
        t = t[(t["p_present"] >= float(min_prob)) & (t["p_present"] > 0) & (t["p_supported"] < 0.5)]
        return t.sort_values("p_present", ascending=False, kind="stable").reset_index(drop=True)

    # ------------------------------------------------------------------ tables
    def frame(self):
        """One row per (layer, b): the ties with b partners, mean and sd over the samples, their share of all samples' ties and,
        when it was computed, the histogram of the point estimate.  The last b is pooled (`pooled` True)."""
        import pandas as pd
        cols = {"layer": np.repeat(np.arange(self.L), self.n_bins), "partners": np.tile(np.arange(self.n_bins), self.L),
                "pooled": np.tile(np.arange(self.n_bins) == self.n_bins - 1, self.L), "mean": self.hist.mean(axis=0).reshape(-1),
                "sd": self.hist.std(axis=0).reshape(-1),
                "share": _ratio(self.hist.sum(axis=0), self.total("ties").sum(axis=0)[..., None]).reshape(-1)}
        if self.inferred is not None:
            cols["inferred"] = np.asarray(self.inferred["hist"], dtype=np.int64).reshape(-1)
        return pd.DataFrame(cols)

    def summary(self, q=(0.025, 0.5, 0.975)):
        """DataFrame with one row per (layer, statistic of `statistics()`): mean, std (population) and the quantiles q over the
        samples."""
        import pandas as pd
        q = tuple(float(x) for x in q)
        rows = []
        stats = self.statistics()
        for l in range(self.L):
            for name, arr in stats.items():
                row = {"layer": l, "statistic": name}
                row.update(quantile_row(arr[:, l], q))
                rows.append(row)
        return pd.DataFrame(rows, columns=["layer", "statistic", "mean", "std"] + ["q%g" % x for x in q])
