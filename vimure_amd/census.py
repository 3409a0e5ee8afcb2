"""Result of `VimureModel.posterior_triad_census`: the Holland-Leinhardt triad census of every posterior sample, as the device
returns it (`CaviEngine.sample_triad_census`), and what is derived from it on the host.
"""
import numpy as np

from ._lib import CENSUS_NAMES
from .node_scores import quantile_row

CLASS_NAMES = tuple(CENSUS_NAMES)
# mutual, asymmetric and null dyads of a class: the digits of its name
MAN = np.array([[int(d) for d in name[:3]] for name in CLASS_NAMES], dtype=np.int64)
# the labelled digraphs on three named nodes that fall in a class (they sum to 64)
LABELLED = np.array([1, 6, 3, 3, 3, 6, 6, 6, 6, 2, 3, 3, 3, 6, 6, 1], dtype=np.int64)
# Holland and Leinhardt's transitivity of a triad: every ordered triple (x, y, z) with x -> y and y -> z is transitive when x -> z
# and intransitive otherwise.  VACUOUS: the classes with no such triple; TRANSITIVE: those with at least one and none intransitive
VACUOUS = ("003", "012", "102", "021D", "021U")
TRANSITIVE = ("030T", "120D", "120U", "300")


def _falling(x, k):
    """x (x - 1) .. (x - k + 1), elementwise in float64; k = 0 gives 1."""
    out = np.ones_like(x, dtype=np.float64)
    for r in range(int(k)):
        out = out * (x - r)
    return out


def dyads_of(counts, N):
    """(mutual, asymmetric, null) dyads, int64 of the shape of counts[..., 0], from a census counts[..., 16] on N >= 3 nodes: every
    dyad lies in N - 2 triads, so M = sum_c m_c T_c / (N - 2), and likewise A and the null dyads; the divisions are exact."""
    if N < 3:
        raise ValueError(f"the dyads follow from the census for N >= 3 only, got N = {N}")
    tot = np.asarray(counts, dtype=np.int64) @ MAN
    if (tot % (N - 2)).any():
        raise ValueError("not a triad census on %d nodes: a dyad count is not a whole number" % N)
    tot //= N - 2
    return tot[..., 0], tot[..., 1], tot[..., 2]


def expected_under_man(counts, N):
    """float64, the shape of counts: per census the Holland-Leinhardt expectation of every class under the uniform distribution
    over the digraphs with the census' own mutual, asymmetric and null dyads (U | MAN):
    E[T_c] = C(N, 3) n_c 2^-a M^(m) A^(a) N^(n) / D^(3), x^(k) the falling factorial, D = C(N, 2) and n_c = `LABELLED`."""
    M, A, Nn = (x.astype(np.float64)[..., None] for x in dyads_of(counts, N))
    D = N * (N - 1) / 2.0
    triples = N * (N - 1) * (N - 2) / 6.0
    out = np.empty(np.shape(counts), np.float64)
    for c, (m, a, n) in enumerate(MAN):
        out[..., c] = (triples * LABELLED[c] * 0.5 ** a * _falling(M, m) * _falling(A, a) * _falling(Nn, n) / (D * (D - 1) * (D - 2)))[..., 0]
    return out


class TriadCensus:
    """The triad census of S posterior samples (sample s is the draw of seed + s), per layer, for A = (Y > 0) without its
    diagonal: `counts` int64 [S, L, 16], the unordered triples of nodes in each of the 16 isomorphism classes `CLASS_NAMES` (003
    012 102 021D 021U 021C 111D 111U 030T 030C 201 120D 120U 120C 210 300: `networkx.triadic_census`); the 16 sum to C(N, 3).
      inferred               int64 [L, 16]: the census of the point estimate `get_inferred_model()`, or None
      mean, sd               float64 [L, 16]: the mean and the (population) standard deviation over the samples
      quantiles(q)           float64 [len(q), L, 16]
      dyads()                {"mutual", "asymmetric", "null"}: int64 [S, L], read off the census
      expected_under_man()   float64 [S, L, 16]: the expectation of every class given the sample's own dyad census (U | MAN)
      excess()               counts - expected_under_man(): what the triads hold beyond what the dyads explain
      transitive_share()     float64 [S, L]: transitive triads over the triads that are not vacuously transitive
      of(name)               int64 [S, L]: one class by name
      frame(), summary()     DataFrames: one row per (layer, class); per (layer, statistic) over the samples."""

    def __init__(self, N, counts, inferred=None, seed=None, n_trials=1):
        self.N = int(N)
        self.counts = np.asarray(counts, dtype=np.int64)
        if self.counts.ndim != 3 or self.counts.shape[2] != len(CLASS_NAMES):
            raise ValueError(f"counts has shape {self.counts.shape}, expected (S, L, {len(CLASS_NAMES)})")
        self.S, self.L = self.counts.shape[:2]
        self.seed, self.n_trials = seed, int(n_trials)
        self.inferred = None if inferred is None else np.asarray(inferred, dtype=np.int64)
        self.mean = self.counts.mean(axis=0)
        self.sd = self.counts.std(axis=0)

    def of(self, name):
        """int64 [S, L]: the triads of the class `name`."""
        return self.counts[..., CLASS_NAMES.index(name)]

    def quantiles(self, q=(0.025, 0.5, 0.975)):
        """float64 [len(q), L, 16]: the quantiles q of every class over the samples."""
        return np.quantile(self.counts, np.asarray(q, dtype=np.float64), axis=0)

    def dyads(self):
        """{"mutual", "asymmetric", "null"} int64 [S, L]: the dyad census, which follows from the triad census (`dyads_of`)."""
        return dict(zip(("mutual", "asymmetric", "null"), dyads_of(self.counts, self.N)))

    def expected_under_man(self):
        """float64 [S, L, 16]: per sample and layer the expected census of a random digraph with the sample's own numbers of
        mutual, asymmetric and null dyads (`expected_under_man`); it sums to C(N, 3)."""
        return expected_under_man(self.counts, self.N)

    def excess(self):
        """float64 [S, L, 16]: counts - expected_under_man()."""
        return self.counts - self.expected_under_man()

    def transitive_share(self):
        """float64 [S, L]: the triads that contain a transitive triple (x -> y, y -> z and x -> z) and no intransitive one --
        030T, 120D, 120U and 300 -- over all triads that are not vacuously transitive, i.e. all but 003, 012, 102, 021D and 021U
        (which hold no x -> y -> z at all); NaN where there is none."""
        tr = sum(self.of(n) for n in TRANSITIVE).astype(np.float64)
        non_vacuous = (self.counts.sum(axis=-1) - sum(self.of(n) for n in VACUOUS)).astype(np.float64)
        return np.divide(tr, non_vacuous, out=np.full(tr.shape, np.nan), where=non_vacuous > 0)

    def frame(self):
        """One row per (layer, class): mean and sd of the count over the samples, the mean of its expectation under U | MAN and of
        the excess, and, when it was computed, the census of the point estimate (`inferred`)."""
        import pandas as pd
        exp = self.expected_under_man().mean(axis=0)
        cols = {"layer": np.repeat(np.arange(self.L), len(CLASS_NAMES)), "class": list(CLASS_NAMES) * self.L,
                "mean": self.mean.reshape(-1), "sd": self.sd.reshape(-1), "expected_under_man": exp.reshape(-1),
                "excess": (self.mean - exp).reshape(-1)}
        if self.inferred is not None:
            cols["inferred"] = self.inferred.reshape(-1)
        return pd.DataFrame(cols)

    def statistics(self):
        """name -> [S, L] array: the 16 classes, the three dyad counts and the transitive share."""
        out = {name: self.counts[..., c] for c, name in enumerate(CLASS_NAMES)}
        out.update(self.dyads())
        out["transitive_share"] = self.transitive_share()
        return out

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
