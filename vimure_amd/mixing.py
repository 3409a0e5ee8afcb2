"""Result of `VimureModel.posterior_mixing`: the integer tables the device returns per posterior sample and layer
(`CaviEngine.sample_mixing`: the mixing matrix by node attribute, its reciprocated part, the overlap between layers), their
analytic expectations (`CaviEngine.expected_mixing`) and what is derived from them on the host; and the helpers that turn node
labels into the engine's group codes.
"""
import numpy as np

from .netstats import _ratio
from .node_scores import quantile_row


def groups_from_frame(meta, column, id="pid"):
    """{node name: label} from a node table such as the villages' `*_meta.csv` (a row per node: `id` holds the node's name as the
    edge list spells it, `column` the attribute): the dict form `VimureModel.posterior_mixing(groups=...)` takes."""
    for c in (id, column):
        if c not in meta.columns:
            raise ValueError(f"the node table has no column {c!r}")
    return dict(zip(meta[id].tolist(), meta[column].tolist()))


def _missing(v):
    import pandas as pd
    if v is None:
        return True
    m = pd.isna(v)
    return bool(m) if np.ndim(m) == 0 else False


def encode_groups(groups, N, node_names=None):
    """(codes int32 [N], labels): the group code of every node, -1 where it is left out (label None or NaN, or a node that a
    dict does not name), and the labels in `np.unique`'s order -- code c stands for labels[c].  groups: N labels in node order, or
    a dict / pandas Series keyed by node name, resolved through node_names (the name of node 0 .. N - 1; None: the names are the
    indices); a key that is no node's name is a ValueError."""
    import pandas as pd
    N = int(N)
    if isinstance(groups, (dict, pd.Series)):
        names = list(range(N)) if node_names is None else list(node_names)
        if len(names) != N:
            raise ValueError(f"{len(names)} node names for {N} nodes")
        where = {n: i for i, n in enumerate(names)}
        vals = [None] * N
        for k, v in groups.items():
            if k not in where:
                raise ValueError(f"groups names {k!r}, which is not a node of the model")
            vals[where[k]] = v
    else:
        vals = list(groups)
        if len(vals) != N:
            raise ValueError(f"groups holds {len(vals)} labels, the model has {N} nodes")
    keep = np.array([not _missing(v) for v in vals], dtype=bool)
    codes = np.full(N, -1, np.int32)
    if not keep.any():
        return codes, np.empty(0, dtype=object)
    labels, inv = np.unique(np.asarray([v for v, k in zip(vals, keep) if k]), return_inverse=True)
    codes[keep] = inv.astype(np.int32)
    return codes, labels


def _assortativity(mix):
    """Newman's coefficient of mixing matrices [..., C, C]: e = mix / mix.sum(), a and b its row and column sums,
    (sum_a e_aa - sum_a a_a b_a) / (1 - sum_a a_a b_a); NaN where there is no edge or the denominator is 0."""
    mix = np.asarray(mix, dtype=np.float64)
    e = _ratio(mix, mix.sum(axis=(-2, -1), keepdims=True))
    ab = (e.sum(-1) * e.sum(-2)).sum(-1)
    return _ratio(np.trace(e, axis1=-2, axis2=-1) - ab, 1.0 - ab)


def _derive(mix, mutual, overlap, sizes, skip_diagonal):
    """name -> array of every ratio, from tables of integers (per sample) or of expectations (then: ratios of expectations)."""
    out = {}
    if mix is not None:
        tot = mix.sum(axis=(-2, -1))
        internal = np.trace(mix, axis1=-2, axis2=-1)
        out["assortativity"] = _assortativity(mix)
        out["ei_index"] = _ratio((tot - internal) - internal, tot)
        out["within_share"] = _ratio(np.diagonal(mix, axis1=-2, axis2=-1), mix.sum(-1))
        pairs = np.outer(sizes, sizes) - (np.diag(sizes) if skip_diagonal else 0)
        out["block_density"] = _ratio(mix, np.broadcast_to(pairs, mix.shape))
        if mutual is not None:
            out["block_reciprocity"] = _ratio(mutual, mix)
    if overlap is not None:
        e = np.diagonal(overlap, axis1=-2, axis2=-1)
        out["jaccard"] = _ratio(overlap, e[..., :, None] + e[..., None, :] - overlap)
    return out


class MixingStats:
    """Per sample s and layer l (sample s is the draw of seed + s); with groups (None otherwise):
      mix, mutual          int64 [S, L, C, C]: mix[s, l, a, b] = #{(i, j) : g_i = a, g_j = b, Y_lij > 0}, mutual the same over the ties
                           that are reciprocated (ordered pairs: symmetric in (a, b))
      labels, group_sizes  [C]: the label code a stands for (`np.unique`'s order) and the number n_a of nodes that carry it
      assortativity        [S, L]: with e = mix / mix.sum(), a its row sums and b its column sums,
                           (sum_a e_aa - sum_a a_a b_a) / (1 - sum_a a_a b_a) -- Newman's coefficient,
                           `networkx.attribute_assortativity_coefficient` of the directed sample restricted to the labelled nodes
      ei_index             [S, L]: (external - internal) / (external + internal), internal = sum_a mix_aa
      within_share         [S, L, C]: mix_aa / sum_b mix_ab
      block_density        [S, L, C, C]: mix_ab / (n_a n_b, less n_a on the diagonal when skip_diagonal)
      block_reciprocity    [S, L, C, C]: mutual_ab / mix_ab
    and with the overlap (None otherwise):
      overlap              int64 [S, L, L]: #{(i, j) : Y_lij > 0 and Y_l'ij > 0} over all nodes; its diagonal is the edge count e_l
      jaccard              [S, L, L]: overlap_ll' / (e_l + e_l' - overlap_ll')
    Every ratio is NaN where its denominator is 0.  expected: dict of float64 arrays without the S axis -- `mix`, `mutual`,
    `overlap` (`CaviEngine.expected_mixing`: exact expectations of the counts under q(Y) = prod rho) and the same ratios formed
    from them: RATIOS OF EXPECTATIONS, not expectations of the ratios -- take those from the samples."""

    def __init__(self, N, counts, codes=None, labels=None, expected=None, skip_diagonal=True, seed=None, n_trials=1):
        self.N, self.skip_diagonal = int(N), bool(skip_diagonal)
        self.seed, self.n_trials = seed, int(n_trials)
        self.mix = self.mutual = self.overlap = self.labels = self.group_sizes = self.codes = None
        for k in ("mix", "mutual", "overlap"):
            if counts.get(k) is not None:
                setattr(self, k, np.asarray(counts[k], dtype=np.int64))
        if self.mix is None and self.overlap is None:
            raise ValueError("neither a mixing matrix nor an overlap table")
        first = self.mix if self.mix is not None else self.overlap
        self.S, self.L = first.shape[:2]
        self.C = 0
        if self.mix is not None:
            self.C = self.mix.shape[-1]
            self.codes = np.asarray(codes, dtype=np.int32)
            self.labels = np.arange(self.C) if labels is None else np.asarray(labels)
            self.group_sizes = np.bincount(self.codes[self.codes >= 0], minlength=self.C).astype(np.int64)
        for k in ("assortativity", "ei_index", "within_share", "block_density", "block_reciprocity", "jaccard"):
            setattr(self, k, None)
        for k, v in _derive(self.mix, self.mutual, self.overlap, self.group_sizes, self.skip_diagonal).items():
            setattr(self, k, v)
        self.expected = None
        if expected is not None:
            ex = {k: np.asarray(expected[k], dtype=np.float64) for k in ("mix", "mutual", "overlap") if expected.get(k) is not None}
            ex.update(_derive(ex.get("mix"), ex.get("mutual"), ex.get("overlap"), self.group_sizes, self.skip_diagonal))
            self.expected = ex

    def statistics(self):
        """name -> [S, L] array of every per-sample statistic of a layer: with groups the assortativity, the E-I index, the
        internal and external edge counts and `within_share:<label>`; with the overlap `edges` and `jaccard:<layer>`."""
        out = {}
        if self.mix is not None:
            internal = np.trace(self.mix, axis1=-2, axis2=-1)
            out.update({"assortativity": self.assortativity, "ei_index": self.ei_index, "internal": internal,
                        "external": self.mix.sum(axis=(-2, -1)) - internal})
            for a in range(self.C):
                out["within_share:%s" % (self.labels[a],)] = self.within_share[..., a]
        if self.overlap is not None:
            out["edges"] = np.diagonal(self.overlap, axis1=-2, axis2=-1)
            for l2 in range(self.L):
                out["jaccard:%d" % l2] = self.jaccard[..., l2]
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
        """The mixing matrix as a long table: one row per (layer, from, to) -- the labels of the two groups -- with the mean, std
        and quantiles q of mix over the samples and, when the expectations are there, `expected`."""
        import pandas as pd
        if self.mix is None:
            raise ValueError("no groups were given: there is no mixing matrix")
        q = tuple(float(x) for x in q)
        rows = []
        for l in range(self.L):
            for a in range(self.C):
                for b in range(self.C):
                    row = {"layer": l, "from": self.labels[a], "to": self.labels[b]}
                    row.update(quantile_row(self.mix[:, l, a, b], q))
                    if self.expected is not None and "mix" in self.expected:
                        row["expected"] = float(self.expected["mix"][l, a, b])
                    rows.append(row)
        cols = ["layer", "from", "to", "mean", "std"] + ["q%g" % x for x in q]
        return pd.DataFrame(rows, columns=cols + (["expected"] if self.expected is not None and "mix" in self.expected else []))
