"""The posterior scored against a ground-truth network: the host side of `VimureModel.score_truth`.

`score_truth_np` restates vmr_score_truth (include/vimure_hip.h) in NumPy -- the oracle of the device pass and the path of a
model whose rho is already on the host; `TruthScore` holds the integers and sums either of them returns and derives what the
reference's synthetic experiments report from them (F1 at a threshold: notebooks/python/experiments/unreliable_reporters.py:189-200;
the threshold choice of `utils.get_optimal_threshold`; AUC, Brier score, calibration).
"""
import numpy as np

from .netstats import _ratio

SCORES = ("rho1", "prob")
CONF_NAMES = ("argmax_tp", "argmax_fp", "argmax_fn", "argmax_equal", "positives")
SUM_NAMES = ("sum_score", "sum_score_positives", "brier_numerator", "mse_numerator")


def default_thresholds():
    return np.linspace(0, 1, 101)


def check_thresholds(thresholds):
    """float64 [n_thr]: finite and non-decreasing (duplicates allowed); None: `default_thresholds()`."""
    thr = default_thresholds() if thresholds is None else np.ascontiguousarray(np.atleast_1d(thresholds), dtype=np.float64)
    if thr.ndim != 1:
        raise ValueError("thresholds: a 1-D sequence expected")
    if not np.all(np.isfinite(thr)):
        raise ValueError("thresholds: a threshold is not finite")
    if np.any(np.diff(thr) < 0):
        raise ValueError("thresholds: the thresholds decrease")
    return thr


def tie_scores_np(rho, score="rho1"):
    """(s, a, mean) of every tie, each [L,N,N]: the score, the first maximum of rho, and sum_k k rho_k; prob and mean as explicit
    ascending loops, every product and sum rounded on its own (np.sum and np.dot add in another order)."""
    rho = np.asarray(rho, dtype=np.float64)
    if score not in SCORES:
        raise ValueError("score must be \"rho1\" or \"prob\"")
    K = rho.shape[-1]
    prob, mean = np.zeros(rho.shape[:-1]), np.zeros(rho.shape[:-1])
    for k in range(1, K):
        prob = prob + rho[..., k]
        mean = mean + float(k) * rho[..., k]
    s = rho[..., 1] if score == "rho1" else prob
    return s, np.argmax(rho, axis=-1), mean


def score_truth_np(rho, Y_true, thresholds=None, score="rho1", skip_diagonal=False):
    """vmr_score_truth in NumPy.  rho [L,N,N,K], Y_true [L,N,N] (non-negative integers).  Returns the dict `CaviEngine.score_truth`
    returns: hist int64 [L, n_thr + 1, 2], conf int64 [L, 5], sums float64 [L, 4] (NumPy's summation order: equal to the device's
    up to rounding), auc float64 [L], auc_pairs int64 [L, 2] = (U2, Q), n_ties int64 [L], thresholds."""
    rho = np.asarray(rho, dtype=np.float64)
    Y = np.asarray(Y_true)
    if rho.ndim != 4 or rho.shape[1] != rho.shape[2] or rho.shape[3] < 2:
        raise ValueError("rho must have shape (L, N, N, K)")
    if Y.shape != rho.shape[:3]:
        raise ValueError(f"Y_true has shape {Y.shape}, the networks {rho.shape[:3]}")
    thr = check_thresholds(thresholds)
    L, N = rho.shape[0], rho.shape[1]
    s, a, mean = tie_scores_np(rho, score)
    if np.isnan(s).any():
        raise ValueError("score_truth: a score is NaN")
    keep = ~np.eye(N, dtype=bool) if skip_diagonal else np.ones((N, N), bool)
    n_thr = thr.shape[0]
    hist = np.zeros((L, n_thr + 1, 2), np.int64)
    conf = np.zeros((L, 5), np.int64)
    sums = np.zeros((L, 4))
    auc = np.full(L, np.nan)
    pairs = np.zeros((L, 2), np.int64)
    n_ties = np.full(L, int(keep.sum()), np.int64)
    for l in range(L):
        sl, al, ml, yl = s[l][keep], a[l][keep], mean[l][keep], Y[l][keep].astype(np.int64)
        b = yl > 0
        c = np.searchsorted(thr, sl, side="right")          # #{tau : thr[tau] <= s}
        for bit in (0, 1):
            hist[l, :, bit] = np.bincount(c[b == bool(bit)], minlength=n_thr + 1)
        conf[l] = [np.sum((al > 0) & b), np.sum((al > 0) & ~b), np.sum((al == 0) & b), np.sum(al == yl), np.sum(b)]
        sums[l] = [sl.sum(), sl[b].sum(), np.sum((sl - b) ** 2), np.sum((ml - yl) ** 2)]
        pos, neg = np.sort(sl[b]), sl[~b]
        P, Q = pos.shape[0], neg.shape[0]
        lo, hi = np.searchsorted(pos, neg, side="left"), np.searchsorted(pos, neg, side="right")
        U2 = int(2 * np.sum(P - hi, dtype=np.int64) + np.sum(hi - lo, dtype=np.int64))
        pairs[l] = (U2, Q)
        if P and Q:
            auc[l] = U2 / (2.0 * P * Q)
    return {"hist": hist, "conf": conf, "sums": sums, "auc": auc, "auc_pairs": pairs, "n_ties": n_ties, "thresholds": thr}


class TruthScore:
    """What `score_truth` returns, per layer l (see vmr_score_truth):
      hist [L, n_thr + 1, 2]   hist[l, c, b]: ties whose score s has exactly c thresholds <= s, by truth b = (Y_true > 0)
      conf [L, 5]              of the arg-max read-out a: #{a>0, b}, #{a>0, not b}, #{a=0, b}, #{a = Y_true}, P = #{b}
      sums [L, 4]              sum s, sum_b s, sum (s - b)^2, sum (mean - Y_true)^2
      auc [L], auc_pairs [L, 2] = (U2, Q)   -- None when the AUC was not asked for
      n_ties [L]               ties scored (N^2, or N^2 - N without the diagonal)
    result: the dict of `CaviEngine.score_truth` or `score_truth_np`; thresholds: those of the call (default: the dict's).
    heuristic: (threshold, hist [L, 2, 2] of a call with that one threshold) -- the reference's 0.54 G_exp_nu - 0.01, for `summary`.
    Every quotient is NaN where its denominator is 0."""

    def __init__(self, result, thresholds=None, heuristic=None, score=None, skip_diagonal=None):
        thr = result.get("thresholds") if thresholds is None else thresholds
        if thr is None:
            raise ValueError("thresholds: the result does not carry them")
        self.thresholds = np.asarray(thr, dtype=np.float64).reshape(-1)
        self.conf = np.asarray(result["conf"], dtype=np.int64)
        self.L = self.conf.shape[0]
        self.hist = np.asarray(result["hist"], dtype=np.int64)
        if self.hist.shape != (self.L, self.thresholds.shape[0] + 1, 2):
            raise ValueError(f"hist has shape {self.hist.shape}, expected {(self.L, self.thresholds.shape[0] + 1, 2)}")
        self.sums = np.asarray(result["sums"], dtype=np.float64)
        self.n_ties = np.asarray(result["n_ties"], dtype=np.int64).reshape(self.L)
        self._auc = None if result.get("auc") is None else np.asarray(result["auc"], dtype=np.float64)
        self.auc_pairs = None if result.get("auc_pairs") is None else np.asarray(result["auc_pairs"], dtype=np.int64)
        self.score, self.skip_diagonal = score, skip_diagonal
        self.heuristic_threshold, self._heuristic_hist = None, None
        if heuristic is not None:
            self.heuristic_threshold = float(heuristic[0])
            self._heuristic_hist = np.asarray(heuristic[1], dtype=np.int64).reshape(self.L, 2, 2)

    # -- counts at every threshold: [L, n_thr]
    @staticmethod
    def _above(hist):
        """[L, n_thr, 2]: ties with s >= thresholds[tau], by truth -- the suffix sums over c > tau."""
        return np.cumsum(hist[:, ::-1, :], axis=1)[:, ::-1, :][:, 1:, :]

    @property
    def positives(self):
        return self.conf[:, 4]

    @property
    def tp(self):
        return self._above(self.hist)[:, :, 1]

    @property
    def fp(self):
        return self._above(self.hist)[:, :, 0]

    @property
    def fn(self):
        return self.positives[:, None] - self.tp

    @property
    def tn(self):
        return (self.n_ties - self.positives)[:, None] - self.fp

    @property
    def precision(self):
        return _ratio(self.tp, self.tp + self.fp)

    @property
    def recall(self):
        return _ratio(self.tp, self.tp + self.fn)

    @property
    def f1(self):
        """[L, n_thr]: 2 tp / (2 tp + fp + fn), sklearn.metrics.f1_score of `s >= threshold` against `Y_true > 0`."""
        return _ratio(2 * self.tp, 2 * self.tp + self.fp + self.fn)

    def curve(self):
        """DataFrame with a row per (layer, threshold): tp, fp, fn, tn, precision, recall, f1."""
        import pandas as pd
        n = self.thresholds.shape[0]
        cols = {"layer": np.repeat(np.arange(self.L), n), "threshold": np.tile(self.thresholds, self.L)}
        for k in ("tp", "fp", "fn", "tn", "precision", "recall", "f1"):
            cols[k] = np.asarray(getattr(self, k)).reshape(-1)
        return pd.DataFrame(cols)

    def _index_of(self, threshold):
        at = np.flatnonzero(self.thresholds == float(threshold))
        if at.size == 0:
            raise ValueError(f"{threshold!r} is not one of the thresholds scored")
        return int(at[0])

    def f1_at(self, threshold):
        """[L]: F1 of `s >= threshold`; the threshold must be one of those scored."""
        return self.f1[:, self._index_of(threshold)]

    def best_threshold(self):
        """[L]: the first threshold of maximal F1 (NaN where no threshold has a defined F1)."""
        out = np.full(self.L, np.nan)
        f1 = self.f1
        for l in range(self.L):
            if f1.shape[1] and not np.all(np.isnan(f1[l])):
                out[l] = self.thresholds[int(np.nanargmax(f1[l]))]
        return out

    def best_f1(self):
        f1 = self.f1
        return np.array([np.nanmax(f1[l]) if f1.shape[1] and not np.all(np.isnan(f1[l])) else np.nan for l in range(self.L)])

    # -- the arg-max read-out and the threshold-free scores: [L]
    @property
    def argmax_f1(self):
        """F1 of `argmax_k rho > 0` against `Y_true > 0` (what `get_inferred_model("rho_max")` infers)."""
        return _ratio(2 * self.conf[:, 0], 2 * self.conf[:, 0] + self.conf[:, 1] + self.conf[:, 2])

    @property
    def accuracy(self):
        """Share of ties whose arg-max category equals Y_true."""
        return _ratio(self.conf[:, 3], self.n_ties)

    @property
    def auc(self):
        return np.full(self.L, np.nan) if self._auc is None else self._auc

    @property
    def brier(self):
        return _ratio(self.sums[:, 2], self.n_ties)

    @property
    def mse(self):
        """mean (sum_k k rho_k - Y_true)^2."""
        return _ratio(self.sums[:, 3], self.n_ties)

    @property
    def heuristic_f1(self):
        """[L]: F1 at the reference's heuristic threshold, or None when it was not scored."""
        if self._heuristic_hist is None:
            return None
        tp, fp = self._heuristic_hist[:, 1, 1], self._heuristic_hist[:, 1, 0]
        fn = self.positives - tp
        return _ratio(2 * tp, 2 * tp + fp + fn)

    def calibration(self):
        """DataFrame with a row per (layer, bin): the bins between consecutive thresholds -- bin c holds the ties with
        thresholds[c - 1] <= s < thresholds[c] (-inf and +inf at the ends) -- with count, positives, and the observed frequency
        positives / count."""
        import pandas as pd
        edges = np.concatenate([[-np.inf], self.thresholds, [np.inf]])
        nb = self.hist.shape[1]
        count, pos = self.hist.sum(axis=2), self.hist[:, :, 1]
        return pd.DataFrame({"layer": np.repeat(np.arange(self.L), nb), "bin": np.tile(np.arange(nb), self.L),
                             "lower": np.tile(edges[:-1], self.L), "upper": np.tile(edges[1:], self.L),
                             "count": count.reshape(-1), "positives": pos.reshape(-1), "frequency": _ratio(pos, count).reshape(-1)})

    def summary(self):
        """DataFrame with a row per layer: n_ties, positives, auc, brier, mse, accuracy, argmax_f1, best_threshold, best_f1 and,
        when scored, heuristic_threshold and heuristic_f1."""
        import pandas as pd
        cols = {"layer": np.arange(self.L), "n_ties": self.n_ties, "positives": self.positives, "auc": self.auc, "brier": self.brier,
                "mse": self.mse, "accuracy": self.accuracy, "argmax_f1": self.argmax_f1, "best_threshold": self.best_threshold(),
                "best_f1": self.best_f1()}
        if self.heuristic_threshold is not None:
            cols["heuristic_threshold"] = np.full(self.L, self.heuristic_threshold)
            cols["heuristic_f1"] = self.heuristic_f1
        return pd.DataFrame(cols)
