"""Shared by tests/test_score_truth_host.py and tests/test_hip_score_truth.py: a brute-force pair count for the AUC, the exact
comparison of the integer outputs of `score_truth`, the derived bound of its sums, and a stub engine that answers `score_truth`
from the NumPy restatement (vimure_amd/scoring.py) so that `VimureModel.score_truth` runs without a GPU."""
import numpy as np

INT_KEYS = ("hist", "conf", "auc_pairs", "n_ties")


def brute_u2(s, b):
    """2 #{(p,n) : s_p > s_n} + #{(p,n) : s_p = s_n} by the O(P Q) definition; s, b flat."""
    pos, neg = s[b][:, None], s[~b][None, :]
    return int(2 * np.sum(pos > neg) + np.sum(pos == neg))


def sums_rtol(n_ties):
    """Any summation order of n non-negative terms, each good to a few ulp: (n + 8) 2^-52 relative."""
    return (int(n_ties) + 8) * 2.0 ** -52


def assert_ints_equal(got, want, keys=INT_KEYS):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (k, g.shape, w.shape)
        assert np.array_equal(g.astype(np.int64), w.astype(np.int64)), (k, np.argwhere(g != w)[:8])


def assert_sums_close(got, want, n_ties):
    g, w = np.asarray(got["sums"]), np.asarray(want["sums"])
    assert g.shape == w.shape
    assert np.all(np.abs(g - w) <= sums_rtol(n_ties) * np.abs(w)), (g, w, np.abs(g - w) / np.maximum(np.abs(w), 1e-300))


def assert_auc_close(got, want, tol=1e-12):
    g, w = np.asarray(got["auc"]), np.asarray(want["auc"])
    assert np.array_equal(np.isnan(g), np.isnan(w)), (g, w)
    assert np.all(np.abs(g - w)[~np.isnan(w)] <= tol), (g, w)


class StubEngine:
    """What a model keeps after fit(keep_engine=True), answering `score_truth` from the restatement (no GPU)."""

    def __init__(self, rho):
        self.rho = rho
        self.calls = []

    def score_truth(self, Y_true, thresholds=None, score="rho1", skip_diagonal=False, auc=True, outputs=None):
        from vimure_amd.scoring import score_truth_np
        self.calls.append((np.asarray(thresholds).tolist(), score, bool(skip_diagonal), bool(auc), outputs))
        out = score_truth_np(self.rho, Y_true, thresholds, score, skip_diagonal)
        if not auc:
            out["auc"], out["auc_pairs"] = None, None
        return out

    def close(self):
        pass
