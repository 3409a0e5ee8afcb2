"""Host helpers of the reference's `utils` module that judge a fit.

`calculate_AUC` is the reference's (latentnetworks/vimure utils.py:40-66): sklearn's `auc(*roc_curve(...)[:2])`, restated as
the exact rank statistic it equals -- the probability that a positive outscores a negative, ties counted half -- so that no
sklearn is needed and the value is the same rational number the device computes (`CaviEngine.report_auc`).

`calculate_overall_reciprocity` (reference utils.py:69-70) and `calculate_expected_reciprocity` (the quotient of the reference's
reciprocity notebook) are the host forms of what `CaviEngine.sample_stats` / `expected_stats` count on the device.
"""
import warnings

import numpy as np


def calculate_AUC(pred, data0, mask=None):
    """AUC of the scores `pred` against the labels `data0 > 0`, over the entries where `mask > 0` (all entries without a
    mask): (#{(p, n) : pred_p > pred_n} + #{(p, n) : pred_p = pred_n} / 2) / (P Q).  NaN with a warning when there are no
    positives or no negatives, as sklearn gives."""
    pred = np.asarray(pred)
    data = np.asarray(data0) > 0
    if mask is None:
        score, label = pred.ravel(), data.ravel()
    else:
        sel = np.asarray(mask) > 0
        score, label = pred[sel], data[sel]
    score = score.astype(np.float64, copy=False)
    pos, neg = score[label], score[~label]
    P, Q = int(pos.size), int(neg.size)
    if P == 0 or Q == 0:
        warnings.warn("No %s samples in the masked labels: the AUC is undefined" % ("positive" if P == 0 else "negative"),
                      UserWarning)
        return float("nan")
    neg = np.sort(neg)
    below = np.searchsorted(neg, pos, side="left")     # negatives strictly below each positive
    upto = np.searchsorted(neg, pos, side="right")     # ... and those equal to it
    u2 = 2 * int(below.sum(dtype=np.int64)) + int((upto - below).sum(dtype=np.int64))
    return u2 / (2 * P * Q)   # (Python integers: the quotient is rounded once)


def calculate_overall_reciprocity(Y):
    """Reciprocity of one network Y [N, N]: #{(i, j) : Y_ij > 0 and Y_ji > 0} / sum Y, over all ordered pairs, the diagonal
    included.  Integer counts, one division: NaN (0 / 0) for an empty network, as NumPy gives."""
    Y = np.asarray(Y)
    if Y.ndim != 2 or Y.shape[0] != Y.shape[1]:
        raise ValueError("Y must be one square adjacency matrix [N, N]")
    on = Y > 0
    mutual = int(np.count_nonzero(on & on.T))
    weight = Y.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float64(mutual) / np.float64(weight)


def calculate_expected_reciprocity(rho1):
    """Expected reciprocity of one layer under independent edges with probabilities p = rho1 [N, N] (for K = 2, rho[l, :, :, 1];
    in general the sum of rho over the categories k >= 1): sum_ij p_ij p_ji / sum_ij p_ij."""
    p = np.asarray(rho1, dtype=np.float64)
    if p.ndim != 2 or p.shape[0] != p.shape[1]:
        raise ValueError("rho1 must be one square matrix of edge probabilities [N, N]")
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float64((p * p.T).sum()) / np.float64(p.sum())
