"""Host helpers of the reference's `utils` module that judge a fit.

`calculate_AUC` is the reference's (latentnetworks/vimure utils.py:40-66): sklearn's `auc(*roc_curve(...)[:2])`, restated as
the exact rank statistic it equals -- the probability that a positive outscores a negative, ties counted half -- so that no
sklearn is needed and the value is the same rational number the device computes (`CaviEngine.report_auc`).
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
