"""The reference's synthetic experiment drivers, with the scoring on the GPU.

`unreliable_reporters` is the counterpart of notebooks/python/experiments/unreliable_reporters.py `main` (`karnataka.main` has
`batch.run_karnataka`): a grid over (seed, theta_ratio, exaggeration_type, mutuality) on one Multitensor ground truth, every cell
a fit scored against the truth.  Where the reference wraps the fit in a scikit-learn estimator and lets `GridSearchCV` score a
dense thresholded read-out with `f1_score` and `mean_squared_error` (:189-200, 358-361), the fit here keeps its posteriors on
the device and `VimureModel.score_truth` returns the counts.
"""
import time
import warnings

import numpy as np
import pandas as pd

from .model import VimureModel
from .synthetic import Multitensor, build_custom_theta

DEFAULT_THETA_RATIO_VALS = [0.01, 0.02, 0.03, 0.05, 0.08, 0.10, 0.15, 0.20, 0.30, 0.40, 0.50]
DEFAULT_PSEUDO_RANDOM_SEEDS = np.arange(10)   # 10 realisations of every scenario
DEFAULT_ETA = 0.0                             # without mutuality
LAMBDA_0, LAMBDA_DIFF = 0.01, 0.99


def make_dataset(gt, theta_ratio, exaggeration_type, seed, eta=DEFAULT_ETA, exact=None):
    """(X, R, theta) of one scenario on the ground truth `gt`: a random `theta_ratio` of the reporters under- or over-report,
    everybody reports on their own ties only -- `build_custom_theta` and `_build_X` called as the reference's estimator calls
    them (unreliable_reporters.py:108-130).  exact: the generator mode of `_build_X` (True: the reference's stream)."""
    theta = build_custom_theta(gt, theta_ratio=theta_ratio, exaggeration_type=exaggeration_type, seed=seed)
    gt._build_X(mutuality=eta, theta=theta, cutoff_X=False, lambda_diff=LAMBDA_DIFF, flag_self_reporter=True, seed=seed, exact=exact)
    return gt.X, gt.R, gt.theta


def unreliable_reporters(available_seeds=DEFAULT_PSEUDO_RANDOM_SEEDS, theta_ratio_vals=DEFAULT_THETA_RATIO_VALS,
                         exaggeration_type=("under", "over"), mutuality=(True, False), reciprocity_Y=0.2, eta=DEFAULT_ETA,
                         gt_network_seed=25, verbose=False, threshold=0.01, device=None, exact=None, N=100, M=None, L=1, C=2, K=2,
                         avg_degree=5, num_realisations=10, max_iter=21):
    """Runs the grid and returns a DataFrame with one row per cell: param_seed, param_theta_ratio, param_exaggeration_type,
    param_mutuality, mean_test_f1 (F1 of `rho_1 >= threshold` against the truth), mean_test_mse = -(fp + fn) / n (the sign the
    reference's `make_scorer(mean_squared_error, greater_is_better=False)` gives; of 0/1 arrays the squared error counts the
    disagreements), auc, brier, mean_fit_time and eta.  Parameters and defaults of the reference's `main` (:36-42, 203-215; its
    keyword extras N, M, L, C, K, avg_degree, num_realisations, max_iter spelled out); threshold: the fixed threshold of its
    `predict` (0.01); device: the GPU of the fits; exact: the generator mode of the ground truth and of X (None: by size).
    One dataset serves both mutuality settings of a (seed, theta_ratio, exaggeration_type).  A plain loop of fits."""
    if L > 1:
        raise ValueError("Invalid L. This experiment only supports single-layer currently.")
    M = N if M is None else M
    gt = Multitensor(N=N, M=M, L=1, C=C, K=K, eta=reciprocity_Y, ExpM=None, avg_degree=avg_degree, sparsify=True, seed=gt_network_seed,
                     exact=exact)
    Y = gt.Y.toarray() if hasattr(gt.Y, "toarray") else np.asarray(gt.Y)
    # the single-layer ground-truth lambda as the prior's mean (:163-166)
    lambda_k_GT = np.array([[LAMBDA_0, LAMBDA_0 + LAMBDA_DIFF]])
    beta_lambda = 10000 * np.ones(lambda_k_GT.shape)
    alpha_lambda = lambda_k_GT * beta_lambda
    rows = []
    for seed in available_seeds:
        for theta_ratio in theta_ratio_vals:
            for ex in exaggeration_type:
                X, R, _ = make_dataset(gt, theta_ratio, ex, int(seed), eta=eta, exact=exact)
                for mut in mutuality:
                    t0 = time.time()
                    with warnings.catch_warnings():
                        if not verbose:
                            warnings.simplefilter("ignore")
                        model = VimureModel(mutuality=bool(mut), verbose=verbose)
                        model.fit(X, K=gt.K, seed=int(seed), theta_prior=(0.1, 0.1), eta_prior=(0.5, 1), alpha_lambda=alpha_lambda,
                                  beta_lambda=beta_lambda, num_realisations=num_realisations, max_iter=max_iter, R=R, bias0=0.2,
                                  keep_engine=True, device=device)
                    fit_time = time.time() - t0
                    try:
                        ts = model.score_truth(Y, thresholds=[threshold])
                    finally:
                        model.close()
                    n = int(ts.n_ties[0])
                    rows.append({"param_seed": str(seed), "param_theta_ratio": float(theta_ratio), "param_exaggeration_type": ex,
                                 "param_mutuality": bool(mut), "mean_test_f1": float(ts.f1[0, 0]),
                                 "mean_test_mse": -float(ts.fp[0, 0] + ts.fn[0, 0]) / n, "auc": float(ts.auc[0]),
                                 "brier": float(ts.brier[0]), "mean_fit_time": fit_time, "eta": eta})
    cols = ["param_seed", "param_theta_ratio", "param_exaggeration_type", "param_mutuality", "mean_test_f1", "mean_test_mse", "auc",
            "brier", "mean_fit_time", "eta"]
    return pd.DataFrame(rows, columns=cols)
