"""The expected-report contract restated in NumPy (reference model.py:1220-1293 over a dense R): what tests/test_ppc_host.py
pins against the reference's recorded values and tests/test_hip_ppc.py holds the device to."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PPC_CASES = ("A_ones_mut", "B_random_mask_K3", "C_ones_nomut", "D_self_mask", "E_undirected", "L_default_K12")


def load_ppc(case):
    return dict(np.load(os.path.join(GOLDEN, "ppc", "P_mean_poisson_" + case.split("_")[0] + ".npz")))


def mean_poisson_np(X, R, rho, G_theta, G_lambda, G_nu, mutuality):
    """(subs, vals) over the support of R (every entry when R is None), lexicographic order:
    vals = sum_k rho[l,i,j,k] (G_theta[l,m] G_lambda[l,k] + G_nu XT[l,i,j,m]), XT = X[l,j,i,m] with mutuality, else 0.
    The sum runs over k ascending from 0.0 in elementwise operations, every product and every sum rounded on its own: the order
    the device states, so that its values can be held to these bit for bit (an einsum's order and fusing vary with the build)."""
    X = np.asarray(X)
    R = np.ones(X.shape, bool) if R is None else (np.asarray(R) != 0)
    l, i, j, m = np.nonzero(R)
    xt = X[l, j, i, m].astype(np.float64) if mutuality else np.zeros(len(l))
    nx = G_nu * xt
    vals = np.zeros(len(l))
    for k in range(rho.shape[-1]):
        vals = vals + rho[l, i, j, k] * (G_theta[l, m] * G_lambda[l, k] + nx)
    return (l, i, j, m), vals


def dense_of(subs, vals, shape):
    out = np.zeros(shape)
    out[tuple(np.asarray(s, dtype=np.int64) for s in subs)] = vals
    return out
