"""The network-statistics contract restated in NumPy (the table of include/vimure_hip.h at vmr_sample_stats): what
tests/test_netstats_host.py pins against `calculate_overall_reciprocity` and tests/test_hip_netstats.py holds the device to."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NETSTATS_CASES = ("A_ones_mut", "B_random_mask_K3", "C_ones_nomut", "D_self_mask", "E_undirected", "L_default_K12", "M_K16_nomut")


def load_netstats(case):
    return dict(np.load(os.path.join(GOLDEN, "netstats", "Q_netstats_" + case.split("_")[0] + ".npz")))


def stats_np(Ys, Y_ref=None):
    """Ys: samples [S][L,N,N] (a list or an array).  Returns the dict `CaviEngine.sample_stats(..., degrees=True)` returns:
    edges, weight, mutual, tp int64 [S, L] over all (i, j) of a layer, the diagonal included; deg_out, deg_in int32 [S, L, N]."""
    Ys = np.asarray(Ys)
    S, L, N, _ = Ys.shape
    out = {k: np.zeros((S, L), np.int64) for k in ("edges", "weight", "mutual", "tp")}
    out["deg_out"], out["deg_in"] = np.zeros((S, L, N), np.int32), np.zeros((S, L, N), np.int32)
    for s in range(S):
        for l in range(L):
            Y = Ys[s, l].astype(np.int64)
            out["edges"][s, l] = (Y > 0).sum()
            out["weight"][s, l] = Y.sum()
            out["mutual"][s, l] = np.logical_and(Y > 0, Y.T > 0).sum()
            if Y_ref is not None:
                out["tp"][s, l] = ((Y > 0) & (np.asarray(Y_ref)[l] > 0)).sum()
            out["deg_out"][s, l] = (Y > 0).sum(axis=1)
            out["deg_in"][s, l] = (Y > 0).sum(axis=0)
    return out


def expected_np(rho):
    """What `CaviEngine.expected_stats()` returns for rho [L,N,N,K], with p_ij = sum_{k>=1} rho_ijk: float64 [L] arrays."""
    rho = np.asarray(rho, dtype=np.float64)
    K = rho.shape[-1]
    p = rho[..., 1:].sum(-1)
    return {"edges": p.sum(axis=(1, 2)), "weight": (rho * np.arange(K)).sum(axis=(1, 2, 3)),
            "mutual": np.einsum("lij,lji->l", p, p), "edges_var": (p * (1.0 - p)).sum(axis=(1, 2))}
