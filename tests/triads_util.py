"""The triad contract restated in NumPy (the tables of include/vimure_hip.h at vmr_sample_triads and vmr_expected_triads), with
int64 / float64 matrix products and nothing of the device code: what tests/test_triads_host.py pins against brute force and exact
enumeration and tests/test_hip_triads.py holds the device to."""
import numpy as np

TRIAD_KEYS = ("transitive", "cyclic", "two_paths", "triangles_u", "wedges_u", "edges_u")


def triads_np(Ys):
    """Ys: samples [S][L,N,N] (a list or an array).  Returns the dict `CaviEngine.sample_triads(..., nodes=True)` returns: the six
    counts int64 [S, L] and node_tri, node_deg int32 [S, L, N], for A = (Y > 0) without its diagonal and U = A | A.T."""
    Ys = np.asarray(Ys)
    S, L, N, _ = Ys.shape
    out = {k: np.zeros((S, L), np.int64) for k in TRIAD_KEYS}
    out["node_tri"], out["node_deg"] = np.zeros((S, L, N), np.int32), np.zeros((S, L, N), np.int32)
    for s in range(S):
        for l in range(L):
            A = (Ys[s, l] > 0).astype(np.int64)
            np.fill_diagonal(A, 0)
            U = ((A + A.T) > 0).astype(np.int64)
            AA, UU = A @ A, U @ U
            d = U.sum(axis=1)
            U3 = np.einsum("ij,ji->i", UU, U)            # diag(U^3): closed walks of length 3 from every node
            out["transitive"][s, l] = ((A @ A.T) * A).sum()
            out["cyclic"][s, l] = (AA * A.T).sum()
            out["two_paths"][s, l] = AA.sum() - np.trace(AA)
            out["triangles_u"][s, l] = U3.sum() // 6
            out["wedges_u"][s, l] = (d * (d - 1) // 2).sum()
            out["edges_u"][s, l] = np.triu(U, 1).sum()
            out["node_tri"][s, l] = U3 // 2
            out["node_deg"][s, l] = d
    return out


def expected_triads_np(rho):
    """rho [L,N,N,K].  Returns the dict `CaviEngine.expected_triads()` returns (float64 [L] per count): p_ij = sum_{k>=1} rho_ijk,
    p_ii := 0, u_ij = 1 - (1 - p_ij)(1 - p_ji) off the diagonal."""
    rho = np.asarray(rho, dtype=np.float64)
    L, N = rho.shape[0], rho.shape[1]
    out = {k: np.zeros(L) for k in TRIAD_KEYS}
    for l in range(L):
        P = rho[l][..., 1:].sum(-1)
        np.fill_diagonal(P, 0.0)
        U = 1.0 - (1.0 - P) * (1.0 - P.T)
        np.fill_diagonal(U, 0.0)
        s = U.sum(axis=1)
        out["transitive"][l] = (P * (P @ P.T)).sum()
        out["cyclic"][l] = ((P @ P) * P.T).sum()
        out["two_paths"][l] = (P.sum(axis=0) * P.sum(axis=1)).sum() - (P * P.T).sum()
        out["triangles_u"][l] = np.trace(U @ U @ U) / 6.0
        out["wedges_u"][l] = ((s * s).sum() - (U * U).sum()) / 2.0
        out["edges_u"][l] = np.triu(U, 1).sum()
    return out
