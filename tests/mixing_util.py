"""The mixing contract restated in NumPy (the tables of include/vimure_hip.h at vmr_sample_mixing and vmr_expected_mixing), with
nothing of the device code: what tests/test_mixing_host.py pins against plain loops and exact enumeration, and
tests/test_hip_mixing.py holds the device to."""
import numpy as np

MIX_KEYS = ("mix", "mutual", "overlap")


def mixing_np(Ys, groups, C, skip_diagonal):
    """Ys: samples [S][L,N,N]; groups: N codes in [0, C), -1 for a node left out of mix and mutual, or None (then C = 0 and the
    two tables are empty).  Returns what `CaviEngine.sample_mixing` returns: mix, mutual int64 [S, L, C, C], overlap int64
    [S, L, L]."""
    Ys = np.asarray(Ys)
    S, L, N, _ = Ys.shape
    C = int(C) if groups is not None else 0
    out = {"mix": np.zeros((S, L, C, C), np.int64), "mutual": np.zeros((S, L, C, C), np.int64), "overlap": np.zeros((S, L, L), np.int64)}
    keep = np.ones((N, N), bool)
    if skip_diagonal:
        np.fill_diagonal(keep, False)
    if groups is not None:
        g = np.asarray(groups, dtype=np.int64)
        lab = (g[:, None] >= 0) & (g[None, :] >= 0)
        gi, gj = np.broadcast_to(g[:, None], (N, N)), np.broadcast_to(g[None, :], (N, N))
    for s in range(S):
        A = (Ys[s] > 0) & keep[None]
        for l in range(L):
            if groups is not None:
                e = A[l] & lab
                np.add.at(out["mix"][s, l], (gi[e], gj[e]), 1)
                m = e & A[l].T
                np.add.at(out["mutual"][s, l], (gi[m], gj[m]), 1)
            for l2 in range(L):
                out["overlap"][s, l, l2] = (A[l] & A[l2]).sum()
    return out


def expected_mixing_np(rho, groups, C, skip_diagonal):
    """What `CaviEngine.expected_mixing` returns for rho [L,N,N,K], with p_lij = sum_{k>=1} rho_lijk: float64 mix, mutual [L, C, C]
    (sum of p_lij, of p_lij p_lji over g_i = a, g_j = b) and overlap [L, L] (sum_ij p_lij p_l'ij, sum_ij p_lij on the diagonal)."""
    rho = np.asarray(rho, dtype=np.float64)
    L, N = rho.shape[:2]
    p = rho[..., 1:].sum(-1)
    if skip_diagonal:
        p = p * (1.0 - np.eye(N))[None]
    C = int(C) if groups is not None else 0
    out = {"mix": np.zeros((L, C, C)), "mutual": np.zeros((L, C, C)), "overlap": np.zeros((L, L))}
    if groups is not None:
        g = np.asarray(groups, dtype=np.int64)
        G = (g[:, None] == np.arange(C)[None, :]).astype(np.float64)   # [N, C] membership; a node left out has an empty row
        out["mix"] = np.stack([G.T @ p[l] @ G for l in range(L)])   # (products with 0 and 1 are exact: sums of p in some order)
        out["mutual"] = np.stack([G.T @ (p[l] * p[l].T) @ G for l in range(L)])
    for l in range(L):
        for l2 in range(L):
            out["overlap"][l, l2] = p[l].sum() if l == l2 else (p[l] * p[l2]).sum()
    return out


# ---------------------------------------------------------------------------------------------- sampling against expectation
SAMPLING_CASE = {"N": 129, "L": 2, "M": 4, "K": 3, "C": 3, "S": 256, "engine_seed": 429, "seed": 4242, "min_expected": 20.0}


def sampling_case_inputs():
    """(X, state, groups) of the "sampling agrees with expectation" case: the random engine of tests/test_hip_triads.py
    (`_random_engine(N, engine_seed)`: X and the state from one RandomState) and groups i % C with node 0 left out.  state[-1] is
    rho."""
    from tests.test_hip_netstats import _random_state
    c = SAMPLING_CASE
    g = np.random.RandomState(c["engine_seed"])
    X = (g.rand(c["L"], c["N"], c["N"], c["M"]) < 0.1).astype(np.uint8)
    st = _random_state(g, c["L"], c["N"], c["M"], c["K"], sparse_p=True)
    groups = (np.arange(c["N"]) % c["C"]).astype(np.int32)
    groups[0] = -1
    return X, st, groups


def check_sampling_against_expectation(got, expected, ref):
    """For every bin whose expectation is at least min_expected (so that the normal approximation is honest) the mean of `got`
    over the samples lies within 5 standard errors of the expectation, the standard error taken from `ref`, the NumPy counts of
    the same samples.  Returns the number of bins compared."""
    c = SAMPLING_CASE
    n = 0
    for k in MIX_KEYS:
        big = expected[k] >= c["min_expected"]
        assert big.any(), k
        for idx in zip(*np.nonzero(big)):
            se = ref[k][(slice(None),) + idx].std(ddof=1) / np.sqrt(c["S"])
            assert se > 0, (k, idx)
            mean = got[k][(slice(None),) + idx].mean()
            assert abs(mean - expected[k][idx]) <= 5.0 * se, (k, idx, mean, expected[k][idx], se)
            n += 1
    return n
