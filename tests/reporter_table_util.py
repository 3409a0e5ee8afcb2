"""Shared by tests/test_reporters_host.py and tests/test_hip_reporter_table.py: the reporter table by brute-force Python loops, the
exact comparison of its counts, the derived bound of its sums, and the table of a self-reporter mask from the report list alone
(no dense [N,N,M] array)."""
import numpy as np

from vimure_amd.reporters import COUNT_NAMES, SUM_NAMES

U = 2.0 ** -52


def brute_table(X, R, rho, g_theta, g_lambda, g_nu, mutuality, method="rho_max", threshold=None):
    """vmr_reporter_table by loops over (l, i, j, m), straight from the definitions of include/vimure_hip.h."""
    L, N, _, M = X.shape
    K = rho.shape[-1]
    counts = np.zeros((L, M, 7), np.int64)
    sums = np.zeros((L, M, 3))
    def in_s(l, i, j, m):
        return R is None or R[l, i, j, m] != 0
    for l in range(L):
        for i in range(N):
            for j in range(N):
                r = rho[l, i, j]
                y = int(r[1] >= threshold) if method == "threshold" else int(np.argmax(r))
                prob = 0.0
                for k in range(1, K):
                    prob = prob + r[k]
                for m in range(M):
                    x = int(X[l, i, j, m])
                    if not in_s(l, i, j, m):
                        counts[l, m, 6] += x > 0
                        continue
                    xt = float(X[l, j, i, m]) if mutuality else 0.0
                    mp = 0.0
                    for k in range(K):
                        mp = mp + r[k] * (g_theta[l, m] * g_lambda[l, k] + g_nu * xt)
                    counts[l, m, 0] += 1
                    counts[l, m, 1] += x > 0
                    counts[l, m, 2] += x
                    counts[l, m, 3] += y > 0
                    counts[l, m, 4] += x > 0 and y > 0
                    counts[l, m, 5] += x > 0 and i != j and in_s(l, j, i, m) and X[l, j, i, m] > 0
                    sums[l, m, 0] += prob
                    sums[l, m, 1] += prob if x > 0 else 0.0
                    sums[l, m, 2] += mp
    return {"counts": counts, "sums": sums}


def assert_counts_equal(got, want):
    g, w = np.asarray(got["counts"]), np.asarray(want["counts"])
    assert g.shape == w.shape, (g.shape, w.shape)
    for c, name in enumerate(COUNT_NAMES):
        assert np.array_equal(g[..., c], w[..., c]), (name, np.argwhere(g[..., c] != w[..., c])[:5])


def sums_bound(want_sums, n_scope, K, q=0.0):
    """|got - want| <= (n K + 16) 2^-52 want + n q: the first term bounds any summation order of n K non-negative terms each good to
    a few ulp (n the reporter's n_scope: no sum has more elements); the second the fixed point's rounding of n terms to the
    quantum q ([L,M,3], `reporters.sum_quanta`; 0 for a floating-point tree).  Derived, not measured."""
    n = np.asarray(n_scope, dtype=np.float64)[..., None]
    return (n * K + 16.0) * U * np.abs(want_sums) + n * q


def assert_sums_close(got, want, n_scope, K, q=0.0):
    g, w = np.asarray(got["sums"]), np.asarray(want["sums"])
    assert g.shape == w.shape, (g.shape, w.shape)
    bound = sums_bound(w, n_scope, K, q)
    err = np.abs(g - w)
    for c, name in enumerate(SUM_NAMES):
        print(f"{name}: max |got - want| {err[..., c].max():.3e}, bound there {bound[..., c].reshape(-1)[err[..., c].argmax()]:.3e}, "
              f"max want {np.abs(w[..., c]).max():.3e}")
    for c, name in enumerate(SUM_NAMES):
        assert (err[..., c] <= bound[..., c]).all(), (name, float((err[..., c] - bound[..., c]).max()))


def self_reporter_table(N, xs, xv, rho, g_theta, g_lambda, g_nu, mutuality, method="rho_max", threshold=None):
    """The table of ONE layer under the self-reporter mask (R[i,j,m] != 0 iff m == i or m == j; M == N), from the report list
    (xs: the (i, j, m) index arrays, xv: the counts) and rho [N,N,K]: S_m is row m plus column m of the tie matrix, so every
    column is a row sum plus a column sum minus the diagonal entry.  No [N,N,M] array is built."""
    from vimure_amd.reporters import tie_readout_np
    i, j, m = (np.asarray(a, dtype=np.int64) for a in xs)
    xv = np.asarray(xv, dtype=np.int64)
    y, prob = tie_readout_np(rho[None], method, threshold)
    y, prob = y[0] > 0, prob[0]

    def cross(a):   # sum of a over row m plus column m, the diagonal once
        return a.sum(axis=1) + a.sum(axis=0) - np.diagonal(a)
    counts = np.zeros((N, 7), np.int64)
    sums = np.zeros((N, 3))
    counts[:, 0] = 2 * N - 1
    counts[:, 3] = cross(y.astype(np.int64))
    sums[:, 0] = cross(prob.astype(np.longdouble)).astype(np.float64)
    ins = (m == i) | (m == j)
    counts[:, 6] = np.bincount(m[~ins], minlength=N)
    ii, jj, mm, xx = i[ins], j[ins], m[ins], xv[ins]
    counts[:, 1] = np.bincount(mm, minlength=N)
    counts[:, 2] = np.bincount(mm, weights=xx, minlength=N).astype(np.int64)
    counts[:, 4] = np.bincount(mm, weights=y[ii, jj], minlength=N).astype(np.int64)
    sums[:, 1] = np.bincount(mm, weights=prob[ii, jj], minlength=N)
    have = {(int(a), int(b), int(c)) for a, b, c in zip(ii, jj, mm)}
    mut = np.array([a != b and (b, a, c) in have for a, b, c in zip(ii.tolist(), jj.tolist(), mm.tolist())], bool)
    counts[:, 5] = np.bincount(mm[mut], minlength=N)
    # exp_total = sum_{S_m} sum_k rho_k (theta_m lambda_k + nu X[j,i,m]): the lambda part over the cross, the nu part at the reports
    K = rho.shape[-1]
    q = np.zeros((N, N), np.longdouble)
    for k in range(K):
        q = q + rho[..., k].astype(np.longdouble) * np.longdouble(g_lambda[k])
    tot = np.asarray(g_theta, np.longdouble) * cross(q)
    if mutuality:
        rs = rho.astype(np.longdouble).sum(axis=-1)
        # the report (i, j, m) is X^T of the tie (j, i), which S_m holds iff m == j or m == i: every report inside the mask
        tot = tot + np.longdouble(g_nu) * np.bincount(mm, weights=(rs[jj, ii] * xx).astype(np.float64), minlength=N)
    sums[:, 2] = tot.astype(np.float64)
    return {"counts": counts[None], "sums": sums[None]}
