"""The diffusion-centrality contract restated in NumPy (the definitions of include/vimure_hip.h at vmr_sample_centrality and
vmr_mean_centrality) and nothing of the device code: what tests/test_centrality_host.py pins against closed forms and against a
second restatement that sums in another order, and tests/test_hip_centrality.py holds the device to."""
import math

import numpy as np

CENT_KEYS = ("node_sum", "node_sumsq", "node_rank_sum", "node_top", "total", "max")
DIRECTIONS = ("out", "in", "union")
EPS = 2.0 ** -53


def adjacency(Y, direction):
    """M [N, N] bool of one layer of one sample: A = (Y > 0) without its diagonal, A.T or A | A.T."""
    A = np.asarray(Y) > 0
    A = A & ~np.eye(A.shape[0], dtype=bool)
    return {"out": A, "in": A.T, "union": A | A.T}[direction]


def walk_np(M, q, T):
    """c = x_1 + .. + x_T, x_0 = 1, x_t = q (M x_{t-1}), added in ascending t; M a float matrix."""
    M = np.asarray(M, dtype=np.float64)
    x = np.ones(M.shape[0])
    c = np.zeros(M.shape[0])
    for _ in range(int(T)):
        x = q * (M @ x)
        c = c + x
    return c


def ranks_np(c):
    """rank[v] = #{u : c[u] > c[v]}, int64."""
    c = np.asarray(c)
    return (c[None, :] > c[:, None]).sum(axis=1).astype(np.int64)


def reduce_values(values, top_k):
    """The dict of `CaviEngine.sample_centrality` from the c of every sample, values [S, L, N]: per-node sums in ascending s (the
    square rounded, then added), ranks by strict comparison, the total and the maximum of every sample."""
    values = np.asarray(values, dtype=np.float64)
    S, L, N = values.shape
    out = {"node_sum": np.zeros((L, N)), "node_sumsq": np.zeros((L, N)), "node_rank_sum": np.zeros((L, N), np.int64),
           "node_top": np.zeros((L, N), np.int64), "total": np.zeros((S, L)), "max": np.zeros((S, L)), "values": values.copy()}
    for s in range(S):
        out["node_sum"] = out["node_sum"] + values[s]
        out["node_sumsq"] = out["node_sumsq"] + values[s] * values[s]
        for l in range(L):
            r = ranks_np(values[s, l])
            out["node_rank_sum"][l] += r
            out["node_top"][l] += r < top_k
            out["total"][s, l] = values[s, l].sum()
            out["max"][s, l] = values[s, l].max()
    return out


def centrality_np(Ys, q, T, direction="out", top_k=10):
    """Ys: samples [S][L,N,N] (a list or an array); q a scalar or [L].  Returns the dict `CaviEngine.sample_centrality(...,
    values=True)` returns, by dense float matrix products."""
    Ys = np.asarray(Ys)
    S, L, N, _ = Ys.shape
    q = np.broadcast_to(np.asarray(q, dtype=np.float64), (L,))
    values = np.zeros((S, L, N))
    for s in range(S):
        for l in range(L):
            values[s, l] = walk_np(adjacency(Ys[s, l], direction), q[l], T)
    return reduce_values(values, top_k)


def walk_other_order(M, q, T):
    """The same c by another route: neighbours added in descending index order, one at a time, and the x_t added in descending
    t."""
    M = np.asarray(M) > 0
    N = M.shape[0]
    nb = [np.nonzero(M[i])[0][::-1] for i in range(N)]
    x = [1.0] * N
    xs = []
    for _ in range(int(T)):
        y = []
        for i in range(N):
            a = 0.0
            for j in nb[i]:
                a += x[j]
            y.append(q * a)
        x = y
        xs.append(x)
    c = np.zeros(N)
    for x in reversed(xs):
        c = c + np.asarray(x)
    return c


def exact_ok(M, q, T):
    """For q = 2^-k: the walk counts w_t = M^t 1 in Python integers; asserts that every node's sum_t w_t 2^{k (T - t)} -- c times
    2^{kT} -- and their sum over the nodes stay below 2^53, so that c, every partial sum of it in any order and the total are
    exactly representable and a comparison for equality cannot pass or fail by the order of the additions.  Returns the exact c."""
    m, e = math.frexp(float(q))
    assert m == 0.5 and e <= 0, "q must be a negative power of two"
    k = 1 - e
    M = np.asarray(M) > 0
    N = M.shape[0]
    nb = [np.nonzero(M[i])[0].tolist() for i in range(N)]
    w = [1] * N
    tot = [0] * N
    for t in range(1, int(T) + 1):
        w = [sum(w[j] for j in nb[i]) for i in range(N)]
        tot = [a + (b << (k * (T - t))) for a, b in zip(tot, w)]
    assert max(tot) < 2 ** 53 and sum(tot) < 2 ** 53, (max(tot).bit_length(), sum(tot).bit_length())
    return np.array([math.ldexp(a, -k * int(T)) for a in tot])


def geometric(q, n):
    """sum_{t=1..n} q^t, added in ascending t."""
    a, p = 0.0, 1.0
    for _ in range(int(n)):
        p *= q
        a += p
    return a


def designed_closed_forms(q, T, N=129):
    """[4, N]: the OUT centrality of `connectivity_util.designed_graphs()` -- on the directed path node i is followed by
    N - 1 - i nodes and has sum_{t=1..min(T, N-1-i)} q^t; on a directed cycle every node has sum_{t<=T} q^t; the node with only a
    self-loop and every node of the empty graph have 0."""
    c = np.zeros((4, N))
    c[0] = [geometric(q, min(T, N - 1 - i)) for i in range(N)]
    c[1] = geometric(q, T)
    c[2, :128] = geometric(q, T)
    return c


def mean_matrix(rho, direction):
    """M [L, N, N] of vmr_mean_centrality from rho [L, N, N, K]: p = sum_{k>=1} rho_k with k ascending, p_ii = 0."""
    rho = np.asarray(rho, dtype=np.float64)
    P = np.zeros(rho.shape[:3])
    for k in range(1, rho.shape[3]):
        P = P + rho[..., k]
    i = np.arange(P.shape[1])
    P[:, i, i] = 0.0
    Pt = np.swapaxes(P, 1, 2)
    if direction == "out":
        return P
    if direction == "in":
        return np.ascontiguousarray(Pt)
    U = 1.0 - (1.0 - P) * (1.0 - Pt)
    U[:, i, i] = 0.0
    return U


def mean_centrality_np(rho, q, T, direction="out"):
    """[L, N]: the recursion on the mean network."""
    M = mean_matrix(rho, direction)
    q = np.broadcast_to(np.asarray(q, dtype=np.float64), (M.shape[0],))
    return np.stack([walk_np(M[l], q[l], T) for l in range(M.shape[0])])
