"""The betweenness contract restated in NumPy (the definitions of include/vimure_hip.h at vmr_sample_betweenness) and nothing of
the device code: what tests/test_betweenness_host.py pins against closed forms and against networkx, and
tests/test_hip_betweenness.py holds the device to.  Brandes' algorithm by levels, from all sources at once: row s of every
array belongs to source s, and a level is one product with the sparse adjacency matrix."""
import numpy as np
from scipy.sparse import csr_matrix

from tests.centrality_util import reduce_values

BTW_KEYS = ("node_sum", "node_sumsq", "node_rank_sum", "node_top", "total", "max")
DIRECTIONS = ("directed", "union")
EPS = 2.0 ** -53


def search_graph(Y, direction):
    """G [N, N] bool of one layer of one sample: A = (Y > 0) without its diagonal, or A | A.T."""
    A = np.asarray(Y) > 0
    A = A & ~np.eye(A.shape[0], dtype=bool)
    return {"directed": A, "union": A | A.T}[direction]


def brandes_levels(G):
    """(D, sigma, delta), each [N, N] with row s for source s, of the bool search graph G: D[s, v] the distance (-1: not
    reached), sigma[s, v] the number of shortest s -> v paths (float64), delta[s, w] = sum over the out-neighbours v of w with
    D[s, v] = D[s, w] + 1 of sigma[s, w] / sigma[s, v] (1 + delta[s, v]) -- evaluated as sigma[s, w] times the sum of
    (1 + delta[s, v]) / sigma[s, v].  delta[s, s] = 0.  At most N - 1 levels."""
    G = np.asarray(G, dtype=bool)
    N = G.shape[0]
    Gs = csr_matrix(G.astype(np.float64))
    GsT = Gs.T.tocsr()
    D = np.full((N, N), -1, np.int32)
    D[np.arange(N), np.arange(N)] = 0
    sigma = np.eye(N)
    deepest = 0
    for lvl in range(1, N):
        paths = (GsT @ np.where(D == lvl - 1, sigma, 0.0).T).T          # paths[s, v] = sum_u sigma[s, u] G[u, v], u at lvl - 1
        new = (paths > 0) & (D < 0)
        if not new.any():
            break
        D[new] = lvl
        sigma[new] = paths[new]
        deepest = lvl
    delta = np.zeros((N, N))
    with np.errstate(divide="ignore", invalid="ignore"):
        for lvl in range(deepest - 1, 0, -1):
            coef = np.where(D == lvl + 1, (1.0 + delta) / sigma, 0.0)
            acc = (Gs @ coef.T).T                                        # acc[s, w] = sum_v G[w, v] coef[s, v]
            here = D == lvl
            delta[here] = sigma[here] * acc[here]
    return D, sigma, delta


def betweenness_graph(G, halve=False, exact_sigma=False):
    """b [N] of the bool search graph G: the sum of delta over the sources in ascending s; halved for an undirected graph.
    exact_sigma: also what `sigma_ok` asserts, from the same search."""
    _, sigma, delta = brandes_levels(G)
    assert not exact_sigma or sigma.max() <= 2.0 ** 53, sigma.max()
    b = np.zeros(delta.shape[0])
    for s in range(delta.shape[0]):
        b = b + delta[s]
    return b * 0.5 if halve else b


def sigma_ok(G):
    """Asserts that no shortest-path count of the bool search graph G exceeds 2^53 (sigma is then exact in FP64 whatever the
    order of its sums); returns (the largest sigma, the largest distance)."""
    D, sigma, _ = brandes_levels(G)
    assert sigma.max() <= 2.0 ** 53, sigma.max()
    return float(sigma.max()), int(D.max())


def betweenness_np(Ys, direction="directed", top_k=10, exact_sigma=False):
    """Ys: samples [S][L,N,N] (a list or an array).  Returns the dict `CaviEngine.sample_betweenness(..., values=True)` returns.
    exact_sigma: asserts on every graph what `sigma_ok` asserts."""
    Ys = np.asarray(Ys)
    S, L, N, _ = Ys.shape
    values = np.zeros((S, L, N))
    for s in range(S):
        for l in range(L):
            values[s, l] = betweenness_graph(search_graph(Ys[s, l], direction), halve=direction == "union", exact_sigma=exact_sigma)
    return reduce_values(values, top_k)


def diamond_chain(n=70):
    """[N, N] uint8, N = 3 n + 1: a chain of n diamonds -- join 3 j has ties to 3 j + 1 and 3 j + 2, both have ties to
    3 j + 3.  There are 2^k shortest paths from join j to join j + k: sigma reaches 2^n and every quantity is dyadic."""
    N = 3 * n + 1
    Y = np.zeros((N, N), np.uint8)
    j = 3 * np.arange(n)
    Y[j, j + 1] = Y[j, j + 2] = Y[j + 1, j + 3] = Y[j + 2, j + 3] = 1
    return Y


def diamond_closed_form(n=70):
    """b [3 n + 1] of `diamond_chain(n)`, directed.  Join j lies on every path from the 3 j nodes before it to the 3 (n - j)
    after it; a side node of diamond j on half of the paths from the 3 j + 1 nodes up to its join to the 3 (n - 1 - j) + 1 from
    the next join on."""
    b = np.zeros(3 * n + 1)
    for j in range(n + 1):
        b[3 * j] = 9 * j * (n - j)
    for j in range(n):
        b[3 * j + 1] = b[3 * j + 2] = (3 * j + 1) * (3 * (n - 1 - j) + 1) / 2
    return b
