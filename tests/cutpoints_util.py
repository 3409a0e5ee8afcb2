"""The cut-point contract (include/vimure_hip.h at vmr_sample_cutpoints) restated with NumPy and
scipy.sparse.csgraph.connected_components and nothing of the device code: for each node, remove it, label the components, read off
the branch sizes and the neighbours per branch.  What tests/test_cutpoints_host.py holds to networkx and to designed graphs, and
tests/test_hip_cutpoints.py holds the device to."""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

from tests.connectivity_util import designed_graphs

MODES = ("union", "mutual")
CUT_KEYS = ("node_sum", "node_sumsq", "node_rank_sum", "node_top", "node_cut", "node_branch_sum", "node_bridge_sum", "n_cut", "n_bridges",
            "max_pairs_cut", "connected_pairs")
CUT_VALUES = ("pairs_cut", "branches", "bridges")
SUMMARY = ("n_cut", "n_bridges", "max_pairs_cut", "connected_pairs")


def graph(Y, mode):
    """G [N, N] bool of one layer of one network: A = (Y > 0) without its diagonal, A | A.T ("union") or A & A.T ("mutual")."""
    A = np.asarray(Y) > 0
    A = A & ~np.eye(A.shape[0], dtype=bool)
    assert mode in MODES
    return A | A.T if mode == "union" else A & A.T


def connected_pairs(G):
    """The connected unordered pairs of G: sum over the components of C(|C|, 2)."""
    _, lab = connected_components(csr_matrix(G.astype(np.int8)), directed=False)
    n = np.bincount(lab).astype(np.int64)
    return int((n * (n - 1) // 2).sum())


def cut_values(G):
    """(pairs_cut, branches, bridges) int64 [N] of the symmetric bool matrix G.  The CSR arrays are built once; removing node v
    drops the entries of its row and of its column from a copy (slicing a dense matrix per node is N times slower)."""
    N = G.shape[0]
    M = csr_matrix(G.astype(np.int8))
    M.sort_indices()
    indptr, indices = M.indptr, M.indices
    row_of = np.repeat(np.arange(N), np.diff(indptr))
    pairs, branches, bridges = np.zeros(N, np.int64), np.zeros(N, np.int64), np.zeros(N, np.int64)
    for v in range(N):
        nb = indices[indptr[v]:indptr[v + 1]]
        if nb.size == 0:
            continue
        keep = (row_of != v) & (indices != v)
        ip = np.concatenate(([0], np.cumsum(np.bincount(row_of[keep], minlength=N))))
        H = csr_matrix((np.ones(int(keep.sum()), np.int8), indices[keep], ip), shape=(N, N))
        _, lab = connected_components(H, directed=False)
        size = np.bincount(lab)
        held = np.bincount(lab[nb], minlength=size.size)        # the neighbours of v per component of G - v
        s = size[held > 0].astype(np.int64)                      # the branches: the components that hold one
        branches[v] = s.size
        pairs[v] = (s.sum() ** 2 - (s * s).sum()) // 2
        bridges[v] = (held == 1).sum()
    return pairs, branches, bridges


def ranks(v):
    """#{u : v[u] > v[w]} along the last axis of the integer array v."""
    v = np.asarray(v)
    out = np.zeros(v.shape, np.int64)
    for idx in np.ndindex(v.shape[:-1]):
        out[idx] = v.shape[-1] - np.searchsorted(np.sort(v[idx]), v[idx], side="right")
    return out


def reduce_values(pairs_cut, branches, bridges, top_k):
    """What `CaviEngine.sample_cutpoints` returns beside the values and `connected_pairs`, from the values [S, L, N]: the fold in
    ascending s (the doubles of integers, added as the device adds them), the ranks, and the summary's first three columns."""
    p = np.asarray(pairs_cut).astype(np.int64)
    b, g = np.asarray(branches).astype(np.int64), np.asarray(bridges).astype(np.int64)
    S = p.shape[0]
    rank = ranks(p)
    pd = p.astype(np.float64)
    node_sum, node_sumsq = np.zeros(p.shape[1:]), np.zeros(p.shape[1:])
    for s in range(S):
        node_sum = node_sum + pd[s]
        node_sumsq = node_sumsq + pd[s] * pd[s]
    return {"node_sum": node_sum, "node_sumsq": node_sumsq, "node_rank_sum": rank.sum(axis=0), "node_top": (rank < top_k).sum(axis=0),
            "node_cut": (b >= 2).sum(axis=0), "node_branch_sum": b.sum(axis=0), "node_bridge_sum": g.sum(axis=0),
            "n_cut": (b >= 2).sum(axis=2), "n_bridges": g.sum(axis=2) // 2, "max_pairs_cut": p.max(axis=2)}


def cutpoints_np(Ys, mode="union", top_k=10):
    """Ys: networks [S][L, N, N] (a list or an array).  Returns the dict `CaviEngine.sample_cutpoints(..., values=True)` returns."""
    Ys = np.asarray(Ys)
    S, L, N, _ = Ys.shape
    p, b, g = np.zeros((S, L, N), np.uint32), np.zeros((S, L, N), np.uint16), np.zeros((S, L, N), np.uint16)
    cp = np.zeros((S, L), np.int64)
    for s in range(S):
        for l in range(L):
            G = graph(Ys[s, l], mode)
            p[s, l], b[s, l], g[s, l] = cut_values(G)
            cp[s, l] = connected_pairs(G)
    out = reduce_values(p, b, g, top_k)
    out.update(connected_pairs=cp, pairs_cut=p, branches=b, bridges=g)
    return out


# ------------------------------------------------------------------------------------------
# designed graphs, N = 129: two blocks of 64 nodes and one node
# ------------------------------------------------------------------------------------------
N_DESIGNED = 129


def tree_sizes(N=N_DESIGNED):
    """int64 [N]: the nodes of the subtree of i in the tree whose node i has the children 2 i + 1 and 2 i + 2 (those below N)."""
    sub = np.ones(N, np.int64)
    for i in range(N - 1, 0, -1):
        sub[(i - 1) // 2] += sub[i]
    return sub


def second_set(N=N_DESIGNED):
    """[4, N, N] uint8: a star whose hub is node 64, every tie both ways (the hub's block runs 128 rounds, the others one); two
    mutual cliques on nodes 0-63 and 64-127 joined through node 128 by the mutual ties 63 - 128 - 64; two mutual triangles {10,
    70, 128} and {128, 5, 100} that share node 128, every other node isolated; the tree i -> 2 i + 1, 2 i + 2 with every tie one
    way: non-trivial in "union", empty in "mutual".  Every diagonal entry is set."""
    assert N == N_DESIGNED
    Y = np.zeros((4, N, N), np.uint8)
    Y[0, 64, :] = Y[0, :, 64] = 1
    Y[1, :64, :64] = Y[1, 64:128, 64:128] = 1
    Y[1, 63, 128] = Y[1, 128, 63] = Y[1, 64, 128] = Y[1, 128, 64] = 1
    for a, b, c in ((10, 70, 128), (128, 5, 100)):
        for u, v in ((a, b), (b, c), (c, a)):
            Y[2, u, v] = Y[2, v, u] = 1
    i = np.arange(1, N)
    Y[3, (i - 1) // 2, i] = 1
    Y[:, np.arange(N), np.arange(N)] = 1
    return Y


def all_designed():
    """[8, N, N]: `connectivity_util.designed_graphs()` (the directed path, the directed cycle, two directed cycles beside a node
    that has only a self-loop, the empty graph), then `second_set()`."""
    return np.concatenate([designed_graphs(), second_set()])


def designed_closed_forms(mode):
    """The closed forms of `all_designed()` under `mode`: {"pairs_cut", "branches", "bridges"} int64 [8, N] and the four summary
    columns int64 [8].  Under "mutual" the four graphs of the first set and the tree have no tie."""
    N = N_DESIGNED
    P = N * (N - 1) // 2
    p, b, g = np.zeros((8, N), np.int64), np.zeros((8, N), np.int64), np.zeros((8, N), np.int64)
    sm = {k: np.zeros(8, np.int64) for k in SUMMARY}
    i = np.arange(N)
    if mode == "union":
        # the path: interior node i splits i nodes from N - 1 - i; every tie is a bridge
        b[0], g[0] = 2, 2
        b[0, [0, N - 1]], g[0, [0, N - 1]] = 1, 1
        p[0] = i * (N - 1 - i)
        sm["n_cut"][0], sm["n_bridges"][0], sm["max_pairs_cut"][0], sm["connected_pairs"][0] = N - 2, N - 1, 64 * 64, P
        # the cycle: one branch, no bridge
        b[1] = 1
        sm["connected_pairs"][1] = P
        # two cycles of 64 beside an isolate
        b[2, :128] = 1
        sm["connected_pairs"][2] = 2 * (64 * 63 // 2)
        # the tree: the subtrees of the children and the rest are the branches, every tie is a bridge
        sub = tree_sizes(N)
        for v in range(N):
            s = [sub[c] for c in (2 * v + 1, 2 * v + 2) if c < N] + ([N - sub[v]] if v else [])
            s = np.asarray(s, np.int64)
            b[7, v] = g[7, v] = s.size
            p[7, v] = (s.sum() ** 2 - (s * s).sum()) // 2
        sm["n_cut"][7], sm["n_bridges"][7], sm["max_pairs_cut"][7], sm["connected_pairs"][7] = 64, N - 1, p[7].max(), P
    # the star: the hub's branches are the 128 leaves; a leaf leaves the rest in one piece, tied to it by a bridge
    b[4], g[4] = 1, 1
    b[4, 64] = g[4, 64] = 128
    p[4, 64] = 128 * 127 // 2
    sm["n_cut"][4], sm["n_bridges"][4], sm["max_pairs_cut"][4], sm["connected_pairs"][4] = 1, 128, 128 * 127 // 2, P
    # two cliques joined through node 128: 63 and 64 are cut points with one bridge each, 128 one with two
    b[5] = 1
    b[5, [63, 64, 128]] = 2
    g[5, [63, 64]], g[5, 128] = 1, 2
    p[5, [63, 64]], p[5, 128] = 63 * 65, 64 * 64
    sm["n_cut"][5], sm["n_bridges"][5], sm["max_pairs_cut"][5], sm["connected_pairs"][5] = 3, 2, 64 * 64, P
    # two triangles sharing node 128: a cut point without any bridge
    b[6, [10, 70, 5, 100]] = 1
    b[6, 128], p[6, 128] = 2, 4
    sm["n_cut"][6], sm["max_pairs_cut"][6], sm["connected_pairs"][6] = 1, 4, 10
    out = {"pairs_cut": p, "branches": b, "bridges": g}
    out.update(sm)
    return out


def random_digraph(N, p_tie, seed):
    """uint8 [N, N]: every ordered pair a tie with probability p_tie, independently; every third diagonal entry set."""
    Y = (np.random.RandomState(seed).rand(N, N) < p_tie).astype(np.uint8)
    Y[np.arange(0, N, 3), np.arange(0, N, 3)] = 1
    return Y
