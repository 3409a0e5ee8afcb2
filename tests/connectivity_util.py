"""The connectivity contract restated with scipy.sparse.csgraph (the table of include/vimure_hip.h at vmr_sample_connectivity) and
nothing of the device code: what tests/test_connectivity_host.py pins against the definitions word for word and against designed
graphs, and tests/test_hip_connectivity.py holds the device to."""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components, shortest_path

CONN_KEYS = ("components_w", "giant_w", "pairs_w", "isolates", "components_s", "giant_s", "pairs_s", "reach_pairs", "dist_sum",
             "diameter")
NODE_KEYS = ("node_comp_w", "node_comp_s", "node_reach_out", "node_reach_in", "node_dist_out", "node_dist_in")
NDIST = 64


def _min_labels(labels):
    """scipy's component numbers -> the smallest node index of every node's component."""
    first = np.full(labels.max() + 1, labels.size, np.int64)
    np.minimum.at(first, labels, np.arange(labels.size))
    return first[labels]


def connectivity_np(Ys):
    """Ys: samples [S][L,N,N] (a list or an array).  Returns the dict `CaviEngine.sample_connectivity(..., hist=True, nodes=True)`
    returns: the ten counts int64 [S, L], dist_hist int64 [S, L, 64] and the six node arrays int32 [S, L, N], for A = (Y > 0)
    without its diagonal."""
    Ys = np.asarray(Ys)
    S, L, N, _ = Ys.shape
    out = {k: np.zeros((S, L), np.int64) for k in CONN_KEYS}
    out["dist_hist"] = np.zeros((S, L, NDIST), np.int64)
    for k in NODE_KEYS:
        out[k] = np.zeros((S, L, N), np.int32)
    for s in range(S):
        for l in range(L):
            A = (Ys[s, l] > 0).astype(np.int8)
            np.fill_diagonal(A, 0)
            G = csr_matrix(A)
            for kind, conn in (("w", "weak"), ("s", "strong")):
                _, lab = connected_components(G, directed=True, connection=conn)
                lab = _min_labels(lab)
                n = np.bincount(lab, minlength=N)
                n = n[n > 0]
                out["components_" + kind][s, l] = n.size
                out["giant_" + kind][s, l] = n.max()
                out["pairs_" + kind][s, l] = (n * (n - 1)).sum()
                out["node_comp_" + kind][s, l] = lab
                if kind == "w":
                    out["isolates"][s, l] = (n == 1).sum()
            D = shortest_path(G, directed=True, unweighted=True)
            fin = np.isfinite(D) & ~np.eye(N, dtype=bool)
            d = np.where(fin, D, 0).astype(np.int64)
            out["reach_pairs"][s, l] = fin.sum()
            out["dist_sum"][s, l] = d.sum()
            out["diameter"][s, l] = d.max()
            out["dist_hist"][s, l] = np.bincount(np.minimum(d[fin], NDIST) - 1, minlength=NDIST)
            out["node_reach_out"][s, l], out["node_reach_in"][s, l] = fin.sum(axis=1), fin.sum(axis=0)
            out["node_dist_out"][s, l], out["node_dist_in"][s, l] = d.sum(axis=1), d.sum(axis=0)
    return out


def designed_graphs(N=129):
    """[4, N, N] uint8, N = 129 = two source blocks and one node: the directed path 0 -> 1 -> .. -> N - 1; the directed cycle over
    all nodes; two directed cycles on nodes 0-63 and 64-127 with node 128 carrying only a self-loop; the empty graph."""
    assert N == 129
    Y = np.zeros((4, N, N), np.uint8)
    i = np.arange(N)
    Y[0, i[:-1], i[:-1] + 1] = 1
    Y[1, i, (i + 1) % N] = 1
    Y[2, i[:64], (i[:64] + 1) % 64] = 1
    Y[2, 64 + i[:64], 64 + (i[:64] + 1) % 64] = 1
    Y[2, 128, 128] = 1
    return Y


def check_designed(c, N=129):
    """The closed forms of `designed_graphs` on sample 0 of the result c (of the restatement or of the device)."""
    got = {k: [int(c[k][0, l]) for l in range(4)] for k in CONN_KEYS}
    P = N * (N - 1)
    # the path: every node its own strong component; i reaches j > i at distance j - i
    assert (got["components_w"][0], got["giant_w"][0], got["pairs_w"][0], got["isolates"][0]) == (1, N, P, 0)
    assert (got["components_s"][0], got["giant_s"][0], got["pairs_s"][0]) == (N, 1, 0)
    assert (got["reach_pairs"][0], got["dist_sum"][0], got["diameter"][0]) == (P // 2, (N - 1) * N * (N + 1) // 6, N - 1) == (8256, 357760, 128)
    # the cycle: j is at distance (j - i) mod N from i
    assert (got["components_w"][1], got["giant_w"][1], got["pairs_w"][1], got["isolates"][1]) == (1, N, P, 0)
    assert (got["components_s"][1], got["giant_s"][1], got["pairs_s"][1]) == (1, N, P)
    assert (got["reach_pairs"][1], got["dist_sum"][1], got["diameter"][1]) == (P, N * (N - 1) * N // 2, N - 1)
    # two cycles of 64 and a node with a self-loop
    assert (got["components_w"][2], got["giant_w"][2], got["pairs_w"][2], got["isolates"][2]) == (3, 64, 2 * 64 * 63, 1)
    assert (got["components_s"][2], got["giant_s"][2], got["pairs_s"][2]) == (3, 64, 2 * 64 * 63)
    assert (got["reach_pairs"][2], got["dist_sum"][2], got["diameter"][2]) == (2 * 64 * 63, 2 * 64 * (63 * 64 // 2), 63)
    # empty
    assert (got["components_w"][3], got["giant_w"][3], got["pairs_w"][3], got["isolates"][3]) == (N, 1, 0, N)
    assert (got["components_s"][3], got["giant_s"][3], got["pairs_s"][3]) == (N, 1, 0)
    assert (got["reach_pairs"][3], got["dist_sum"][3], got["diameter"][3]) == (0, 0, 0)
    if "dist_hist" in c:
        h = c["dist_hist"][0]
        assert h.shape == (4, NDIST)
        assert np.array_equal(h[0, :NDIST - 1], N - np.arange(1, NDIST)) and h[0, NDIST - 1] == 2145   # N - d pairs at distance d
        assert np.array_equal(h[1, :NDIST - 1], np.full(NDIST - 1, N)) and h[1, NDIST - 1] == N * (N - NDIST)
        assert np.array_equal(h[2, :NDIST - 1], np.full(NDIST - 1, 128)) and h[2, NDIST - 1] == 0
        assert not h[3].any()
    if "node_dist_out" in c:
        assert c["node_dist_out"][0, 0, 0] == 8256 and c["node_dist_in"][0, 0, N - 1] == 8256
        assert c["node_reach_out"][0, 0, 0] == N - 1 and c["node_reach_out"][0, 0, N - 1] == 0
        assert np.array_equal(c["node_comp_s"][0, 0], np.arange(N)) and not c["node_comp_w"][0, 0].any()
        assert not c["node_comp_s"][0, 1].any()
        want2 = np.r_[np.zeros(64, np.int32), np.full(64, 64, np.int32), 128]
        assert np.array_equal(c["node_comp_w"][0, 2], want2) and np.array_equal(c["node_comp_s"][0, 2], want2)
        assert np.array_equal(c["node_comp_w"][0, 3], np.arange(N)) and not c["node_reach_in"][0, 3].any()
