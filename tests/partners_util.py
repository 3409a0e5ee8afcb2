"""Host-only yardsticks of the shared partners (vmr_sample_shared_partners, vmr_network_shared_partners;
vimure_amd/csrc/partners.hip).  Nothing here touches the device or reads the kernel's tables.

For A = (Y > 0) with the diagonal cleared a mode names the counted ties T and two 0/1 matrices P and Q; the partners of the tie
(i, j) are sum_k P[i, k] Q[j, k]:
  union    P = Q = A | A^T, T = its upper triangle          mutual   P = Q = A & A^T, T = its upper triangle
  path     P = A, Q = A^T (sum_k A[i, k] A[k, j]), T = A
`partners_np` is that definition as dense products, `partners_slow` the same in three loops; designed networks with closed forms;
and the kernel's launch shape restated from N."""
import numpy as np

from tests.census_util import adjacency, complete, empty, path, star, three_cycle
from tests.graph_shapes_util import shape_of

MODES = ("union", "mutual", "path")
TOTALS = ("ties", "supported", "partners", "max_partners")


def _ptq(Y, mode):
    """(P, Q, T) bool [N, N] of one network under a mode."""
    B = adjacency(Y)
    if mode == "path":
        return B, B.T, B
    P = (B | B.T) if mode == "union" else (B & B.T)
    return P, P, np.triu(P, 1)


def fold(hist, n_bins):
    """A histogram [..., m] folded into n_bins bins: the last one holds every count >= n_bins - 1."""
    hist = np.asarray(hist)
    out = np.zeros(hist.shape[:-1] + (n_bins,), hist.dtype)
    m = min(hist.shape[-1], n_bins - 1)
    out[..., :m] = hist[..., :m]
    out[..., -1] = hist[..., m:].sum(axis=-1)
    return out


def _reduce(C, T, mode, n_bins, pairs_l):
    """What the calls return for one network, from its tie set T (bool) and the partner counts C (int64, valid where T)."""
    N = len(T)
    c = C[T]
    hist = fold(np.bincount(c, minlength=1), n_bins).astype(np.int64)
    totals = np.array([c.size, (c > 0).sum(), c.sum(), c.max() if c.size else 0], np.int64)
    Sup = T & (C > 0)
    node_ties = (T.sum(axis=1) + T.sum(axis=0)).astype(np.int32)            # (an unordered tie stands in the upper triangle once)
    node_sup = (Sup.sum(axis=1) + Sup.sum(axis=0)).astype(np.int32)
    pp = np.full(len(pairs_l), -1, np.int64)
    for q, (i, j) in enumerate(pairs_l):
        if mode != "path" and i > j:
            i, j = j, i
        if T[i, j]:
            pp[q] = C[i, j]
    return hist, totals, node_ties, node_sup, pp


def _collect(Ys, mode, n_bins, pairs, counts_of):
    Ys = np.asarray(Ys)
    S, L, N, _ = Ys.shape
    assert mode in MODES and n_bins >= 2
    pairs = np.zeros((0, 3), np.int64) if pairs is None else np.asarray(pairs, np.int64).reshape(-1, 3)
    out = {"hist": np.zeros((S, L, n_bins), np.int64), "totals": np.zeros((S, L, 4), np.int64), "node_ties": np.zeros((S, L, N), np.int32),
           "node_supported": np.zeros((S, L, N), np.int32), "pair_partners_net": np.full((S, len(pairs)), -1, np.int64)}
    for s in range(S):
        for l in range(L):
            P, Q, T = _ptq(Ys[s, l], mode)
            sel = np.nonzero(pairs[:, 0] == l)[0]
            h, t, nt, ns, pp = _reduce(counts_of(P, Q, T), T, mode, n_bins, [tuple(pairs[q, 1:]) for q in sel])
            out["hist"][s, l], out["totals"][s, l], out["node_ties"][s, l], out["node_supported"][s, l] = h, t, nt, ns
            out["pair_partners_net"][s, sel] = pp
    net = out["pair_partners_net"]
    out["pair_present"] = (net >= 0).sum(axis=0).astype(np.int64)
    out["pair_supported"] = (net > 0).sum(axis=0).astype(np.int64)
    out["pair_partners"] = np.where(net > 0, net, 0).sum(axis=0).astype(np.int64)
    return out


def partners_np(Ys, mode, n_bins=64, pairs=None):
    """The definition, for networks Ys [S, L, N, N] (an entry > 0 is a tie, the diagonal is ignored), by dense 0/1 products
    (P @ Q.T) * T -- float32, exact below 2^24 partners.  Returns a dict: hist int64 [S, L, n_bins] (the last bin pools),
    totals int64 [S, L, 4] (`TOTALS`), node_ties and node_supported int32 [S, L, N], and for pairs [n_pairs, 3] = (layer, i, j)
    pair_partners_net int64 [S, n_pairs] (-1: no counted tie) with its sums over the samples pair_present, pair_supported and
    pair_partners int64 [n_pairs]."""
    def counts_of(P, Q, T):
        assert len(P) < 2 ** 24
        return np.rint((P.astype(np.float32) @ Q.T.astype(np.float32)) * T).astype(np.int64)
    return _collect(Ys, mode, n_bins, pairs, counts_of)


def partners_slow(Ys, mode, n_bins=64, pairs=None):
    """The same dict tie by tie and node by node in Python loops, written from the words of the definition; N <= 40."""
    def counts_of(P, Q, T):
        N = len(T)
        assert N <= 40
        A = P if mode == "path" else None
        C = np.zeros((N, N), np.int64)
        for i in range(N):
            for j in range(N):
                if not T[i, j]:
                    continue
                for k in range(N):
                    if k == i or k == j:
                        continue
                    if mode == "path":
                        C[i, j] += bool(A[i, k] and A[k, j])
                    else:   # P is the symmetric relation "tied either way" or "tied both ways"
                        C[i, j] += bool(P[i, k] and P[j, k])
        return C
    return _collect(Ys, mode, n_bins, pairs, counts_of)


def transposed_ends(pairs):
    """The pair list with the two ends of every pair swapped."""
    p = np.asarray(pairs).reshape(-1, 3)
    return np.ascontiguousarray(p[:, [0, 2, 1]])


# ------------------------------------------------------------------------------------------ designs
def transitive_triple(N):
    """One transitive triple a -> b -> c, a -> c on the nodes 0, N // 2 and N - 1."""
    a, b, c = 0, N // 2, N - 1
    Y = np.zeros((N, N), np.uint8)
    Y[a, b] = Y[b, c] = Y[a, c] = 1
    return Y


def book(N):
    """A mutual spine between the nodes 0 and N - 1 and every other node tied mutually to both: the spine has N - 2 partners and
    each of the 2 (N - 2) pages exactly one, the other end of the spine.  The spine's bits sit in the first and in the last word
    of a row."""
    Y = np.zeros((N, N), np.uint8)
    Y[0, 1:] = Y[1:, 0] = 1
    Y[N - 1, :N - 1] = Y[:N - 1, N - 1] = 1
    return Y


def closed_forms(N):
    """name -> (Y [N, N], {mode: (ties, supported, partners, max_partners)}) for N >= 4."""
    m, pairs = N - 2, N * (N - 1) // 2
    zero = (0, 0, 0, 0)
    line = {"union": (N - 1, 0, 0, 0), "mutual": zero, "path": (N - 1, 0, 0, 0)}
    return {
        "empty": (empty(N)[0], dict.fromkeys(MODES, zero)),
        "complete": (complete(N)[0], {"union": (pairs, pairs, pairs * m, m), "mutual": (pairs, pairs, pairs * m, m),
                                      "path": (2 * pairs, 2 * pairs, 2 * pairs * m, m)}),
        "path": (path(N)[0], line),
        "out-star": (star(N, "out")[0], line),
        "in-star": (star(N, "in", N - 1)[0], line),
        "mutual star": (star(N, "mutual", N // 2)[0], {"union": (N - 1, 0, 0, 0), "mutual": (N - 1, 0, 0, 0), "path": (2 * N - 2, 0, 0, 0)}),
        "3-cycle": (three_cycle(N)[0], {"union": (3, 3, 3, 1), "mutual": zero, "path": (3, 0, 0, 0)}),
        "transitive triple": (transitive_triple(N), {"union": (3, 3, 3, 1), "mutual": zero, "path": (3, 1, 1, 1)}),
        "book": (book(N), {"union": (2 * m + 1, 2 * m + 1, 3 * m, m), "mutual": (2 * m + 1, 2 * m + 1, 3 * m, m),
                           "path": (4 * m + 2, 4 * m + 2, 6 * m, m)}),
    }


# ------------------------------------------------------------------------------------------ the launch shape
SP_BLK = 32                 # words of row i whose neighbours k_sp_count lists at a time (partners.hip)
SP_LIST = SP_BLK * 64       # the slots of that list
MAX_BINS = 1024

# The N the GPU file enters k_sp_count at, and what each is for (test_partners_host.py holds the list to `partners_shape`)
SHAPE_NS = {
    63: "one word, one lane per neighbour, 63 of its bits valid",
    64: "one word, full",
    65: "two words, two lanes per neighbour; node 64 the only bit of the last word",
    129: "three words on two lanes: the word stride takes a second trip (W > G)",
    257: "five words on four lanes, W > G",
    300: "five words on four lanes, W > G: the closed forms",
    513: "nine words on 8 lanes, W > G",
    1024: "16 words on 16 lanes: row i in a register",
    1025: "17 words on 16 lanes, W > G",
    2048: "32 words on 32 lanes in a register: one full list block",
    2049: "33 words on 32 lanes: two list blocks, W > G",
    4097: "65 words on 64 lanes: three list blocks, a second trip of the word stride; the book's spine beyond the last bin",
}


def partners_shape(N):
    """(W, G, one, blocks, trips) of k_sp_count on N nodes, restated: W words per bit row, G lanes per neighbour (`shape_of`),
    `one` when row i's word stays in a register (W <= G), the list blocks of SP_BLK words node 0 walks, and the trips of the word
    stride (ceil(W / G))."""
    W, lG = shape_of(N)[:2]
    G = 1 << lG
    return W, G, W <= G, (W + SP_BLK - 1) // SP_BLK, (W + G - 1) // G
