"""Host-only yardsticks of the structural holes (vmr_sample_structural_holes, vmr_network_structural_holes;
vimure_amd/csrc/holes.hip).  Nothing here touches the device or reads the kernel's tables.

For A = (Y > 0) with the diagonal cleared, U = A | A^T and z = U ("union") or A + A^T ("weighted"): d_i = sum_j U_ij, s_i = sum_j
z_ij, mx_j = max_x z_jx, f_j = 2 / mx_j,
  R_i = sum_{j in U_i} f_j sum_q z_iq z_jq        ES_i = d_i - R_i / (2 s_i) = (2 s_i d_i - R_i) / (2 s_i)
  c_i = sum_{j in U_i} ((z_ij + sum_q z_iq z_qj / s_q) / s_i)^2
and a node with d_i = 0 is undefined.  `holes_np` is that definition as dense integer and FP64 products, `holes_loops` the same in
three loops of exact rationals; `reduce_values` rebuilds every accumulator of the sampled call from per-sample values; designed
networks with closed forms; and the kernels' launch shape restated from N."""
import math
from fractions import Fraction

import numpy as np
from scipy.sparse import csr_matrix

from tests.graph_shapes_util import shape_of

MODES = ("union", "weighted")
MEASURES = ("effective_size", "constraint")
ACC_KEYS = ("node_sum", "node_sumsq", "node_rank_sum", "node_top", "node_defined", "n_defined")
SUM_KEYS = ("effective_size_sum", "constraint_sum")
VALUE_KEYS = ("degree", "strength", "redundancy", "effective_size", "constraint")
U = 2.0 ** -53   # the unit roundoff of FP64


def adjacency(Y):
    """bool [N, N]: (Y > 0) with the diagonal cleared."""
    B = np.asarray(Y) > 0
    return B & ~np.eye(len(B), dtype=bool)


def weights(Y, mode):
    """(Un, Z) int64 [N, N] of one network: the symmetrised ties and the mode's weights."""
    assert mode in MODES
    A = adjacency(Y).astype(np.int64)
    Un = A | A.T
    return Un, (Un if mode == "union" else A + A.T)


def holes_one(Y, mode):
    """(d, s, R int64 [N], ES, c float64 [N], NaN where d = 0) of one network by dense products: R from Z @ Z.T, ES from the
    integers by the device's expression, the constraint from P + P @ P.  The products are scipy.sparse where fewer than 5 % of the
    pairs are tied and the network is large, BLAS otherwise (FP64 holds the integers exactly: they are below 4 N)."""
    Un, Z = weights(Y, mode)
    N = len(Un)
    d, s = Un.sum(axis=1), Z.sum(axis=1)
    f = np.where(Z.max(axis=1, initial=0) == 2, 1, 2)
    some = d > 0
    Zf = Z.astype(np.float64)
    P = Zf / np.where(some, s, 1).astype(np.float64)[:, None]
    if N > 512 and Un.sum() < 0.05 * N * N:
        Zs, Ps = csr_matrix(Zf), csr_matrix(P)
        ZZ, PP = (Zs @ Zs.T).toarray(), (Ps @ Ps).toarray()
    else:
        ZZ, PP = Zf @ Zf.T, P @ P
    R = (Un * np.rint(ZZ).astype(np.int64) * f[None, :]).sum(axis=1)
    den = 2 * s
    ES = np.where(some, (den * d - R).astype(np.float64) / np.where(some, den, 1).astype(np.float64), np.nan)
    local = (P + PP) * Un
    c = np.where(some, (local * local).sum(axis=1), np.nan)
    return d, s, R, ES, c


def holes_loops(Y, mode):
    """The same in three loops (node, neighbour, third) of `fractions.Fraction`: (d, s, R lists of int, ES, c lists of Fraction,
    None where d = 0)."""
    Un, Z = weights(Y, mode)
    N = len(Un)
    Z = [[int(x) for x in row] for row in Z]
    nb = [[j for j in range(N) if Un[i, j]] for i in range(N)]
    d = [len(nb[i]) for i in range(N)]
    s = [sum(Z[i]) for i in range(N)]
    mx = [max(Z[i]) if N else 0 for i in range(N)]
    R, ES, c = [0] * N, [None] * N, [None] * N
    for i in range(N):
        if d[i] == 0:
            continue
        red, con = Fraction(0), Fraction(0)
        for j in nb[i]:
            inner, ind = 0, Fraction(0)
            for q in nb[i]:
                if Z[j][q]:
                    inner += Z[i][q] * Z[j][q]
                    ind += Fraction(Z[i][q] * Z[q][j], s[q])
            R[i] += (2 // mx[j]) * inner
            red += Fraction(inner, mx[j] * s[i])          # sum_q p_iq m_jq: Burt's redundancy of contact j
            con += (Fraction(Z[i][j], s[i]) + ind / s[i]) ** 2
        ES[i] = d[i] - red
        c[i] = con
    return d, s, R, ES, c


def ranks(es, con, defined):
    """(rank by effective size, rank by constraint, #defined) of one (sample, layer): among the defined nodes #{u : ES_u > ES_v}
    and #{u : c_u < c_v}; an undefined node gets #defined."""
    nd = int(defined.sum())
    e, c = np.sort(es[defined]), np.sort(con[defined])
    re = nd - np.searchsorted(e, es, side="right")
    rc = np.searchsorted(c, con, side="left")
    return np.where(defined, re, nd), np.where(defined, rc, nd), nd


def reduce_values(degree, effective_size, constraint, top_k):
    """Every per-call accumulator of `CaviEngine.sample_structural_holes` from per-sample values [S, L, N] (NaN or anything where
    degree = 0: such a sample adds 0): the sums in ascending s, the squares rounded before they are added, the ranks and top
    counts by the rank rule, node_defined, n_defined; and the summary's two sums by `math.fsum` (a yardstick within rounding, not
    the device's bits)."""
    degree = np.asarray(degree)
    S, L, N = degree.shape
    defined = degree > 0
    vals = [np.where(defined, np.asarray(v, dtype=np.float64), 0.0) for v in (effective_size, constraint)]
    out = {"node_sum": np.zeros((2, L, N)), "node_sumsq": np.zeros((2, L, N)), "node_rank_sum": np.zeros((2, L, N), np.int64),
           "node_top": np.zeros((2, L, N), np.int64), "node_defined": defined.sum(axis=0).astype(np.int64),
           "n_defined": defined.sum(axis=2).astype(np.float64), "effective_size_sum": np.zeros((S, L)), "constraint_sum": np.zeros((S, L))}
    for s in range(S):
        for m in range(2):
            v = vals[m][s]
            out["node_sum"][m] = out["node_sum"][m] + v
            out["node_sumsq"][m] = out["node_sumsq"][m] + v * v
        for l in range(L):
            rk = ranks(vals[0][s, l], vals[1][s, l], defined[s, l])
            for m in range(2):
                out["node_rank_sum"][m, l] += rk[m]
                out["node_top"][m, l] += rk[m] < top_k
                out[SUM_KEYS[m]][s, l] = math.fsum(vals[m][s, l][defined[s, l]])
    return out


def holes_np(Ys, mode="union", top_k=10):
    """Ys: networks [S][L, N, N] (a list or an array).  Returns the dict `CaviEngine.sample_structural_holes(..., values=True)`
    returns (the summary's sums by `math.fsum`)."""
    Ys = np.asarray(Ys)
    S, L, N, _ = Ys.shape
    vals = {"degree": np.zeros((S, L, N), np.int32), "strength": np.zeros((S, L, N), np.int32), "redundancy": np.zeros((S, L, N), np.int64),
            "effective_size": np.zeros((S, L, N)), "constraint": np.zeros((S, L, N))}
    for s in range(S):
        for l in range(L):
            for k, a in zip(VALUE_KEYS, holes_one(Ys[s, l], mode)):
                vals[k][s, l] = a
    out = reduce_values(vals["degree"], vals["effective_size"], vals["constraint"], top_k)
    out.update(vals)
    return out


def constraint_bound(N):
    """The relative bound between the device's constraint and `holes_np`'s on N nodes, 8 N 2^-53.  Every term is non-negative, so
    errors are relative and add.  Device, per local term: one division per common neighbour (the scaling by 1, 2 or 4 is exact)
    and the additions of at most N - 2 of them, (N - 1) u; one addition of z_ij and one division by s_i, 2 u; the square doubles
    that and rounds once, 2 (N + 1) u + u; the sum over at most N - 1 neighbours adds (N - 2) u: (3 N + 1) u.  `holes_np`: p_iq,
    p_qj and their product are three roundings in place of one division, P + P @ P adds p_ij (two more): (3 N + 7) u.  Both: (6 N +
    8) u <= 8 N u from N = 4 on.  A dropped or doubled term moves a value by at least about 1 / (4 N^2)."""
    assert N >= 4
    return 8 * N * U


# ------------------------------------------------------------------------------------------ designs
def star(N, n_leaves, kind="out"):
    """The centre 0 tied to the leaves 1 .. n_leaves ("out": it sends, "in": it receives, "mutual": both); the rest isolated; every
    diagonal entry set."""
    Y = np.eye(N, dtype=np.uint8)
    if kind in ("out", "mutual"):
        Y[0, 1:n_leaves + 1] = 1
    if kind in ("in", "mutual"):
        Y[1:n_leaves + 1, 0] = 1
    return Y


def clique(N, n):
    """Every tie among the nodes N - n .. N - 1, both ways; the rest isolated."""
    Y = np.zeros((N, N), np.uint8)
    Y[N - n:, N - n:] = 1
    return Y


def path(N):
    """0 -> 1 -> .. -> N - 1, entries 3."""
    Y = np.zeros((N, N), np.uint8)
    Y[np.arange(N - 1), np.arange(1, N)] = 3
    return Y


def clique_and_star(N, n_clique, n_leaves):
    """A mutual clique on the nodes 0 .. n_clique - 1 and a star of n_leaves out-ties from node 0 to the LAST n_leaves nodes: node 0
    bridges the two, the rest between them is isolated."""
    Y = np.zeros((N, N), np.uint8)
    Y[:n_clique, :n_clique] = 1
    Y[0, N - n_leaves:] = 1
    return Y


def pair_and_spokes(N, n_spokes):
    """A mutual pair (0, N - 1); node 0 sends to the spokes 1 .. n_spokes, which send to node N - 1 (all asymmetric): in weighted
    mode the pair's tie weighs 2, the two hubs have mx = 2 and the spokes mx = 1."""
    Y = np.zeros((N, N), np.uint8)
    Y[0, N - 1] = Y[N - 1, 0] = 2
    Y[0, 1:n_spokes + 1] = 1
    Y[1:n_spokes + 1, N - 1] = 1
    return Y


def designs(N=300):
    """name -> Y [N, N] of the designed networks at N nodes (N >= 300)."""
    return {"star": star(N, 256), "mutual star": star(N, 256, "mutual"), "clique": clique(N, 17), "path": path(N),
            "clique and star": clique_and_star(N, 12, 40), "pair and spokes": pair_and_spokes(N, 70), "empty": np.zeros((N, N), np.uint8)}


def clique_constraint(n):
    """The constraint of a node of an n-clique, an exact rational: (n - 1) (1 / (n - 1) + (n - 2) / (n - 1)^2)^2."""
    return (n - 1) * (Fraction(1, n - 1) + Fraction(n - 2, (n - 1) ** 2)) ** 2


# ------------------------------------------------------------------------------------------ the launch shape
SH_BLK = 32                 # words of row i whose neighbours k_sh_node lists at a time (holes.hip)
SH_TILE = 256               # nodes of a tile of k_sh_rank

# The N the GPU file enters the kernels at, and what each is for (test_holes_host.py holds the list to `holes_shape`)
SHAPE_NS = {
    63: "one word, one lane per neighbour, 63 of its bits valid; one rank tile",
    64: "one word, full",
    65: "two words, two lanes per neighbour; node 64 the only bit of the last word",
    129: "three words on two lanes: the word stride takes a second trip (W > G)",
    257: "five words on four lanes, W > G; two rank tiles, the second with one node",
    300: "five words on four lanes, W > G: the closed forms",
    513: "nine words on 8 lanes, W > G; three rank tiles",
    1024: "16 words on 16 lanes: row i in registers",
    1025: "17 words on 16 lanes, W > G",
    2048: "32 words on 32 lanes in registers: one full list block",
    2049: "33 words on 32 lanes: two list blocks, W > G",
    4097: "65 words on 64 lanes: three list blocks, a second trip of the word stride; 17 rank tiles",
}


def holes_shape(N):
    """(W, G, one, blocks, trips, tiles) of the kernels on N nodes, restated: W words per bit row, G lanes per neighbour
    (`shape_of`), `one` when row i's words stay in registers (W <= G), the list blocks of SH_BLK words a node walks, the trips of
    the word stride (ceil(W / G)) and the tiles of SH_TILE nodes k_sh_rank streams."""
    W, lG = shape_of(N)[:2]
    G = 1 << lG
    return W, G, W <= G, (W + SH_BLK - 1) // SH_BLK, (W + G - 1) // G, (N + SH_TILE - 1) // SH_TILE


def planted(N, ties, n_clique, seed, last=True):
    """uint8 [N, N]: a random digraph with `ties` expected out-ties per node and entries 1..3, random diagonal entries, forced
    mutual ties, and a mutual n_clique-clique -- on nodes spread over the index range with node N - 1 among them, or (last=False)
    on the last n_clique nodes.  Sparse ones keep isolates and nodes with in-ties only."""
    g = np.random.RandomState(seed)
    Y = ((g.random_sample((N, N)) < ties / N) * g.randint(1, 4, (N, N))).astype(np.uint8)
    Y[np.arange(0, N, 3), np.arange(0, N, 3)] = 1
    m = g.choice(N, max(N // 8, 2), replace=False)
    Y[m[:-1], m[1:]] = 1
    Y[m[1:], m[:-1]] = 2
    members = np.unique(np.r_[g.choice(N - 1, n_clique - 1, replace=False), N - 1]) if last else np.arange(N - n_clique, N)
    Y[np.ix_(members, members)] = 1
    return Y
