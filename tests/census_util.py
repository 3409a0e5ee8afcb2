"""Host-only yardsticks of the triad census (vmr_sample_triad_census, vmr_network_triad_census; vimure_amd/csrc/census.hip).
Nothing here touches the device or reads the kernel's class table.

The class table is derived from the definition: the 64 digraphs on three named nodes are codes of six bits -- 1: 0 -> 1, 2: 1 -> 0,
4: 0 -> 2, 8: 2 -> 0, 16: 1 -> 2, 32: 2 -> 1 -- two codes are one class when a permutation of the nodes maps one onto the other,
and a class is named by its mutual, asymmetric and null dyads plus, where that leaves a choice, the letter of a fixed
representative.  Three counters on top of it: `census_np` (every triple, the definition), `census_pairs` (the kernel's scheme,
connected pair by connected pair, in NumPy) and `census_fast` (the same counts as matrix products, for large N); designed networks
with closed forms; and the kernel's launch shape restated from N."""
import functools
import itertools
from math import comb

import numpy as np
from scipy.sparse import csr_matrix

from tests.graph_shapes_util import shape_of

CLASS_NAMES = ("003", "012", "102", "021D", "021U", "021C", "111D", "111U", "030T", "030C", "201", "120D", "120U", "120C", "210", "300")
CLASS_SIZES = (1, 6, 3, 3, 3, 6, 6, 6, 6, 2, 3, 3, 3, 6, 6, 1)      # the labelled digraphs of each class
EDGE_BITS = {(0, 1): 1, (1, 0): 2, (0, 2): 4, (2, 0): 8, (1, 2): 16, (2, 1): 32}
# a fixed representative per name, as ties among the nodes a = 0, b = 1, c = 2
REPRESENTATIVES = {
    "003": (), "012": ((0, 1),), "102": ((0, 1), (1, 0)),
    "021D": ((1, 0), (1, 2)),                       # a <- b -> c: one node sends Down to both
    "021U": ((0, 1), (2, 1)),                       # a -> b <- c: both send Up to one
    "021C": ((0, 1), (1, 2)),                       # a -> b -> c
    "111D": ((0, 1), (1, 0), (2, 1)),               # a <-> b <- c
    "111U": ((0, 1), (1, 0), (1, 2)),               # a <-> b -> c
    "030T": ((0, 1), (2, 1), (0, 2)),               # a -> b <- c, a -> c
    "030C": ((0, 1), (1, 2), (2, 0)),               # a -> b -> c -> a
    "201": ((0, 1), (1, 0), (1, 2), (2, 1)),
    "120D": ((1, 0), (1, 2), (0, 2), (2, 0)),       # a <- b -> c, a <-> c
    "120U": ((0, 1), (2, 1), (0, 2), (2, 0)),       # a -> b <- c, a <-> c
    "120C": ((0, 1), (1, 2), (0, 2), (2, 0)),       # a -> b -> c, a <-> c
    "210": ((0, 1), (1, 2), (2, 1), (0, 2), (2, 0)),
    "300": tuple(EDGE_BITS),
}
CONNECTED = tuple(int(n[0]) + int(n[1]) for n in CLASS_NAMES)       # connected dyads of a triad of each class


def code_of(edges):
    return sum(EDGE_BITS[e] for e in edges)


def edges_of(code):
    return tuple(e for e, b in EDGE_BITS.items() if code & b)


def canonical(code):
    """The smallest code among the six relabellings of the digraph `code`."""
    return min(code_of((p[a], p[b]) for a, b in edges_of(code)) for p in itertools.permutations(range(3)))


def man_digits(code):
    """(mutual, asymmetric, null) dyads of the digraph `code`."""
    pairs = [(code >> s) & 3 for s in (0, 2, 4)]
    return sum(p == 3 for p in pairs), sum(p in (1, 2) for p in pairs), sum(p == 0 for p in pairs)


@functools.lru_cache(maxsize=None)
def class_table():
    """int64 [64] (read-only): the index into CLASS_NAMES of every code, by canonicalisation -- 16 classes of the sizes
    CLASS_SIZES, each named by its digits and, where several classes share them, by the representative it contains."""
    canon = [canonical(c) for c in range(64)]
    classes = sorted(set(canon))
    assert len(classes) == 16
    index = {}
    for name, edges in REPRESENTATIVES.items():
        k = canonical(code_of(edges))
        assert "%d%d%d" % man_digits(k) == name[:3] and k not in index, name
        index[k] = CLASS_NAMES.index(name)
    assert sorted(index) == classes
    table = np.array([index[k] for k in canon], dtype=np.int64)
    assert tuple(np.bincount(table, minlength=16)) == CLASS_SIZES
    table.flags.writeable = False
    return table


def adjacency(Y):
    """bool [N, N]: (Y > 0) with the diagonal cleared."""
    B = np.asarray(Y) > 0
    return B & ~np.eye(len(B), dtype=bool)


def census_one(Y):
    """int64 [16]: the census of one network [N, N] from the definition -- the code of every triple i < j < k, row by row."""
    B = adjacency(Y).astype(np.int64)
    N = len(B)
    codes = np.zeros(64, np.int64)
    for i in range(N - 2):
        r = np.arange(i + 1, N)
        sub = B[np.ix_(r, r)]
        c = (B[i, r] + 2 * B[r, i])[:, None] + (4 * B[i, r] + 8 * B[r, i])[None, :] + 16 * sub + 32 * sub.T     # [j, k]
        codes += np.bincount(c[np.triu_indices(len(r), 1)], minlength=64)
    return np.bincount(class_table(), weights=codes, minlength=16).astype(np.int64)


def census_np(Ys):
    """int64 [S, L, 16] of networks Ys [S, L, N, N] (an entry > 0 is a tie, the diagonal is ignored)."""
    Ys = np.asarray(Ys)
    return np.array([[census_one(Y) for Y in Yl] for Yl in Ys], dtype=np.int64).reshape(Ys.shape[0], Ys.shape[1], 16)


def states(Y):
    """int64 [N, N]: st[i, k] = 0 none, 1 out (i -> k), 2 in (k -> i), 3 both; 0 on the diagonal."""
    B = adjacency(Y).astype(np.int64)
    return B + 2 * B.T


def census_pairs(Y):
    """int64 [16] of one network [N, N] by the kernel's scheme: for every connected pair i < j the thirds k in each of the 15
    combinations (st(i, k), st(j, k)) other than (none, none) -- with i and j themselves left out -- the thirds tied to neither as
    N - 2 - their sum, the class of (i, j, k) as the code st(i, j) + 4 st(i, k) + 16 st(j, k), every class total divided by the
    connected dyads of its triads (asserted exact) and 003 = C(N, 3) - the rest."""
    st = states(Y)
    N = len(st)
    table = class_table()
    tot = np.zeros(16, np.int64)
    keep = np.ones(N, bool)
    for i, j in zip(*np.nonzero(np.triu(st, 1))):
        keep[[i, j]] = False
        ab = np.bincount((st[i] + 4 * st[j])[keep], minlength=16)
        keep[[i, j]] = True
        ab[0] = N - 2 - ab[1:].sum()
        np.add.at(tot, table[st[i, j] + 4 * (np.arange(16) % 4) + 16 * (np.arange(16) // 4)], ab)
    assert tot[0] == 0
    for c in range(1, 16):
        assert tot[c] % CONNECTED[c] == 0, (CLASS_NAMES[c], tot[c])
        tot[c] //= CONNECTED[c]
    tot[0] = comb(N, 3) - tot[1:].sum()
    return tot


def _fast_one(Y, sparse):
    B = adjacency(Y)
    N = len(B)
    S = [None, B & ~B.T, B.T & ~B, B & B.T]
    S = [None] + [csr_matrix(x.astype(np.float64)) if sparse else x.astype(np.float64) for x in S[1:]]
    had = (lambda X, Z: X.multiply(Z).sum()) if sparse else (lambda X, Z: (X * Z).sum())
    row = [None] + [np.asarray(x.sum(axis=1)).ravel() for x in S[1:]]
    col = [None] + [np.asarray(x.sum(axis=0)).ravel() for x in S[1:]]
    P = {(a, b): S[a] @ S[b].T for a in (1, 2, 3) for b in (1, 2, 3)}      # P[a, b][i, j] = #{k : st(i, k) = a, st(j, k) = b}
    F = np.zeros((4, 4, 4))                                                 # ordered (i, j, k) with st(i, j) = t, st(i, k) = a, st(j, k) = b
    mirror = (0, 2, 1, 3)                                                   # st(j, i) of st(i, j)
    for t in (1, 2, 3):
        pairs = row[t].sum()
        for a in (1, 2, 3):
            for b in (1, 2, 3):
                F[t, a, b] = had(S[t], P[a, b])
        for a in (1, 2, 3):      # k in state a from i and tied to j not at all: all of i's, less j itself, less those tied to j
            F[t, a, 0] = row[t] @ row[a] - (pairs if a == t else 0.0) - F[t, a, 1:].sum()
            F[t, 0, a] = col[t] @ row[a] - (pairs if a == mirror[t] else 0.0) - F[t, 1:, a].sum()
        F[t, 0, 0] = pairs * (N - 2) - F[t].sum()
    assert F.max() < 2.0 ** 53 and np.array_equal(F, np.rint(F))
    t, a, b = np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij")
    tot = np.bincount(class_table()[(t + 4 * a + 16 * b).ravel()], weights=F.ravel(), minlength=16).astype(np.int64)
    for c in range(1, 16):       # every connected dyad of a triad is met in both orders
        assert tot[c] % (2 * CONNECTED[c]) == 0, CLASS_NAMES[c]
        tot[c] //= 2 * CONNECTED[c]
    tot[0] = comb(N, 3) - tot[1:].sum()
    return tot


def census_fast(Ys):
    """int64 [S, L, 16] of Ys [S, L, N, N] as matrix products: with S_x the 0/1 matrix of the pairs in state x, the ordered triples
    with st(i, j) = t, st(i, k) = a, st(j, k) = b are sum(S_t o (S_a S_b^T)) for t, a, b >= 1; a = 0 or b = 0 follow from the row and
    column sums, t = 0 is never needed (every class but 003 has a connected dyad).  float64 products of 0/1 matrices, exact below
    2^53 (asserted); scipy.sparse where fewer than 5 % of the pairs are tied, BLAS otherwise."""
    Ys = np.asarray(Ys)
    out = np.zeros(Ys.shape[:2] + (16,), np.int64)
    for s in range(Ys.shape[0]):
        for l in range(Ys.shape[1]):
            out[s, l] = _fast_one(Ys[s, l], sparse=np.count_nonzero(Ys[s, l]) < 0.05 * Ys[s, l].size)
    return out


# ------------------------------------------------------------------------------------------ designs
_LADDER_ORDER = (4, 7, 12, 9, 13, 5, 14, 15, 10, 8, 11, 6, 3, 2, 1, 0)


def ladder_classes(N):
    """The classes of the N // 3 disjoint triples of `class_ladder(N)`: round r = 0, 1, .. adds one triple of every class q >= r,
    so that 136 triples (N >= 408) hold q + 1 copies of class q and any two swapped classes show.  A shorter ladder stops where
    the nodes end and tells fewer classes apart; within a round 021U, 111U, 120U, 030C and 120C come first, so that the 21 triples
    of N = 63, 64 and 65 hold them twice and 021D, 111D, 120D and 030T once."""
    seq = [q for r in range(16) for q in _LADDER_ORDER if q >= r]
    return seq[:N // 3]


def class_ladder(N, seed=5):
    """uint8 [N, N]: disjoint triples, each a representative of the class `ladder_classes(N)` names, on a fixed random permutation
    of the nodes (triples straddle the 64-bit words of a row); ties carry values 1 to 3 and a third of the diagonal is set.  Nodes
    of different triples are not tied, so every class from 021D on is counted exactly as often as the ladder holds it."""
    g = np.random.RandomState(seed + N)
    perm = g.permutation(N)
    Y = np.zeros((N, N), np.uint8)
    for q, cls in enumerate(ladder_classes(N)):
        nodes = perm[3 * q:3 * q + 3]
        for a, b in REPRESENTATIVES[CLASS_NAMES[cls]]:
            Y[nodes[a], nodes[b]] = 1 + (q + a + b) % 3
    Y[np.arange(0, N, 3), np.arange(0, N, 3)] = 2
    return Y


def ladder_census(N):
    """int64 [16]: the census of `class_ladder(N)` in closed form.  A triple inside a ladder triple has that triple's class; two
    nodes of one ladder triple and a node outside it see one dyad: 012, 102 or 003; everything else is 003."""
    tot = np.zeros(16, np.int64)
    for cls in ladder_classes(N):
        tot[cls] += 1
        m, a, n = (int(d) for d in CLASS_NAMES[cls][:3])
        tot[1] += a * (N - 3)
        tot[2] += m * (N - 3)
    tot[0] += comb(N, 3) - tot.sum()
    return tot


def _census(N, **classes):
    tot = np.zeros(16, np.int64)
    for name, v in classes.items():
        tot[CLASS_NAMES.index(name.lstrip("c"))] = v
    tot[0] = comb(N, 3) - tot[1:].sum()
    return tot


def path(N):
    """(Y, census) of the directed path 0 -> 1 -> .. -> N - 1: N - 2 triads 021C, (N - 2)(N - 3) of 012."""
    Y = np.zeros((N, N), np.uint8)
    Y[np.arange(N - 1), np.arange(1, N)] = 1
    return Y, _census(N, c021C=N - 2, c012=(N - 2) * (N - 3))


def star(N, kind, centre=0):
    """(Y, census) of a star: kind "out" (the centre sends to everybody: C(N - 1, 2) of 021D), "in" (021U) or "mutual" (201); the
    C(N - 1, 3) triples without the centre are 003."""
    Y = np.zeros((N, N), np.uint8)
    if kind in ("out", "mutual"):
        Y[centre, :] = 1
    if kind in ("in", "mutual"):
        Y[:, centre] = 1
    Y[centre, centre] = 0
    name = {"out": "c021D", "in": "c021U", "mutual": "c201"}[kind]
    return Y, _census(N, **{name: comb(N - 1, 2)})


def three_cycle(N):
    """(Y, census) of one directed 3-cycle on the nodes 0, N // 2 and N - 1: one 030C, and each of its three ties with each of the
    N - 3 other nodes a 012."""
    a, b, c = 0, N // 2, N - 1
    Y = np.zeros((N, N), np.uint8)
    Y[a, b] = Y[b, c] = Y[c, a] = 1
    return Y, _census(N, c030C=1, c012=3 * (N - 3))


def complete(N):
    return np.ones((N, N), np.uint8), _census(N, c300=comb(N, 3))


def empty(N):
    return np.zeros((N, N), np.uint8), _census(N)


def random_digraph(N, p, seed, vmax=3):
    """uint8 [N, N]: a tie with probability p, values 1..vmax, the diagonal drawn like the rest."""
    g = np.random.RandomState(seed)
    return ((g.random_sample((N, N)) < p) * g.randint(1, vmax + 1, (N, N))).astype(np.uint8)


def boundary_graph(N, degree, seed):
    """uint8 [N, N] for the word-boundary tests: `degree` ties per node on average with values 1..3, the diagonal drawn like the
    rest and set at node N - 1, and node N - 1 tied both ways (to node 0, from node 1, and mutually with node N // 2)."""
    Y = random_digraph(N, degree / N, seed)
    Y[N - 1, N - 1] = 1
    Y[N - 1, 0], Y[1, N - 1] = 1, 2
    Y[N - 1, N // 2] = Y[N // 2, N - 1] = 3
    return Y


# ------------------------------------------------------------------------------------------ the launch shape
CEN_BLK = 32                 # words of row i whose neighbours k_census lists at a time (census.hip)
CEN_LIST = CEN_BLK * 64      # the slots of that list

# The N the GPU file enters k_census at, and what each is for (test_census_host.py holds the list to `census_shape`)
SHAPE_NS = {
    63: "one word, one lane per neighbour, 63 of its bits valid",
    64: "one word, full",
    65: "two words, two lanes per neighbour; node 64 the only bit of the last word",
    129: "three words on two lanes: the word stride takes a second trip (W > G)",
    257: "five words on four lanes, W > G",
    300: "five words on four lanes, W > G: the closed forms",
    513: "nine words on 8 lanes, W > G",
    1024: "16 words on 16 lanes: row i in registers",
    1025: "17 words on 16 lanes, W > G",
    2048: "32 words on 32 lanes in registers: one full list block",
    2049: "33 words on 32 lanes: two list blocks, W > G",
    4097: "65 words on 64 lanes: three list blocks, a second trip of the word stride, the hub's lists of exactly CEN_LIST entries",
}


def reversed_nodes(Y):
    """Y [..., N, N] with the nodes in reverse order: node v becomes N - 1 - v.  k_census lists the neighbours j > i only, and the
    hub of `graph_shapes_util.design` is the LAST node, whose lists are empty; reversed it is node 0 and lists everybody."""
    return np.ascontiguousarray(np.asarray(Y)[..., ::-1, ::-1])


def list_sizes(Y, i):
    """The entries of node i's neighbour list in k_census, block by block of CEN_BLK words from the block that holds bit i: the
    j > i tied to i either way."""
    B = adjacency(Y)
    u = B[i] | B[:, i]
    u[:i + 1] = False
    first = (i // 64) // CEN_BLK
    blocks = (shape_of(len(B))[0] + CEN_BLK - 1) // CEN_BLK
    return [int(u[b * CEN_LIST:(b + 1) * CEN_LIST].sum()) for b in range(first, blocks)]


def census_shape(N):
    """(W, G, one, blocks, trips) of k_census on N nodes, restated: W words per bit row, G lanes per neighbour (`shape_of`), `one`
    when row i's words stay in registers (W <= G), the list blocks of CEN_BLK words node 0 walks, and the trips of the word
    stride (ceil(W / G))."""
    W, lG = shape_of(N)[:2]
    G = 1 << lG
    return W, G, W <= G, (W + CEN_BLK - 1) // CEN_BLK, (W + G - 1) // G
