"""Host-only helpers of the launch-shape tests of the graph read-outs (triads.hip, connectivity.hip, centrality.hip,
betweenness.hip, cores.hip): the launch shape restated from N, designed networks that make every lane, word and node slot of a
shape matter, and two references that stay cheap where `triads_np` and `betweenness_np` do not.  Nothing here touches the device;
tests/test_graph_shapes_host.py holds this file to the restatements the suite already trusts, tests/test_hip_graph_shapes.py uses
it to hold the kernels."""
import functools

import numpy as np
from scipy.sparse import csr_matrix

from tests.triads_util import TRIAD_KEYS

TRI_BLK = 32                 # words of a row whose neighbours k_tri_count lists at a time (triads.hip)
TRI_LIST = TRI_BLK * 64      # the slots of that list
TPB = 256                    # threads of a workgroup: node v belongs to thread v % 256, slot v / 256
RUNGS = (1, 2, 4, 8)         # the KPT the kernels with a template argument are instantiated for (with_kpt)

# The N the GPU file enters the kernels at; test_graph_shapes_host.py::test_the_lists_cover_every_shape_class names what each is for.
MAIN_NS = (513, 1024, 1025)       # four layers, all five units
BOUND_N = 2048                    # two layers: connectivity at its node bound, triads on the register path with W = 32
TRIAD_FOUR_NS = (256, 512)        # four layers, triads alone
TRIAD_LARGE_NS = (2049, 4097)     # one layer (design_large), triads alone
Q, T = 0.5, 4                     # the passing probability and the rounds of the centrality comparisons


def shape_of(N):
    """(W, lG, kpt, rung, tri_one, tri_blocks) of a handle with N nodes: `bit_rows()` and `with_kpt()` of
    vimure_amd/csrc/sampled_side.h and the branches of k_tri_count, restated.  W words per bit row; G = 1 << lG lanes stride a row,
    the largest power of two <= min(W, 64); kpt = ceil(N / 256) nodes per thread and the smallest rung >= kpt (8 beyond the
    ladder, where only triads accepts the handle); tri_one: triads keeps row i in registers (W <= G); tri_blocks: the blocks of 32
    words its neighbour list is built from."""
    W = (N + 63) // 64
    lG = 0
    while (2 << lG) <= W and lG < 6:
        lG += 1
    kpt = (N + TPB - 1) // TPB
    rung = next((r for r in RUNGS if kpt <= r), RUNGS[-1])
    return W, lG, kpt, rung, W <= (1 << lG), (W + TRI_BLK - 1) // TRI_BLK


def _frozen(a):
    a.flags.writeable = False
    return a


def _sparse_layer(g, N):
    return ((g.random_sample((N, N)) < 3.0 / N) * g.randint(1, 3, (N, N))).astype(np.uint8)


def _hub_layer(N):
    i = np.arange(N)
    Y = np.eye(N, dtype=np.uint8)
    Y[i, (i + 64) % N] = 1
    Y[N - 1, :] = 1
    Y[:, N - 1] = 1
    return Y


@functools.lru_cache(maxsize=None)
def design(N, seed=None):
    """Y [4, N, N] uint8 (read-only, cached; seed None: N), four layers chosen for what they make a kernel do:
    0  sparse: 3 ties per node on average, values 1 and 2 (an entry above 1 is a tie), the diagonal drawn like the rest: a
       different set of words has bits in every row, many nodes tie in every score.  The entries above 1 reach the packer
       through the calls that take networks (`network_cores`, `network_betweenness`) only: a sample drawn from `one_hot_rho`
       holds 0 and 1;
    1  the directed path i -> i + 1: N - 1 levels, every frontier and every list has one node, and the ties cross every word
       boundary;
    2  dense: a tie with probability 1/4, the diagonal too: every word of every row has bits, lists are long, most pairs are joined
       by several shortest paths;
    3  stride and hub: i -> (i + 64) mod N, so that every tie lands one word on, node N - 1 tied to and from everybody, the whole
       diagonal set.  At N = 64 m + 1 node N - 1 is the only valid bit of the last word, at N = 256 m + 1 the only node of the last
       slot."""
    g = np.random.RandomState(N if seed is None else seed)
    Y = np.zeros((4, N, N), np.uint8)
    Y[0] = _sparse_layer(g, N)
    i = np.arange(N - 1)
    Y[1, i, i + 1] = 1
    Y[2] = g.random_sample((N, N)) < 0.25
    Y[3] = _hub_layer(N)
    return _frozen(Y)


@functools.lru_cache(maxsize=2)
def design_large(N, seed=None):
    """Y [1, N, N] uint8 (read-only): the union of layers 0 and 3 of `design` -- for N >= 2048, where four one-hot layers of rho
    would be hundreds of MB.  The hub has N - 1 neighbours: at N = 4097 two neighbour lists of exactly TRI_LIST entries and an
    empty third."""
    g = np.random.RandomState(N if seed is None else seed)
    return _frozen(np.maximum(_sparse_layer(g, N), _hub_layer(N))[None])


def one_hot_rho(Y):
    """rho [L, N, N, 2] that puts all mass on (Y > 0): every posterior sample is then the design whatever the seed."""
    t = np.asarray(Y) > 0
    return np.stack([~t, t], axis=-1).astype(np.float64)


def triads_sparse(Ys):
    """The dict of `triads_util.triads_np` (the six counts int64 [S, L], node_tri and node_deg int32 [S, L, N]) through
    scipy.sparse products: the same definitions, without the dense int64 N^3 products that take minutes beyond N = 2000."""
    Ys = np.asarray(Ys)
    S, L, N, _ = Ys.shape
    out = {k: np.zeros((S, L), np.int64) for k in TRIAD_KEYS}
    out["node_tri"], out["node_deg"] = np.zeros((S, L, N), np.int32), np.zeros((S, L, N), np.int32)
    for s in range(S):
        for l in range(L):
            B = Ys[s, l] > 0
            B = B & ~np.eye(N, dtype=bool)
            A = csr_matrix(B.astype(np.int64))
            U = csr_matrix((B | B.T).astype(np.int64))
            At = A.T.tocsr()
            AA = A @ A
            d = np.asarray(U.sum(axis=1)).ravel()
            U3 = np.asarray((U @ U).multiply(U).sum(axis=1)).ravel()     # U is symmetric: sum_j (UU)_ij U_ji = diag(U^3)_i
            out["transitive"][s, l] = (A @ At).multiply(A).sum()
            out["cyclic"][s, l] = AA.multiply(At).sum()
            out["two_paths"][s, l] = AA.sum() - AA.diagonal().sum()
            out["triangles_u"][s, l] = U3.sum() // 6
            out["wedges_u"][s, l] = (d * (d - 1) // 2).sum()
            out["edges_u"][s, l] = U.sum() // 2
            out["node_tri"][s, l] = U3 // 2
            out["node_deg"][s, l] = d
    return out


def path_betweenness(N):
    """b [N] float64 of the path on N nodes, i (N - 1 - i): node i lies on the one shortest path from each of the i nodes before it
    to each of the N - 1 - i after it.  The same for the directed path and, halved over both orders of a pair, for the undirected
    one; every value is an integer below 2^53."""
    i = np.arange(N, dtype=np.float64)
    return i * (N - 1.0 - i)


@functools.lru_cache(maxsize=None)
def centrality_values(N, direction):
    """c [4, N] of `design(N)` at q = Q, T = T by `centrality_np`, after `exact_ok` on every layer: every number of the walk is
    then exactly representable, and the comparison with the device is for equality.  Cached: the host file asserts the
    precondition, the GPU file compares with the values."""
    from tests.centrality_util import adjacency, centrality_np, exact_ok
    Y = design(N)
    want = centrality_np([Y], Q, T, direction)["values"][0]
    for l in range(4):
        assert np.array_equal(exact_ok(adjacency(Y[l], direction), Q, T), want[l]), (N, direction, l)
    return _frozen(want)


@functools.lru_cache(maxsize=None)
def betweenness_values(N, direction):
    """b [4, N] of `design(N)`: layers 0, 2 and 3 by `betweenness_np(exact_sigma=True)` -- no shortest-path count beyond 2^53 --
    and the path layer by `path_betweenness`, which the restatement would walk level by level for half a minute.  Cached."""
    from tests.betweenness_util import betweenness_np
    Y = design(N)
    want = np.empty((4, N))
    want[[0, 2, 3]] = betweenness_np([Y[[0, 2, 3]]], direction, exact_sigma=True)["values"][0]
    want[1] = path_betweenness(N)
    return _frozen(want)


def last_word_nodes(N):
    """The nodes of the last word of a bit row."""
    return np.arange(64 * (shape_of(N)[0] - 1), N)


def last_slot_nodes(N):
    """The nodes of the last slot of a thread: what only N - 256 (kpt - 1) of the 256 threads own."""
    return np.arange(TPB * (shape_of(N)[2] - 1), N)


def repeat_samples(ref, S):
    """The reference of one sample [1, ...] as that of S equal samples, for the arrays whose first axis is the sample."""
    return {k: np.repeat(v, S, axis=0) for k, v in ref.items()}
