"""CPU: tests/graph_shapes_util.py held to what the suite already trusts, so that tests/test_hip_graph_shapes.py cannot pass by
being vacuous -- `triads_sparse` against `triads_np`, `path_betweenness` against `betweenness_np`, the N lists against the shape
classes they are there for, and per design the preconditions that make a comparison with the device mean something.  No GPU
needed."""
import numpy as np
import pytest

from tests.betweenness_util import DIRECTIONS as BTW_DIRECTIONS
from tests.betweenness_util import betweenness_np
from tests.centrality_util import DIRECTIONS as CENT_DIRECTIONS
from tests.centrality_util import ranks_np
from tests.golden_util import load_case
from tests.graph_shapes_util import (BOUND_N, MAIN_NS, TRI_LIST, TRIAD_FOUR_NS, TRIAD_LARGE_NS, betweenness_values, centrality_values,
                                     design, design_large, last_slot_nodes, last_word_nodes, path_betweenness, shape_of, triads_sparse)
from tests.triads_util import triads_np


def _assert_same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("N", [65, 129, 300])
def test_triads_sparse_equals_triads_np_on_the_designs(N):
    Y = design(N)
    want = triads_np([Y])
    assert want["triangles_u"][0, [0, 2, 3]].min() > 0 and want["cyclic"][0, 2:].min() > 0 and not want["triangles_u"][0, 1]
    _assert_same(triads_sparse([Y]), want)
    _assert_same(triads_sparse([design_large(N)]), triads_np([design_large(N)]))


def test_triads_sparse_equals_triads_np_on_the_networks_of_the_triad_tests():
    """The random samples with self-loops and entries up to 3 and the known graphs of tests/test_triads_host.py, and every
    reporter's reports of the golden cases tests/test_hip_triads.py draws its samples from."""
    g = np.random.RandomState(5)
    Ys = (g.rand(3, 2, 7, 7) < 0.45) * g.randint(1, 4, (3, 2, 7, 7))
    _assert_same(triads_sparse(Ys), triads_np(Ys))
    cyc, tr, full = np.zeros((5, 5), np.int64), np.zeros((5, 5), np.int64), np.ones((5, 5), np.int64)
    cyc[0, 1] = cyc[1, 2] = cyc[2, 0] = 1
    tr[0, 1] = tr[1, 2] = tr[0, 2] = 1
    _assert_same(triads_sparse([[cyc, tr, full]]), triads_np([[cyc, tr, full]]))
    for case in ("A_ones_mut", "B_random_mask_K3", "D_self_mask", "E_undirected"):
        X = load_case(case)["X"]
        Ys = np.moveaxis(X, -1, 0)                      # [M][L, N, N]: one network per reporter
        want = triads_np(Ys)
        assert want["two_paths"].max() > 0, case
        _assert_same(triads_sparse(Ys), want)


def test_path_betweenness_equals_the_restatement():
    N = 129
    Y = design(N)[1]
    for d in BTW_DIRECTIONS:
        assert np.array_equal(path_betweenness(N), betweenness_np([[Y]], d)["values"][0, 0]), d


def test_shape_of_restates_the_launch_shape():
    """Against the shapes the existing files name in words: 65 -> two words, 129 -> three, 257 and 300 -> five words and two nodes
    per thread, 2048 -> 32 words and eight nodes."""
    assert shape_of(5) == (1, 0, 1, 1, True, 1) and shape_of(64) == (1, 0, 1, 1, True, 1)
    assert shape_of(65) == (2, 1, 1, 1, True, 1) and shape_of(129) == (3, 1, 1, 1, False, 1)
    assert shape_of(211) == (4, 2, 1, 1, True, 1) and shape_of(256) == (4, 2, 1, 1, True, 1)
    assert shape_of(257) == (5, 2, 2, 2, False, 1) and shape_of(300) == (5, 2, 2, 2, False, 1)
    assert shape_of(2048) == (32, 5, 8, 8, True, 1) and shape_of(4096) == (64, 6, 16, 8, True, 2)
    assert shape_of(65536) == (1024, 6, 256, 8, False, 32)
    for N in range(1, 2049):                               # the rung holds the thread's nodes and is the smallest that does
        W, lG, kpt, rung, one, blocks = shape_of(N)
        assert (1 << lG) <= min(W, 64) < (2 << lG) and kpt <= rung and (rung == 1 or rung // 2 < kpt) and 4 * rung >= W


def test_the_lists_cover_every_shape_class():
    """The one place where the shape classes are named.  Each class with the N of the GPU file that must enter it: if a bound of
    the kernels or the ladder of rungs changes, `shape_of` changes with it and this says which class lost its case."""
    main, triads = set(MAIN_NS), set(MAIN_NS) | {BOUND_N} | set(TRIAD_FOUR_NS) | set(TRIAD_LARGE_NS)
    sh = {N: dict(zip(("W", "lG", "kpt", "rung", "one", "blocks"), shape_of(N))) for N in triads}
    classes = {
        # all five units
        "G = 8": (main, 513, lambda s: s["lG"] == 3),
        "G = 16": (main, 1024, lambda s: s["lG"] == 4),
        "G = 8, second trip of the word stride": (main, 513, lambda s: s["lG"] == 3 and s["W"] > 8),
        "G = 16, second trip of the word stride": (main, 1025, lambda s: s["lG"] == 4 and s["W"] > 16),
        "G = 16, one trip": (main, 1024, lambda s: s["lG"] == 4 and s["W"] == 16),
        "rung 4 with kpt = 3": (main, 513, lambda s: (s["rung"], s["kpt"]) == (4, 3)),
        "rung 4 with kpt = 4": (main, 1024, lambda s: (s["rung"], s["kpt"]) == (4, 4)),
        "rung 8 with kpt = 5": (main, 1025, lambda s: (s["rung"], s["kpt"]) == (8, 5)),
        # connectivity at its node bound
        "connectivity: N = CONN_NMAX": ({BOUND_N}, 2048, lambda s: (s["W"], s["kpt"]) == (32, 8)),
        # triads
        "triads: register path, W = 4": (triads, 256, lambda s: s["one"] and s["W"] == 4),
        "triads: register path, W = 8": (triads, 512, lambda s: s["one"] and s["W"] == 8),
        "triads: register path, W = 16": (triads, 1024, lambda s: s["one"] and s["W"] == 16),
        "triads: register path, W = 32": (triads, 2048, lambda s: s["one"] and s["W"] == 32),
        "triads: two blocks of 32 words": (triads, 2049, lambda s: s["blocks"] == 2),
        "triads: three blocks of 32 words": (triads, 4097, lambda s: s["blocks"] == 3),
        "triads: G = 64, second trip of the degree loop": (triads, 4097, lambda s: s["lG"] == 6 and s["W"] > 64),
    }
    for name, (pool, N, holds) in classes.items():
        assert N in pool and holds(sh[N]), "no N of the GPU file enters the class '%s' any more: N = %d has %r" % (name, N, sh[N])
        print("%-50s N = %4d  %r" % (name, N, sh[N]))
    # the last word holds one valid bit and the last slot one node where the designs put the hub
    assert {N % 64 for N in (513, 1025, 2049, 4097)} == {1} and {N % 256 for N in (513, 1025)} == {1}
    from vimure_amd import _lib
    assert BOUND_N == _lib.CONN_NMAX == _lib.CENT_NMAX == _lib.BTW_NMAX == _lib.CORE_NMAX


def _ties_both_ways(A, nodes):
    return bool((A[nodes].any(axis=1) & A[:, nodes].any(axis=0)).any())


@pytest.mark.parametrize("N", MAIN_NS + (BOUND_N,) + TRIAD_FOUR_NS)
def test_design_preconditions(N):
    """What every layer is there for, and that the last word and the last slot are not idle: in the sparse, the dense and the
    hub layer one of their nodes has ties both ways (on the path the last node has one tie by design: N - 2 -> N - 1)."""
    Y = design(N)
    assert Y.shape == (4, N, N) and Y.dtype == np.uint8
    A = (Y > 0) & ~np.eye(N, dtype=bool)
    assert (Y[0] > 1).any() and Y[0].diagonal().any() and Y[2].diagonal().any() and Y[3].diagonal().all()
    assert 2.0 * N <= A[0].sum() <= 4.0 * N
    assert A[1].sum() == N - 1 and A[1][N - 2, N - 1] and not A[1][N - 1].any()
    W = shape_of(N)[0]
    words = A[2][:, :64 * (W - 1)].reshape(N, W - 1, 64).any(axis=2)       # every full word of every row has bits
    assert words.all() and A[2][:, 64 * (W - 1):].any(axis=1).mean() > (0.2 if N % 64 == 1 else 0.9)
    assert A[3][N - 1, :N - 1].all() and A[3][:N - 1, N - 1].all() and A[3].sum() == (N - 2) + 2 * (N - 1)
    for l in (0, 2, 3):
        assert _ties_both_ways(A[l], last_word_nodes(N)) and _ties_both_ways(A[l], last_slot_nodes(N)), l


@pytest.mark.parametrize("N", TRIAD_LARGE_NS)
def test_design_large_preconditions(N):
    Y = design_large(N)
    assert Y.shape == (1, N, N) and Y.dtype == np.uint8 and (Y > 1).any() and Y[0].diagonal().all()
    A = (Y[0] > 0) & ~np.eye(N, dtype=bool)
    deg = (A | A.T).sum(axis=1)
    assert deg[N - 1] == N - 1 and 5 <= np.median(deg[:N - 1]) <= 12
    if N == 4097:       # the hub's neighbours fill two lists to the last slot and leave the third empty
        assert (A | A.T)[N - 1, :TRI_LIST].sum() == TRI_LIST and (A | A.T)[N - 1, TRI_LIST:2 * TRI_LIST].sum() == TRI_LIST


@pytest.mark.parametrize("N", MAIN_NS)
def test_exactness_preconditions(N):
    """`exact_ok` at q = 1/2, T = 4 for every layer and direction (asserted where the reference is computed), no shortest-path
    count beyond 2^53 (`exact_sigma`), and a sparse layer with at least 8 distinct centrality values and tied ranks."""
    for d in CENT_DIRECTIONS:
        c = centrality_values(N, d)
        assert c.shape == (4, N) and (c.max(axis=1) > 0).all(), d
        distinct = np.unique(c[0]).size
        assert 8 <= distinct < N, (d, distinct)
        r = ranks_np(c[0])
        assert np.unique(r).size < N, d                 # tied ranks
    for d in BTW_DIRECTIONS:
        b = betweenness_values(N, d)
        assert b.shape == (4, N) and (b.max(axis=1) > 0).all(), d
