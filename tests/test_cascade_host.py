"""CPU: the restatement of the cascade calls (tests/cascade_util.py) held to closed forms, to scipy.sparse.csgraph and to the
distribution its draws must have -- the yardstick tests/test_hip_cascades.py holds the device to."""
import numpy as np
import pytest
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import shortest_path

from tests.cascade_util import (DIRECTIONS, NPER, adjacency, live_graph, outreach_values, path, path_outreach, random_digraph, reduce_values,
                                seed_outreach_np, set_words, star, star_outreach, tie_uniforms, two_cliques, two_cliques_outreach)


@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("T", [1, 3, 11, 12, 500])
def test_path_closed_form(direction, T):
    """q = 1 on the path of N: node i reaches min(T, N - 1 - i) nodes ahead ("out"), min(T, i) behind ("in"), both ("union");
    T = N - 1 is where the cut stops binding."""
    N = 12
    got = outreach_values(path(N)[None, None], 7, 2, 1.0, T, direction)
    assert got.dtype == np.uint32 and got.shape == (1, 1, N)
    assert np.array_equal(got[0, 0], 2 * path_outreach(N, T, direction))
    if direction == "out":
        assert np.array_equal(path_outreach(N, T, "out"), np.minimum(T, N - 1 - np.arange(N)))


@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("T", [1, 2, 5])
def test_star_and_two_cliques_closed_forms(direction, T):
    N = 50
    Y = np.stack([star(N), two_cliques(N)])[None]
    got = outreach_values(Y, 3, 1, 1.0, T, direction)
    assert np.array_equal(got[0, 0], star_outreach(N, T, direction))
    assert np.array_equal(got[0, 1], two_cliques_outreach(N, T, direction))
    assert not got[0, 1, 42:].any()                                              # the isolated nodes, diagonal entries ignored


def test_q_zero_gives_zeros_and_q_one_keeps_every_tie():
    Y = random_digraph(40, 4.0, 1)[None, None]
    for d in DIRECTIONS:
        assert not outreach_values(Y, 5, 3, 0.0, 4, d).any()
    A = adjacency(Y[0])
    assert np.array_equal(live_graph(A, 9, 0, [1.0], "out"), A)
    assert np.array_equal(live_graph(A, 9, 0, [1.0], "in"), A.transpose(0, 2, 1))
    assert np.array_equal(live_graph(A, 9, 0, [1.0], "union"), A | A.transpose(0, 2, 1))
    res = seed_outreach_np(Y, 5, 3, 0.0, 4, "out", [[0, 1], []])
    assert not res["values"].any() and not res["curve"].any()
    assert np.array_equal(res["node_hits"][0, 0], 3 * (np.arange(40) < 2)) and not res["node_hits"][0, 1].any()


def test_the_draw_belongs_to_the_tie():
    """The live ties of "in" are those of "out" transposed; "union" is symmetric and draws a pair once, at (min, max), whether A
    holds the pair one way, the other way or both; the key, the cascade and the layer all change the draw."""
    N = 60
    Y = np.stack([random_digraph(N, 5.0, 2), random_digraph(N, 5.0, 3)])
    A = adjacency(Y)
    q = [0.5, 0.3]
    out, inn, uni = (live_graph(A, 11, 4, q, d) for d in DIRECTIONS)
    assert out.any() and (out != A).any() and np.array_equal(inn, out.transpose(0, 2, 1))
    assert np.array_equal(uni, uni.transpose(0, 2, 1)) and uni.any() and not (uni & ~(A | A.transpose(0, 2, 1))).any()
    assert np.array_equal(live_graph(A.transpose(0, 2, 1), 11, 4, q, "union"), uni)
    assert np.array_equal(live_graph(A | A.transpose(0, 2, 1), 11, 4, q, "union"), uni)
    i, j = np.nonzero(np.triu(A[1] | A[1].T, 1))
    u = tie_uniforms(11, 4, (N + i) * N + j)
    assert np.array_equal(uni[1, i, j], u < 0.3)
    for other in (live_graph(A, 12, 4, q, "out"), live_graph(A, 11, 5, q, "out")):
        assert (other != out).any()
    assert (live_graph(A[::-1], 11, 4, [0.5, 0.5], "out")[1] != live_graph(A, 11, 4, [0.5, 0.5], "out")[0]).any()
    assert (tie_uniforms(11, 4, np.arange(50)) != tie_uniforms(11, 4, np.arange(50) + 2 ** 32)).all()   # the high word of the tie
    assert (tie_uniforms(1, 0, np.arange(50)) != tie_uniforms(1 + 2 ** 32, 0, np.arange(50))).all()     # ... and of the key


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_full_reach_equals_csgraph(direction):
    """q = 1 and T >= N - 1: the outreach is the number of nodes reachable in the spread's graph; with a T below the diameter it
    is the number within T steps."""
    N = 70
    Y = random_digraph(N, 1.6, 4)
    A = adjacency(Y)
    G = {"out": A, "in": A.T, "union": A | A.T}[direction]
    dist = shortest_path(csr_matrix(G.astype(np.int8)), unweighted=True)
    np.fill_diagonal(dist, np.inf)
    for T in (2, N - 1, 65535):
        got = outreach_values(Y[None, None], 0, 1, 1.0, T, direction)[0, 0]
        assert np.array_equal(got, (dist <= T).sum(axis=1))
    assert np.isfinite(dist).sum(axis=1).max() > (dist <= 2).sum(axis=1).max()


def test_seed_sets_restatement():
    """Sets on the path at q = 1: the curve's bins are the periods, the last bin collects every period >= 64, a set's bins sum to
    its outreach; the singleton {v} is the every-node outreach of v; the empty set and the full set reach nobody."""
    N, T = 100, 80
    Y = path(N)[None, None]
    sets = [[0], [], list(range(N)), [10, 50], [98]]
    res = seed_outreach_np(Y, 1, 2, 1.0, T, "out", sets)
    assert res["values"].dtype == np.uint32 and np.array_equal(res["values"][0, 0], 2 * np.array([80, 0, 0, 39 + 49, 1]))
    assert np.array_equal(res["curve"][0].sum(axis=-1), res["values"][0, 0])
    assert np.array_equal(res["curve"][0, 0], 2 * np.r_[np.ones(NPER - 1, np.int64), 80 - 63])
    assert np.array_equal(res["curve"][0, 3, :3], [4, 4, 4]) and res["curve"][0, 3, 40] == 2
    assert np.array_equal(res["node_hits"][0, 0], 2 * (np.arange(N) <= 80)) and np.array_equal(res["node_hits"][0, 2], np.full(N, 2))
    assert set_words(sets, N)[10] == 0b1100 and set_words(sets, N)[0] == 0b101
    Yr = np.stack([random_digraph(30, 3.0, 5), random_digraph(30, 3.0, 6)])[None]
    for d in DIRECTIONS:
        one = outreach_values(Yr, 8, 3, [0.6, 0.4], 3, d)
        single = seed_outreach_np(Yr, 8, 3, [0.6, 0.4], 3, d, [[v] for v in range(30)])
        assert one.any() and np.array_equal(single["values"], one)


def test_reductions():
    vals = np.array([[[4, 0, 4, 1]], [[2, 2, 0, 3]]], np.uint32)
    r = reduce_values(vals, 2, 2)
    assert np.array_equal(r["node_sum"], [[3.0, 1.0, 2.0, 2.0]]) and np.array_equal(r["node_sumsq"], [[5.0, 1.0, 4.0, 2.5]])
    assert np.array_equal(r["node_rank_sum"], [[0 + 1, 3 + 1, 0 + 3, 2 + 0]]) and np.array_equal(r["node_top"], [[2, 1, 1, 1]])
    assert np.array_equal(r["total"], [[9], [7]]) and np.array_equal(r["max"], [[4], [3]])
    assert r["total"].dtype == r["max"].dtype == r["node_rank_sum"].dtype == r["node_top"].dtype == np.int64


def test_hub_outreach_is_binomial():
    """One statistical check of the draw.  The hub of a star of d leaves informs each leaf with probability q, independently over
    the leaves and the cascades: its outreach summed over K cascades is Binomial(d K, q), mean d K q and standard deviation
    sqrt(d K q (1 - q)).  The sum must lie within 6 of those standard deviations (a chance of 2e-9 for a correct draw), and so
    must the sum of every single leaf's indicator over the cascades, Binomial(K, q), for all d leaves at once (Bonferroni: 6
    standard deviations leave d times 2e-9)."""
    d, q, K = 200, 0.3, 400
    A = adjacency(star(d + 1)[None])
    hub = np.zeros(d + 1, np.int64)
    for k in range(K):
        hub += live_graph(A, 77, k, [q], "out")[0, 0]
    assert not hub[0]
    total, sd = hub.sum(), np.sqrt(d * K * q * (1.0 - q))
    assert abs(total - d * K * q) <= 6.0 * sd, (total, d * K * q, sd)
    sd1 = np.sqrt(K * q * (1.0 - q))
    assert np.abs(hub[1:] - K * q).max() <= 6.0 * sd1
    # and the restatement's outreach is that count
    assert outreach_values(star(d + 1)[None, None], 77, 5, q, 3, "out")[0, 0, 0] == sum(
        live_graph(A, 77, k, [q], "out")[0, 0].sum() for k in range(5))
