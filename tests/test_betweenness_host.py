"""CPU: the host pieces of the posterior betweenness -- the NumPy restatement the GPU tests use (tests/betweenness_util.py) against
closed forms and against networkx, the binding's constants, and what `BetweennessStats` derives from the sums."""
import numpy as np
import pytest

from tests.betweenness_util import (BTW_KEYS, DIRECTIONS, betweenness_graph, betweenness_np, brandes_levels, diamond_chain,
                                    diamond_closed_form, search_graph, sigma_ok)
from tests.connectivity_util import designed_graphs


def test_restatement_on_designed_graphs():
    """N = 129: on the directed path node i lies on the i (N - 1 - i) pairs it separates; on a directed cycle of n nodes a path of
    k ties has k - 1 inner nodes, (n - 1)(n - 2) / 2 per node; a node with only a self-loop and the empty graph have 0."""
    Y = designed_graphs()
    N = Y.shape[1]
    i = np.arange(N)
    got = betweenness_np([Y], "directed", top_k=3)
    assert sorted(got) == sorted(BTW_KEYS + ("values",))
    b = got["values"][0]
    assert np.array_equal(b[0], i * (N - 1.0 - i))
    assert np.array_equal(b[1], np.full(N, (N - 1) * (N - 2) / 2.0))
    assert np.array_equal(b[2], np.r_[np.full(128, 63 * 62 / 2.0), 0.0])
    assert not b[3].any()
    assert np.array_equal(got["total"][0], b.sum(axis=1)) and np.array_equal(got["max"][0], b.max(axis=1))
    assert np.array_equal(got["node_rank_sum"][1], np.zeros(N)) and got["node_top"][2, 128] == 0 and got["node_top"][2, 0] == 1
    # union: the path is an undirected path, every unordered pair once; the cycle has two shortest ways round for no pair (N odd)
    u = betweenness_np([Y], "union")["values"][0]
    assert np.array_equal(u[0], i * (N - 1.0 - i))
    h = (N - 1) // 2
    assert np.array_equal(u[1], np.full(N, h * (h - 1) / 2.0))
    for l in range(4):
        assert sigma_ok(search_graph(Y[l], "directed"))[0] == 1.0


def test_restatement_on_a_star_and_on_diamonds():
    N = 17
    Y = np.zeros((N, N), np.uint8)
    Y[0, 1:] = 1                                                  # ties leave the centre only: directed, nothing lies between
    assert not betweenness_graph(search_graph(Y, "directed")).any()
    b = betweenness_graph(search_graph(Y, "union"), halve=True)
    assert b[0] == (N - 1) * (N - 2) / 2.0 and not b[1:].any()
    # a 4-cycle searched undirected: opposite nodes are joined by two paths, each inner node carries half a pair
    Y = np.zeros((4, 4), np.uint8)
    Y[[0, 1, 2, 3], [1, 2, 3, 0]] = 1
    assert np.array_equal(betweenness_graph(search_graph(Y, "union"), halve=True), np.full(4, 0.5))
    D, sigma, _ = brandes_levels(search_graph(Y, "union"))
    assert sigma[0].tolist() == [1.0, 1.0, 2.0, 1.0] and D[0].tolist() == [0, 1, 2, 1]
    Y = diamond_chain()
    assert Y.shape == (211, 211)
    G = search_graph(Y, "directed")
    D, sigma, _ = brandes_levels(G)
    assert sigma.max() == 2.0 ** 70 and sigma[0, 210] == 2.0 ** 70 and D.max() == 140
    with pytest.raises(AssertionError):
        sigma_ok(G)
    b = betweenness_graph(G)
    assert np.array_equal(b, diamond_closed_form()) and (b[1], b[3], b[4]) == (104.0, 621.0, 410.0)


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_restatement_against_networkx(direction):
    nx = pytest.importorskip("networkx")
    N = 65
    g = np.random.RandomState(12)
    for _ in range(3):
        Y = (g.rand(N, N) < 3.0 / N).astype(np.uint8)
        G = search_graph(Y, direction)
        smax, depth = sigma_ok(G)
        assert smax >= 2 and depth >= 4
        H = nx.from_numpy_array(G.astype(np.uint8), create_using=nx.DiGraph if direction == "directed" else nx.Graph)
        want = nx.betweenness_centrality(H, normalized=False)
        want = np.array([want[v] for v in range(N)])
        got = betweenness_graph(G, halve=direction == "union")
        assert (want > 0).sum() >= 16
        assert np.allclose(got, want, rtol=1e-12, atol=0)


def test_binding_constants_and_null_handle():
    from vimure_amd import _lib, build
    assert "vmr_sample_betweenness" in _lib.SIGNATURES and "vmr_network_betweenness" in _lib.SIGNATURES
    assert _lib.BTW_DIRECTIONS == DIRECTIONS
    hdr = open(build.HEADERS[-1]).read()
    for name, val in (("VMR_BTW_NMAX", _lib.BTW_NMAX), ("VMR_BTW_DIRECTED", 0), ("VMR_BTW_UNION", 1)):
        assert "#define %s %d" % (name, val) in hdr
    assert _lib.BTW_NMAX == 2048
    build.build()
    lib = _lib.load()
    out, Y = np.zeros((1, 4)), np.zeros((1, 1, 4, 4), np.uint8)
    assert lib.vmr_sample_betweenness(None, 1, 2, 1, 0, 1, out.ctypes.data, *[None] * 5) == _lib.VMR_EINVAL
    assert lib.vmr_network_betweenness(None, Y.ctypes.data, 1, 0, out.ctypes.data) == _lib.VMR_EINVAL


def _counts():
    """S = 4, L = 2, N = 4."""
    return {"node_sum": np.array([[4.0, 8.0, 0.0, 0.0], [2.0, 2.0, 1.0, 0.0]]),
            "node_sumsq": np.array([[6.0, 16.0 - 1e-13, 0.0, 0.0], [1.0, 3.0, 0.25, 0.0]]),
            "node_rank_sum": np.array([[4, 0, 8, 8], [0, 2, 8, 12]]), "node_top": np.array([[2, 4, 0, 0], [4, 4, 0, 0]]),
            "total": np.arange(8.0).reshape(4, 2), "max": np.ones((4, 2))}


def test_betweenness_stats():
    from vimure_amd.betweenness import BTW_KEYS as keys, BetweennessStats
    assert keys == BTW_KEYS
    inf = np.array([[3.0, 6.0, 0.0, 0.0], [0.0, 0.0, 1.5, 0.0]])
    r = BetweennessStats(4, _counts(), direction="directed", top_k=2, inferred=inf, seed=9, n_trials=2)
    assert (r.S, r.L, r.N, r.top_k, r.direction, r.seed, r.n_trials) == (4, 2, 4, 2, "directed", 9, 2)
    assert r.values is None
    assert np.array_equal(r.mean, [[1.0, 2.0, 0.0, 0.0], [0.5, 0.5, 0.25, 0.0]])
    assert np.array_equal(r.sd[0], [np.sqrt(0.5), 0.0, 0.0, 0.0])               # 4 - 1e-13 / 4 - 4 < 0: clipped, not NaN
    assert np.array_equal(r.sd[1], [0.0, np.sqrt(0.5), 0.0, 0.0])
    assert np.array_equal(r.expected_rank, [[1.0, 0.0, 2.0, 2.0], [0.0, 0.5, 2.0, 3.0]])
    assert np.array_equal(r.top_prob, [[0.5, 1.0, 0.0, 0.0], [1.0, 1.0, 0.0, 0.0]])
    assert np.array_equal(r.inferred, inf)
    # (N - 1)(N - 2) = 6 ordered pairs for directed, 3 unordered for union
    assert r.scale == 6.0
    n = r.normalized()
    assert np.array_equal(n["mean"], r.mean / 6.0) and np.array_equal(n["sd"], r.sd / 6.0) and np.array_equal(n["inferred"], inf / 6.0)
    u = BetweennessStats(4, _counts(), direction="union")
    assert u.scale == 3.0 and u.inferred is None and u.normalized()["inferred"] is None
    assert np.array_equal(u.normalized()["mean"][0], [1.0 / 3.0, 2.0 / 3.0, 0.0, 0.0])
    assert r.top(2, layer=0).tolist() == [1, 0] and r.top(3, layer=0).tolist() == [1, 0, 2]
    assert r.top(1, layer=1).tolist() == [0]                                    # equal top_prob and mean: the smaller index
    fr = r.frame(node_names=["a", "b", "c", "d"])
    assert list(fr.columns) == ["layer", "node", "name", "mean", "sd", "expected_rank", "top_prob", "inferred"]
    assert len(fr) == 8 and fr.name.tolist() == ["a", "b", "c", "d"] * 2 and fr.layer.tolist() == [0] * 4 + [1] * 4
    assert list(u.frame().columns) == ["layer", "node", "mean", "sd", "expected_rank", "top_prob"]
    with pytest.raises(ValueError, match="node_names"):
        r.frame(node_names=["a"])
    sm = r.summary()
    assert len(sm) == 4 and list(sm.columns) == ["layer", "statistic", "mean", "std", "q0.025", "q0.5", "q0.975"]
    assert sm[(sm.layer == 1) & (sm.statistic == "total")]["mean"].iloc[0] == 4.0
    assert BetweennessStats(4, dict(_counts(), values=np.zeros((4, 2, 4)))).values.shape == (4, 2, 4)


def test_argument_error_class():
    from vimure_amd.engine import BetweennessArgumentError, EngineError
    assert issubclass(BetweennessArgumentError, EngineError) and issubclass(BetweennessArgumentError, ValueError)
