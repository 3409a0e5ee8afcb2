"""CPU: the host pieces of the posterior centrality -- the NumPy restatement the GPU tests use (tests/centrality_util.py) against
closed forms on designed graphs and against a second restatement that sums in another order, `exact_ok`, the binding's constants,
what `CentralityStats` derives from the sums, and the rule for q when none is given."""
import numpy as np
import pytest

from tests.centrality_util import (CENT_KEYS, DIRECTIONS, adjacency, centrality_np, designed_closed_forms, exact_ok, geometric,
                                   mean_centrality_np, ranks_np, reduce_values, walk_np, walk_other_order)
from tests.connectivity_util import designed_graphs


def test_restatement_on_designed_graphs():
    Y = designed_graphs()
    q, T = 0.5, 16
    got = centrality_np([Y, Y], q, T, "out", top_k=3)
    want = designed_closed_forms(q, T)
    assert got["values"].shape == (2, 4, 129) and np.array_equal(got["values"][0], want) and np.array_equal(got["values"][1], want)
    assert want[0, 0] == 1.0 - 2.0 ** -16 and want[0, 127] == 0.5 and want[0, 128] == 0.0 and want[2, 128] == 0.0
    for l in range(4):
        assert np.array_equal(exact_ok(adjacency(Y[l], "out"), q, T), want[l])
    # the path: the 113 nodes followed by at least T others tie at rank 0, then one node per rank
    assert np.array_equal(ranks_np(want[0]), np.r_[np.zeros(113, np.int64), np.arange(113, 129)])
    assert np.array_equal(got["node_top"][0], 2 * (np.arange(129) < 113)) and np.array_equal(got["node_rank_sum"][1], np.zeros(129))
    assert np.array_equal(got["node_top"][3], np.full(129, 2))                 # the empty graph: every node ties at rank 0
    assert np.array_equal(got["node_rank_sum"][2], np.r_[np.zeros(128, np.int64), 2 * 128])
    assert np.array_equal(got["total"][0], want.sum(axis=1)) and np.array_equal(got["max"][0], [want[0, 0], want[1, 0], want[1, 0], 0.0])
    assert np.array_equal(got["node_sum"], 2 * want) and np.array_equal(got["node_sumsq"], 2 * (want * want))
    # IN on the path is the path turned round; UNION of the cycle has degree 2
    assert np.array_equal(centrality_np([Y], q, T, "in")["values"][0, 0], want[0, ::-1])
    assert np.array_equal(centrality_np([Y], 0.25, 5, "union")["values"][0, 1], np.full(129, geometric(0.5, 5)))
    deg = np.stack([adjacency(Y[l], "out").sum(axis=1) for l in range(4)])      # T = 1, q = 1: the out-degree, self-loops left out
    assert np.array_equal(centrality_np([Y], 1.0, 1, "out")["values"][0], deg) and deg[2, 128] == 0


@pytest.mark.parametrize("N, deg", [(65, 1.5), (129, 3.0), (300, 6.0)])
def test_restatement_is_exact_in_any_order(N, deg):
    """q = 1/2 on random digraphs: `exact_ok` holds, and three summation orders agree bit for bit."""
    g = np.random.RandomState(N)
    Y = (g.rand(N, N) < deg / N).astype(np.uint8)
    Y[np.arange(N), np.arange(N)] = 1                  # self-loops: they change nothing
    for d in DIRECTIONS:
        T = 8 if d == "union" else 16                   # (twice the degree: 12^16 would not fit)
        M = adjacency(Y, d)
        assert not M.diagonal().any()
        exact = exact_ok(M, 0.5, T)
        a, b = walk_np(M, 0.5, T), walk_other_order(M, 0.5, T)
        assert np.array_equal(a, exact) and np.array_equal(b, exact), d
    T = 16
    c = walk_np(adjacency(Y, "out"), 0.5, T)
    if deg == 1.5:                                      # tied ranks are exercised
        assert 8 <= np.unique(c).size < N
    with pytest.raises(AssertionError):
        exact_ok(adjacency(Y, "out"), 0.3, T)           # not a power of two
    with pytest.raises(AssertionError):
        exact_ok(np.ones((64, 64)) - np.eye(64), 0.5, 16)   # 63^16 does not fit


def test_restatement_general_q_two_orders():
    g = np.random.RandomState(3)
    N, T, q = 80, 64, 0.3
    Y = (g.rand(N, N) < 3.0 / N).astype(np.uint8)
    for d in DIRECTIONS:
        M = adjacency(Y, d)
        a, b = walk_np(M, q, T), walk_other_order(M, q, T)
        assert (a > 0).any() and np.all(np.abs(a - b) <= 2 * T * (N + 1) * 2.0 ** -53 * np.abs(b))


def test_reductions_and_ranks():
    v = np.array([[[3.0, 1.0, 3.0, 0.0]], [[0.5, 2.0, 0.25, 2.0]]])          # S = 2, L = 1, N = 4
    r = reduce_values(v, top_k=2)
    assert sorted(r) == sorted(CENT_KEYS + ("values",))
    assert np.array_equal(ranks_np(v[0, 0]), [0, 2, 0, 3]) and np.array_equal(ranks_np(v[1, 0]), [2, 0, 3, 0])
    assert np.array_equal(r["node_rank_sum"], [[2, 2, 3, 3]]) and np.array_equal(r["node_top"], [[1, 1, 1, 1]])
    assert np.array_equal(r["node_sum"], [[3.5, 3.0, 3.25, 2.0]]) and np.array_equal(r["node_sumsq"], [[9.25, 5.0, 9.0625, 4.0]])
    assert np.array_equal(r["total"], [[7.0], [4.75]]) and np.array_equal(r["max"], [[3.0], [2.0]])
    assert r["node_rank_sum"].dtype == np.int64 and r["node_top"].dtype == np.int64


def test_mean_restatement():
    """One-hot rho: the mean network is the graph; T <= 2 on a random rho: the mean of c over all graphs of 3 nodes."""
    Y = designed_graphs()
    rho = np.stack([1.0 - Y, Y], axis=-1).astype(np.float64)
    assert np.array_equal(mean_centrality_np(rho, 0.5, 16, "out"), designed_closed_forms(0.5, 16))
    g = np.random.RandomState(8)
    N = 3
    rho = g.rand(1, N, N, 3)
    rho /= rho.sum(-1, keepdims=True)
    P = rho[0, :, :, 1] + rho[0, :, :, 2]
    off = [(i, j) for i in range(N) for j in range(N) if i != j]
    for d in ("out", "in"):
        want = np.zeros(N)
        for bits in range(2 ** len(off)):                # every graph without self-loops, weighted by its probability
            A, w = np.zeros((N, N)), 1.0
            for b, (i, j) in enumerate(off):
                on = (bits >> b) & 1
                A[i, j] = on
                w *= P[i, j] if on else 1.0 - P[i, j]
            want += w * walk_np(adjacency(A, d), 0.5, 2)
        assert np.allclose(mean_centrality_np(rho, 0.5, 2, d)[0], want, rtol=1e-13, atol=0)
    u = mean_centrality_np(rho, 1.0, 1, "union")[0]
    assert np.allclose(u[0], 2 - (1 - P[0, 1]) * (1 - P[1, 0]) - (1 - P[0, 2]) * (1 - P[2, 0]), rtol=1e-14)


def test_binding_constants_and_null_handle():
    from vimure_amd import _lib, build
    assert "vmr_sample_centrality" in _lib.SIGNATURES and "vmr_mean_centrality" in _lib.SIGNATURES
    assert _lib.CENT_DIRECTIONS == DIRECTIONS
    hdr = open(build.HEADERS[-1]).read()
    for name, val in (("VMR_CENT_NMAX", _lib.CENT_NMAX), ("VMR_CENT_TMAX", _lib.CENT_TMAX), ("VMR_CENT_OUT", 0), ("VMR_CENT_IN", 1),
                      ("VMR_CENT_UNION", 2)):
        assert "#define %s %d" % (name, val) in hdr
    assert (_lib.CENT_NMAX, _lib.CENT_TMAX) == (2048, 64)
    build.build()
    lib = _lib.load()
    q, out = np.full(1, 0.5), np.zeros((1, 4))
    assert lib.vmr_sample_centrality(None, 1, 2, 1, q.ctypes.data, 2, 0, 1, out.ctypes.data, *[None] * 5) == _lib.VMR_EINVAL
    assert lib.vmr_mean_centrality(None, q.ctypes.data, 2, 0, out.ctypes.data) == _lib.VMR_EINVAL


def _counts():
    """S = 4, L = 2, N = 3."""
    return {"node_sum": np.array([[4.0, 8.0, 0.0], [2.0, 2.0, 1.0]]), "node_sumsq": np.array([[6.0, 16.0 - 1e-13, 0.0], [1.0, 3.0, 0.25]]),
            "node_rank_sum": np.array([[4, 0, 8], [0, 2, 8]]), "node_top": np.array([[2, 4, 0], [4, 4, 0]]),
            "total": np.arange(8.0).reshape(4, 2), "max": np.ones((4, 2))}


def test_centrality_stats():
    from vimure_amd.centrality import CentralityStats
    r = CentralityStats(3, _counts(), [0.5, 0.25], 3, direction="in", top_k=2, plug_in=np.ones((2, 3)), seed=9, n_trials=2)
    assert (r.S, r.L, r.N, r.T, r.top_k, r.direction, r.seed, r.n_trials) == (4, 2, 3, 3, 2, "in", 9, 2)
    assert np.array_equal(r.q, [0.5, 0.25]) and r.values is None
    assert np.array_equal(r.mean, [[1.0, 2.0, 0.0], [0.5, 0.5, 0.25]])
    assert np.array_equal(r.sd[0], [np.sqrt(0.5), 0.0, 0.0])                    # 4 - 1e-13 / 4 - 4 < 0: clipped, not NaN
    assert np.array_equal(r.sd[1], [0.0, np.sqrt(0.5), 0.0])
    assert np.array_equal(r.expected_rank, [[1.0, 0.0, 2.0], [0.0, 0.5, 2.0]])
    assert np.array_equal(r.top_prob, [[0.5, 1.0, 0.0], [1.0, 1.0, 0.0]])
    assert r.top(2, layer=0).tolist() == [1, 0] and r.top(3, layer=0).tolist() == [1, 0, 2]
    assert r.top(1, layer=1).tolist() == [0]                                    # equal top_prob and mean: the smaller index
    c = _counts()
    c["node_sum"][1, 1] = 3.0
    assert CentralityStats(3, c, 0.5, 3).top(2, layer=1).tolist() == [1, 0]     # equal top_prob: the higher mean first
    fr = r.frame(node_names=["a", "b", "c"])
    assert list(fr.columns) == ["layer", "node", "name", "mean", "sd", "expected_rank", "top_prob", "plug_in"]
    assert len(fr) == 6 and fr.name.tolist() == ["a", "b", "c"] * 2 and fr.layer.tolist() == [0, 0, 0, 1, 1, 1]
    assert fr["top_prob"].tolist() == [0.5, 1.0, 0.0, 1.0, 1.0, 0.0]
    assert list(CentralityStats(3, _counts(), 0.5, 3).frame().columns) == ["layer", "node", "mean", "sd", "expected_rank", "top_prob"]
    with pytest.raises(ValueError, match="node_names"):
        r.frame(node_names=["a"])
    sm = r.summary()
    assert len(sm) == 4 and list(sm.columns) == ["layer", "statistic", "mean", "std", "q0.025", "q0.5", "q0.975"]
    assert sm[(sm.layer == 1) & (sm.statistic == "total")]["mean"].iloc[0] == 4.0
    v = np.zeros((4, 2, 3))
    assert CentralityStats(3, dict(_counts(), values=v), 0.5, 3).values.shape == (4, 2, 3)


def test_default_q_rule():
    """min(1, N / expected edges) per layer, from a hand-made `expected_stats`."""
    from vimure_amd.centrality import default_q
    es = {"edges": np.array([400.0, 50.0, 100.0, 0.0])}
    assert np.array_equal(default_q(100, es["edges"]), [0.25, 1.0, 1.0, 1.0])


def test_argument_error_class():
    from vimure_amd.engine import CentralityArgumentError, EngineError
    assert issubclass(CentralityArgumentError, EngineError) and issubclass(CentralityArgumentError, ValueError)
