"""Host: the three results that score every node over the posterior samples (`CentralityStats`, `BetweennessStats`, `CoreStats`)
built from a small counts dict -- S = 3, L = 2, N = 5 -- and held to numbers written out by hand: the attributes, the columns of
`frame()` in their order with the optional ones, the rows and columns of `summary()`, and `top()` on a tie (equal probability:
the higher mean first, then the smaller index)."""
import numpy as np
import pytest

from vimure_amd.betweenness import BetweennessStats
from vimure_amd.centrality import CentralityStats
from vimure_amd.cores import CoreStats

N = 5
FRAME = ["layer", "node", "mean", "sd", "expected_rank", "top_prob"]
SUMMARY = ["layer", "statistic", "mean", "std", "q0.025", "q0.5", "q0.975"]


def _counts():
    """The per-node sums of three samples.  Layer 0: nodes 0, 1 and 3 are always among the top, node 1 with the highest mean,
    nodes 0 and 3 with the same; node 0's sum of squares is below its squared mean times S (the variance is clipped)."""
    return {"node_sum": np.array([[6.0, 9.0, 3.0, 6.0, 0.0], [3.0, 3.0, 6.0, 0.0, 12.0]]),
            "node_sumsq": np.array([[11.0, 39.0, 3.0, 15.0, 0.0], [3.0, 6.0, 12.0, 0.0, 75.0]]),
            "node_rank_sum": np.array([[3, 0, 9, 6, 12], [6, 6, 3, 12, 0]], np.int64),
            "node_top": np.array([[3, 3, 0, 3, 0], [0, 0, 3, 0, 3]], np.int64)}


def _check_shared(res, top_k, seed, n_trials):
    assert (res.N, res.S, res.L, res.top_k, res.seed, res.n_trials) == (5, 3, 2, top_k, seed, n_trials)
    assert res.values is None
    assert res.node_sum.dtype == np.float64 and res.node_sumsq.dtype == np.float64
    assert res.node_rank_sum.dtype == np.int64 and res.node_top.dtype == np.int64
    assert res.mean.tolist() == [[2.0, 3.0, 1.0, 2.0, 0.0], [1.0, 1.0, 2.0, 0.0, 4.0]]
    assert res.sd.tolist() == [[0.0, 2.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.0, 0.0, 3.0]]
    assert res.expected_rank.tolist() == [[1.0, 0.0, 3.0, 2.0, 4.0], [2.0, 2.0, 1.0, 4.0, 0.0]]
    assert res.top_prob.tolist() == [[1.0, 1.0, 0.0, 1.0, 0.0], [0.0, 0.0, 1.0, 0.0, 1.0]]


def _check_frame(df, columns, names=None):
    assert list(df.columns) == columns and len(df) == 10
    assert df["layer"].tolist() == [0] * 5 + [1] * 5 and df["node"].tolist() == [0, 1, 2, 3, 4] * 2
    assert df["mean"].tolist() == [2.0, 3.0, 1.0, 2.0, 0.0, 1.0, 1.0, 2.0, 0.0, 4.0]
    assert df["top_prob"].tolist() == [1.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0]
    if names is not None:
        assert df["name"].tolist() == names * 2


def _walk_counts():
    c = _counts()
    c["total"] = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])
    c["max"] = np.array([[1.0, 1.0], [2.0, 2.0], [3.0, 3.0]])
    return c


def _check_walk_summary(res):
    sm = res.summary()
    assert list(sm.columns) == SUMMARY
    assert sm["layer"].tolist() == [0, 0, 1, 1] and sm["statistic"].tolist() == ["total", "max", "total", "max"]
    assert sm["mean"].tolist() == [3.0, 2.0, 4.0, 2.0] and sm["q0.5"].tolist() == [3.0, 2.0, 4.0, 2.0]
    assert sm["std"].tolist() == pytest.approx([1.632993161855452, 0.816496580927726, 1.632993161855452, 0.816496580927726], rel=1e-15)
    assert sm["q0.025"].tolist() == pytest.approx([1.1, 1.05, 2.1, 1.05], rel=1e-12)
    assert list(res.summary(q=(0.5,)).columns) == ["layer", "statistic", "mean", "std", "q0.5"]
    assert list(res.statistics()) == ["total", "max"] and res.statistics()["total"] is res.total


def test_centrality_stats():
    res = CentralityStats(N, _walk_counts(), q=0.25, T=3, direction="in", top_k=2, seed=7, n_trials=2)
    _check_shared(res, 2, 7, 2)
    assert res.q.tolist() == [0.25] and (res.T, res.direction, res.plug_in) == (3, "in", None)
    assert res.total.tolist() == [[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]] and res.max.tolist() == [[1.0, 1.0], [2.0, 2.0], [3.0, 3.0]]
    assert res.top(5, 0).tolist() == [1, 0, 3, 2, 4] and res.top(5, 1).tolist() == [4, 2, 0, 1, 3]
    assert res.top(3).tolist() == [1, 0, 3] and res.top(0).tolist() == [] and res.top(9).tolist() == [1, 0, 3, 2, 4]
    _check_frame(res.frame(), FRAME)
    names = ["a", "b", "c", "d", "e"]
    _check_frame(res.frame(node_names=names), ["layer", "node", "name"] + FRAME[2:], names)
    with pytest.raises(ValueError, match="node_names has 4 entries"):
        res.frame(node_names=names[:4])
    _check_walk_summary(res)
    vals = np.arange(30.0).reshape(3, 2, 5)
    res = CentralityStats(N, dict(_walk_counts(), values=vals), q=[0.5, 1.0], T=1, plug_in=np.arange(10).reshape(2, 5))
    assert res.values is vals and res.q.tolist() == [0.5, 1.0] and (res.direction, res.top_k, res.seed, res.n_trials) == ("out", 10, None, 1)
    df = res.frame()
    _check_frame(df, FRAME + ["plug_in"])
    assert df["plug_in"].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0] and res.plug_in.dtype == np.float64


def test_betweenness_stats():
    res = BetweennessStats(N, _walk_counts(), direction="union", top_k=2, seed=7, n_trials=2)
    _check_shared(res, 2, 7, 2)
    assert (res.direction, res.inferred) == ("union", None)
    assert res.top(5, 0).tolist() == [1, 0, 3, 2, 4] and res.top(2, 1).tolist() == [4, 2]
    _check_frame(res.frame(), FRAME)
    _check_walk_summary(res)
    assert res.scale == 6.0
    nz = res.normalized()
    assert sorted(nz) == ["inferred", "mean", "sd"] and nz["inferred"] is None
    assert nz["mean"][1].tolist() == [1.0 / 6.0, 1.0 / 6.0, 2.0 / 6.0, 0.0, 4.0 / 6.0] and nz["sd"][0].tolist() == [0.0, 2.0 / 6.0, 0.0, 1.0 / 6.0, 0.0]
    res = BetweennessStats(N, _walk_counts(), inferred=np.full((2, 5), 6))
    assert (res.direction, res.top_k, res.seed, res.n_trials, res.scale) == ("directed", 10, None, 1, 12.0)
    df = res.frame(node_names=list("abcde"))
    _check_frame(df, ["layer", "node", "name"] + FRAME[2:] + ["inferred"], list("abcde"))
    assert df["inferred"].tolist() == [6.0] * 10 and res.normalized()["inferred"].tolist() == [[0.5] * 5] * 2


def test_core_stats():
    c = _counts()
    c["node_main"] = np.array([[3, 3, 0, 0, 3], [0, 3, 0, 0, 3]], np.int64)
    c["node_atleast"] = np.array([[3, 3, 0, 3, 0], [0, 0, 3, 0, 3]], np.int64)
    c["degeneracy"] = np.array([[1, 2], [3, 4], [5, 6]], np.int64)
    c["main_core_size"] = np.array([[1, 1], [2, 2], [3, 3]], np.int64)
    c["core_sum"] = np.array([[9, 9], [9, 9], [9, 9]], np.int64)
    c["kcore_size"] = np.array([[2, 0], [2, 0], [2, 4]], np.int64)
    res = CoreStats(N, c, mode="total", k_min=2, top_k=2, seed=7, n_trials=2)
    _check_shared(res, 2, 7, 2)
    assert (res.mode, res.k_min, res.inferred) == ("total", 2, None)
    assert res.node_main.dtype == np.int64 and res.degeneracy.dtype == np.int64
    assert res.main_core_prob.tolist() == [[1.0, 1.0, 0.0, 0.0, 1.0], [0.0, 1.0, 0.0, 0.0, 1.0]]
    assert res.kcore_prob.tolist() == [[1.0, 1.0, 0.0, 1.0, 0.0], [0.0, 0.0, 1.0, 0.0, 1.0]]
    # by main_core_prob, not by top_prob: nodes 0, 1, 4 tie at 1 (means 2, 3, 0), then node 3 (mean 2) before node 2 (mean 1)
    assert res.top(5, 0).tolist() == [1, 0, 4, 3, 2] and res.top(5, 1).tolist() == [4, 1, 2, 0, 3] and res.top(2).tolist() == [1, 0]
    assert res.core_members().tolist() == [[True, True, False, True, False], [False, False, True, False, True]]
    cols = FRAME + ["main_core_prob", "kcore_prob"]
    df = res.frame()
    _check_frame(df, cols)
    assert df["main_core_prob"].tolist() == [1.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 1.0]
    sm = res.summary()
    assert list(sm.columns) == SUMMARY and sm["layer"].tolist() == [0] * 4 + [1] * 4
    assert sm["statistic"].tolist() == ["degeneracy", "main_core_size", "kcore_size", "core_sum"] * 2
    assert sm["mean"].tolist() == [3.0, 2.0, 2.0, 9.0, 4.0, 2.0, 4.0 / 3.0, 9.0]
    assert sm["q0.5"].tolist() == [3.0, 2.0, 2.0, 9.0, 4.0, 2.0, 0.0, 9.0]
    assert list(res.statistics()) == ["degeneracy", "main_core_size", "kcore_size", "core_sum"]
    res = CoreStats(N, c, inferred=np.arange(10, dtype=np.uint16).reshape(2, 5))
    assert (res.mode, res.k_min, res.top_k, res.seed, res.n_trials) == ("union", 0, 10, None, 1) and res.inferred.dtype == np.int64
    df = res.frame(node_names=list("abcde"))
    _check_frame(df, ["layer", "node", "name"] + cols[2:] + ["inferred"], list("abcde"))
    assert df["inferred"].tolist() == list(range(10))
