"""Host: the restatement of the cut-point contract (tests/cutpoints_util.py) held to networkx on random graphs in both modes and to
the closed forms of the designed graphs; its reductions; `cutpoints.CutpointStats` from a hand-made dict.  No device."""
import numpy as np
import pytest

from tests.cutpoints_util import (CUT_KEYS, CUT_VALUES, MODES, SUMMARY, all_designed, connected_pairs, cut_values, cutpoints_np,
                                  designed_closed_forms, graph, random_digraph, ranks, reduce_values, tree_sizes)
from vimure_amd.cutpoints import CUT_KEYS as LIB_KEYS, CutpointStats


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,seed", [(65, 5), (129, 2), (300, 3)])
def test_restatement_against_networkx(N, seed, mode):
    nx = pytest.importorskip("networkx")
    # union: 1.5 / N per ordered pair; mutual: sqrt(2 / N), so that the reciprocated network has about 2 ties per node
    Y = random_digraph(N, 1.5 / N if mode == "union" else np.sqrt(2.0 / N), seed)
    assert Y.diagonal().any()
    D = nx.from_numpy_array((Y > 0).astype(np.int8), create_using=nx.DiGraph)
    D.remove_edges_from(list(nx.selfloop_edges(D)))
    if mode == "union":
        G = D.to_undirected()
    else:
        G = nx.Graph()
        G.add_nodes_from(range(N))
        G.add_edges_from((u, v) for u, v in D.edges() if D.has_edge(v, u))
    Gm = graph(Y, mode)
    assert np.array_equal(Gm, nx.to_numpy_array(G, nodelist=range(N)) > 0)
    pairs, branches, bridges = cut_values(Gm)
    cut = set(np.nonzero(branches >= 2)[0].tolist())
    assert cut == set(nx.articulation_points(G)) and len(cut) >= 4
    deg = np.zeros(N, np.int64)
    for u, v in nx.bridges(G):
        deg[u] += 1
        deg[v] += 1
    assert np.array_equal(bridges, deg) and deg.any()
    comps = [len(c) for c in nx.connected_components(G)]
    assert connected_pairs(Gm) == sum(c * (c - 1) // 2 for c in comps)
    assert (branches[np.asarray([G.degree(v) for v in range(N)]) == 0] == 0).all()
    # pairs_cut a second way: the connected pairs among the OTHER nodes before and after the removal
    comp_of = {}
    for c in nx.connected_components(G):
        for v in c:
            comp_of[v] = len(c)
    for v in range(N):
        H = G.copy()
        H.remove_node(v)
        after = sum(len(c) * (len(c) - 1) // 2 for c in nx.connected_components(H))
        n = comp_of[v]
        before = sum(c * (c - 1) // 2 for c in comps) - (n - 1)      # without the pairs that hold v
        assert pairs[v] == before - after, v
        assert branches[v] == nx.number_connected_components(H) - (len(comps) - 1), v
    assert (branches >= 3).any()


@pytest.mark.parametrize("mode", MODES)
def test_restatement_against_closed_forms(mode):
    Y = all_designed()
    closed = designed_closed_forms(mode)
    got = cutpoints_np([Y], mode, top_k=3)
    for k in CUT_VALUES + SUMMARY:
        assert np.array_equal(got[k][0], closed[k]), (mode, k)
    if mode == "union":
        assert closed["branches"][4, 64] == 128 and closed["pairs_cut"][4, 64] == 8128 and closed["bridges"][4, 64] == 128
        assert closed["branches"][7].max() == 3 and tree_sizes()[0] == 129
        assert closed["branches"][6, 128] == 2 and closed["bridges"][6, 128] == 0
    else:
        for l in (0, 1, 2, 3, 7):
            assert not any(closed[k][l].any() for k in CUT_VALUES) and not any(closed[k][l] for k in SUMMARY)
    # sum_v bridges[v] = 2 x bridges, and the ranks: all non-cut nodes share the rank "number of cut points with pairs_cut > 0"
    assert np.array_equal(got["bridges"][0].astype(np.int64).sum(axis=1), 2 * closed["n_bridges"])
    assert np.array_equal(got["node_top"][5] > 0, np.isin(np.arange(129), [63, 64, 128]))
    assert np.array_equal(got["node_top"][1], np.ones(129, np.int64))           # no cut point: every node has rank 0


def test_reduce_values_and_ranks():
    assert np.array_equal(ranks(np.array([[5, 0, 5, 7, 0]])), [[1, 3, 1, 0, 3]])
    p = np.array([[[0, 6, 2, 0]], [[3, 3, 0, 0]], [[0, 0, 0, 0]]], np.uint32)
    b = np.array([[[1, 3, 2, 0]], [[2, 2, 1, 1]], [[1, 1, 1, 1]]], np.uint16)
    g = np.array([[[1, 2, 1, 0]], [[1, 1, 0, 0]], [[0, 0, 0, 0]]], np.uint16)
    r = reduce_values(p, b, g, top_k=2)
    assert np.array_equal(r["node_sum"], [[3.0, 9.0, 2.0, 0.0]]) and np.array_equal(r["node_sumsq"], [[9.0, 45.0, 4.0, 0.0]])
    assert r["node_sum"].dtype == np.float64 and r["node_rank_sum"].dtype == np.int64
    assert np.array_equal(r["node_rank_sum"], [[2 + 0 + 0, 0 + 0 + 0, 1 + 2 + 0, 2 + 2 + 0]])
    assert np.array_equal(r["node_top"], [[2, 3, 2, 1]])          # the sample without a cut point counts every node
    assert np.array_equal(r["node_cut"], [[1, 2, 1, 0]]) and np.array_equal(r["node_branch_sum"], [[4, 6, 4, 2]])
    assert np.array_equal(r["node_bridge_sum"], [[2, 3, 1, 0]])
    assert np.array_equal(r["n_cut"], [[2], [2], [0]]) and np.array_equal(r["n_bridges"], [[2], [1], [0]])
    assert np.array_equal(r["max_pairs_cut"], [[6], [3], [0]])
    assert tuple(LIB_KEYS) == tuple(CUT_KEYS)


def test_cutpoint_stats_from_a_dict():
    Y = all_designed()[[0, 5]]
    S = 4
    counts = cutpoints_np([Y] * S, "union", top_k=2)
    inferred = {k: counts[k][0] for k in CUT_VALUES}
    res = CutpointStats(129, counts, mode="union", top_k=2, inferred=inferred, seed=3)
    assert (res.S, res.L, res.N) == (S, 2, 129)
    assert np.array_equal(res.cut_prob[0], np.r_[0.0, np.ones(127), 0.0]) and np.array_equal(res.cut_prob[1] > 0, np.isin(np.arange(129), [63, 64, 128]))
    assert np.array_equal(res.mean[0], np.arange(129) * (128 - np.arange(129))) and not res.sd.any()
    assert np.array_equal(res.mean_branches[1, [0, 63, 128]], [1, 2, 2]) and np.array_equal(res.mean_bridges[1, [0, 63, 128]], [0, 1, 2])
    assert res.expected_rank[0, 64] == 0 and res.top_prob[0, 64] == 1 and res.top_prob[0, 0] == 0
    assert np.array_equal(res.n_cut, np.tile([127, 3], (S, 1))) and np.array_equal(res.n_bridges, np.tile([128, 2], (S, 1)))
    assert np.array_equal(res.connected_pairs, np.full((S, 2), 8256)) and np.array_equal(res.max_pairs_cut, np.full((S, 2), 4096))
    f = res.fragmentation()
    assert f.shape == (S, 2, 129) and f[0, 1, 128] == 4096 / 8256 and f.max() < 1 and f.min() == 0
    q = res.quantiles((0.5,))
    assert sorted(q) == sorted(SUMMARY) and q["n_cut"].shape == (1, 2) and np.array_equal(q["n_cut"][0], [127, 3])
    assert res.top(1, layer=1)[0] == 128 and res.top(3, layer=1).tolist() == [128, 63, 64] and res.top(1, layer=0)[0] == 64
    assert np.array_equal(res.key_players(), res.cut_prob >= 0.5) and res.key_players(0.5).sum() == 130
    assert np.array_equal(res.inferred["pairs_cut"], counts["pairs_cut"][0]) and res.inferred["branches"].dtype == np.int64
    fr = res.frame()
    assert len(fr) == 2 * 129 and {"cut_prob", "mean", "mean_branches", "mean_bridges", "inferred_pairs_cut"} <= set(fr.columns)
    assert len(res.summary()) == 4 * 2
    plain = CutpointStats(129, {k: counts[k] for k in CUT_KEYS}, top_k=2)
    assert plain.pairs_cut is None and plain.inferred is None and "inferred_pairs_cut" not in plain.frame().columns
    with pytest.raises(ValueError, match="values"):
        plain.fragmentation()
    empty = dict(counts, connected_pairs=np.zeros((S, 2), np.int64))
    assert not CutpointStats(129, empty, top_k=2).fragmentation().any()
