"""CPU: the host pieces of the posterior k-cores -- the NumPy restatement of the peeling the GPU tests use (tests/cores_util.py)
against the definition applied literally, against networkx and against closed forms, the binding's constants, and what `CoreStats`
derives from the sums."""
import numpy as np
import pytest

from tests.cores_util import (CORE_KEYS, MODES, adjacency, clique, core_definition, core_peel, cores_np, cycle, mixed_design,
                              mixed_design_cores, out_star, path, random_planted, reduce_values)


def _random_graphs(n_graphs, seed):
    g = np.random.RandomState(seed)
    for _ in range(n_graphs):
        N = int(g.randint(2, 41))
        p = float(g.choice([0.02, 0.05, 0.1, 0.2, 0.4, 0.8]))
        Y = (g.rand(N, N) < p).astype(np.uint8)
        Y[np.arange(N), np.arange(N)] = g.rand(N) < 0.5      # self-loops that must be ignored
        yield Y


def test_peeling_equals_the_definition():
    """300 random digraphs of up to 40 nodes at densities 0.02 .. 0.8, all four modes; the rounds never exceed N + 1 jumps."""
    deep = 0
    for Y in _random_graphs(300, 1):
        A = adjacency(Y)
        for mode in MODES:
            core, rounds = core_peel(A, mode)
            assert np.array_equal(core, core_definition(A, mode)), mode
            assert rounds <= 2 * A.shape[0]
            deep = max(deep, int(core.max()))
    assert deep >= 20                                          # dense graphs were among them


def test_peeling_equals_networkx():
    nx = pytest.importorskip("networkx")
    for Y in _random_graphs(300, 2):
        A = adjacency(Y)
        N = A.shape[0]
        D = nx.from_numpy_array(A.astype(np.uint8), create_using=nx.DiGraph)     # (the self-loops are gone: networkx raises on them)
        want = nx.core_number(D)
        assert np.array_equal(core_peel(A, "total")[0], [want[v] for v in range(N)])
        want = nx.core_number(D.to_undirected())
        assert np.array_equal(core_peel(A, "union")[0], [want[v] for v in range(N)])


def _cores(Y):
    return {m: core_peel(adjacency(Y), m)[0] for m in MODES}


def test_closed_forms():
    """Every design has diagonal entries set, which must be ignored."""
    n = 9
    c = _cores(clique(n))
    assert all(np.array_equal(c[m], np.full(n, n - 1)) for m in ("union", "in", "out")) and np.array_equal(c["total"], np.full(n, 2 * (n - 1)))
    for Y in (path(n), path(n, directed=False), out_star(n), out_star(n).T):
        assert np.array_equal(_cores(Y)["union"], np.ones(n))
    assert np.array_equal(_cores(cycle(n, directed=False))["union"], np.full(n, 2))
    assert np.array_equal(_cores(cycle(n, directed=False))["total"], np.full(n, 4))
    c = _cores(cycle(n))
    assert np.array_equal(c["in"], np.ones(n)) and np.array_equal(c["out"], np.ones(n)) and np.array_equal(c["total"], np.full(n, 2))
    assert np.array_equal(c["union"], np.full(n, 2))
    # out-star: the centre's out-neighbours have no out-tie themselves, so the centre's out-degree inside any 1-core is 0
    c = _cores(out_star(n))
    assert not c["out"].any() and not c["in"].any() and np.array_equal(c["total"], np.ones(n))
    c = _cores(np.eye(n, dtype=np.uint8))
    assert all(not c[m].any() for m in MODES)
    want = mixed_design_cores()
    got = _cores(mixed_design())
    for m in MODES:
        assert np.array_equal(got[m], want[m]), m
        assert np.array_equal(core_definition(adjacency(mixed_design(210)), m), mixed_design_cores(210)[m]), m


def test_round_counts():
    """A path of 300 nodes: one jump to k = 1, then two nodes per round.  N = 2000 with 5 ties per node: a few dozen rounds."""
    core, rounds = core_peel(adjacency(path(300)), "union")
    assert rounds == 151 and np.array_equal(core, np.ones(300))
    g = np.random.RandomState(0)
    A = adjacency((g.rand(2000, 2000) < 5.0 / 2000).astype(np.uint8))
    core, rounds = core_peel(A, "union")
    assert 5 <= core.max() <= 9 and 20 <= rounds <= 60 and (core == core.max()).sum() > 1000
    core, rounds = core_peel(A, "out")
    assert 1 <= core.max() <= 3 and rounds <= 60


def test_reductions_and_planted_clique():
    Y = random_planted(200, 3.0, 24, 5)
    got = cores_np([[Y]], "union", k_min=23, top_k=5)
    assert sorted(got) == sorted(CORE_KEYS + ("values",)) and got["values"].dtype == np.uint16
    assert got["degeneracy"][0, 0] == 23 and got["main_core_size"][0, 0] == 24 and got["kcore_size"][0, 0] == 24
    assert got["node_main"][0, 199] == 1 and got["node_atleast"].sum() == 24 and got["core_sum"][0, 0] == got["values"].sum()
    # a whole shell shares a rank: the 24 members have rank 0 and all of them count among the top 5
    assert got["node_top"].sum() == 24 and got["node_rank_sum"][0, 199] == 0
    v = np.array([[[3, 1, 3, 0]], [[2, 2, 0, 0]]], np.uint16)
    r = reduce_values(v, k_min=2, top_k=1)
    assert r["node_sum"].tolist() == [[5.0, 3.0, 3.0, 0.0]] and r["node_sumsq"].tolist() == [[13.0, 5.0, 9.0, 0.0]]
    assert r["node_rank_sum"].tolist() == [[0, 2, 2, 5]] and r["node_top"].tolist() == [[2, 1, 1, 0]]
    assert r["node_main"].tolist() == [[2, 1, 1, 0]] and r["node_atleast"].tolist() == [[2, 1, 1, 0]]
    assert r["degeneracy"].tolist() == [[3], [2]] and r["main_core_size"].tolist() == [[2], [2]]
    assert r["core_sum"].tolist() == [[7], [4]] and r["kcore_size"].tolist() == [[2], [2]]


def test_binding_constants_and_null_handle():
    from vimure_amd import _lib, build
    assert "vmr_sample_cores" in _lib.SIGNATURES and "vmr_network_cores" in _lib.SIGNATURES
    assert _lib.CORE_MODES == MODES
    hdr = open(build.HEADERS[-1]).read()
    for name, val in (("VMR_CORE_NMAX", _lib.CORE_NMAX), ("VMR_CORE_UNION", 0), ("VMR_CORE_TOTAL", 1), ("VMR_CORE_IN", 2), ("VMR_CORE_OUT", 3)):
        assert "#define %s %d" % (name, val) in hdr
    assert _lib.CORE_NMAX == 2048
    build.build()
    lib = _lib.load()
    out, vals, Y = np.zeros((1, 4)), np.zeros((1, 1, 4), np.uint16), np.zeros((1, 1, 4, 4), np.uint8)
    assert lib.vmr_sample_cores(None, 1, 2, 1, 0, 0, 1, out.ctypes.data, *[None] * 7) == _lib.VMR_EINVAL
    assert lib.vmr_network_cores(None, Y.ctypes.data, 1, 0, 0, vals.ctypes.data, None) == _lib.VMR_EINVAL


def _counts():
    """S = 4, L = 2, N = 4."""
    return {"node_sum": np.array([[4.0, 8.0, 0.0, 0.0], [2.0, 2.0, 1.0, 0.0]]),
            "node_sumsq": np.array([[6.0, 16.0 - 1e-13, 0.0, 0.0], [2.0, 4.0, 1.0, 0.0]]),
            "node_rank_sum": np.array([[4, 0, 8, 8], [0, 2, 8, 12]]), "node_top": np.array([[2, 4, 0, 0], [4, 4, 0, 0]]),
            "node_main": np.array([[2, 4, 0, 0], [4, 2, 1, 0]]), "node_atleast": np.array([[3, 4, 0, 0], [1, 2, 0, 0]]),
            "degeneracy": np.arange(8).reshape(4, 2), "main_core_size": np.ones((4, 2), np.int64),
            "core_sum": np.full((4, 2), 3), "kcore_size": np.array([[1, 2], [2, 2], [2, 0], [2, 1]])}


def test_core_stats():
    from vimure_amd.cores import CORE_KEYS as keys, CoreStats
    assert keys == CORE_KEYS
    inf = np.array([[1, 2, 0, 0], [1, 1, 0, 0]])
    r = CoreStats(4, _counts(), mode="union", k_min=1, top_k=2, inferred=inf, seed=9, n_trials=2)
    assert (r.S, r.L, r.N, r.top_k, r.k_min, r.mode, r.seed, r.n_trials) == (4, 2, 4, 2, 1, "union", 9, 2)
    assert r.values is None
    assert np.array_equal(r.mean, [[1.0, 2.0, 0.0, 0.0], [0.5, 0.5, 0.25, 0.0]])
    assert np.array_equal(r.sd[0], [np.sqrt(0.5), 0.0, 0.0, 0.0])               # 4 - 1e-13 / 4 - 4 < 0: clipped, not NaN
    assert np.array_equal(r.sd[1], [0.5, np.sqrt(0.75), np.sqrt(0.1875), 0.0])
    assert np.array_equal(r.expected_rank, [[1.0, 0.0, 2.0, 2.0], [0.0, 0.5, 2.0, 3.0]])
    assert np.array_equal(r.top_prob, [[0.5, 1.0, 0.0, 0.0], [1.0, 1.0, 0.0, 0.0]])
    assert np.array_equal(r.main_core_prob, [[0.5, 1.0, 0.0, 0.0], [1.0, 0.5, 0.25, 0.0]])
    assert np.array_equal(r.kcore_prob, [[0.75, 1.0, 0.0, 0.0], [0.25, 0.5, 0.0, 0.0]])
    assert np.array_equal(r.inferred, inf) and r.inferred.dtype == np.int64
    assert np.array_equal(r.core_members(), [[True, True, False, False], [False, True, False, False]])
    assert np.array_equal(r.core_members(prob=0.2), [[True, True, False, False], [True, True, False, False]])
    assert not r.core_members(prob=1.01).any()
    assert r.top(2, layer=0).tolist() == [1, 0] and r.top(3, layer=0).tolist() == [1, 0, 2]
    assert r.top(4, layer=1).tolist() == [0, 1, 2, 3]
    fr = r.frame(node_names=["a", "b", "c", "d"])
    assert list(fr.columns) == ["layer", "node", "name", "mean", "sd", "expected_rank", "top_prob", "main_core_prob", "kcore_prob", "inferred"]
    assert len(fr) == 8 and fr.name.tolist() == ["a", "b", "c", "d"] * 2 and fr.layer.tolist() == [0] * 4 + [1] * 4
    assert fr.kcore_prob.tolist() == [0.75, 1.0, 0.0, 0.0, 0.25, 0.5, 0.0, 0.0] and fr.inferred.tolist() == [1, 2, 0, 0, 1, 1, 0, 0]
    u = CoreStats(4, _counts(), mode="in")
    assert u.inferred is None and u.k_min == 0
    assert list(u.frame().columns) == ["layer", "node", "mean", "sd", "expected_rank", "top_prob", "main_core_prob", "kcore_prob"]
    with pytest.raises(ValueError, match="node_names"):
        r.frame(node_names=["a"])
    sm = r.summary()
    assert len(sm) == 8 and list(sm.columns) == ["layer", "statistic", "mean", "std", "q0.025", "q0.5", "q0.975"]
    assert sorted(set(sm.statistic)) == ["core_sum", "degeneracy", "kcore_size", "main_core_size"]
    assert sm[(sm.layer == 1) & (sm.statistic == "degeneracy")]["mean"].iloc[0] == 4.0
    assert sm[(sm.layer == 0) & (sm.statistic == "kcore_size")]["mean"].iloc[0] == 1.75
    assert CoreStats(4, dict(_counts(), values=np.zeros((4, 2, 4), np.uint16))).values.shape == (4, 2, 4)


def test_argument_error_class():
    from vimure_amd.engine import CoresArgumentError, EngineError
    assert issubclass(CoresArgumentError, EngineError) and issubclass(CoresArgumentError, ValueError)
