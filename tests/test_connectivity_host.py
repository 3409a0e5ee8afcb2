"""CPU: the host pieces of the posterior connectivity -- the scipy restatement the GPU tests use (tests/connectivity_util.py)
against the definitions of include/vimure_hip.h word for word and against designed graphs, the binding's constants, and what
`ConnectivityStats` derives from the integers."""
import numpy as np
import pytest

from tests.connectivity_util import CONN_KEYS, NDIST, NODE_KEYS, check_designed, connectivity_np, designed_graphs


def _by_definition(Y):
    """The definitions at vmr_sample_connectivity, word for word: a Floyd-Warshall loop for d, then every count from d."""
    N = Y.shape[0]
    INF = 10 ** 9
    A = [[bool(Y[i, j] > 0) and i != j for j in range(N)] for i in range(N)]
    U = [[A[i][j] or A[j][i] for j in range(N)] for i in range(N)]

    def dist(E):
        d = [[0 if i == j else (1 if E[i][j] else INF) for j in range(N)] for i in range(N)]
        for k in range(N):
            for i in range(N):
                for j in range(N):
                    if d[i][k] + d[k][j] < d[i][j]:
                        d[i][j] = d[i][k] + d[k][j]
        return d
    d, du = dist(A), dist(U)
    c = dict.fromkeys(CONN_KEYS, 0)
    comp_w = [min(j for j in range(N) if du[i][j] < INF) for i in range(N)]
    comp_s = [min(j for j in range(N) if d[i][j] < INF and d[j][i] < INF) for i in range(N)]
    for kind, lab in (("w", comp_w), ("s", comp_s)):
        sizes = [lab.count(r) for r in sorted(set(lab))]
        c["components_" + kind], c["giant_" + kind] = len(sizes), max(sizes)
    c["isolates"] = sum(1 for i in range(N) if not any(U[i]))
    hist = [0] * NDIST
    for i in range(N):
        for j in range(N):
            if i == j:
                continue
            c["pairs_w"] += du[i][j] < INF
            c["pairs_s"] += d[i][j] < INF and d[j][i] < INF
            if d[i][j] < INF:
                c["reach_pairs"] += 1
                c["dist_sum"] += d[i][j]
                c["diameter"] = max(c["diameter"], d[i][j])
                hist[min(d[i][j], NDIST) - 1] += 1
    fin = [[i != j and d[i][j] < INF for j in range(N)] for i in range(N)]
    nodes = {"node_comp_w": comp_w, "node_comp_s": comp_s,
             "node_reach_out": [sum(fin[i]) for i in range(N)],
             "node_reach_in": [sum(fin[i][j] for i in range(N)) for j in range(N)],
             "node_dist_out": [sum(d[i][j] for j in range(N) if fin[i][j]) for i in range(N)],
             "node_dist_in": [sum(d[i][j] for i in range(N) if fin[i][j]) for j in range(N)]}
    return c, hist, nodes


def test_restatement_against_the_definitions():
    g = np.random.RandomState(5)
    Ys = []
    for N, p in ((1, 0.5), (2, 0.5), (7, 0.15), (12, 0.08), (12, 0.2), (11, 0.0)):
        Y = (g.rand(2, N, N) < p).astype(np.uint8) * g.randint(1, 4, (2, N, N)).astype(np.uint8)
        Y[0, np.arange(N), np.arange(N)] = 1            # self-loops: they change nothing
        Ys.append(Y)
    for Y in Ys:
        got = connectivity_np([Y])
        for k in CONN_KEYS:
            assert got[k].dtype == np.int64 and got[k].shape == (1, 2), k
        assert got["dist_hist"].dtype == np.int64 and got["dist_hist"].shape == (1, 2, NDIST)
        for l in range(2):
            c, hist, nodes = _by_definition(Y[l])
            for k in CONN_KEYS:
                assert got[k][0, l] == c[k], (k, Y.shape)
            assert got["dist_hist"][0, l].tolist() == hist
            for k in NODE_KEYS:
                assert got[k].dtype == np.int32 and got[k][0, l].tolist() == nodes[k], k
    assert any(connectivity_np([Y])["components_w"].max() > 1 for Y in Ys)
    assert any(connectivity_np([Y])["giant_s"].max() > 1 for Y in Ys)


def test_restatement_on_designed_graphs():
    Y = designed_graphs()
    check_designed(connectivity_np([Y, Y]))


def test_binding_constants_and_null_handle():
    from vimure_amd import _lib, build
    from vimure_amd.connectivity import CONN_KEYS as keys, NODE_KEYS as node_keys
    assert "vmr_sample_connectivity" in _lib.SIGNATURES
    assert _lib.CONN_NSTAT == len(_lib.CONN_NAMES) == 10 and tuple(_lib.CONN_NAMES) == CONN_KEYS == keys
    assert _lib.CONN_NDIST == NDIST and tuple(_lib.CONN_NODE_NAMES) == NODE_KEYS == node_keys
    hdr = open(build.HEADERS[-1]).read()
    for name, val in (("VMR_CONN_NSTAT", _lib.CONN_NSTAT), ("VMR_CONN_NDIST", _lib.CONN_NDIST), ("VMR_CONN_NMAX", _lib.CONN_NMAX)):
        assert "#define %s %d" % (name, val) in hdr
    assert _lib.CONN_NMAX >= 2048
    build.build()
    lib = _lib.load()
    counts = np.zeros((2, 1, _lib.CONN_NSTAT), np.uint64)
    assert lib.vmr_sample_connectivity(None, 1, 2, 1, counts.ctypes.data, *[None] * 7) == _lib.VMR_EINVAL
    assert lib.vmr_sample_connectivity(None, 1, 0, 0, *[None] * 8) == _lib.VMR_EINVAL


def _counts(S=3, L=2, N=5, nodes=False):
    c = {k: np.zeros((S, L), np.int64) for k in CONN_KEYS}
    c["dist_hist"] = np.zeros((S, L, NDIST), np.int64)
    # sample 0, layer 0: the directed path on 5 nodes; layer 1: empty
    c["components_w"][0], c["giant_w"][0], c["pairs_w"][0], c["isolates"][0] = (1, 5), (5, 1), (20, 0), (0, 5)
    c["components_s"][0], c["giant_s"][0] = (5, 5), (1, 1)
    c["reach_pairs"][0], c["dist_sum"][0], c["diameter"][0] = (10, 0), (20, 0), (4, 0)
    c["dist_hist"][0, 0, :4] = (4, 3, 2, 1)
    # sample 1: layer 0 with a pair beyond the bins; layer 1 the 5-cycle
    c["giant_w"][1], c["giant_s"][1], c["pairs_w"][1] = (5, 5), (1, 5), (20, 20)
    c["reach_pairs"][1], c["dist_sum"][1] = (3, 20), (70, 50)
    c["dist_hist"][1, 0, (0, 1, NDIST - 1)] = 1
    c["dist_hist"][1, 1, :4] = 5
    if nodes:
        for k in NODE_KEYS:
            c[k] = np.zeros((S, L, N), np.int32)
        c["node_comp_w"][:] = np.arange(N)
        c["node_comp_s"][:] = np.arange(N)
        c["node_comp_w"][0, 0] = 0
        c["node_comp_w"][1, 1], c["node_comp_s"][1, 1] = 0, 0
        c["node_comp_w"][2, 0] = (0, 0, 2, 2, 4)
        c["node_reach_out"][0, 0], c["node_dist_out"][0, 0] = (4, 3, 2, 1, 0), (10, 6, 3, 1, 0)
        c["node_reach_in"][0, 0], c["node_dist_in"][0, 0] = (0, 1, 2, 3, 4), (0, 1, 3, 6, 10)
    return c


def test_connectivity_stats_derived_quantities():
    from vimure_amd.connectivity import ConnectivityStats
    r = ConnectivityStats(5, _counts(nodes=True), seed=9, n_trials=2)
    assert (r.S, r.L, r.N, r.seed, r.n_trials) == (3, 2, 5, 9, 2)
    for k in CONN_KEYS:
        assert getattr(r, k).dtype == np.int64 and np.array_equal(getattr(r, k), _counts()[k]), k
    assert np.array_equal(r.giant_fraction_w[0], [1.0, 0.2]) and np.array_equal(r.giant_fraction_s[1], [0.2, 1.0])
    assert np.array_equal(r.connectedness[0], [1.0, 0.0]) and np.array_equal(r.reach_fraction[0], [0.5, 0.0])
    assert r.avg_path_length[0, 0] == 2.0 and np.isnan(r.avg_path_length[0, 1])          # nothing reachable: NaN
    assert np.isnan(r.avg_path_length[2]).all()
    assert np.isclose(r.global_efficiency[0, 0], (4 + 3 / 2 + 2 / 3 + 1 / 4) / 20, rtol=1e-15)
    assert r.global_efficiency[0, 1] == 0.0
    assert np.isnan(r.global_efficiency[1, 0])                                            # the overflow bin is not empty
    assert np.isclose(r.global_efficiency[1, 1], (1 + 1 / 2 + 1 / 3 + 1 / 4) / 4, rtol=1e-15)
    # closeness: (r / (N - 1)) (r / dist), 0 where nothing is reached
    assert np.allclose(r.closeness_out[0, 0], [4 / 4 * 4 / 10, 3 / 4 * 3 / 6, 2 / 4 * 2 / 3, 1 / 4 * 1 / 1, 0.0], rtol=1e-15, atol=0)
    assert np.allclose(r.closeness_in[0, 0], [0.0, 1 / 4, 2 / 4 * 2 / 3, 3 / 4 * 3 / 6, 4 / 4 * 4 / 10], rtol=1e-15, atol=0)
    assert not r.closeness_out[0, 1].any() and not np.isnan(r.closeness_out).any()
    assert np.array_equal(r.same_component(0, 1), [2 / 3, 1 / 3]) and np.array_equal(r.same_component(0, 4), [1 / 3, 1 / 3])
    assert np.array_equal(r.same_component(0, 1, strong=True), [0.0, 1 / 3]) and np.array_equal(r.same_component(3, 3), [1.0, 1.0])
    st = r.statistics()
    assert set(CONN_KEYS) | {"giant_fraction_w", "giant_fraction_s", "connectedness", "reach_fraction", "avg_path_length",
                             "global_efficiency"} == set(st)
    sm = r.summary()
    assert len(sm) == r.L * len(st) and list(sm.columns) == ["layer", "statistic", "mean", "std", "q0.025", "q0.5", "q0.975"]
    row = sm[(sm.layer == 0) & (sm.statistic == "avg_path_length")].iloc[0]
    assert np.isclose(row["mean"], np.mean([2.0, 70 / 3]))                              # the NaN sample is left out
    fr = r.frame()
    assert list(fr.columns)[:2] == ["layer", "distance"]
    assert fr[fr.layer == 0].distance.tolist() == list(range(1, NDIST + 1)) and fr[fr.layer == 1].distance.tolist() == [1, 2, 3, 4]
    assert np.isclose(fr[(fr.layer == 1) & (fr.distance == 1)]["mean"].iloc[0], 5 / 3)


def test_connectivity_stats_without_hist_or_nodes():
    from vimure_amd.connectivity import ConnectivityStats
    c = _counts()
    del c["dist_hist"]
    r = ConnectivityStats(5, c)
    assert r.dist_hist is None and r.global_efficiency is None and "global_efficiency" not in r.statistics()
    assert r.closeness_out is None and r.node_comp_w is None and not r.has_nodes
    with pytest.raises(ValueError, match="nodes=True"):
        r.same_component(0, 1)
    with pytest.raises(ValueError, match="histogram"):
        r.frame()
    assert len(r.summary()) == r.L * len(r.statistics())
    one = ConnectivityStats(1, {k: np.ones((1, 1), np.int64) * (k in ("components_w", "giant_w", "isolates", "components_s", "giant_s"))
                                for k in CONN_KEYS})
    assert np.isnan(one.connectedness).all() and np.isnan(one.reach_fraction).all() and one.giant_fraction_w[0, 0] == 1.0


def test_argument_error_class():
    from vimure_amd.engine import ConnectivityArgumentError, EngineError
    assert issubclass(ConnectivityArgumentError, EngineError) and issubclass(ConnectivityArgumentError, ValueError)
