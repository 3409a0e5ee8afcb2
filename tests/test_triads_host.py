"""CPU: the host pieces of the posterior triad statistics -- the NumPy restatement the GPU tests use (tests/triads_util.py)
against a brute-force triple loop and against exact enumeration of every graph, the new entry points' argument checks, and the
result object's derived ratios.  No GPU needed."""
import itertools

import numpy as np

from tests.triads_util import TRIAD_KEYS, expected_triads_np, triads_np


def _brute(Y):
    """The definitions of include/vimure_hip.h at vmr_sample_triads, word for word: loops over pairwise distinct (i, j, k)."""
    N = Y.shape[0]
    A = Y > 0
    U = A | A.T
    c = dict.fromkeys(TRIAD_KEYS, 0)
    tri = np.zeros(N, np.int64)
    deg = np.zeros(N, np.int64)
    for i in range(N):
        for j in range(N):
            if j == i:
                continue
            deg[i] += U[i, j]
            if i < j:
                c["edges_u"] += int(U[i, j])
            for k in range(N):
                if k == i or k == j:
                    continue
                c["transitive"] += int(A[i, j] and A[j, k] and A[i, k])
                c["cyclic"] += int(A[i, j] and A[j, k] and A[k, i])
                c["two_paths"] += int(A[i, j] and A[j, k])
                if j < k and U[i, j] and U[j, k] and U[i, k]:
                    tri[i] += 1                          # the triangle {i, j, k}, once per node i
    c["triangles_u"] = int(tri.sum()) // 3
    c["wedges_u"] = int((deg * (deg - 1) // 2).sum())
    return c, tri, deg


def test_triads_np_against_brute_force():
    g = np.random.RandomState(5)
    S, L, N = 3, 2, 7
    Ys = (g.rand(S, L, N, N) < 0.45) * g.randint(1, 4, (S, L, N, N))
    assert all(np.diag(Ys[s, l]).any() for s in range(S) for l in range(L))   # self-loops are present, and must not count
    got = triads_np(Ys)
    for k in TRIAD_KEYS:
        assert got[k].dtype == np.int64 and got[k].shape == (S, L)
    assert got["node_tri"].dtype == np.int32 and got["node_deg"].shape == (S, L, N)
    for s in range(S):
        for l in range(L):
            c, tri, deg = _brute(Ys[s, l])
            for k in TRIAD_KEYS:
                assert got[k][s, l] == c[k], (k, s, l)
            assert np.array_equal(got["node_tri"][s, l], tri) and np.array_equal(got["node_deg"][s, l], deg)
    assert got["triangles_u"].min() > 0 and got["cyclic"].min() > 0
    # without the self-loops: the same counts
    Yn = Ys.copy()
    for s in range(S):
        for l in range(L):
            np.fill_diagonal(Yn[s, l], 0)
    again = triads_np(Yn)
    assert all(np.array_equal(again[k], got[k]) for k in got)


def test_triads_np_known_graphs():
    N = 5
    cyc = np.zeros((N, N), np.int64)
    cyc[0, 1] = cyc[1, 2] = cyc[2, 0] = 1                 # one directed 3-cycle
    tr = np.zeros((N, N), np.int64)
    tr[0, 1] = tr[1, 2] = tr[0, 2] = 1                    # one transitive triple
    full = np.ones((N, N), np.int64)                      # complete, with self-loops
    got = triads_np([[cyc, tr, full]])
    assert [got[k][0, 0] for k in TRIAD_KEYS] == [0, 3, 3, 1, 3, 3]
    assert [got[k][0, 1] for k in TRIAD_KEYS] == [1, 0, 1, 1, 3, 3]
    assert [got[k][0, 2] for k in TRIAD_KEYS] == [60, 60, 60, 10, 30, 10]
    assert np.array_equal(got["node_tri"][0, 2], np.full(N, 6)) and np.array_equal(got["node_deg"][0, 0], [2, 2, 2, 0, 0])


def test_expected_triads_np_against_exact_enumeration():
    """N = 3: the expectation over all 2^6 graphs on the six off-diagonal ties, each with its probability under q."""
    g = np.random.RandomState(8)
    L, N, K = 2, 3, 3
    rho = g.rand(L, N, N, K)
    rho /= rho.sum(-1, keepdims=True)                     # (the diagonal carries mass too: p_ii must be ignored)
    got = expected_triads_np(rho)
    off = [(i, j) for i in range(N) for j in range(N) if i != j]
    for l in range(L):
        p = rho[l][..., 1:].sum(-1)
        want = dict.fromkeys(TRIAD_KEYS, 0.0)
        total = 0.0
        for bits in itertools.product((0, 1), repeat=len(off)):
            Y = np.zeros((N, N), np.int64)
            pr = 1.0
            for b, (i, j) in zip(bits, off):
                Y[i, j] = b
                pr *= p[i, j] if b else 1.0 - p[i, j]
            c = triads_np([[Y]])
            total += pr
            for k in TRIAD_KEYS:
                want[k] += pr * float(c[k][0, 0])
        assert abs(total - 1.0) < 1e-14
        for k in TRIAD_KEYS:
            assert want[k] > 0
            np.testing.assert_allclose(got[k][l], want[k], rtol=1e-13, atol=0, err_msg=k)   # 64 terms of <= 7 factors each


def test_entry_points_exported_bound_and_refuse_null_handle():
    from vimure_amd import _lib
    lib = _lib.load()
    assert "vmr_sample_triads" in _lib.SIGNATURES and "vmr_expected_triads" in _lib.SIGNATURES
    assert _lib.TRIAD_NSTAT == len(_lib.TRIAD_NAMES) == 6 and tuple(_lib.TRIAD_NAMES) == TRIAD_KEYS
    counts = np.zeros((2, 1, 6), np.uint64)
    out = np.zeros((1, 6))
    assert lib.vmr_sample_triads(None, 1, 2, 1, counts.ctypes.data, None, None) == _lib.VMR_EINVAL
    assert lib.vmr_sample_triads(None, 1, 0, 0, None, None, None) == _lib.VMR_EINVAL
    assert lib.vmr_expected_triads(None, out.ctypes.data) == _lib.VMR_EINVAL
    assert lib.vmr_expected_triads(None, None) == _lib.VMR_EINVAL


def _counts():
    # S = 3 samples, L = 2 layers, N = 4
    return {"edges": np.array([[4, 0], [5, 2], [6, 1]]), "weight": np.array([[4, 0], [5, 2], [6, 1]]),
            "mutual": np.array([[2, 0], [2, 0], [4, 0]]), "tp": np.zeros((3, 2), np.int64)}


def _triads(nodes=False):
    t = {"transitive": np.array([[2, 0], [1, 0], [6, 0]]), "cyclic": np.array([[3, 0], [0, 0], [6, 0]]),
         "two_paths": np.array([[8, 0], [4, 1], [12, 0]]), "triangles_u": np.array([[1, 0], [1, 0], [2, 0]]),
         "wedges_u": np.array([[5, 0], [3, 1], [8, 0]]), "edges_u": np.array([[4, 0], [3, 2], [5, 1]])}
    if nodes:
        t["node_tri"] = np.zeros((3, 2, 4), np.int32)
        t["node_deg"] = np.zeros((3, 2, 4), np.int32)
        t["node_tri"][0, 0] = [1, 1, 1, 0]
        t["node_deg"][0, 0] = [3, 2, 2, 1]                # a triangle with a pendant node
        t["node_deg"][1, 1] = [1, 1, 0, 0]                # nobody has two neighbours: no clustering defined
    return t


def test_result_object_triad_ratios_and_nan_cases():
    from vimure_amd.netstats import NetworkStats
    exp = {"edges": np.array([5.0, 1.0]), "weight": np.array([5.0, 1.0]), "mutual": np.array([2.0, 0.0]), "edges_var": np.array([1.0, 0.5])}
    et = {k: np.array([1.5 + q, 0.25 * q]) for q, k in enumerate(TRIAD_KEYS)}
    t = _triads(nodes=True)
    r = NetworkStats(4, _counts(), expected=exp, triads=t, expected_triads=et)
    for k in TRIAD_KEYS:
        assert getattr(r, k).dtype == np.int64 and np.array_equal(getattr(r, k), t[k])
        assert np.array_equal(r.expected["exp_" + k], et[k])
    assert np.array_equal(r.transitivity_directed, np.array([[2 / 8, np.nan], [1 / 4, 0 / 1], [6 / 12, np.nan]]), equal_nan=True)
    assert np.array_equal(r.cyclicity, np.array([[3 / 8, np.nan], [0 / 4, 0 / 1], [6 / 12, np.nan]]), equal_nan=True)
    assert np.array_equal(r.transitivity, np.array([[3 / 5, np.nan], [3 / 3, 0 / 1], [6 / 8, np.nan]]), equal_nan=True)
    assert r.local_clustering.shape == (3, 2, 4)
    assert np.array_equal(r.local_clustering[0, 0], np.array([2 / 6, 2 / 2, 2 / 2, np.nan]), equal_nan=True)
    assert r.avg_clustering[0, 0] == (2 / 6 + 1.0 + 1.0) / 3
    assert np.isnan(r.local_clustering[1, 1]).all() and np.isnan(r.avg_clustering[1, 1])
    assert np.isnan(r.avg_clustering[1, 0])               # (all degrees 0)
    stats = r.statistics()
    for k in TRIAD_KEYS + ("transitivity_directed", "cyclicity", "transitivity", "avg_clustering"):
        assert stats[k].shape == (3, 2), k
    assert len(r.summary()) == r.L * len(stats)
    assert set(r.summary()["statistic"]) == set(stats)
    # triads without the node arrays: the ratios, no clustering
    r1 = NetworkStats(4, _counts(), expected=exp, triads=_triads())
    assert r1.local_clustering is None and "avg_clustering" not in r1.statistics() and "transitivity" in r1.statistics()
    assert "exp_transitive" not in r1.expected


def test_statistics_without_triads_are_todays():
    from vimure_amd.netstats import NetworkStats
    r = NetworkStats(4, _counts())
    assert tuple(r.statistics()) == ("edges", "weight", "mutual", "reciprocity", "density")
    assert r.transitive is None and r.transitivity is None and r.local_clustering is None and r.expected is None
    r = NetworkStats(4, _counts(), ref_edges=np.array([3, 1]),
                     expected={"edges": np.ones(2), "weight": np.ones(2), "mutual": np.ones(2), "edges_var": np.ones(2)})
    assert tuple(r.statistics()) == ("edges", "weight", "mutual", "reciprocity", "density", "tp", "precision", "recall", "f1")
    assert tuple(r.expected) == ("edges", "weight", "mutual", "edges_var", "expected_reciprocity")
    assert len(r.summary()) == 2 * 9
