"""Host only: the yardsticks of the structural holes (tests/holes_util.py) held to each other -- dense products against three
loops of exact rationals -- to networkx, to closed forms and to the rank rule; the launch shapes of the GPU file restated; and
`holes.StructuralHoles` on hand-made counts."""
from fractions import Fraction

import numpy as np
import pytest

from tests.holes_util import (MODES, SHAPE_NS, SH_BLK, SH_TILE, U, clique, clique_constraint, designs, holes_loops, holes_np, holes_one,
                              holes_shape, pair_and_spokes, planted, ranks, reduce_values, star)


def _random(N, p, seed):
    """A random digraph with entries up to 3, a drawn diagonal and two isolated nodes."""
    g = np.random.RandomState(seed)
    Y = ((g.random_sample((N, N)) < p) * g.randint(1, 4, (N, N))).astype(np.uint8)
    iso = g.choice(N, 2, replace=False)
    Y[iso, :] = 0
    Y[:, iso] = 0
    Y[iso, iso] = 1
    return Y


@pytest.mark.parametrize("mode", MODES)
def test_products_equal_exact_loops_on_random_digraphs(mode):
    """N = 5, 30, 65, sparse to dense, diagonal entries and isolates: the integers `==`; the effective size `==` the correctly
    rounded value of the exact rational (one division of two exact integers); the constraint within 6 N 2^-53 relative of the
    rational -- `constraint_bound`'s count of `holes_np`'s operations is (3 N + 7) 2^-53."""
    seen = set()
    for N, p, seed in ((5, 0.5, 1), (30, 0.1, 2), (30, 0.5, 3), (65, 0.05, 4), (65, 0.3, 5)):
        Y = _random(N, p, seed)
        assert Y.diagonal().any() and Y.max() == 3
        d, s, R, ES, c = holes_one(Y, mode)
        dl, sl, Rl, ESl, cl = holes_loops(Y, mode)
        assert d.tolist() == dl and s.tolist() == sl and R.tolist() == Rl, (N, mode)
        assert (d == 0).sum() >= 2
        for i in range(N):
            if dl[i] == 0:
                assert ESl[i] is None and np.isnan(ES[i]) and np.isnan(c[i])
                continue
            assert ESl[i] == dl[i] - Fraction(Rl[i], 2 * sl[i]) and ESl[i] >= 1          # R is the numerator of Burt's redundancy
            assert ES[i] == float(ESl[i]), (N, mode, i)                                    # float(Fraction) rounds correctly
            assert abs(Fraction(c[i]) - cl[i]) <= Fraction(6 * N * U) * cl[i], (N, mode, i)
        if mode == "weighted":
            seen |= {"mutual"} if (s > d).any() else set()
            seen |= {"none mutual"} if (s == d)[d > 0].any() else set()
    assert mode == "union" or seen == {"mutual", "none mutual"}          # nodes with mx = 2 and with mx = 1


def test_against_networkx():
    """Union mode against networkx on `to_undirected()`, every node; weighted mode against the DiGraph on the nodes with out-ties
    (networkx reports NaN for the others, whatever their in-ties); to 1e-12 relative.  Isolates are NaN on both sides."""
    nx = pytest.importorskip("networkx")
    for N, p, seed in ((30, 0.12, 11), (40, 0.3, 12), (65, 0.06, 13)):
        Y = _random(N, p, seed)
        A = (Y > 0) & ~np.eye(N, dtype=bool)
        G = nx.DiGraph()
        G.add_nodes_from(range(N))
        G.add_edges_from(zip(*np.nonzero(A)))
        for mode, H, nodes in (("union", G.to_undirected(), range(N)), ("weighted", G, np.nonzero(A.any(axis=1))[0])):
            d, s, R, ES, c = holes_one(Y, mode)
            es_nx, c_nx = nx.effective_size(H), nx.constraint(H)
            seen = 0
            for i in nodes:
                i = int(i)
                if d[i] == 0:
                    assert np.isnan(es_nx[i]) and np.isnan(c_nx[i])
                    continue
                assert abs(ES[i] - es_nx[i]) <= 1e-12 * abs(es_nx[i]), (N, mode, i)
                assert abs(c[i] - c_nx[i]) <= 1e-12 * abs(c_nx[i]), (N, mode, i)
                seen += 1
            assert seen >= N // 2
        in_only = np.nonzero(~A.any(axis=1) & A.any(axis=0))[0]
        if len(in_only):
            assert all(np.isnan(nx.constraint(G)[int(i)]) for i in in_only) and not np.isnan(holes_one(Y, "weighted")[4][in_only]).any()


@pytest.mark.parametrize("mode", MODES)
def test_closed_forms(mode):
    """The centre of a star with n leaves: ES = n, c = 1 / n; a leaf: ES = 1, c = 1; a node of an n-clique: ES = 1, c = (n - 1)
    (1 / (n - 1) + (n - 2) / (n - 1)^2)^2 -- exact where they are dyadic rationals, else within the rounding of the products."""
    for n, kind in ((256, "out"), (256, "mutual"), (7, "in")):
        d, s, R, ES, c = holes_one(star(300, n, kind), mode)
        assert d[0] == n and s[0] == (2 * n if (kind == "mutual" and mode == "weighted") else n)
        assert ES[0] == n and np.array_equal(ES[1:n + 1], np.ones(n)) and np.array_equal(c[1:n + 1], np.ones(n))
        assert c[0] == 1.0 / n if n == 256 else abs(c[0] - 1.0 / n) <= 8 * U / n
        assert np.isnan(ES[n + 1:]).all() and np.isnan(c[n + 1:]).all()
    for n in (3, 17, 40):
        d, s, R, ES, c = holes_one(clique(64, n), mode)
        want = clique_constraint(n)
        assert np.array_equal(ES[64 - n:], np.ones(n)) and np.isnan(ES[:64 - n]).all()
        assert all(abs(Fraction(x) - want) <= Fraction(6 * 64 * U) * want for x in c[64 - n:])
    # the mutual pair with asymmetric spokes, weighted: the pair's tie weighs 2 and a hub's strength exceeds its degree
    d, s, R, ES, c = holes_one(pair_and_spokes(300, 70), "weighted")
    assert d[0] == 71 and s[0] == 72 and d[1] == 2 and s[1] == 2 and d[299] == 71
    for name, Y in designs(300).items():
        dl, sl, Rl, ESl, cl = holes_loops(Y, mode)
        d, s, R, ES, c = holes_one(Y, mode)
        assert d.tolist() == dl and s.tolist() == sl and R.tolist() == Rl, name
        assert all((e is None and np.isnan(x)) or x == float(e) for x, e in zip(ES, ESl)), name


def test_the_shapes_the_gpu_file_enters():
    """`SHAPE_NS` covers what `holes_shape` says the kernels branch on."""
    shapes = {N: holes_shape(N) for N in SHAPE_NS}
    assert {s[1] for s in shapes.values()} >= {1, 2, 4, 8, 16, 32, 64}                    # lanes per neighbour
    assert {s[2] for s in shapes.values()} == {True, False}                               # row i in registers or not
    assert {s[3] for s in shapes.values()} == {1, 2, 3}                                   # list blocks
    assert any(s[4] > 1 and s[1] == 64 for s in shapes.values())                          # a second trip on 64 lanes
    assert {s[5] for s in shapes.values()} >= {1, 2, 3, 17}                               # rank tiles
    assert shapes[2048] == (32, 32, True, 1, 1, 8) and shapes[2049] == (33, 32, False, 2, 2, 9) and shapes[4097] == (65, 64, False, 3, 2, 17)
    assert shapes[63][:3] == (1, 1, True) and shapes[65][:3] == (2, 2, True) and shapes[129][:3] == (3, 2, False)
    assert shapes[257][5] == 2 and SH_BLK == 32 and SH_TILE == 256


def test_the_rank_rule():
    """Equal values share the smaller rank; undefined nodes are not counted and rank behind every defined one; effective size
    ranks downwards, constraint upwards."""
    es = np.array([3.0, 1.0, 3.0, 0.0, 2.0, 0.0])
    con = np.array([0.5, 1.0, 0.25, 0.0, 0.5, 0.0])
    defined = np.array([True, True, True, False, True, False])
    re, rc, nd = ranks(es, con, defined)
    assert nd == 4 and re.tolist() == [0, 3, 0, 4, 2, 4] and rc.tolist() == [1, 3, 0, 4, 1, 4]
    re, rc, nd = ranks(np.zeros(3), np.zeros(3), np.zeros(3, bool))
    assert nd == 0 and re.tolist() == [0, 0, 0] and rc.tolist() == [0, 0, 0]
    # two samples of one layer folded: the undefined sample adds 0 to the sums, its rank to the rank sums
    deg = np.array([[[2, 1, 0]], [[1, 0, 1]]])
    ES = np.array([[[2.0, 1.0, np.nan]], [[1.0, np.nan, 1.0]]])
    C = np.array([[[0.5, 1.0, np.nan]], [[1.0, np.nan, 1.0]]])
    out = reduce_values(deg, ES, C, top_k=1)
    assert out["node_sum"].tolist() == [[[3.0, 1.0, 1.0]], [[1.5, 1.0, 1.0]]] and out["node_sumsq"][0].tolist() == [[5.0, 1.0, 1.0]]
    assert out["node_rank_sum"].tolist() == [[[0, 3, 2]], [[0, 3, 2]]] and out["node_top"].tolist() == [[[2, 0, 1]], [[2, 0, 1]]]
    assert out["node_defined"].tolist() == [[2, 1, 1]] and out["n_defined"].tolist() == [[2.0], [2.0]]
    assert out["effective_size_sum"].tolist() == [[3.0], [2.0]] and out["constraint_sum"].tolist() == [[1.5], [2.0]]


def test_holes_np_folds_its_own_values():
    Ys = np.stack([planted(65, 2.0, 5, 7 + q) for q in range(4)]).reshape(2, 2, 65, 65)
    for mode in MODES:
        out = holes_np(Ys, mode, top_k=3)
        assert (out["degree"] == 0).any() and out["effective_size"].shape == (2, 2, 65)
        assert np.array_equal(np.isnan(out["effective_size"]), out["degree"] == 0)
        again = reduce_values(out["degree"], out["effective_size"], out["constraint"], 3)
        for k, v in again.items():
            assert np.array_equal(out[k], v), k
        assert (out["node_top"].sum(axis=2) >= 2 * 3).all() and (out["node_defined"] <= 2).all()


# ------------------------------------------------------------------------------------------ holes.StructuralHoles
def test_structural_holes_result():
    from vimure_amd.holes import StructuralHoles
    Ys = np.stack([planted(65, 2.0, 5, 20 + q) for q in range(6)]).reshape(6, 1, 65, 65)
    Ys[:, 0, 64, :] = 0
    Ys[:, 0, :, 64] = 0                                    # node 64 is isolated in every sample
    counts = holes_np(Ys, "weighted", top_k=5)
    inferred = {k: holes_np(Ys[:1], "weighted")[k][0] for k in ("effective_size", "constraint")}
    res = StructuralHoles(65, counts, mode="weighted", top_k=5, inferred=inferred, seed=3)
    assert (res.S, res.L, res.N) == (6, 1, 65) and res.effective_size.values.shape == (6, 1, 65)
    nd = counts["node_defined"]
    assert nd[0, 64] == 0 and (nd > 0).sum() >= 40 and ((nd > 0) & (nd < 6)).any()
    for q, view in enumerate((res.effective_size, res.constraint)):
        some = nd > 0
        assert np.array_equal(view.mean[some], (counts["node_sum"][q][some] / nd[some])) and np.isnan(view.mean[~some]).all()
        assert np.isnan(view.sd[~some]).all() and (view.sd[some] >= 0).all()
        assert np.array_equal(view.expected_rank, counts["node_rank_sum"][q] / 6.0) and np.array_equal(view.top_prob, counts["node_top"][q] / 6.0)
        assert np.array_equal(view.defined_prob, nd / 6.0) and view.top(4).shape == (4,) and len(view.frame()) == 65
    v = counts["effective_size"]
    some = nd[0] == 6
    assert np.allclose(res.effective_size.mean[0][some], v[:, 0][:, some].mean(axis=0), rtol=1e-14)
    assert np.allclose(res.effective_size.sd[0][some], v[:, 0][:, some].std(axis=0), atol=1e-7)
    eff = res.efficiency()
    assert eff.shape == (6, 1, 65) and np.array_equal(np.isnan(eff), counts["degree"] == 0) and np.nanmax(eff) <= 1.0 and np.nanmin(eff) > 0
    b = res.brokers(5)
    assert b.shape == (5,) and res.constraint.top_prob[0][b[0]] == res.constraint.top_prob[0].max()
    f = res.frame(node_names=["n%d" % i for i in range(65)])
    assert len(f) == 65 and {"defined_prob", "effective_size_mean", "constraint_mean", "constraint_top_prob", "effective_size_inferred",
                             "constraint_inferred", "name"} <= set(f.columns)
    assert len(res.summary()) == 3 and list(res.summary()["statistic"]) == ["n_defined", "effective_size_sum", "constraint_sum"]
    plain = dict(counts)
    for k in ("degree", "strength", "redundancy", "effective_size", "constraint"):
        plain.pop(k)
    res = StructuralHoles(65, plain)
    assert res.efficiency() is None and res.effective_size.values is None and res.inferred is None and "effective_size_inferred" not in res.frame()
