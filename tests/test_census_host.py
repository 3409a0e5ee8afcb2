"""CPU: the yardsticks of the triad census (tests/census_util.py) held to networkx, to each other and to closed forms; the host
side of `vimure_amd.census` (the dyads read off a census, the expectation under U | MAN by enumeration at N = 4, the transitive
share, shapes); and the list of N at which tests/test_hip_census.py enters the kernel, against the launch shape restated."""
import itertools
from math import comb

import numpy as np
import pytest

from tests.census_util import (CEN_LIST, CLASS_NAMES, CLASS_SIZES, CONNECTED, REPRESENTATIVES, SHAPE_NS, _fast_one, adjacency, boundary_graph,
                               census_fast, census_np, census_one, census_pairs, census_shape, class_ladder, class_table, code_of,
                               complete, edges_of, empty, ladder_census, ladder_classes, list_sizes, path, random_digraph,
                               reversed_nodes, star, three_cycle)
from tests.graph_shapes_util import design, design_large

RANDOM = [(20, 0.1), (25, 0.3), (30, 0.6)]


def _graphs():
    out = {"random %d %.1f" % (N, p): random_digraph(N, p, 100 + N) for N, p in RANDOM}
    out["ladder 63"], out["ladder 420"] = class_ladder(63), class_ladder(420)
    return out


def test_class_table():
    t = class_table()
    assert t.shape == (64,) and tuple(np.bincount(t)) == CLASS_SIZES and sum(CLASS_SIZES) == 64
    for name, edges in REPRESENTATIVES.items():
        assert CLASS_NAMES[t[code_of(edges)]] == name
    assert t[0] == 0 and t[63] == 15
    for code in range(64):      # reversing every tie swaps D and U and nothing else
        rev = code_of((b, a) for a, b in edges_of(code))
        swapped = CLASS_NAMES[t[code]].translate(str.maketrans("DU", "UD"))
        assert CLASS_NAMES[t[rev]] == swapped, code
    assert CONNECTED == (0, 1, 1, 2, 2, 2, 2, 2, 3, 3, 2, 3, 3, 3, 3, 3)


def test_class_names_are_the_package_s():
    from vimure_amd import _lib
    from vimure_amd.census import CLASS_NAMES as NAMES, LABELLED, MAN
    assert tuple(NAMES) == CLASS_NAMES == tuple(_lib.CENSUS_NAMES) and _lib.CENSUS_NCLASS == 16
    assert tuple(LABELLED) == CLASS_SIZES
    assert np.array_equal(MAN.sum(axis=1), np.full(16, 3)) and tuple(MAN[:, 0] + MAN[:, 1]) == CONNECTED


def _nx_census(Y):
    import networkx as nx
    G = nx.from_numpy_array(adjacency(Y).astype(np.uint8), create_using=nx.DiGraph)
    c = nx.triadic_census(G)
    assert tuple(c) == CLASS_NAMES
    return np.array([c[k] for k in CLASS_NAMES], dtype=np.int64)


def test_against_networkx():
    nx = pytest.importorskip("networkx")
    t = class_table()
    assert tuple(nx.algorithms.triads.TRIAD_NAMES) == CLASS_NAMES
    for code in range(64):
        G = nx.DiGraph()
        G.add_nodes_from(range(3))
        G.add_edges_from(edges_of(code))
        c = nx.triadic_census(G)
        assert [k for k, v in c.items() if v] == [CLASS_NAMES[t[code]]], code
    for name, Y in _graphs().items():
        assert Y.diagonal().any() and Y.max() > 1, name
        assert np.array_equal(census_one(Y), _nx_census(Y)), name


def test_the_three_counters_agree():
    graphs = _graphs()
    graphs["random 130"] = random_digraph(130, 0.08, 7)
    graphs["boundary 65"] = boundary_graph(65, 2.0, 3)
    for name, Y in graphs.items():
        want = census_one(Y)
        assert want.sum() == comb(len(Y), 3), name
        assert np.array_equal(census_pairs(Y), want), name
        for sparse in (False, True):
            assert np.array_equal(_fast_one(Y, sparse), want), (name, sparse)
    Ys = np.stack([graphs["random 30 0.6"], graphs["random 30 0.6"].T])[None]
    assert np.array_equal(census_fast(Ys)[0], census_np(Ys)[0]) and census_np(Ys).shape == (1, 2, 16)
    assert census_one(graphs["random 30 0.6"]).all()           # the dense one holds every class


@pytest.mark.parametrize("N", [5, 63, 130, 300])
def test_closed_forms(N):
    for name, (Y, want) in {"path": path(N), "out": star(N, "out"), "in": star(N, "in", N - 1), "mutual": star(N, "mutual", N // 2),
                            "cycle": three_cycle(N), "complete": complete(N), "empty": empty(N)}.items():
        assert want.sum() == comb(N, 3) and (want >= 0).all(), name
        got = census_one(Y) if N <= 130 else census_fast(Y[None, None])[0, 0]
        assert np.array_equal(got, want), (name, N)
        if N <= 63:
            assert np.array_equal(census_pairs(Y), want), (name, N)
    assert path(N)[1][CLASS_NAMES.index("021C")] == N - 2 and path(N)[1][1] == (N - 2) * (N - 3)
    assert star(N, "out")[1][CLASS_NAMES.index("021D")] == comb(N - 1, 2) and star(N, "out")[1][0] == comb(N - 1, 3)
    assert star(N, "in")[1][CLASS_NAMES.index("021U")] == comb(N - 1, 2) and star(N, "mutual")[1][CLASS_NAMES.index("201")] == comb(N - 1, 2)


@pytest.mark.parametrize("N", [63, 64, 65, 129, 257, 420])
def test_class_ladder(N):
    Y = class_ladder(N)
    cls = ladder_classes(N)
    assert len(cls) == min(N // 3, 136) and Y.diagonal().any() and Y.max() == 3
    mult = np.bincount(cls, minlength=16)
    assert (mult >= 1).all()                                # every class at least once from N = 48 on
    if N >= 408:
        assert np.array_equal(mult, np.arange(1, 17))      # q + 1 copies of class q: no two classes alike
    if N in (63, 64, 65):                                   # one round and five triples: the U's and C's have two, the D's and T one
        for d, u in (("021D", "021U"), ("111D", "111U"), ("120D", "120U"), ("030T", "030C"), ("120D", "120C")):
            assert mult[CLASS_NAMES.index(d)] == 1 and mult[CLASS_NAMES.index(u)] == 2, (d, u)
    want = ladder_census(N)
    assert np.array_equal(want[3:], mult[3:]) and want.sum() == comb(N, 3)
    assert np.array_equal(census_fast(Y[None, None])[0, 0], want)
    if N <= 129:
        assert np.array_equal(census_one(Y), want)
    i, j = np.nonzero(adjacency(Y))
    assert ((i // 64) != (j // 64)).any() or N <= 64         # triples straddle the words of a row


def test_designs_of_the_gpu_file():
    """Layer 2 of `design(N)` has every class, and tells D from U in 021, 111 and 120 (the sparse layer in 021 and 111), at every
    N the GPU file takes the design at.  The hub layer does not: its ties are the stride's, all asymmetric and never two at a
    node the same way round, and the hub's, all mutual -- it holds 003, 012, 021C, 201 and 210 only, which is what it is for:
    one node that is a third of every pair.  The large designs are not trivial either."""
    for N in (513, 1024, 1025):
        c = census_fast(design(N)[None])[0]
        assert c.sum(axis=1).tolist() == [comb(N, 3)] * 4
        assert (c[2] > 0).all(), N
        assert c[2, 3] != c[2, 4] and c[2, 6] != c[2, 7] and c[2, 11] != c[2, 12], N
        assert c[0, 3] != c[0, 4] and c[0, 6] != c[0, 7], N
        assert [CLASS_NAMES[q] for q in np.nonzero(c[3])[0]] == ["003", "012", "021C", "201", "210"], N
        swapped = census_fast(design(N)[2].T[None, None])[0, 0]       # reversing every tie swaps D and U and nothing else
        assert np.array_equal(swapped, c[2][[0, 1, 2, 4, 3, 5, 7, 6, 8, 9, 10, 12, 11, 13, 14, 15]]), N
        assert c[1, CLASS_NAMES.index("021C")] == N - 2 and c[1, 1] == (N - 2) * (N - 3)
    c = census_fast(design(2048)[[0, 3]][None])[0]
    assert (c[1, [10, 14]] > 0).all() and (c[0, [1, 3, 4, 5]] > 0).all()
    assert census_fast(design_large(2049)[None])[0, 0].sum() == comb(2049, 3)


def test_the_shape_list_covers_every_shape_class():
    """k_census' branches -- row i in registers or not, one or several trips of the word stride, one, two or three list blocks,
    every G from 1 to 64 -- each met by an N of SHAPE_NS."""
    shapes = {N: census_shape(N) for N in SHAPE_NS}
    assert {s[1] for s in shapes.values()} == {1, 2, 4, 8, 16, 32, 64}
    assert {s[2] for s in shapes.values()} == {True, False}
    assert {s[3] for s in shapes.values()} == {1, 2, 3}
    assert shapes[63][:3] == (1, 1, True) and shapes[65][:3] == (2, 2, True) and shapes[129] == (3, 2, False, 1, 2)
    assert shapes[257] == (5, 4, False, 1, 2) and shapes[513] == (9, 8, False, 1, 2)
    assert shapes[1024] == (16, 16, True, 1, 1) and shapes[1025] == (17, 16, False, 1, 2)
    assert shapes[2048] == (32, 32, True, 1, 1) and shapes[2049] == (33, 32, False, 2, 2)
    assert shapes[4097] == (65, 64, False, 3, 2)
    # j > i only: the hub of the designs, their last node, lists nobody; with the nodes reversed it is node 0 and lists everybody --
    # at N = 4097 a list one short of full (bit 0 is the hub itself), a list of exactly CEN_LIST entries and a list of one
    Y = design_large(4097)[0]
    assert list_sizes(Y, 4096) == [0] and sum(list_sizes(Y, 0)) < 64 and list_sizes(Y, 0)[-1] >= 1
    assert list_sizes(reversed_nodes(Y), 0) == [CEN_LIST - 1, CEN_LIST, 1]
    assert list_sizes(reversed_nodes(design_large(2049)[0]), 0) == [CEN_LIST - 1, 1]
    assert list_sizes(reversed_nodes(design(2048)[3]), 0) == [CEN_LIST - 1]
    R = reversed_nodes(Y)                                     # the walk starts at the block that holds bit i
    assert [len(list_sizes(R, i)) for i in (2047, 2048, 4095, 4096)] == [3, 2, 2, 1]


# ------------------------------------------------------------------------------------------ vimure_amd.census
def _all_digraphs(N):
    pairs = list(itertools.combinations(range(N), 2))
    for states in itertools.product(range(4), repeat=len(pairs)):
        Y = np.zeros((N, N), np.uint8)
        for (i, j), s in zip(pairs, states):
            Y[i, j], Y[j, i] = s & 1, s >> 1
        yield Y, states


def test_expected_under_man_by_enumeration():
    """N = 4: the expectation equals the average census over all digraphs with the same mutual, asymmetric and null dyads, from
    the 4^6 digraphs; it sums to C(4, 3); the dyads read off the census are the direct counts."""
    from vimure_amd.census import dyads_of, expected_under_man
    groups = {}
    for Y, states in _all_digraphs(4):
        man = (sum(s == 3 for s in states), sum(s in (1, 2) for s in states), sum(s == 0 for s in states))
        c = census_one(Y)
        assert tuple(int(x) for x in dyads_of(c, 4)) == man
        groups.setdefault(man, []).append(c)
    assert len(groups) == 28 and sum(len(v) for v in groups.values()) == 4 ** 6
    for man, cs in groups.items():
        cs = np.array(cs)
        exp = expected_under_man(cs[:1], 4)[0]
        assert abs(exp.sum() - 4.0) < 1e-12, man
        np.testing.assert_allclose(exp, cs.mean(axis=0), rtol=0, atol=1e-12, err_msg=str(man))


def test_triad_census_result():
    from vimure_amd.census import TRANSITIVE, VACUOUS, TriadCensus
    N, S, L = 30, 5, 2
    Ys = np.array([[random_digraph(N, 0.1 + 0.1 * l, 10 * s + l) for l in range(L)] for s in range(S)])
    counts = census_np(Ys)
    res = TriadCensus(N, counts, inferred=counts[0], seed=3, n_trials=1)
    assert (res.S, res.L, res.N) == (S, L, N) and res.counts.dtype == np.int64 and res.inferred.shape == (L, 16)
    assert res.mean.shape == res.sd.shape == (L, 16) and np.array_equal(res.mean, counts.mean(axis=0))
    assert res.quantiles((0.1, 0.5)).shape == (2, L, 16) and np.array_equal(res.quantiles((0.5,))[0], np.median(counts, axis=0))
    d = res.dyads()
    B = np.array([[adjacency(Y) for Y in Yl] for Yl in Ys])
    mutual = (B & B.transpose(0, 1, 3, 2)).sum(axis=(2, 3)) // 2
    asym = (B ^ B.transpose(0, 1, 3, 2)).sum(axis=(2, 3)) // 2
    assert np.array_equal(d["mutual"], mutual) and np.array_equal(d["asymmetric"], asym)
    assert np.array_equal(d["null"], comb(N, 2) - mutual - asym) and d["null"].dtype == np.int64
    exp = res.expected_under_man()
    assert exp.shape == (S, L, 16) and np.allclose(exp.sum(axis=-1), comb(N, 3), rtol=1e-12)
    assert np.array_equal(res.excess(), counts - exp) and np.array_equal(res.of("030T"), counts[..., 8])
    # the transitive share from the definition: the classes by brute force over the ordered triples of a representative
    kinds = {}
    for name, edges in REPRESENTATIVES.items():
        E = set(edges)
        two = [(x, y, z) for x, y, z in itertools.permutations(range(3)) if (x, y) in E and (y, z) in E]
        kinds[name] = "vacuous" if not two else ("transitive" if all((x, z) in E for x, y, z in two) else "intransitive")
    assert tuple(sorted(VACUOUS)) == tuple(sorted(k for k, v in kinds.items() if v == "vacuous"))
    assert tuple(sorted(TRANSITIVE)) == tuple(sorted(k for k, v in kinds.items() if v == "transitive"))
    tr = sum(counts[..., CLASS_NAMES.index(k)] for k in TRANSITIVE)
    non_vacuous = sum(counts[..., CLASS_NAMES.index(k)] for k, v in kinds.items() if v != "vacuous")
    assert np.array_equal(res.transitive_share(), tr / non_vacuous) and res.transitive_share().shape == (S, L)
    assert np.isnan(TriadCensus(5, np.array([[empty(5)[1]]])).transitive_share()).all()
    f = res.frame()
    assert len(f) == L * 16 and list(f.columns) == ["layer", "class", "mean", "sd", "expected_under_man", "excess", "inferred"]
    assert list(f["class"][:16]) == list(CLASS_NAMES)
    assert "inferred" not in TriadCensus(N, counts).frame().columns
    sm = res.summary(q=(0.25, 0.75))
    assert len(sm) == L * 20 and list(sm.columns) == ["layer", "statistic", "mean", "std", "q0.25", "q0.75"]
    with pytest.raises(ValueError):
        TriadCensus(N, counts[..., :15])
    with pytest.raises(ValueError):
        TriadCensus(2, np.zeros((1, 1, 16), np.int64)).dyads()
