"""Host: the yardsticks of the shared partners (tests/partners_util.py) held to each other, to closed forms and to what the suite
already trusts (`graph_shapes_util.triads_sparse`), and `partners.SharedPartners` on hand-made arrays.  No device."""
import numpy as np
import pytest

from tests.census_util import random_digraph
from tests.graph_shapes_util import triads_sparse
from tests.partners_util import (MAX_BINS, MODES, SHAPE_NS, SP_BLK, TOTALS, book, closed_forms, fold, partners_np, partners_shape, partners_slow,
                                 transposed_ends)

KEYS = ("hist", "totals", "node_ties", "node_supported", "pair_partners_net", "pair_present", "pair_supported", "pair_partners")


def _same(a, b, what=""):
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (what, k)


def _all_pairs(L, N):
    l, i, j = np.meshgrid(np.arange(L), np.arange(N), np.arange(N), indexing="ij")
    p = np.stack([l.ravel(), i.ravel(), j.ravel()], axis=1)
    return p[p[:, 1] != p[:, 2]]


@pytest.mark.parametrize("mode", MODES)
def test_products_equal_loops_on_random_digraphs(mode):
    """Random digraphs with a drawn diagonal and entries up to 3, N = 5 .. 40, sparse to dense, every ordered pair listed."""
    for N, p, seed in ((5, 0.5, 1), (17, 0.15, 2), (23, 0.6, 3), (40, 0.3, 4)):
        Ys = np.stack([random_digraph(N, p, seed + 10 * q) for q in range(4)]).reshape(2, 2, N, N)
        assert Ys.max() == 3 and Ys[0, 0].diagonal().any()
        pairs = _all_pairs(2, N)
        a, b = partners_np(Ys, mode, 8, pairs), partners_slow(Ys, mode, 8, pairs)
        _same(a, b, (mode, N))
        assert (N < 20 or a["totals"][..., 2].all()) and (a["hist"].sum(axis=-1) == a["totals"][..., 0]).all()
        if mode != "path":      # (i, j) and (j, i) name the same tie
            assert np.array_equal(partners_np(Ys, mode, 8, transposed_ends(pairs))["pair_partners_net"], a["pair_partners_net"])


@pytest.mark.parametrize("N", [4, 5, 40, 130])
def test_closed_forms(N):
    for name, (Y, want) in closed_forms(N).items():
        for mode in MODES:
            got = partners_np(Y[None, None], mode, MAX_BINS)
            assert tuple(got["totals"][0, 0]) == want[mode], (name, mode, N)
            if N <= 40:
                _same(got, partners_slow(Y[None, None], mode, MAX_BINS), (name, mode))
    Y = book(N)
    got = partners_np(Y[None, None], "union", MAX_BINS, [(0, 0, N - 1), (0, N - 1, 0), (0, 0, 1), (0, 2, N - 1), (0, 1, 2)])
    assert got["pair_partners_net"][0].tolist() == [N - 2, N - 2, 1, 1, -1]          # the spine in both orders, two pages, two untied pages
    h = got["hist"][0, 0]
    assert h[1] == 2 * (N - 2) and h[N - 2] == 1 and h.sum() == 2 * N - 3
    assert got["node_ties"][0, 0, 0] == N - 1 and got["node_ties"][0, 0, 1] == 2 and (got["node_supported"] == got["node_ties"]).all()


def test_the_book_overflows_any_legal_histogram():
    """Beyond N = 1025 the spine's N - 2 partners land in the last bin of the largest histogram the device offers."""
    N = 1027
    got = partners_np(book(N)[None, None], "mutual", MAX_BINS)
    assert got["hist"][0, 0, -1] == 1 and got["hist"][0, 0, 1] == 2 * (N - 2) and got["totals"][0, 0].tolist() == [2 * N - 3, 2 * N - 3, 3 * (N - 2), N - 2]


def test_identities_against_the_triads():
    """Every triangle of U = A | A^T is met from each of its three ties; a tie i -> j with a partner k closes i -> k -> j: the
    transitive triples; the union ties are the edges of U."""
    Ys = np.stack([random_digraph(60, p, 7 + q) for q, p in enumerate((0.05, 0.2, 0.5, 0.02))]).reshape(2, 2, 60, 60)
    tri = triads_sparse(Ys)
    u, p = partners_np(Ys, "union", MAX_BINS), partners_np(Ys, "path", MAX_BINS)
    assert np.array_equal(u["totals"][..., 2], 3 * tri["triangles_u"]) and tri["triangles_u"].all()
    assert np.array_equal(p["totals"][..., 2], tri["transitive"]) and tri["transitive"].all()
    assert np.array_equal(u["totals"][..., 0], tri["edges_u"])
    assert np.array_equal(u["node_ties"], tri["node_deg"])


@pytest.mark.parametrize("mode", MODES)
def test_pooling(mode):
    Ys = random_digraph(50, 0.7, 3)[None, None]
    full = partners_np(Ys, mode, MAX_BINS)
    assert full["totals"][0, 0, 3] >= 8 and not full["hist"][..., -1].any()
    pooled = partners_np(Ys, mode, 8)
    assert np.array_equal(pooled["hist"], fold(full["hist"], 8)) and pooled["hist"][0, 0, 7] == full["hist"][0, 0, 7:].sum() > 0
    assert np.array_equal(pooled["totals"], full["totals"])


def test_shape_list_covers_every_class():
    shapes = {N: partners_shape(N) for N in SHAPE_NS}
    assert {s[1] for s in shapes.values()} >= {1, 2, 4, 8, 16, 32, 64}                    # lanes per neighbour
    assert {s[2] for s in shapes.values()} == {True, False}                               # row i in a register or not
    assert {s[3] for s in shapes.values()} == {1, 2, 3}                                   # list blocks
    assert any(s[4] > 1 and s[1] == 64 for s in shapes.values())                          # a second trip on 64 lanes
    assert shapes[2048] == (32, 32, True, 1, 1) and shapes[2049] == (33, 32, False, 2, 2) and shapes[4097] == (65, 64, False, 3, 2)
    assert shapes[63][:3] == (1, 1, True) and shapes[65][:3] == (2, 2, True) and shapes[129][:3] == (3, 2, False)
    assert SP_BLK == 32


# ------------------------------------------------------------------------------------------ partners.SharedPartners
def _hand_made():
    from vimure_amd.partners import SharedPartners
    hist = np.zeros((3, 2, 4), np.int64)
    hist[0, 0] = [2, 1, 1, 0]       # 4 ties: 2 bridges, partners 0 0 1 2
    hist[1, 0] = [0, 4, 0, 0]
    hist[2, 0] = [1, 0, 3, 0]
    hist[1, 1] = [5, 0, 0, 0]       # layer 1: no tie in samples 0 and 2
    totals = np.zeros((3, 2, 4), np.int64)
    totals[:, 0] = [[4, 2, 3, 2], [4, 4, 4, 1], [4, 3, 6, 2]]
    totals[1, 1] = [5, 0, 0, 0]
    pairs = np.array([[0, 1, 2], [0, 2, 3], [1, 0, 4]])
    inferred = {"hist": np.array([[1, 2, 1, 0], [0, 0, 0, 0]]), "totals": np.zeros((2, 4), np.int64), "pair_partners": np.array([2, -1, -1])}
    return SharedPartners(5, "union", hist, totals, pairs=pairs, pair_present=[3, 2, 0], pair_supported=[3, 0, 0], pair_partners=[5, 0, 0],
                          inferred=inferred, seed=1)


def test_shared_partners_support_and_tables():
    sp = _hand_made()
    assert (sp.S, sp.L, sp.n_bins) == (3, 2, 4)
    s = sp.support()
    assert s[:, 0].tolist() == [0.5, 1.0, 0.75] and np.isnan(s[[0, 2], 1]).all() and s[1, 1] == 0.0
    assert sp.mean_partners()[:, 0].tolist() == [0.75, 1.0, 1.5] and sp.local_bridges()[:, 0].tolist() == [2, 0, 1]
    assert sp.mean["support"][0] == 0.75 and sp.mean["support"][1] == 0.0 and sp.mean["ties"].tolist() == [4.0, 5.0 / 3.0]
    assert sp.quantiles((0.5,))["support"].shape == (1, 2) and sp.quantiles((0.5,))["support"][0, 0] == 0.75
    t = sp.ties_frame()
    assert list(t.columns) == ["layer", "i", "j", "p_present", "p_supported", "mean_partners", "inferred_partners"] and len(t) == 3
    assert t["p_present"].tolist() == [1.0, 2.0 / 3.0, 0.0] and t["p_supported"].tolist()[:2] == [1.0, 0.0] and np.isnan(t["p_supported"][2])
    assert t["mean_partners"].tolist()[:2] == [5.0 / 3.0, 0.0] and t["inferred_partners"].tolist() == [2, -1, -1]
    b = sp.bridges(0.5)
    assert len(b) == 1 and (b["i"][0], b["j"][0]) == (2, 3) and len(sp.bridges(0.9)) == 0
    f = sp.frame()
    assert len(f) == 2 * 4 and f["pooled"].sum() == 2 and f["inferred"].tolist()[:4] == [1, 2, 1, 0] and f["mean"][0] == 1.0
    assert len(sp.summary()) == 2 * len(sp.statistics()) and "q0.5" in sp.summary().columns
    with pytest.raises(ValueError, match="nodes=True"):
        sp.node_support()


def test_shared_partners_gwesp_and_its_refusal():
    from vimure_amd.partners import SharedPartners, gwesp_of
    sp = _hand_made()
    assert np.array_equal(sp.gwesp(0.0), sp.totals[..., 1].astype(float))                     # decay 0: the supported ties
    d = 0.7
    w = np.exp(d) * (1 - (1 - np.exp(-d)) ** np.arange(4))
    assert np.allclose(sp.gwesp(d), sp.hist @ w, rtol=1e-15) and np.allclose(gwesp_of([0, 1, 0], 50.0), 1.0) and np.allclose(gwesp_of([0, 0, 1], 50.0), 2.0)
    hist = sp.hist.copy()
    hist[2, 0] = [1, 0, 0, 3]
    totals = sp.totals.copy()
    totals[2, 0] = [4, 3, 27, 11]
    pooled = SharedPartners(5, "union", hist, totals)
    with pytest.raises(ValueError, match="n_bins >= 13"):
        pooled.gwesp(d)
    with pytest.raises(ValueError, match="ties='inferred'"):
        pooled.ties_frame()
    with pytest.raises(ValueError, match="mode"):
        SharedPartners(5, "either", hist, totals)


def test_node_support():
    from vimure_amd.partners import SharedPartners
    nt = np.array([[[2, 1, 0]], [[2, 3, 0]]], np.int32)
    ns = np.array([[[1, 1, 0]], [[1, 0, 0]]], np.int32)
    sp = SharedPartners(3, "path", np.zeros((2, 1, 2), np.int64), np.zeros((2, 1, 4), np.int64), node_ties=nt, node_supported=ns)
    got = sp.node_support()
    assert got.shape == (1, 3) and got[0, :2].tolist() == [0.5, 0.25] and np.isnan(got[0, 2])
    assert TOTALS == ("ties", "supported", "partners", "max_partners")
