"""Host side of the reporter influence (no GPU): `influence.influence_np` against the oracle's `update_rho` on the problem with one
mask entry cleared -- the claim the feature rests on -- the structural cases (a row of zeros, a zero category, both flips, K = 2),
the argument errors, `ReporterInfluence.frame()`, and the top-n selection from a hand-made histogram."""
import copy

import numpy as np
import pytest
from scipy.special import psi


def _tables(st, mutuality):
    g_nu = float(np.exp(psi(st.nu_shp) - np.log(st.nu_rte))) if mutuality else 0.0
    return (st.gamma_shp / st.gamma_rte, psi(st.gamma_shp) - np.log(st.gamma_rte), st.phi_shp / st.phi_rte,
            psi(st.phi_shp) - np.log(st.phi_rte), g_nu)


@pytest.mark.parametrize("mutuality", [True, False])
def test_restatement_against_the_oracle_with_one_mask_entry_cleared(mutuality):
    from oracle import vimure_oracle as vo
    from vimure_amd.influence import influence_np
    g = np.random.RandomState(5)
    L, N, M, K = 2, 7, 5, 3
    R = (g.rand(L, N, N, M) < 0.6).astype(np.uint8)
    X = ((g.rand(L, N, N, M) < 0.4) * g.randint(1, K + 1, (L, N, N, M))).astype(np.int64) * R
    pb = vo.Problem(X, R, K, mutuality, vo.make_priors(L, M, K))
    st = vo.init_state(pb, np.random.RandomState(11))
    for _ in range(3):
        vo.cavi_step(pb, st)
    vo.update_rho(pb, st)                                       # rho is now the update's output for the tables of st
    tabs = _tables(st, mutuality)
    al = influence_np(st.rho, X, R, *tabs, mutuality=mutuality, select="none", min_tv=0.0)
    n = len(al["l"])
    assert n == int(R.sum()) and al["q"].shape == (n, K)
    worst = 0.0
    picks = g.choice(n, 40, replace=False)
    assert (al["x"][picks] > 0).sum() >= 5 and (al["x"][picks] == 0).sum() >= 5
    for e in picks:
        l, i, j, m = (int(al[c][e]) for c in "lijm")
        X2, R2 = X.copy(), R.copy()
        X2[l, i, j, m] = R2[l, i, j, m] = 0
        pb2, st2 = vo.Problem(X2, R2, K, mutuality, pb.priors), copy.deepcopy(st)
        vo.update_rho(pb2, st2)
        worst = max(worst, float(np.abs(st2.rho[l, i, j] - al["q"][e]).max()))
        assert abs(al["prob_loo"][e] - st2.rho[l, i, j, 1:].sum()) <= 1e-12
        assert abs(al["tv"][e] - 0.5 * np.abs(st2.rho[l, i, j] - st.rho[l, i, j]).sum()) <= 1e-12
    print(f"mutuality {mutuality}: worst |update_rho row - q| over 40 elements = {worst:.3e}")
    assert worst <= 1e-12
    assert al["tv"].max() > 1e-3                                 # the rows do move


def _case(K=3):
    """2 x 6 x 6 x 4: a partial mask with an empty row, a row of zeros, a zero category, and rows near the readout's boundary."""
    g = np.random.RandomState(21)
    L, N, M = 2, 6, 4
    X = ((g.rand(L, N, N, M) < 0.4) * g.randint(1, 4, (L, N, N, M))).astype(np.int64)
    R = (g.rand(L, N, N, M) < 0.7).astype(np.uint8)
    R[0, 0, 0] = 0
    R[0, 1, 2] = R[1, 3, 4] = 1
    rho = g.rand(L, N, N, K) + 0.05
    rho = rho / rho.sum(-1, keepdims=True)
    rho[0, 1, 2] = 0.0                                           # a row of zeros, one the engine keeps
    if K > 2:
        rho[:, ::2, 1::2, 1] = 0.0                               # a zero category
        rho[:, ::2, 1::2] /= rho[:, ::2, 1::2].sum(-1, keepdims=True).clip(1e-300)
    gs, gr = g.gamma(2.0, 1.0, (L, M)) + 0.5, g.gamma(2.0, 1.0, (L, M)) + 0.5
    ps, pr = g.gamma(5.0, 1.0, (L, K)) + 0.5, g.gamma(2.0, 1.0, (L, K)) + 0.5
    ps.sort(axis=1)
    tabs = (gs / gr, psi(gs) - np.log(gr), ps / pr, psi(ps) - np.log(pr), 0.2)
    return X, R, rho, tabs


def test_structural_cases():
    from vimure_amd.influence import influence_np
    X, R, rho, tabs = _case()
    al = influence_np(rho, X, R, *tabs, select="none", min_tv=0.0)
    n = len(al["l"])
    assert n == int(R.sum()) == al["counts"][:, :, 0].sum() == al["counts"][:, :, 3].sum()
    assert np.array_equal(al["counts"][:, :, 0], R.sum(axis=(1, 2)))
    assert np.lexsort((al["m"], al["j"], al["i"], al["l"])).tolist() == list(range(n))     # lexicographic order
    assert np.array_equal(al["x"], X[al["l"], al["i"], al["j"], al["m"]]) and np.array_equal(al["xt"], X[al["l"], al["j"], al["i"], al["m"]])
    # a row of zeros gives q = 0, tv = 0, no flip
    z = (al["l"] == 0) & (al["i"] == 1) & (al["j"] == 2)
    assert z.sum() == 4 and not al["q"][z].any() and not al["tv"][z].any() and not al["lost"][z].any() and not al["gained"][z].any()
    # a zero category stays zero; every other row is a distribution
    r = rho[al["l"], al["i"], al["j"]]
    assert (r == 0).any() and not al["q"][r == 0].any()
    assert np.allclose(al["q"][~z].sum(axis=1), 1.0, rtol=0, atol=1e-14)
    assert (al["tv"] >= 0).all() and (al["tv"] <= 1.0).all()
    # both flips occur, and they are what the readouts say
    y, yq = np.argmax(r, axis=1), np.argmax(al["q"], axis=1)
    assert al["lost"].sum() > 0 and al["gained"].sum() > 0
    assert np.array_equal(al["lost"], (y > 0) & (yq == 0)) and np.array_equal(al["gained"], (y == 0) & (yq > 0))
    assert al["counts"][:, :, 1].sum() == al["lost"].sum() and al["counts"][:, :, 2].sum() == al["gained"].sum()
    # the flag rule: flips by select, or tv >= min_tv
    cut = float(np.median(al["tv"]))
    for select, bits in (("none", 0), ("lost", 1), ("gained", 2), ("both", 3)):
        got = influence_np(rho, X, R, *tabs, select=select, min_tv=cut)
        want = (al["lost"] & bool(bits & 1)) | (al["gained"] & bool(bits & 2)) | (al["tv"] >= cut)
        assert len(got["l"]) == want.sum() == got["counts"][:, :, 3].sum()
        assert np.array_equal(got["tv"], al["tv"][want]) and np.array_equal(got["m"], al["m"][want])
    only = influence_np(rho, X, R, *tabs, select="both")          # min_tv = +inf: flips only
    assert len(only["l"]) == (al["lost"] | al["gained"]).sum() and (only["lost"] | only["gained"]).all()
    # sums, histogram, one layer
    assert np.isclose(al["sums"][:, :, 0].sum(), al["tv"].sum()) and np.isclose(al["sums"][:, :, 1].sum(), (al["prob_loo"] - al["prob"]).sum())
    ed = np.array([0.0, cut, cut, 2.0])
    h = influence_np(rho, X, R, *tabs, edges=ed)["hist"]
    assert h.shape == (2, 5, 2) and h.sum() == n and h[:, 0].sum() == 0 and h[:, 2].sum() == 0
    assert h[:, 3:].sum() == (al["tv"] >= cut).sum() and h[:, :, 0].sum() == (al["x"] > 0).sum()
    one = influence_np(rho, X, R, *tabs, select="none", min_tv=0.0, layer=1)
    w = al["l"] == 1
    assert one["counts"].shape == (1, 4, 4) and np.array_equal(one["counts"][0], al["counts"][1])
    assert np.array_equal(one["tv"], al["tv"][w]) and (one["l"] == 1).all() and one["layers"].tolist() == [1]
    # the threshold readout
    thr = influence_np(rho, X, R, *tabs, method="threshold", threshold=0.3, select="none", min_tv=0.0)
    assert np.array_equal(thr["lost"], (r[:, 1] >= 0.3) & (thr["q"][:, 1] < 0.3))
    # mutuality off: no mirror count enters
    off = influence_np(rho, X, R, *tabs, mutuality=False, select="none", min_tv=0.0)
    assert not off["xt"].any() and not np.array_equal(off["tv"], al["tv"])


def test_two_categories_prob_is_rho_1():
    from vimure_amd.influence import influence_np
    X, R, rho, tabs = _case(K=2)
    al = influence_np(rho, X, R, *tabs, select="none", min_tv=0.0)
    r = rho[al["l"], al["i"], al["j"]]
    assert np.array_equal(al["prob"].view(np.uint64), np.ascontiguousarray(r[:, 1]).view(np.uint64))
    assert np.array_equal(al["prob_loo"].view(np.uint64), np.ascontiguousarray(al["q"][:, 1]).view(np.uint64))


def test_argument_errors():
    from vimure_amd import VimureModel
    from vimure_amd.influence import InfluenceArgumentError, influence_np, method_code, select_code, sum_quantum
    X, R, rho, tabs = _case()
    bad = [dict(select="all"), dict(select=4), dict(min_tv=float("nan")), dict(min_tv=-0.1), dict(method="rho_mean"), dict(method=1),
           dict(layer=2), dict(edges=[0.5, 0.4]), dict(edges=[0.1, np.inf])]
    for kw in bad:
        with pytest.raises(InfluenceArgumentError):
            influence_np(rho, X, R, *tabs, **kw)
    for q, v in ((0, -1.0), (1, np.inf), (2, np.nan), (3, -np.inf)):
        t = [np.array(a, dtype=np.float64) for a in tabs[:4]]
        t[q][0, 1] = v
        with pytest.raises(InfluenceArgumentError):
            influence_np(rho, X, R, *t, tabs[4])
    with pytest.raises(InfluenceArgumentError):
        influence_np(rho, X, R, *tabs[:4], -0.5)
    with pytest.raises(InfluenceArgumentError):
        influence_np(rho, X, R, tabs[0][:1], *tabs[1:])
    assert issubclass(InfluenceArgumentError, ValueError)
    assert [select_code(s) for s in ("none", "lost", "gained", "both")] == [0, 1, 2, 3] and method_code("threshold") == 2
    nan_rho = rho.copy()
    nan_rho[1, 3, 4, 0] = np.nan
    with pytest.raises(ValueError, match="NaN") as ei:
        influence_np(nan_rho, X, R, *tabs)
    assert not isinstance(ei.value, InfluenceArgumentError)
    assert sum_quantum(7) == 2.0 ** -55 and sum_quantum(8) == 2.0 ** -55 and sum_quantum(9) == 2.0 ** -54 and sum_quantum(1) == 2.0 ** -61
    m = VimureModel()
    for kw in (dict(top=3, min_shift=0.1), dict(select="all"), dict(top=0), dict(min_shift=-1.0), dict()):
        with pytest.raises(ValueError):
            m.reporter_influence(**kw)                            # (the last: not fitted)


def test_frame_rows_and_fragile_ties():
    from vimure_amd.influence import ReporterInfluence, influence_np, top_rows
    X, R, rho, tabs = _case()
    res = influence_np(rho, X, R, *tabs, select="both", min_tv=0.2, edges=[0.1, 0.2])
    ri = ReporterInfluence(res)
    f = ri.frame()
    assert list(f.columns) == ["layer", "reporter", "n_scope", "lost", "gained", "flagged", "mean_tv", "mean_shift"]
    assert len(f) == 2 * 4 and f["layer"].tolist() == [0] * 4 + [1] * 4 and f["reporter"].tolist() == list(range(4)) * 2
    assert np.array_equal(f["n_scope"], res["counts"][:, :, 0].ravel()) and np.array_equal(f["lost"], res["counts"][:, :, 1].ravel())
    assert np.allclose(f["mean_tv"] * f["n_scope"], res["sums"][:, :, 0].ravel()) and (f["mean_tv"] >= 0).all()
    assert np.allclose(f["mean_shift"] * f["n_scope"], res["sums"][:, :, 1].ravel())
    r = ri.rows()
    assert list(r.columns) == ["layer", "source", "target", "reporter", "x", "x_mirror", "prob", "prob_loo", "shift", "tv", "lost", "gained"]
    assert len(r) == len(ri) == res["counts"][:, :, 3].sum() and np.array_equal(r["shift"], res["prob_loo"] - res["prob"])
    frag = ri.fragile_ties()
    assert len(frag) == res["counts"][:, :, 1].sum() > 0 and frag["lost"].all() and (frag["shift"] < 0).all()
    assert ri.summary()["lost"] == len(frag) and ri.hist.shape == (2, 3, 2)
    t = top_rows(res, 5)
    assert len(t["tv"]) == 5 and np.array_equal(t["tv"], np.sort(res["tv"])[::-1][:5]) and set(t) == set(r_ for r_ in res if r_ in t)
    bare = ReporterInfluence({k: v for k, v in res.items() if k not in ("l", "lost", "gained")})
    with pytest.raises(ValueError, match="rows"):
        bare.rows()
    no_marks = ReporterInfluence({k: v for k, v in res.items() if k not in ("lost", "gained")})
    with pytest.raises(ValueError, match="marks"):
        no_marks.fragile_ties()


def test_top_selection_on_a_hand_made_histogram():
    from vimure_amd.influence import GRID_EDGES, grid_edges, min_tv_for_top
    ed = grid_edges()
    assert len(ed) == GRID_EDGES == 4096 and ed[0] == 0.0 and ed[1] == 2.0 ** -12 and ed[-1] == 1.0 - 2.0 ** -12
    edges = np.array([0.0, 0.25, 0.5, 0.75])
    hist = np.zeros((2, 5, 2), np.int64)                          # bin c: exactly c edges <= tv
    hist[0, 1] = [10, 20]                                         # tv in [0, 0.25)
    hist[1, 2] = [3, 0]                                           # [0.25, 0.5)
    hist[0, 3] = [1, 1]                                           # [0.5, 0.75)
    hist[1, 4] = [0, 2]                                           # [0.75, ..)
    assert min_tv_for_top(hist, edges, 1) == (0.75, 2)
    assert min_tv_for_top(hist, edges, 2) == (0.75, 2)
    assert min_tv_for_top(hist, edges, 3) == (0.5, 4)
    assert min_tv_for_top(hist, edges, 5) == (0.25, 7)
    assert min_tv_for_top(hist, edges, 8) == (0.0, 37)
    assert min_tv_for_top(hist, edges, 1000) == (0.0, 37)        # more than there are: everything
    with pytest.raises(ValueError, match="max_rows"):
        min_tv_for_top(hist, edges, 8, max_rows=10)
    with pytest.raises(ValueError, match="top"):
        min_tv_for_top(hist, edges, 0)
