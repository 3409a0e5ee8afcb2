"""Host side of the report scores (no GPU): `residuals.report_scores_np` against a from-scratch loop with `math.lgamma` and a direct
sum of Poisson pmfs, the histogram and flag conventions at an edge, `ReportScores.frame()`, the argument errors of
`VimureModel.surprising_reports`, and the top-n selection from a hand-made histogram."""
import math

import numpy as np
import pytest


def _case():
    """1 x 5 x 5 x 3, K = 3: a zero rho category on some ties, theta[0, 1] = 0 with positive counts of reporter 1 (one of them
    without a mirrored count: logp = -inf with mutuality on or off), a partial mask."""
    g = np.random.RandomState(12)
    L, N, M, K = 1, 5, 3, 3
    X = ((g.rand(L, N, N, M) < 0.45) * g.randint(1, 4, (L, N, N, M))).astype(np.int64)
    X[0, 1, 2, 1], X[0, 2, 1, 1] = 2, 0          # reporter 1 (theta = 0): a count against no mirrored count ...
    X[0, 3, 4, 1], X[0, 4, 3, 1] = 1, 3          # ... and one against a mirrored count (finite with mutuality)
    R = (g.rand(L, N, N, M) < 0.8).astype(np.uint8)
    R[0, 1, 2, 1] = R[0, 3, 4, 1] = R[0, 4, 3, 1] = 1
    R[0, 0, 0] = 0                               # an empty row
    rho = g.rand(L, N, N, K) + 0.05
    rho[0, ::2, 1::2, 1] = 0.0                   # a zero category
    rho[0, 1, 2] = [0.2, 0.0, 0.8]
    rho = rho / rho.sum(-1, keepdims=True)
    theta = g.gamma(2.0, 0.5, (L, M)) + 0.1
    theta[0, 1] = 0.0
    lam = g.gamma(2.0, 1.0, (L, K)) + 0.1
    return X, R, rho, theta, lam, 0.35


def _loop(X, R, rho, theta, lam, eta, mutuality):
    """(subs, x, xt, logp, mean) over the support in lexicographic order, element by element: p = sum_k rho_k Poisson(x; mu_k)."""
    L, N, _, M = X.shape
    rows = []
    for l in range(L):
        for i in range(N):
            for j in range(N):
                for m in range(M):
                    if R is not None and not R[l, i, j, m]:
                        continue
                    x = int(X[l, i, j, m])
                    xt = int(X[l, j, i, m]) if mutuality else 0
                    p = mean = 0.0
                    for k in range(rho.shape[-1]):
                        mu = theta[l, m] * lam[l, k] + eta * xt
                        mean += rho[l, i, j, k] * mu
                        pmf = (1.0 if x == 0 else 0.0) if mu == 0.0 else math.exp(x * math.log(mu) - mu - math.lgamma(x + 1.0))
                        p += rho[l, i, j, k] * pmf
                    rows.append((l, i, j, m, x, xt, math.log(p) if p > 0.0 else -math.inf, mean))
    return [np.array(c) for c in zip(*rows)]


@pytest.mark.parametrize("mutuality", [True, False])
def test_restatement_against_a_loop(mutuality):
    from vimure_amd.residuals import report_scores_np
    X, R, rho, theta, lam, eta = _case()
    eta = eta if mutuality else 0.0
    l, i, j, m, x, xt, logp, mean = _loop(X, R, rho, theta, lam, eta, mutuality)
    s = -logp
    fin = np.sort(s[np.isfinite(s)])
    n_inf = int((logp == -np.inf).sum())
    assert n_inf >= (1 if mutuality else 2) and x[logp == -np.inf].min() > 0           # the zero theta against x > 0
    assert (rho == 0.0).any()
    gaps = np.diff(fin)
    at = int(np.argmax(gaps[len(fin) // 2:])) + len(fin) // 2                          # a wide gap in the upper half
    thr = 0.5 * (fin[at] + fin[at + 1])
    wide = np.flatnonzero(gaps > 1e-3)                                                 # no edge inside a cluster of near-equal values
    edges = np.array([0.5 * (fin[q] + fin[q + 1]) for q in (wide[0], wide[len(wide) // 3], at)])
    assert (np.diff(edges) > 0).all() and gaps[at] > 1e-3
    for select, code in (("both", 3), ("reports", 1), ("omissions", 2)):
        got = report_scores_np(rho, X, R, theta, lam, eta, thr, select, edges, mutuality)
        cls = (x == 0).astype(int)
        flag = (s >= thr) & (((code & 1) != 0) & (cls == 0) | ((code & 2) != 0) & (cls == 1))
        assert got["counts"][0].tolist() == [len(x), int((x > 0).sum()), n_inf, int(flag.sum())]
        for name, col in zip(("l", "i", "j", "m", "x", "xt"), (l, i, j, m, x, xt)):
            assert np.array_equal(got[name], col[flag]), name
        assert np.array_equal(got["logp"] == -np.inf, logp[flag] == -np.inf)
        f = np.isfinite(got["logp"])
        assert np.allclose(got["logp"][f], logp[flag][f], rtol=0, atol=1e-12) and np.allclose(got["mean"], mean[flag], rtol=1e-13)
        hist = np.zeros((1, len(edges) + 1, 2), np.int64)
        for q in range(len(x)):
            hist[0, int((edges <= s[q]).sum()), cls[q]] += 1
        assert np.array_equal(got["hist"], hist) and got["hist"].sum() == len(x) and got["hist"][0, -1].sum() >= n_inf
        rep = np.zeros((1, X.shape[3], 2), np.int64)
        for q in np.flatnonzero(flag):
            rep[0, m[q], cls[q]] += 1
        assert np.array_equal(got["by_reporter"], rep)
        assert np.isclose(got["sums"][0, 0], logp[np.isfinite(logp)].sum(), rtol=1e-12)
        assert np.allclose(got["sums"][0, 1:], [((x - mean) ** 2).sum(), x.sum(), mean.sum()], rtol=1e-12)
    only_inf = report_scores_np(rho, X, R, theta, lam, eta, np.inf, "both", None, mutuality)
    assert only_inf["counts"][0, 3] == n_inf == len(only_inf["l"]) and (only_inf["logp"] == -np.inf).all()
    assert only_inf["hist"] is None
    assert report_scores_np(rho, X, R, theta, lam, eta, np.inf, "omissions", None, mutuality)["counts"][0, 3] == 0
    everything = report_scores_np(rho, X, None, theta, lam, eta, -1.0, "both", None, mutuality)    # no mask: the diagonal included
    assert everything["counts"][0, 0] == X.size == len(everything["l"])


def test_conventions_at_an_edge():
    """s == edges[tau] counts as edges[tau] <= s; s == threshold is flagged."""
    from vimure_amd.crossval import counts_at, heldout_loglik_np, mirror_counts, support
    from vimure_amd.residuals import report_scores_np
    X, R, rho, theta, lam, eta = _case()
    sup = support(X, R)
    x = counts_at(X, sup)
    s = -heldout_loglik_np(rho, sup, x, mirror_counts(X, sup), theta, lam, eta)[0]
    fin = np.unique(s[np.isfinite(s)])
    v = float(fin[len(fin) // 2])                               # a value some element has, exactly
    got = report_scores_np(rho, X, R, theta, lam, eta, v, "both", [v, v], True)
    assert got["counts"][0, 3] == int((s >= v).sum()) and v in (-got["logp"]).tolist()
    assert got["hist"][0, 2].sum() == int((s >= v).sum()) and got["hist"][0, 1].sum() == 0       # a doubled edge: an empty bin
    assert got["hist"][0, 0].sum() == int((s < v).sum())
    above = report_scores_np(rho, X, R, theta, lam, eta, np.nextafter(v, np.inf), "both", [np.nextafter(v, np.inf)], True)
    assert above["counts"][0, 3] == int((s > v).sum()) < got["counts"][0, 3]
    assert above["hist"][0, 1].sum() == int((s > v).sum())
    for bad in (np.nan, -np.inf):
        with pytest.raises(ValueError, match="threshold"):
            report_scores_np(rho, X, R, theta, lam, eta, bad)
    with pytest.raises(ValueError, match="edges"):
        report_scores_np(rho, X, R, theta, lam, eta, 1.0, "both", [2.0, 1.0])
    with pytest.raises(ValueError, match="select"):
        report_scores_np(rho, X, R, theta, lam, eta, 1.0, "all")


def test_frame_columns_and_ordering():
    from vimure_amd.residuals import ReportScores, report_scores_np, top_rows
    X, R, rho, theta, lam, eta = _case()
    res = report_scores_np(rho, X, R, theta, lam, eta, 1.0, "both", [0.0, 1.0, 2.0], True)
    rs = ReportScores(res)
    f = rs.frame()
    assert list(f.columns) == ["layer", "source", "target", "reporter", "x", "x_mirror", "logp", "surprise", "expected", "residual"]
    assert len(f) == len(rs) == rs.n_flagged == res["counts"][0, 3] > 3
    key = f[["layer", "source", "target", "reporter"]].to_numpy()
    assert (np.diff(np.ravel_multi_index(key.T, X.shape)) > 0).all()                  # lexicographic, no repeats
    assert np.array_equal(f["surprise"], -f["logp"]) and (f["surprise"] >= 1.0).all()
    assert np.array_equal(f["residual"], f["x"] - f["expected"])
    assert np.array_equal(f["x"], X[tuple(key.T)]) and np.array_equal(f["x_mirror"], X[key[:, 0], key[:, 2], key[:, 1], key[:, 3]])
    rep = rs.reporters()
    assert list(rep.columns) == ["layer", "reporter", "flagged_reports", "flagged_omissions", "flagged"] and len(rep) == X.shape[3]
    assert rep["flagged"].sum() == len(f) and rep["flagged_reports"].sum() == int((f["x"] > 0).sum())
    assert rs.lppd.shape == (1,) and rs.lppd[0] == res["sums"][0, 0]
    assert np.isclose(rs.lppd_per_element[0], res["sums"][0, 0] / (res["counts"][0, 0] - res["counts"][0, 2]))
    assert np.array_equal(rs.hist, res["hist"]) and rs.edges.tolist() == [0.0, 1.0, 2.0]
    # the top rows: by surprise (the -inf logp first), then by subscripts
    top = ReportScores({**res, **top_rows(res, 4)}).frame()
    want = f.sort_values(["surprise", "layer", "source", "target", "reporter"], ascending=[False, True, True, True, True], kind="stable").head(4)
    assert np.array_equal(top.to_numpy(), want.to_numpy()) and top["surprise"].iloc[0] == np.inf
    with pytest.raises(ValueError, match="rows"):
        ReportScores({**res, "l": None}).frame()


def test_top_n_selection_from_a_histogram():
    from vimure_amd.residuals import GRID_EDGES, grid_edges, threshold_for_top
    edges = np.array([0.0, 1.0, 2.0, 3.0])
    hist = np.zeros((2, 5, 2), np.int64)
    hist[0, :, 0] = [0, 10, 4, 2, 1]      # reports of layer 0: 1 with s >= 3, 3 with s >= 2, 7 with s >= 1, 17 in all
    hist[1, :, 1] = [0, 100, 5, 0, 2]     # omissions of layer 1: 2, 2, 7, 107
    assert threshold_for_top(hist, edges, 3, "reports") == (2.0, 3)
    assert threshold_for_top(hist, edges, 3, "both") == (3.0, 3)
    assert threshold_for_top(hist, edges, 4, "both") == (2.0, 5)
    assert threshold_for_top(hist, edges, 3, "omissions") == (1.0, 7)
    assert threshold_for_top(hist, edges, 1, "omissions") == (3.0, 2)
    assert threshold_for_top(hist, edges, 18, "reports") == (0.0, 17)        # fewer selected elements than asked for: all of them
    assert threshold_for_top(hist, edges, 124, "both") == (0.0, 124)
    assert threshold_for_top(hist, edges, 100, "both", max_rows=124) == (0.0, 124)
    with pytest.raises(ValueError, match="124 elements"):
        threshold_for_top(hist, edges, 100, "both", max_rows=123)
    with pytest.raises(ValueError, match="7 elements"):
        threshold_for_top(hist, edges, 6, "omissions", max_rows=6)
    with pytest.raises(ValueError, match="top"):
        threshold_for_top(hist, edges, 0)
    g = grid_edges()
    assert len(g) == GRID_EDGES == 4096 and g[0] == 0.0 and g[1] == 1.0 / 64.0 and g[-1] == 4095.0 / 64.0


class _FakeEngine:
    """Stands in for the engine of a fitted model: a hand-made histogram for the aggregates-only call."""

    def __init__(self, hist):
        self.hist, self.calls = hist, []

    def report_scores(self, theta, lam, eta, threshold, **kw):
        self.calls.append((threshold, kw))
        if kw.get("rows", True):
            raise AssertionError("the table must not be fetched")
        return {"hist": self.hist, "edges": kw["edges"]}


def test_surprising_reports_argument_errors():
    from vimure_amd import VimureModel
    from vimure_amd.residuals import GRID_EDGES
    m = VimureModel()
    for kw in (dict(top=5, threshold=1.0), dict(top=None), dict(threshold=2.0)):          # (the default top=100 beside a threshold)
        with pytest.raises(ValueError, match="exactly one"):
            m.surprising_reports(**kw)
    with pytest.raises(ValueError, match="select"):
        m.surprising_reports(top=5, select="everything")
    with pytest.raises(ValueError, match="top"):
        m.surprising_reports(top=0)
    with pytest.raises(ValueError, match="not been fitted"):
        m.surprising_reports(top=5)
    with pytest.raises(ValueError, match="not been fitted"):
        m.surprising_reports(top=None, threshold=3.0)
    # a fitted model whose level of the top rows holds too many: refused before the table is fetched
    m.L, m.N, m.M, m.K = 1, 4, 2, 2
    m.gamma_shp_f = m.gamma_rte_f = np.ones((1, 2))
    m.phi_shp_f = m.phi_rte_f = np.ones((1, 2))
    m.nu_shp_f = m.nu_rte_f = 1.0
    hist = np.zeros((1, GRID_EDGES + 1, 2), np.int64)
    hist[0, 65, 0], hist[0, 10, 1] = 50, 1000            # 50 reports with a surprise in [1, 1 + 1/64), 1000 omissions below
    m._engine = _FakeEngine(hist)
    with pytest.raises(ValueError, match="1050 elements"):
        m.surprising_reports(top=60, max_rows=500)
    with pytest.raises(ValueError, match="50 elements"):
        m.surprising_reports(top=10, max_rows=49)
    assert len(m._engine.calls) == 2 and all(c[0] == np.inf and not c[1]["rows"] for c in m._engine.calls)
    with pytest.raises(ValueError, match="layer"):
        m.surprising_reports(top=10, layer=1)
    m._engine = None
