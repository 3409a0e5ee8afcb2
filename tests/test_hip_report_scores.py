"""GPU: every report of the support scored under the posterior (vmr_report_scores) against its NumPy restatement
(`residuals.report_scores_np`), with the state set from the golden fits (the `fit_*_f` arrays) or from synthetic arrays.

Exact: `counts`, `hist`, `by_reporter`, and the set and order of the flagged rows with their x and xt.  What makes exactness fair:
on the reference scores the test puts the threshold and every histogram edge at the MIDPOINT OF A GAP between consecutive
distinct values, and asserts about its own inputs that the gap is at least 1000 times the logp bound of both neighbours
(tests/heldout_util.py: C_LOGP 2^-52 T) -- no element is borderline and none is excluded.  Floating point: logp and mean of the
rows -- of EVERY element, through a second call with a threshold below every score -- and the sums within the bounds of
tests/heldout_util.py (`compare_entries`, `compare_sums`), which print the worst ratios.  Two calls give the same bits; the size
call gives the row count; a table one row short is refused with nothing written; rows=False gives the same aggregates; and
`heldout_loglik` over the flagged rows returns the same logp bits with every entry inside the mask: one definition, two entry points."""
import warnings

import numpy as np
import pytest

from tests.golden_util import case_config, load_case
from tests.heldout_util import C_LOGP, U, compare_entries, compare_sums, term_size

pytestmark = pytest.mark.gpu

PRI = (0.1, 0.1, 10.0, 10.0, 0.5, 1.0)
GAP_RULE = 1000.0
ROWS = ("l", "i", "j", "m", "x", "xt")


def _golden(name):
    d = load_case(name)
    K, mut, _, _, _, _, _ = case_config(d)
    X, R = np.asarray(d["X"]), np.asarray(d["R"])
    st = (d["fit_gamma_shp_f"], d["fit_gamma_rte_f"], d["fit_phi_shp_f"], d["fit_phi_rte_f"], float(d["fit_nu_shp_f"]),
          float(d["fit_nu_rte_f"]), np.ascontiguousarray(d["fit_rho_f"]))
    theta, lam = st[0] / st[1], st[2] / st[3]
    eta = st[4] / st[5] if mut else 0.0
    return dict(X=X, R=None if R.all() else R, K=K, mut=mut, st=st, rho=st[6], theta=theta, lam=lam, eta=eta)


def _synthetic(seed, L, N, M, K, density, x_rate=0.2, big=None):
    g = np.random.RandomState(seed)
    X = ((g.rand(L, N, N, M) < x_rate) * g.randint(1, 5, (L, N, N, M))).astype(np.int64)
    R = None
    if density is not None:
        R = (g.rand(L, N, N, M) < density).astype(np.uint8)
        R[:, 2] = 0                               # empty rows
        R[:, 3], R[0, :, 5] = 1, 1                # rows made all ones
    if big is not None:
        X[big[0]] = big[1]
        if R is not None:
            R[big[0]] = 1
    rho = g.rand(L, N, N, K)
    rho[..., 0] *= 4.0
    if K > 2:
        rho[:, ::3, 1::2, K - 2] = 0.0            # a zero category
    rho = np.ascontiguousarray(rho / rho.sum(-1, keepdims=True))
    gs, gr = g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(2.0, 1.0, (L, M)) + 0.1
    ps, pr = g.gamma(5.0, 1.0, (L, K)) + 0.1, g.gamma(2.0, 1.0, (L, K)) + 0.1
    theta, lam = g.gamma(2.0, 0.5, (L, M)) + 0.05, np.sort(g.gamma(2.0, 1.0, (L, K)) + 0.05, axis=1)
    return dict(X=X, R=R, K=K, mut=True, st=(gs, gr, ps, pr, 3.0, 2.5, rho), rho=rho, theta=theta, lam=lam, eta=0.3)


def _engine(c, coo=False):
    from vimure_amd import CaviEngine
    X, R = c["X"], c["R"]
    if coo:
        xs = np.nonzero(X)
        eng = CaviEngine.from_coo(xs, X[xs], X.shape, R=None if R is None else np.nonzero(R), K=c["K"], mutuality=c["mut"])
    else:
        eng = CaviEngine(X.astype(np.uint8), R, K=c["K"], mutuality=c["mut"])
    eng.set_priors(*PRI)
    eng.set_state(*c["st"])
    return eng


def _reference(c):
    """Every element of the support scored by the restatement, the bound of every logp, and the gaps of the distinct scores that
    satisfy the rule: (all, want, T, gaps) with gaps = [(midpoint, width, index into the distinct values)]."""
    from vimure_amd.crossval import heldout_loglik_np
    from vimure_amd.residuals import report_scores_np
    if "ref" in c:
        return c["ref"]
    al = report_scores_np(c["rho"], c["X"], c["R"], c["theta"], c["lam"], c["eta"], -1e300, "both", None, c["mut"])
    subs = tuple(al[k] for k in "lijm")
    xt = al["xt"] if c["mut"] else None
    want = heldout_loglik_np(c["rho"], subs, al["x"], xt, c["theta"], c["lam"], c["eta"], R=c["R"])
    assert np.array_equal(want[0], al["logp"]) and not np.isnan(want[0]).any()
    T = term_size(c["rho"], subs, al["x"], xt, c["theta"], c["lam"], c["eta"])
    s = -al["logp"]
    fin = np.isfinite(s)
    vals, inv = np.unique(s[fin], return_inverse=True)
    bound = np.zeros(len(vals))
    np.maximum.at(bound, inv, C_LOGP * U * T[fin])                     # the widest bound among the elements that share a value
    width = np.diff(vals)
    ok = width >= GAP_RULE * np.maximum(bound[:-1], bound[1:])
    gaps = [(0.5 * (vals[q] + vals[q + 1]), width[q], q) for q in np.flatnonzero(ok)]
    c["ref"] = (al, want, T, gaps, vals)
    return c["ref"]


def _pick(c, n_edges=9):
    """The threshold -- the midpoint of the qualifying gap nearest to the 98 % quantile of the elements' scores, so that about one
    element in fifty is flagged -- and edges at qualifying gaps spread over the distinct values."""
    al, _, _, gaps, vals = _reference(c)
    assert len(gaps) >= n_edges, (len(gaps), len(vals))
    s = -al["logp"]
    q98 = float(np.quantile(s[np.isfinite(s)], 0.98))
    thr = min(gaps, key=lambda g: abs(g[0] - q98))
    assert vals[0] < thr[0] < vals[-1]
    edges = sorted({gaps[int(round(p * (len(gaps) - 1)))][0] for p in np.linspace(0.0, 1.0, n_edges)} | {thr[0]})
    print(f"threshold {thr[0]:.6f} in a gap of {thr[1]:.3e} nat; {len(edges)} edges, narrowest gap "
          f"{min(g[1] for g in gaps if g[0] in edges):.3e}; {len(vals)} distinct scores, {len(gaps)} gaps satisfy the rule")
    return float(thr[0]), np.array(edges)


def _slice(res, layer):
    """A result of all layers cut to one: the aggregates' row, the rows of that layer."""
    if layer is None:
        return res
    w = res["l"] == layer
    out = {k: (v[layer:layer + 1] if k in ("counts", "sums", "hist", "by_reporter") and v is not None else v) for k, v in res.items()}
    out.update({k: res[k][w] for k in ROWS + ("logp", "mean")})
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check(eng, c, what, threshold=None, select="both", layer=None):
    from vimure_amd.engine import ReportScoresArgumentError
    from vimure_amd.residuals import report_scores_np
    K = c["K"]
    al, want_all, T, _, _ = _reference(c)
    thr, edges = _pick(c)
    if threshold is not None:
        thr = threshold
    args = (c["theta"], c["lam"], c["eta"])
    want = _slice(report_scores_np(c["rho"], c["X"], c["R"], *args, thr, select, edges, c["mut"]), layer)
    got = eng.report_scores(*args, thr, select=select, layer=layer, edges=edges)
    # exact integers, and the set and order of the rows
    for k in ("counts", "hist", "by_reporter"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for k in ROWS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (what, k)
    n = int(want["counts"][:, 3].sum())
    assert len(got["l"]) == n and got["hist"].sum() == want["counts"][:, 0].sum()
    # every element's logp and mean, and the sums, within the bounds of heldout_util
    full = eng.report_scores(*args, -1e300, layer=layer, by_reporter=False)
    w = np.ones(len(al["l"]), bool) if layer is None else al["l"] == layer
    for k in ROWS:
        assert np.array_equal(full[k], al[k][w]), (what, "all rows", k)
    compare_entries({"counts": want_all[3], "logp": full["logp"], "mean": full["mean"]},
                    (want_all[0][w], want_all[1][w], None, want_all[3]), T[w], K, what)
    sums = want_all[2].copy()
    sums[[layer] if layer is not None else slice(None)] = got["sums"]
    compare_sums(sums, want_all, tuple(al[k] for k in "lijm"), al["x"], T, K, what)
    assert np.array_equal(_bits(full["sums"]), _bits(got["sums"])) and np.array_equal(full["counts"][:, :3], got["counts"][:, :3])
    at = np.isin(np.ravel_multi_index(tuple(full[k] for k in "lijm"), c["X"].shape),
                 np.ravel_multi_index(tuple(got[k] for k in "lijm"), c["X"].shape))
    assert np.array_equal(_bits(full["logp"][at]), _bits(got["logp"])) and np.array_equal(_bits(full["mean"][at]), _bits(got["mean"]))
    # determinism
    again = eng.report_scores(*args, thr, select=select, layer=layer, edges=edges)
    for k in ("counts", "hist", "by_reporter") + ROWS:
        assert np.array_equal(again[k], got[k]), (what, k)
    for k in ("sums", "logp", "mean"):
        assert np.array_equal(_bits(again[k]), _bits(got[k])), (what, k)
    # size, capacity, aggregates alone
    assert eng.report_scores_size(*args, thr, select=select, layer=layer) == n
    if n:
        out = {k: np.full(n - 1, -7, np.int32) for k in ROWS}
        out.update(logp=np.full(n - 1, -7.0), mean=np.full(n - 1, -7.0))
        with pytest.raises(ReportScoresArgumentError, match="flagged"):
            eng.report_scores(*args, thr, select=select, layer=layer, out=out)
        assert all((v == -7).all() for v in out.values())
    agg = eng.report_scores(*args, thr, select=select, layer=layer, edges=edges, rows=False)
    assert agg["l"] is None and agg["logp"] is None
    for k in ("counts", "hist", "by_reporter"):
        assert np.array_equal(agg[k], got[k]), (what, k)
    assert np.array_equal(_bits(agg["sums"]), _bits(got["sums"]))
    # the in-sample flag: the other entry point, the same definition
    if n:
        ho = eng.heldout_loglik(tuple(got[k] for k in "lijm"), got["x"], got["xt"] if c["mut"] else None, theta=args[0], lam=args[1], eta=args[2])
        assert np.array_equal(_bits(ho["logp"]), _bits(got["logp"])) and np.array_equal(_bits(ho["mean"]), _bits(got["mean"])), what
        assert ho["counts"][:, 3].sum() == n == ho["counts"][:, 0].sum()
    return got, want


def test_all_ones_rows_with_mutuality(vmr_format):
    c = _golden("A_ones_mut")
    eng = _engine(c)
    try:
        assert eng.data_format()[0] == vmr_format
        got, _ = _check(eng, c, f"A_ones_mut {vmr_format}")
        assert 0 < len(got["l"]) < got["counts"][0, 0] == c["X"].size
        for select in ("reports", "omissions"):
            _check(eng, c, f"A_ones_mut {vmr_format} {select}", select=select)
    finally:
        eng.close()


def test_mutuality_off():
    c = _golden("C_ones_nomut")
    eng = _engine(c)
    try:
        got, _ = _check(eng, c, "C_ones_nomut")
        assert c["eta"] == 0.0 and not got["xt"].any() and len(got["l"]) > 0
    finally:
        eng.close()


@pytest.mark.parametrize("layer,words", [(None, True), (1, True), (None, False)])
def test_partial_mask_three_categories_two_layers(layer, words, monkeypatch):
    """The mask words of partial rows (the short reporter lists switched off), and the handle's default layout."""
    if words:
        monkeypatch.setenv("VMR_NO_RLISTS", "1")
    c = _golden("B_random_mask_K3")
    eng = _engine(c)
    try:
        assert (eng.mask_format()[0] == "words") or not words
        got, _ = _check(eng, c, f"B_random_mask_K3 layer {layer} {eng.mask_format()[0]}", layer=layer)
        assert got["counts"].shape == ((2, 4) if layer is None else (1, 4)) and got["counts"][:, 0].sum() < c["X"].size
        assert set(got["l"].tolist()) == ({0, 1} if layer is None else {1})
    finally:
        eng.close()


def test_reporter_list_mask_rows():
    c = _golden("D_self_mask")
    eng = _engine(c)
    try:
        assert eng.mask_format()[0] == "lists"
        got, _ = _check(eng, c, "D_self_mask")
        assert got["counts"][:, 0].sum() == int(c["R"].sum())
    finally:
        eng.close()


def test_two_mask_words_and_two_rounds_per_tie(vmr_format, monkeypatch):
    monkeypatch.setenv("VMR_NO_RLISTS", "1")
    c = _synthetic(31, 1, 16, 70, 2, 0.6)
    eng = _engine(c)
    try:
        assert eng.data_format()[0] == vmr_format and eng.mask_format()[0] == "words"
        _check(eng, c, f"M = 70 masked {vmr_format}")
    finally:
        eng.close()


def test_rho_rows_beyond_kmax():
    c = _synthetic(32, 1, 12, 6, 12, 0.7)
    eng = _engine(c)
    try:
        assert eng.K == 12 and eng.data_format()[0] == "sparse"
        _check(eng, c, "K = 12")
    finally:
        eng.close()


def test_coo_handle_with_a_count_of_300():
    """Counts above 255 (the report lists only), and lgamma's Stirling branch."""
    at = (0, 4, 7, 2)
    c = _synthetic(33, 1, 10, 5, 2, 0.7, big=(at, 300))
    eng = _engine(c, coo=True)
    try:
        assert eng.data_format()[0] == "sparse"
        full = eng.report_scores(c["theta"], c["lam"], c["eta"], -1e300, by_reporter=False)
        q = int(np.flatnonzero((full["i"] == at[1]) & (full["j"] == at[2]) & (full["m"] == at[3]))[0])
        assert full["x"][q] == 300 and np.isfinite(full["logp"][q]) and full["logp"][q] < -300
        mirror = int(np.flatnonzero((full["i"] == at[2]) & (full["j"] == at[1]) & (full["m"] == at[3]))[0]) if (
            c["R"][0, at[2], at[1], at[3]]) else None
        assert mirror is None or full["xt"][mirror] == 300
        got, _ = _check(eng, c, "coo, a count of 300")
        assert 300 in got["x"].tolist()
    finally:
        eng.close()


def test_minus_infinity_rows_at_an_infinite_threshold():
    c = dict(_golden("A_ones_mut"))
    c["theta"] = c["theta"].copy()
    c["theta"][0, 3] = 0.0
    eng = _engine(c)
    try:
        got, want = _check(eng, c, "A_ones_mut, theta[0, 3] = 0", threshold=np.inf)
        n_inf = int(want["counts"][0, 2])
        assert n_inf > 0 and got["counts"][0, 2] == n_inf == got["counts"][0, 3] == len(got["l"])
        assert (got["logp"] == -np.inf).all() and (got["m"] == 3).all() and (got["x"] > 0).all() and not got["xt"].any()
        assert got["hist"][0, -1].sum() >= n_inf
        some, _ = _check(eng, c, "A_ones_mut, theta[0, 3] = 0, finite threshold")
        assert some["counts"][0, 3] > n_inf and (some["logp"] == -np.inf).sum() == n_inf      # flagged at any threshold
    finally:
        eng.close()


def test_refusals():
    from vimure_amd import CaviEngine, _lib
    from vimure_amd.engine import EngineError, ReportScoresArgumentError
    c = _golden("B_random_mask_K3")
    eng = CaviEngine(c["X"], c["R"], K=c["K"], mutuality=c["mut"])
    eng.set_priors(*PRI)                          # no state yet: an argument is refused before the state is even looked at
    try:
        L, M = c["theta"].shape
        th, la = np.ascontiguousarray(c["theta"]), np.ascontiguousarray(c["lam"])
        cn, sm = np.zeros((L, _lib.RS_NCOUNT), np.uint64), np.zeros((L, _lib.RS_NSUM))
        ed = np.array([0.5, 1.0, 1.0, 4.0])
        hist = np.zeros((L, len(ed) + 1, 2), np.uint64)
        fn, fs = eng.lib.vmr_report_scores, eng.lib.vmr_report_scores_size
        n_out = __import__("ctypes").c_uint64(7)

        def call(h=eng._h, layer=-1, theta=th, lam=la, eta=0.3, select=3, threshold=2.0, n_edges=len(ed), edges=ed, hist_=hist, outs=True):
            return fn(h, layer, None if theta is None else theta.ctypes.data, None if lam is None else lam.ctypes.data, eta, select,
                      threshold, n_edges, None if edges is None else edges.ctypes.data, None if hist_ is None else hist_.ctypes.data,
                      sm.ctypes.data if outs else None, cn.ctypes.data if outs else None, None, 0, *([None] * 8), 0)
        assert call(h=None) == _lib.VMR_EINVAL
        bad_t, inf_l = th.copy(), la.copy()
        bad_t[1, 2], inf_l[0, 1] = -0.5, np.inf
        for kw, word in ((dict(theta=None), b"theta"), (dict(lam=None), b"lambda"), (dict(theta=bad_t), b"theta"), (dict(lam=inf_l), b"lambda"),
                         (dict(eta=float("nan")), b"eta"), (dict(eta=-0.1), b"eta"), (dict(select=0), b"select"), (dict(select=4), b"select"),
                         (dict(threshold=float("nan")), b"threshold"), (dict(threshold=-np.inf), b"threshold"), (dict(layer=L), b"layer"),
                         (dict(hist_=None, outs=False), b"output"), (dict(n_edges=-1), b"n_edges"), (dict(n_edges=4097), b"n_edges"),
                         (dict(edges=None), b"edges"), (dict(edges=np.array([0.5, 0.4, 1.0, 4.0])), b"edges"),
                         (dict(edges=np.array([0.5, 1.0, np.inf, np.inf])), b"edges")):
            assert call(**kw) == _lib.VMR_EINVAL, kw
            msg = eng.lib.vmr_last_error(eng._h)
            assert b"vmr_report_scores" in msg and word in msg, (kw, msg)
        assert fs(eng._h, -1, th.ctypes.data, la.ctypes.data, 0.3, 0, 2.0, n_out) == _lib.VMR_EINVAL
        assert b"vmr_report_scores_size" in eng.lib.vmr_last_error(eng._h)
        assert call() == _lib.VMR_ESTATE and b"vmr_set_state" in eng.lib.vmr_last_error(eng._h)
        assert fs(eng._h, -1, th.ctypes.data, la.ctypes.data, 0.3, 3, 2.0, n_out) == _lib.VMR_ESTATE and n_out.value == 7
        assert not cn.any() and not sm.any() and not hist.any()                              # nothing was launched or written
        with pytest.raises(EngineError, match="vmr_set_state") as ei:
            eng.report_scores(th, la, 0.3, 2.0)
        assert not isinstance(ei.value, ReportScoresArgumentError)
        eng.set_state(*c["st"])
        assert call(threshold=np.inf) == _lib.VMR_OK and cn[:, 0].sum() == int(c["R"].sum())   # +inf is a threshold
        for kw in (dict(select="all"), dict(layer=2), dict(edges=[1.0, 0.5]), dict(edges=np.zeros(4097))):
            with pytest.raises(ReportScoresArgumentError):
                eng.report_scores(th, la, 0.3, 2.0, **kw)
        for a in ((th[:1], la), (th, la[:, :1]), (None, la)):
            with pytest.raises(ReportScoresArgumentError):
                eng.report_scores(a[0], a[1], 0.3, 2.0)
        # a NaN in rho: reported after the pass, as a ValueError that is no argument error
        rho = c["rho"].copy()
        rho[0, 3, 4] = np.nan
        eng.set_state(*c["st"][:6], rho)
        with pytest.raises(ValueError, match="NaN") as ei:
            eng.report_scores(th, la, 0.3, 2.0)
        assert not isinstance(ei.value, ReportScoresArgumentError)
    finally:
        eng.close()


def test_device_rows_and_snapshot_restore():
    import torch
    c = _golden("B_random_mask_K3")
    eng = _engine(c)
    try:
        thr, edges = _pick(c)
        args = (c["theta"], c["lam"], c["eta"], thr)
        host = eng.report_scores(*args, edges=edges)
        dev = eng.report_scores(*args, edges=edges, device=True)
        assert dev["logp"].is_cuda and dev["l"].dtype == torch.int32
        for k in ROWS:
            assert np.array_equal(dev[k].cpu().numpy(), host[k]), k
        for k in ("logp", "mean"):
            assert np.array_equal(_bits(dev[k].cpu().numpy()), _bits(host[k])), k
        assert np.array_equal(dev["hist"], host["hist"]) and np.array_equal(_bits(dev["sums"]), _bits(host["sums"]))
        eng.snapshot()
        eng.step(3)
        later = eng.report_scores(*args, edges=edges)
        eng.restore()
        back = eng.report_scores(*args, edges=edges)
        assert not np.array_equal(_bits(later["sums"]), _bits(host["sums"]))
        for k in ("sums", "logp", "mean"):
            assert np.array_equal(_bits(back[k]), _bits(host[k])), k
        assert np.array_equal(back["hist"], host["hist"]) and np.array_equal(back["counts"], host["counts"])
    finally:
        eng.close()


def test_top_n_through_the_model():
    from vimure_amd import VimureModel
    from vimure_amd.crossval import plug_in_tables
    from vimure_amd.residuals import report_scores_np, top_rows
    d = load_case("A_ones_mut")
    X = np.asarray(d["X"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VimureModel(mutuality=True)
        m.fit(X, K=2, seed=1, max_iter=30, num_realisations=1, keep_engine=True)
    try:
        assert m._rho_f is None
        theta, lam, eta = plug_in_tables(m, m._engine, "mean")
        first = m.surprising_reports(top=40)
        by_thr = m.surprising_reports(top=None, threshold=first.threshold)
        omitted = m.surprising_reports(top=15, select="omissions")
        one = m.surprising_reports(top=10 ** 9)                    # more than there are: everything above 0, sorted
        assert m._rho_f is None                                    # scored where rho lives
        c = dict(rho=m.rho_f, X=X, R=None, theta=theta, lam=lam, eta=eta, mut=True)
        al, _, T, _, _ = _reference(c)
        s = -al["logp"]
        order = np.lexsort((al["m"], al["j"], al["i"], al["l"], -s))
        ss, bound = s[order], C_LOGP * U * T[order]
        wide = np.diff(ss) <= -GAP_RULE * np.maximum(bound[:-1], bound[1:])          # [q]: the q-th and (q + 1)-th are well apart
        n = int(np.flatnonzero(wide[20:])[0]) + 21                                   # the n-th and (n + 1)-th differ by more than the rule
        assert 20 < n <= 40 and wide[n - 1]
        got = m.surprising_reports(top=n)
        f = got.frame()
        want = top_rows(al, n)
        key = lambda r: np.ravel_multi_index(tuple(np.asarray(r[k], np.int64) for k in "lijm"), X.shape)
        gk = np.ravel_multi_index((f["layer"], f["source"], f["target"], f["reporter"]), X.shape)
        assert len(f) == n == got.top and set(gk.tolist()) == set(key(want).tolist())
        srt = np.lexsort((f["reporter"], f["target"], f["source"], f["layer"], -f["surprise"]))
        assert np.array_equal(srt, np.arange(n))                                     # sorted by (-surprise, l, i, j, m)
        apart = np.r_[True, wide[:n - 1]] & np.r_[wide[:n - 1], True]                # rows no rounding can move
        assert apart.sum() > n // 2 and np.array_equal(gk[apart], key(want)[apart])
        assert np.array_equal(f["x"], X[0, f["source"], f["target"], f["reporter"]])
        assert np.allclose(np.sort(f["logp"]), np.sort(want["logp"]), rtol=0, atol=1e-9)
        # the pieces: the grid's histogram, the threshold it gave, the same rows by that threshold
        assert got.hist.shape == (1, 4097, 2) and got.hist.sum() == X.size and got.edges[1] == 1.0 / 64.0
        assert first.threshold * 64 == int(first.threshold * 64) and len(first) == 40 and len(by_thr) >= 40
        assert (by_thr.frame()["surprise"] >= first.threshold).all() and (first.frame()["surprise"] >= first.threshold).all()
        assert len(omitted) == 15 and not omitted.frame()["x"].any()
        assert len(one) == int((one.hist[0, 1:].sum())) <= X.size and np.isfinite(got.lppd[0])
        assert got.lppd[0] == first.lppd[0] == by_thr.lppd[0]
        with pytest.raises(ValueError, match="max_rows"):
            m.surprising_reports(top=10 ** 9, max_rows=10)
    finally:
        m.close()
