"""GPU: the posterior scored against a ground-truth network on the device (vmr_score_truth).  The integer outputs -- the
threshold histogram, the arg-max counts, the AUC's pair counts -- are held exactly to the NumPy restatement
(vimure_amd/scoring.py) from the rho given to `set_state`; the sums within (n_ties + 8) 2^-52 relative, the bound of any
summation order of non-negative terms each good to a few ulp (derived, not measured).  Over both data layouts, a coordinate-list
handle with a self-reporter mask, the K = 2 and the general kernels, both scores, with and without the diagonal; and against the
merged read-outs, a brute-force pair count, sklearn, a restored snapshot, the reference's known-answer fits and the experiment
driver."""
import ctypes
import warnings

import numpy as np
import pytest

from tests.golden_util import case_config, load_case
from tests.score_truth_util import assert_auc_close, assert_ints_equal, assert_sums_close, brute_u2

pytestmark = pytest.mark.gpu

PRI = (0.1, 0.1, 10.0, 10.0, 0.5, 1.0)
L, N, M = 2, 70, 5            # N: no multiple of 64, more than one wave; 4900 ties: 20 workgroups per layer


def _state(g, K, rho):
    gs, gr = g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(2.0, 1.0, (L, M)) + 0.1
    ps, pr = g.gamma(5.0, 1.0, (L, K)) + 0.1, g.gamma(2.0, 1.0, (L, K)) + 0.1
    return gs, gr, ps, pr, 3.0, 2.5, rho


_CASES = {}


def _case(K, eighths=False):
    """X sparse counts; rho random and normalised (eighths: every entry a multiple of 1/8, so equal scores abound), with rows
    planted whose score is exactly 0, 1, 0.25 and 0.5; Y_true differs between the layers, categories 0..K-1."""
    key = (K, eighths)
    if key not in _CASES:
        g = np.random.RandomState(40 + K + 100 * eighths)
        X = ((g.rand(L, N, N, M) < 0.05) * g.randint(1, 4, (L, N, N, M))).astype(np.uint8)
        if eighths:
            cut = np.sort(g.randint(0, 9, (L, N, N, K - 1)), axis=-1)
            rho = np.diff(np.concatenate([np.zeros((L, N, N, 1), int), cut, np.full((L, N, N, 1), 8)], -1), axis=-1) / 8.0
        else:
            rho = g.rand(L, N, N, K)
            rho[..., 0] *= 6.0
            rho = rho / rho.sum(-1, keepdims=True)
            for q, s in enumerate((0.0, 1.0, 0.25, 0.5)):
                row = np.zeros(K)
                row[0], row[1] = 1.0 - s, s
                rho[:, 3 + q, ::7] = row
                rho[1, 40:44, 5 + q] = row
            if K > 2:
                rho[0, 9, ::5] = np.r_[0.5, 0.25, 0.25, np.zeros(K - 3)]    # prob 0.5 exactly, rho_1 0.25
        Y = (g.rand(L, N, N) < np.array([0.05, 0.3])[:, None, None]) * g.randint(1, K, (L, N, N)) if K > 2 else \
            (g.rand(L, N, N) < np.array([0.05, 0.3])[:, None, None]).astype(int)
        Y = np.where(rho.argmax(-1) > 0, np.where(g.rand(L, N, N) < 0.7, rho.argmax(-1), Y), Y).astype(np.uint8)
        _CASES[key] = dict(X=X, rho=np.ascontiguousarray(rho), Y=Y, st=_state(g, K, np.ascontiguousarray(rho)))
    return _CASES[key]


def _thresholds(rho):
    """On planted scores (0, 0.25, 0.5, 1), a duplicate, and one that IS a rho_1 of the random part."""
    return np.sort(np.r_[0.0, 0.1, 0.25, 0.25, 0.5, float(rho[0, 11, 13, 1]), 0.8, 1.0])


def _engine(X, R, K, st, coo=False):
    from vimure_amd import CaviEngine
    if coo:
        xs = np.nonzero(X)
        eng = CaviEngine.from_coo(xs, X[xs], X.shape, R=None if R is None else np.nonzero(R), K=K, mutuality=True)
    else:
        eng = CaviEngine(X, R, K=K, mutuality=True)
    eng.set_priors(*PRI)
    if st is not None:
        eng.set_state(*st)
    return eng


def _check(eng, rho, Y, thr, score, skip):
    from vimure_amd.scoring import score_truth_np
    want = score_truth_np(rho, Y, thr, score, skip)
    got = eng.score_truth(Y, thresholds=thr, score=score, skip_diagonal=skip)
    assert_ints_equal(got, want)
    assert_sums_close(got, want, want["n_ties"][0])
    assert_auc_close(got, want)
    assert got["hist"].sum() == want["n_ties"].sum()
    return got, want


# ---------------------------------------------------------------------------------------------- 1. integers exact
def _integers_exact(K, fmt):
    c = _case(K)
    eng = _engine(c["X"], None, K, c["st"])
    try:
        assert eng.data_format()[0] == fmt
        thr = _thresholds(c["rho"])
        for score in ("rho1", "prob"):
            for skip in (False, True):
                got, want = _check(eng, c["rho"], c["Y"], thr, score, skip)
                assert got["hist"][:, -1].sum() > 0                                          # s = 1 reaches the last bin
                assert got["conf"][:, 0].min() > 0 and got["conf"][:, 2].min() > 0
        if K > 2:
            a = eng.score_truth(c["Y"], thresholds=thr, score="rho1")["hist"]
            b = eng.score_truth(c["Y"], thresholds=thr, score="prob")["hist"]
            assert not np.array_equal(a, b)
    finally:
        eng.close()


@pytest.mark.parametrize("K", [2, 3])
def test_integers_exact_both_scores_both_diagonals(K, vmr_format):
    _integers_exact(K, vmr_format)


def test_integers_exact_general_kernels_k12():
    """More than 8 categories: the general kernels, which exist over the report lists only (a handle of dense tiles is refused)."""
    _integers_exact(12, "sparse")


def test_from_coo_handle_with_self_reporter_mask():
    from vimure_amd.synthetic import self_reporter_mask
    g = np.random.RandomState(8)
    n = 70
    R = np.asarray(self_reporter_mask(1, n, n)).astype(np.uint8)
    X = ((g.rand(1, n, n, n) < 0.3) * g.randint(1, 3, (1, n, n, n))).astype(np.uint8) * R
    rho = g.rand(1, n, n, 2)
    rho[..., 0] *= 4.0
    rho = rho / rho.sum(-1, keepdims=True)
    Y = (g.rand(1, n, n) < 0.1).astype(np.uint8)
    gs, gr = g.gamma(2.0, 1.0, (1, n)) + 0.1, g.gamma(2.0, 1.0, (1, n)) + 0.1
    ps, pr = g.gamma(5.0, 1.0, (1, 2)) + 0.1, g.gamma(2.0, 1.0, (1, 2)) + 0.1
    eng = _engine(X, R, 2, (gs, gr, ps, pr, 3.0, 2.5, rho), coo=True)
    try:
        assert eng.mask_format()[0] == "lists"
        for skip in (False, True):
            _check(eng, rho, Y, np.linspace(0, 1, 11), "rho1", skip)
    finally:
        eng.close()


@pytest.mark.parametrize("n_thr", [0, 1, 101, 4096])
def test_threshold_counts_from_none_to_the_maximum(n_thr):
    c = _case(2)
    eng = _engine(c["X"], None, 2, c["st"])
    try:
        thr = np.linspace(0, 1, n_thr) if n_thr > 1 else np.full(n_thr, 0.5)
        got, _ = _check(eng, c["rho"], c["Y"], thr, "rho1", False)
        assert got["hist"].shape == (L, n_thr + 1, 2)
    finally:
        eng.close()


def test_layer_without_positives_and_layer_of_positives_only():
    c = _case(2)
    Y = np.zeros((L, N, N), np.uint8)
    Y[1] = 1
    eng = _engine(c["X"], None, 2, c["st"])
    try:
        got, _ = _check(eng, c["rho"], Y, _thresholds(c["rho"]), "rho1", False)
        assert np.isnan(got["auc"]).all()
        assert got["conf"][0, 4] == 0 and got["conf"][1, 4] == N * N and got["auc_pairs"][1, 1] == 0
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 2. the merged read-outs
@pytest.mark.parametrize("K", [2, 3])
def test_counts_agree_with_the_readouts(K):
    c = _case(K)
    eng = _engine(c["X"], None, K, c["st"])
    try:
        thr = np.sort(np.r_[0.0, 0.25, float(c["rho"][0, 11, 13, 1]), 0.5, 1.0])
        got = eng.score_truth(c["Y"], thresholds=thr, score="rho1")
        above = np.cumsum(got["hist"][:, ::-1], axis=1)[:, ::-1][:, 1:].sum(axis=2)          # tp + fp, [L, n_thr]
        for q, t in enumerate(thr):
            assert np.array_equal(above[:, q], eng.readout("threshold", float(t)).reshape(L, -1).sum(axis=1)), t
        amax = eng.readout("rho_max")
        assert np.array_equal(got["conf"][:, 0] + got["conf"][:, 1], (amax > 0).reshape(L, -1).sum(axis=1))
        assert np.array_equal(got["conf"][:, 3], (amax == c["Y"]).reshape(L, -1).sum(axis=1))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 3. AUC with equal scores
@pytest.mark.parametrize("K", [2, 3])
def test_auc_with_ties_against_brute_force_and_sklearn(K):
    from sklearn.metrics import roc_auc_score
    from vimure_amd.scoring import tie_scores_np
    c = _case(K, eighths=True)
    eng = _engine(c["X"], None, K, c["st"])
    try:
        for score in ("rho1", "prob"):
            got = eng.score_truth(c["Y"], thresholds=[0.5], score=score)
            s = tie_scores_np(c["rho"], score)[0]
            for l in range(L):
                b = c["Y"][l].reshape(-1) > 0
                assert got["auc_pairs"][l, 0] == brute_u2(s[l].reshape(-1), b)
                assert got["auc_pairs"][l, 1] == int((~b).sum())
                assert abs(got["auc"][l] - roc_auc_score(b, s[l].reshape(-1))) <= 1e-12
            assert len(np.unique(s)) <= 9
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 4. sums
def test_sums_bit_identical_between_calls_and_close_between_formats(monkeypatch):
    c = _case(3)
    thr = _thresholds(c["rho"])
    res = {}
    for fmt in ("sparse", "dense"):
        monkeypatch.setenv("VMR_FORMAT", fmt)
        eng = _engine(c["X"], None, 3, c["st"])
        try:
            assert eng.data_format()[0] == fmt
            a = eng.score_truth(c["Y"], thresholds=thr, score="prob")
            b = eng.score_truth(c["Y"], thresholds=thr, score="prob")
            assert np.array_equal(a["sums"].view(np.uint64), b["sums"].view(np.uint64))
            assert np.array_equal(a["auc"].view(np.uint64), b["auc"].view(np.uint64))
            assert_ints_equal(a, b)
            assert (a["sums"] > 0).all()
            res[fmt] = a
        finally:
            eng.close()
    assert_ints_equal(res["sparse"], res["dense"])
    assert_sums_close(res["sparse"], res["dense"], N * N)


# ---------------------------------------------------------------------------------------------- 5. subsets of the outputs
def test_subsets_of_outputs_give_the_same_numbers():
    import torch
    c = _case(2)
    eng = _engine(c["X"], None, 2, c["st"])
    try:
        thr = _thresholds(c["rho"])
        full = eng.score_truth(c["Y"], thresholds=thr)
        only_hist = eng.score_truth(c["Y"], thresholds=thr, outputs=("hist",))
        only_auc = eng.score_truth(c["Y"], thresholds=thr, outputs=("auc",))
        no_auc = eng.score_truth(c["Y"], thresholds=thr, auc=False)
        assert np.array_equal(only_hist["hist"], full["hist"]) and only_hist["conf"] is None and only_hist["auc"] is None
        assert np.array_equal(only_auc["auc"].view(np.uint64), full["auc"].view(np.uint64)) and only_auc["hist"] is None
        assert no_auc["auc"] is None and no_auc["auc_pairs"] is None
        assert_ints_equal(no_auc, full, keys=("hist", "conf", "n_ties"))
        assert np.array_equal(no_auc["sums"].view(np.uint64), full["sums"].view(np.uint64))
        # the ground truth as a device tensor
        dev = eng.score_truth(torch.as_tensor(c["Y"]).cuda(), thresholds=thr)
        assert_ints_equal(dev, full)
        assert np.array_equal(dev["sums"].view(np.uint64), full["sums"].view(np.uint64))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_refusals():
    from vimure_amd import _lib
    from vimure_amd.engine import EngineError, ScoreArgumentError
    c = _case(2)
    eng = _engine(c["X"], None, 2, None)          # no state yet: an argument is refused before the state is even looked at
    try:
        Y = c["Y"]
        for kw in (dict(thresholds=[0.5, 0.4]), dict(thresholds=[0.1, np.nan]), dict(thresholds=[np.inf]),
                   dict(thresholds=np.linspace(0, 1, _lib.SCORE_MAX_THR + 1)), dict(outputs=()), dict(score="mean")):
            with pytest.raises(ScoreArgumentError):
                eng.score_truth(Y, **kw)
        with pytest.raises(ScoreArgumentError):
            eng.score_truth(Y[:1])
        with pytest.raises(ScoreArgumentError):
            eng.score_truth(None)
        # the C entry point itself: a NULL truth, an unknown score, n_thr out of range, hist without thresholds
        out = np.zeros((L, 3, 2), np.uint64)
        yk = np.ascontiguousarray(Y)
        t2 = np.array([0.25, 0.5])
        for args in ((None, 0, 0, 0, 2, t2.ctypes.data, out.ctypes.data), (yk.ctypes.data, 0, 7, 0, 2, t2.ctypes.data, out.ctypes.data),
                     (yk.ctypes.data, 0, 0, 0, -1, t2.ctypes.data, out.ctypes.data), (yk.ctypes.data, 0, 0, 0, 4097, t2.ctypes.data, out.ctypes.data),
                     (yk.ctypes.data, 0, 0, 0, 2, None, out.ctypes.data), (yk.ctypes.data, 0, 0, 0, 2, t2.ctypes.data, None)):
            assert eng.lib.vmr_score_truth(eng._h, *args, None, None, None, None) == _lib.VMR_EINVAL, args
            assert b"vmr_score_truth" in eng.lib.vmr_last_error(eng._h)
        assert not out.any()
        with pytest.raises(EngineError, match="vmr_set_state") as ei:
            eng.score_truth(Y)
        assert not isinstance(ei.value, ScoreArgumentError)
        # a NaN among the scores
        rho = c["rho"].copy()
        rho[1, 17, 19] = np.nan
        eng.set_state(*c["st"][:6], rho)
        with pytest.raises(ValueError, match="NaN") as ei:
            eng.score_truth(Y)
        assert not isinstance(ei.value, ScoreArgumentError)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 7. the rho that is scored
def test_after_restore_the_scores_are_the_snapshots():
    from oracle import vimure_oracle as vo
    from vimure_amd import CaviEngine
    from vimure_amd.scoring import score_truth_np
    from vimure_amd.synthetic import standard_sbm
    net = standard_sbm(N=24, M=12, L=2, K=2, avg_degree=4.0, eta=0.4, seed=3)
    X = np.asarray(net.X).astype(np.uint8)
    R = (np.random.RandomState(0).rand(*X.shape) < 0.8).astype(np.uint8)
    Y = (np.random.RandomState(1).rand(2, 24, 24) < 0.2).astype(np.uint8)
    pr = vo.make_priors(2, 12, 2)
    st = vo.init_state(vo.Problem(X, R, 2, True, pr), np.random.RandomState(1))
    eng = CaviEngine(X, R, K=2, mutuality=True)
    try:
        eng.set_priors(pr.alpha_theta, pr.beta_theta, pr.alpha_lambda, pr.beta_lambda, pr.alpha_eta, pr.beta_eta)
        eng.set_state(st.gamma_shp, st.gamma_rte, st.phi_shp, st.phi_rte, st.nu_shp, st.nu_rte, st.pr_rho)
        eng.step(2)
        rho_snap = eng.get_state()["rho"].copy()
        eng.snapshot()
        eng.step(4)
        later = eng.score_truth(Y)
        eng.restore()
        got, want = eng.score_truth(Y), score_truth_np(rho_snap, Y)
        assert_ints_equal(got, want)
        assert_sums_close(got, want, 24 * 24)
        assert not np.array_equal(later["sums"], got["sums"])
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 8. end to end
@pytest.mark.parametrize("tag", ["over", "under"])
def test_known_answer_f1_through_the_model(tag):
    """The fit of tests/test_hip_fit.py::test_reference_known_answer_f1, scored on the device instead of through the read-out."""
    from vimure_amd import VimureModel
    from vimure_amd.scoring import TruthScore, score_truth_np
    d = load_case(f"H_ref_f1_{tag}")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VimureModel(mutuality=bool(d["mutuality"]), undirected=und)
        m.fit(d["X"], R=d["R"], seed=seed, rho_prior=rho_prior, K=K, keep_engine=True, **priors, **fitargs)
    try:
        assert m._rho_f is None
        ts = m.score_truth(d["Y_true"][None], thresholds=[0.5])
        assert m._rho_f is None                           # scored where rho lives
        assert abs(ts.f1_at(0.5)[0] - float(d["f1"])) <= 1e-12
        host = TruthScore(score_truth_np(m.rho_f, d["Y_true"][None], [0.5]))
        assert np.array_equal(ts.hist, host.hist) and np.array_equal(ts.conf, host.conf)
        assert ts.f1_at(0.5)[0] == host.f1_at(0.5)[0]
        again = m.score_truth(d["Y_true"][None], thresholds=[0.5])        # rho_f has been read: the host path
        assert np.array_equal(again.hist, ts.hist) and again.heuristic_threshold == ts.heuristic_threshold
        assert "heuristic_f1" in ts.summary().columns
    finally:
        m.close()


def test_unreliable_reporters_driver(monkeypatch):
    from vimure_amd import experiments
    from vimure_amd.model import VimureModel
    made, scored = [], []
    make, score = experiments.make_dataset, VimureModel.score_truth

    def counting_make(*a, **k):
        out = make(*a, **k)
        made.append(out[0])
        return out

    def recording_score(self, *a, **k):
        ts = score(self, *a, **k)
        scored.append((ts, self.mutuality))
        return ts
    monkeypatch.setattr(experiments, "make_dataset", counting_make)
    monkeypatch.setattr(VimureModel, "score_truth", recording_score)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        df = experiments.unreliable_reporters(available_seeds=[0, 1], theta_ratio_vals=[0.2], exaggeration_type=["under", "over"],
                                              mutuality=[True, False], N=60, num_realisations=1)
    assert list(df.columns) == ["param_seed", "param_theta_ratio", "param_exaggeration_type", "param_mutuality", "mean_test_f1",
                                "mean_test_mse", "auc", "brier", "mean_fit_time", "eta"]
    assert len(df) == 8 and len(made) == 4 and len(scored) == 8          # one dataset serves both mutuality settings
    assert df[["param_seed", "param_exaggeration_type", "param_mutuality"]].drop_duplicates().shape[0] == 8
    assert [s[1] for s in scored] == [True, False] * 4
    for (ts, _), (_, row) in zip(scored, df.iterrows()):
        assert ts.thresholds.tolist() == [0.01] and ts.n_ties[0] == 3600
        assert row["mean_test_mse"] == -float(ts.fp[0, 0] + ts.fn[0, 0]) / 3600
        assert row["mean_test_f1"] == ts.f1[0, 0] and 0.0 <= row["mean_test_f1"] <= 1.0
        assert row["auc"] == ts.auc[0] and row["brier"] == ts.brier[0]
    assert (df["eta"] == 0.0).all() and (df["mean_fit_time"] > 0).all()
