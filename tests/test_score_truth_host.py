"""CPU: the host pieces of scoring against a ground truth -- the C entry point's export, binding, constants and NULL-handle
answer; `scoring.score_truth_np` against its definitions, sklearn and a brute-force pair count; the reference-recorded known
answers (tests/golden/H_ref_f1_*.npz); `VimureModel.score_truth` with a stub engine and without one; and
`experiments.make_dataset` against the inputs the reference generated for those fixtures.  No GPU needed."""
import itertools
import os
import warnings

import numpy as np
import pytest

from tests.golden_util import GOLDEN
from tests.score_truth_util import StubEngine, brute_u2


def test_entry_point_exported_bound_and_refuses_null_handle():
    from vimure_amd import _lib
    from vimure_amd.engine import EngineError, ScoreArgumentError
    lib = _lib.load()
    assert "vmr_score_truth" in _lib.SIGNATURES and hasattr(lib, "vmr_score_truth")
    assert (_lib.SCORE_RHO1, _lib.SCORE_PROB, _lib.SCORE_NCONF, _lib.SCORE_NSUM, _lib.SCORE_MAX_THR) == (0, 1, 5, 4, 4096)
    y = np.zeros(16, np.uint8)
    thr = np.array([0.5])
    bufs = [np.zeros(64, np.uint64), np.zeros(64, np.uint64), np.zeros(64), np.zeros(64), np.zeros(64, np.uint64)]
    for mask in itertools.product((False, True), repeat=5):
        ptrs = [b.ctypes.data if on else None for b, on in zip(bufs, mask)]
        assert lib.vmr_score_truth(None, y.ctypes.data, 0, 0, 0, 1, thr.ctypes.data, *ptrs) == -1
    assert lib.vmr_score_truth(None, None, 0, 0, 0, 0, None, *([None] * 5)) == -1
    assert issubclass(ScoreArgumentError, EngineError) and issubclass(ScoreArgumentError, ValueError)


def _random(K, seed, L=2, N=13, eighths=False):
    g = np.random.RandomState(seed)
    if eighths:
        cut = np.sort(g.randint(0, 9, (L, N, N, K - 1)), axis=-1)
        rho = np.diff(np.concatenate([np.zeros((L, N, N, 1), int), cut, np.full((L, N, N, 1), 8)], -1), axis=-1) / 8.0
    else:
        rho = g.rand(L, N, N, K)
        rho[..., 0] *= 3.0
        rho = rho / rho.sum(-1, keepdims=True)
        rho[0, 2, 3] = np.r_[1.0, np.zeros(K - 1)]           # s = 0
        rho[1, 4, 4] = np.r_[0.0, 1.0, np.zeros(K - 2)]      # s = 1, on the diagonal
    Y = ((g.rand(L, N, N) < 0.25) * g.randint(1, K, (L, N, N))).astype(np.uint8) if K > 2 else (g.rand(L, N, N) < 0.25).astype(np.uint8)
    return rho, Y


@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("skip", [False, True])
def test_restatement_against_its_definitions_and_sklearn(K, skip):
    from sklearn.metrics import f1_score, roc_auc_score
    from vimure_amd.scoring import TruthScore, score_truth_np
    rho, Y = _random(K, 7 + K)
    L, N = Y.shape[:2]
    thr = np.sort(np.r_[0.0, 0.2, 0.2, float(rho[0, 5, 6, 1]), float(rho[1, 1, 8, 1]), 0.6, 1.0])      # exact scores, a duplicate, 0 and 1
    res = score_truth_np(rho, Y, thr, "rho1", skip)
    ts = TruthScore(res)
    keep = ~np.eye(N, dtype=bool) if skip else np.ones((N, N), bool)
    assert res["n_ties"].tolist() == [int(keep.sum())] * L
    mean = np.zeros(Y.shape)
    for k in range(1, K):
        mean = mean + float(k) * rho[..., k]
    for l in range(L):
        s, b, y = rho[l, :, :, 1][keep], Y[l][keep] > 0, Y[l][keep].astype(float)
        for q, t in enumerate(thr):
            pred = s >= t
            assert (ts.tp[l, q], ts.fp[l, q], ts.fn[l, q], ts.tn[l, q]) == ((pred & b).sum(), (pred & ~b).sum(), (~pred & b).sum(), (~pred & ~b).sum())
            assert abs(ts.f1[l, q] - f1_score(b, pred)) <= 1e-15
        assert abs(res["auc_pairs"][l, 0] / (2.0 * b.sum() * (~b).sum()) - roc_auc_score(b, s)) <= 1e-12
        assert abs(ts.auc[l] - roc_auc_score(b, s)) <= 1e-12 and res["auc_pairs"][l, 1] == (~b).sum()
        assert abs(ts.brier[l] - np.mean((s - b) ** 2)) <= 1e-15
        assert abs(ts.mse[l] - np.mean((mean[l][keep] - y) ** 2)) <= 1e-15
        a = rho[l].argmax(-1)[keep]
        assert res["conf"][l].tolist() == [((a > 0) & b).sum(), ((a > 0) & ~b).sum(), ((a == 0) & b).sum(), (a == Y[l][keep]).sum(), b.sum()]
        assert abs(ts.argmax_f1[l] - f1_score(b, a > 0)) <= 1e-15 and abs(ts.accuracy[l] - np.mean(a == Y[l][keep])) <= 1e-15
    assert res["hist"].sum(axis=(1, 2)).tolist() == res["n_ties"].tolist()
    # the views: a row per (layer, threshold) / (layer, bin) / layer
    cur, cal, summ = ts.curve(), ts.calibration(), ts.summary()
    assert list(cur.columns) == ["layer", "threshold", "tp", "fp", "fn", "tn", "precision", "recall", "f1"] and len(cur) == L * len(thr)
    assert len(cal) == L * (len(thr) + 1) and cal["count"].sum() == res["n_ties"].sum()
    assert np.array_equal(cal["positives"].to_numpy().reshape(L, -1).sum(axis=1), res["conf"][:, 4])
    empty = cal["count"] == 0
    assert empty.any() and cal["frequency"][empty].isna().all() and not cal["frequency"][~empty].isna().any()     # 0 / 0 is NaN
    best = ts.best_threshold()
    for l in range(L):
        assert best[l] == thr[int(np.nanargmax(ts.f1[l]))] and ts.f1_at(best[l])[l] == np.nanmax(ts.f1[l])
    assert len(summ) == L and "best_threshold" in summ.columns and "heuristic_f1" not in summ.columns
    with pytest.raises(ValueError, match="not one of the thresholds"):
        ts.f1_at(0.123)
    if K > 2:
        prob = score_truth_np(rho, Y, thr, "prob", skip)
        assert not np.array_equal(prob["hist"], res["hist"]) and np.array_equal(prob["conf"], res["conf"])
    else:
        assert np.array_equal(score_truth_np(rho, Y, thr, "prob", skip)["hist"], res["hist"])


@pytest.mark.parametrize("K", [2, 3, 5])
def test_pair_count_with_equal_scores_is_the_brute_force_count(K):
    from vimure_amd.scoring import score_truth_np, tie_scores_np
    rho, Y = _random(K, 20 + K, eighths=True)
    for score in ("rho1", "prob"):
        res = score_truth_np(rho, Y, [0.5], score, False)
        s = tie_scores_np(rho, score)[0]
        for l in range(Y.shape[0]):
            b = Y[l].reshape(-1) > 0
            sl = s[l].reshape(-1)
            assert (sl[b][:, None] == sl[~b][None, :]).any()
            assert res["auc_pairs"][l, 0] == brute_u2(sl, b)


def test_degenerate_layers_and_refused_arguments():
    from vimure_amd.scoring import TruthScore, score_truth_np
    rho, Y = _random(2, 3)
    Y[0], Y[1] = 0, 1
    res = score_truth_np(rho, Y, [], "rho1", False)
    assert np.isnan(res["auc"]).all() and res["hist"].shape == (2, 1, 2)
    ts = TruthScore(res)
    assert np.isnan(ts.best_threshold()).all() and ts.curve().shape[0] == 0
    assert ts.conf[0, 4] == 0 and ts.conf[1, 4] == ts.n_ties[1] and np.isnan(ts.recall).all()
    for bad in ([0.5, 0.4], [np.nan], [np.inf]):
        with pytest.raises(ValueError):
            score_truth_np(rho, Y, bad)
    with pytest.raises(ValueError):
        score_truth_np(rho, Y, [0.5], "mean")
    with pytest.raises(ValueError):
        score_truth_np(rho, Y[:1], [0.5])


@pytest.mark.parametrize("tag,counts", [("over", (213, 4, 38)), ("under", (251, 15, 0))])
def test_reference_recorded_known_answers(tag, counts):
    """fit_rho_f, Y_true and f1 as the reference plus sklearn produced them."""
    from vimure_amd.scoring import TruthScore, score_truth_np
    d = np.load(os.path.join(GOLDEN, f"H_ref_f1_{tag}.npz"))
    ts = TruthScore(score_truth_np(d["fit_rho_f"], d["Y_true"][None], [0.5]))
    assert (int(ts.tp[0, 0]), int(ts.fp[0, 0]), int(ts.fn[0, 0])) == counts
    assert abs(ts.f1_at(0.5)[0] - float(d["f1"])) <= 1e-12


def _model(rho, engine):
    from vimure_amd import VimureModel
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VimureModel(mutuality=True)
    m.L, m.N, m.K = rho.shape[0], rho.shape[1], rho.shape[3]
    m.M = m.N
    m.gamma_shp_f = np.ones((m.L, m.M))
    m.G_exp_nu = np.float64(0.9)
    if engine:
        m._rho_f, m._engine = None, StubEngine(rho)
    else:
        m._rho_f, m._engine = rho, None
    return m


def test_model_score_truth_with_and_without_an_engine():
    from vimure_amd.scoring import TruthScore, score_truth_np
    from vimure_amd.tensor import SparseTensor
    rho, Y = _random(3, 11)
    on, off = _model(rho, True), _model(rho, False)
    a, b = on.score_truth(Y), off.score_truth(Y)
    assert on._rho_f is None and len(on._engine.calls) == 2
    thr, heur = np.linspace(0, 1, 101), float(0.54 * 0.9 - 0.01)
    assert on._engine.calls[0] == (thr.tolist(), "rho1", False, True, None)
    assert on._engine.calls[1][0] == [heur] and on._engine.calls[1][3] is False
    want = TruthScore(score_truth_np(rho, Y, thr))
    for ts in (a, b):
        assert np.array_equal(ts.thresholds, thr)
        for k in ("hist", "conf", "sums", "n_ties", "auc_pairs"):
            assert np.array_equal(getattr(ts, k), getattr(want, k)), k
        assert np.array_equal(ts.auc, want.auc) and ts.heuristic_threshold == heur
        pred = rho[..., 1] >= heur
        tp, fp, fn = (pred & (Y > 0)).sum(axis=(1, 2)), (pred & (Y == 0)).sum(axis=(1, 2)), (~pred & (Y > 0)).sum(axis=(1, 2))
        assert np.allclose(ts.heuristic_f1, 2 * tp / (2 * tp + fp + fn), rtol=0, atol=1e-15)
        assert {"heuristic_threshold", "heuristic_f1"} <= set(ts.summary().columns)
    # a COO ground truth, the other score, without the diagonal and without the AUC
    c = on.score_truth(SparseTensor.fromarray(Y), thresholds=[0.3, 0.6], score="prob", skip_diagonal=True, auc=False)
    d = off.score_truth(SparseTensor.fromarray(Y), thresholds=[0.3, 0.6], score="prob", skip_diagonal=True, auc=False)
    assert on._engine.calls[-2] == ([0.3, 0.6], "prob", True, False, None)
    e = score_truth_np(rho, Y, [0.3, 0.6], "prob", True)
    for ts in (c, d):
        assert np.array_equal(ts.hist, e["hist"]) and np.isnan(ts.auc).all() and ts.auc_pairs is None
        assert ts.n_ties.tolist() == [13 * 12] * 2
    # argument errors
    for m in (on, off):
        for kw in (dict(thresholds=[0.5, 0.1]), dict(thresholds=[np.nan]), dict(score="mean")):
            with pytest.raises(ValueError):
                m.score_truth(Y, **kw)
        with pytest.raises(ValueError, match="shape"):
            m.score_truth(Y[:1])
        with pytest.raises(ValueError):
            m.score_truth(None)
    with pytest.raises(ValueError, match="R= is taken with X= only"):
        off.score_truth(Y, R=np.ones((2, 13, 13, 13)))
    from vimure_amd import VimureModel
    with pytest.raises(ValueError, match="has not been fitted"):
        VimureModel().score_truth(Y)


@pytest.mark.parametrize("tag", ["over", "under"])
def test_make_dataset_reproduces_the_reference_generated_inputs(tag):
    from vimure_amd.experiments import make_dataset
    from vimure_amd.synthetic import Multitensor
    d = np.load(os.path.join(GOLDEN, f"H_ref_f1_{tag}.npz"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gt = Multitensor(N=100, M=100, L=1, C=2, K=2, avg_degree=5, sparsify=True, seed=25, eta=0.2, exact=True)
        X, R, theta = make_dataset(gt, 0.1, tag, 25, eta=0.2, exact=True)
    Xd = X.toarray()
    xs = np.nonzero(Xd)
    assert np.array_equal(np.stack(xs), d["X_subs"]) and np.array_equal(Xd[xs], d["X_vals"])
    assert np.array_equal(np.stack(np.nonzero(R.toarray())), d["R_subs"])
    assert np.array_equal(gt.Y.toarray()[0], d["Y_true"])
    assert theta.shape == (1, 100) and sorted(set(theta.ravel())) == sorted({1.0, 50.0 if tag == "over" else 0.5})
