"""GPU: k-fold cross-validation (`crossval.cross_validate`, `compare_models`) on a small synthetic network with a self-reporter
mask: the folds' lists partition the support, no held-out entry lies inside its fold's training mask, every fold's device sums
agree with the restatement applied to that fold's own rho_f within the bounds of tests/heldout_util.py, the same seed reproduces
the frame, and two candidates run on identical folds.  Nothing is asserted about which model wins: that is a property of the
data, not of the code."""
import numpy as np
import pytest

from tests.heldout_util import compare_entries, compare_sums, term_size

pytestmark = pytest.mark.gpu

FIT = dict(max_iter=20, num_realisations=1)
_NET = {}


def _net():
    if not _NET:
        from vimure_amd.synthetic import standard_sbm
        net = standard_sbm(N=60, M=60, L=2, K=2, avg_degree=5.0, eta=0.3, seed=11, flag_self_reporter=True)
        _NET["X"], _NET["R"] = np.asarray(net.X).astype(np.uint8), np.asarray(net.R).astype(np.uint8)
    return _NET["X"], _NET["R"]


@pytest.fixture
def reproducible(monkeypatch):
    """Bit-reproducible fits (report lists, integer cross-workgroup sums), so that two runs of one seed give one frame."""
    monkeypatch.setenv("VMR_FORMAT", "sparse")
    monkeypatch.setenv("VMR_DETERMINISTIC", "1")


def test_three_folds_against_the_restatement(reproducible):
    from vimure_amd.crossval import cross_validate, heldout_loglik_np, train_mask
    X, R = _net()
    seen = {}

    def on_fold(f, model, subs_out, x_out, xt_out, tables):
        theta, lam, eta = tables
        Rt = train_mask(X, R, subs_out)
        want = heldout_loglik_np(model.rho_f, subs_out, x_out, xt_out, theta, lam, eta, R=Rt)
        got = model._engine.heldout_loglik(subs_out, x_out, xt_out, theta=theta, lam=lam, eta=eta)
        T = term_size(model.rho_f, subs_out, x_out, xt_out, theta, lam, eta)
        compare_entries(got, want, T, 2, f"fold {f}")
        assert np.allclose(theta, model.gamma_shp_f / model.gamma_rte_f) and np.isclose(eta, model.nu_shp_f / model.nu_rte_f)
        seen[f] = (got, want, T, subs_out, x_out)

    res = cross_validate(X, R, K=2, mutuality=True, n_folds=3, seed=4, on_fold=on_fold, **FIT)
    # the folds' lists partition the support
    assert np.array_equal(np.stack(res.subs), np.stack(np.nonzero(R)))
    assert sorted(set(res.folds.tolist())) == [0, 1, 2]
    l, i, j, m = res.subs
    mirror = {(a, b, c, d): q for a, b, c, d, q in zip(l.tolist(), i.tolist(), j.tolist(), m.tolist(), res.folds.tolist())}
    assert all(mirror[(a, c, b, d)] == q for (a, b, c, d), q in mirror.items())             # pairs are held out together
    assert res.counts[..., 0].sum() == len(res.folds) == int(R.sum())
    for f in range(3):
        assert res.counts[f, :, 0].tolist() == [int(((res.folds == f) & (l == q)).sum()) for q in range(2)]
    # no held-out entry inside its fold's training mask; every in-sample entry inside it
    assert (res.counts[..., 3] == 0).all() and np.array_equal(res.in_counts[..., 3], res.in_counts[..., 0])
    assert np.array_equal(res.in_counts[..., 0].sum(axis=1), res.counts[..., 0].sum(axis=1))  # same-sized samples
    # every fold's device sums against the restatement on that fold's rho_f
    assert sorted(seen) == [0, 1, 2]
    for f, (got, want, T, subs_out, x_out) in seen.items():
        assert np.array_equal(res.counts[f], want[3])
        assert np.array_equal(res.sums[f].view(np.uint64), got["sums"].view(np.uint64))     # (the driver's call, bit for bit)
        compare_sums(res.sums[f], want, subs_out, x_out, T, 2, f"fold {f}")
    assert np.isfinite(res.lpd).all() and np.isfinite(res.in_lpd).all() and (res.mse > 0).all()
    assert np.isclose(res.lpd_mean, res.lpd.mean()) and np.isclose(res.lpd_se, res.lpd.std(ddof=1) / np.sqrt(3))
    fr = res.frame()
    assert len(fr) == 6 and fr["n"].sum() == int(R.sum()) and (fr["n_in_mask"] == 0).all() and (fr["in_n_in_mask"] == fr["in_n"]).all()
    # the same seed reproduces the frame
    again = cross_validate(X, R, K=2, mutuality=True, n_folds=3, seed=4, **FIT)
    assert np.array_equal(again.folds, res.folds)
    assert fr.equals(again.frame()), (fr.compare(again.frame()))
    other = cross_validate(X, R, K=2, mutuality=True, n_folds=3, seed=5, **FIT)
    assert not np.array_equal(other.folds, res.folds)


def test_compare_models_runs_the_candidates_on_identical_folds():
    from vimure_amd.crossval import compare_models
    X, R = _net()
    cmp_ = compare_models(X, R, [dict(mutuality=True), dict(mutuality=False)], n_folds=3, seed=4, **FIT)
    a, b = cmp_.results
    assert a.mutuality and not b.mutuality
    assert np.array_equal(a.folds, b.folds) and all(np.array_equal(u, v) for u, v in zip(a.subs, b.subs))
    assert np.array_equal(a.counts[..., :2], b.counts[..., :2])                             # the same entries, the same counts
    assert (a.counts[..., 3] == 0).all() and (b.counts[..., 3] == 0).all()
    t = cmp_.table
    assert len(t) == 2 and sorted(t["candidate"].tolist()) == [0, 1] and sorted(t["mutuality"].tolist()) == [False, True]
    assert t["lpd"].iloc[0] >= t["lpd"].iloc[1] and t["d_lpd"].iloc[0] == 0.0 and t["d_lpd"].iloc[1] <= 0.0
    best, rest = cmp_.results[int(t["candidate"].iloc[0])], cmp_.results[int(t["candidate"].iloc[1])]
    d = rest.lpd - best.lpd
    assert np.isclose(t["d_lpd"].iloc[1], d.mean()) and np.isclose(t["d_lpd_se"].iloc[1], d.std(ddof=1) / np.sqrt(3))
