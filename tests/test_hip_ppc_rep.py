"""GPU: posterior predictive replicates reduced on the device (vmr_ppc_replicates) and the same reduction of the observed data
(vmr_ppc_observed).  A replicate's statistics are held, integer for integer, to the NumPy restatement (tests/ppc_rep_util.py)
of the dense replicate composed from the entry points that existed before (CaviEngine.sample, a torch gather of lambda,
vmr_generate_x) -- over both data layouts, every mask layout, the K = 3 and K = 12 kernels, coordinate-list handles, several
chunks; a wide reporter set (no dense replicate can exist) to its invariants; the totals to the model's own mean; the model's
method end to end."""
import os
import warnings

import numpy as np
import pytest

from tests.golden_util import GOLDEN, case_config, load_case
from tests.ppc_rep_util import compose_replicate, stats_coo, stats_np

pytestmark = pytest.mark.gpu

PRI = (0.1, 0.1, 10.0, 10.0, 0.5, 1.0)
SEED_Y, SEED_X = 1234, 98765


def _random_state(g, L, N, M, K, sparse_p=True):
    gs, gr = g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(2.0, 1.0, (L, M)) + 0.1
    ps, pr = g.gamma(5.0, 1.0, (L, K)) + 0.1, g.gamma(2.0, 1.0, (L, K)) + 0.1
    rho = g.rand(L, N, N, K)
    if sparse_p:
        rho[..., 0] *= 3.0
    rho = rho / rho.sum(-1, keepdims=True)       # rows sum to 1
    return gs, gr, ps, pr, 3.0, 2.5, rho


def _engine_for(X, R, K, st, mut=True, coo=False):
    from vimure_amd import CaviEngine
    if coo:
        xs = np.nonzero(X)
        eng = CaviEngine.from_coo(xs, X[xs], X.shape, R=None if R is None else np.nonzero(R), K=K, mutuality=mut)
    else:
        eng = CaviEngine(X, R, K=K, mutuality=mut)
    eng.set_priors(*PRI)
    if st is not None:
        eng.set_state(*st)
    return eng


def _params(g, n_rep, L, M, lam_row, eta=0.3):
    theta = 0.5 + 1.5 * g.rand(n_rep, L, M)
    lam = np.broadcast_to(np.asarray(lam_row, dtype=np.float64), (n_rep, L, len(lam_row))).copy()
    return theta, lam, np.full(n_rep, eta)


def _want(eng, R, theta, lam, eta, n_trials=1, seed_y=SEED_Y, seed_x=SEED_X):
    """(counts [n_rep, L, 6], by_reporter [n_rep, L, M, 2]) of the composed dense replicates."""
    cs, bs = [], []
    for r in range(len(eta)):
        X = compose_replicate(eng, r, theta, lam, eta, seed_y, seed_x, n_trials)
        assert X.max() < 255       # no clamp in the composition: it is the unclamped draw
        c, b = stats_np(X, R)
        cs.append(c)
        bs.append(b)
    return np.stack(cs), np.stack(bs)


def _assert_replicates(eng, R, theta, lam, eta, n_trials=1, want=None):
    want = want if want is not None else _want(eng, R, theta, lam, eta, n_trials)
    counts, by_rep = eng.ppc_replicates(theta, lam, eta, SEED_Y, SEED_X, n_trials=n_trials, by_reporter=True)
    assert counts.dtype == np.int64 and by_rep.dtype == np.int64
    assert np.array_equal(counts, want[0]), (counts, want[0])
    assert np.array_equal(by_rep, want[1])
    assert np.array_equal(eng.ppc_replicates(theta, lam, eta, SEED_Y, SEED_X, n_trials=n_trials), counts)   # without by_reporter
    assert counts[..., 0].min() > 0      # the case is not vacuous
    return want


# ---------------------------------------------------------------------------------------------- 1. the composition, exactly
_CASE1 = {}


def _case1():
    """L = 2, N = 23 (odd), M = 70 (crosses a 64-bit mask word), K = 2; Bernoulli(0.3) mask with rows forced empty and full."""
    if not _CASE1:
        g = np.random.RandomState(5)
        L, N, M, K = 2, 23, 70, 2
        X = (g.rand(L, N, N, M) < 0.05).astype(np.uint8) * g.randint(1, 4, (L, N, N, M)).astype(np.uint8)
        R = (g.rand(L, N, N, M) < 0.3).astype(np.uint8)
        R[0, 3, :5], R[1, 7, 10:13], R[0, 20, 22] = 0, 0, 0
        R[0, 4, :4], R[1, 22, 0], R[1, 0, 22], R[0, 9, 9] = 1, 1, 1, 1
        _CASE1.update(X=X, R=R, st=_random_state(g, L, N, M, K), par=_params(g, 3, L, M, (0.01, 1.5)), want={})
    return _CASE1


@pytest.mark.parametrize("n_trials", [1, 3])
@pytest.mark.parametrize("mask", ["none", "bernoulli"])
def test_replicates_equal_the_composition(mask, n_trials, vmr_format):
    c = _case1()
    R = c["R"] if mask == "bernoulli" else None
    eng = _engine_for(c["X"], R, 2, c["st"])
    try:
        assert eng.data_format()[0] == vmr_format
        # (a draw depends neither on the mask nor on the layout: one composition per n_trials serves every case)
        if n_trials not in c["want"]:
            c["want"][n_trials] = [compose_replicate(eng, r, *c["par"], SEED_Y, SEED_X, n_trials) for r in range(3)]
        Xs = c["want"][n_trials]
        assert max(int(X.max()) for X in Xs) < 255
        want = tuple(np.stack(v) for v in zip(*[stats_np(X, R) for X in Xs]))
        _assert_replicates(eng, R, *c["par"], n_trials=n_trials, want=want)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 2. mask lists, from_coo
def test_self_reporter_mask_through_from_coo():
    from vimure_amd.synthetic import self_reporter_mask
    g = np.random.RandomState(6)
    L, N, M, K = 1, 40, 40, 2
    R = self_reporter_mask(L, N, M)
    X = ((g.rand(L, N, N, M) < 0.3) & (R != 0)).astype(np.uint8)
    eng = _engine_for(X, R, K, _random_state(g, L, N, M, K), coo=True)
    try:
        assert eng.mask_format()[0] == "lists"
        par = _params(g, 3, L, M, (0.01, 1.5))
        # the composition draws every (pair, reporter) and R is applied in NumPy: a draw does not depend on the mask
        _assert_replicates(eng, R, *par)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 3. K = 3 golden, K = 12
def test_replicates_on_golden_k3():
    d = load_case("B_random_mask_K3")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    assert K == 3
    st = (d["fit_gamma_shp_f"], d["fit_gamma_rte_f"], d["fit_phi_shp_f"], d["fit_phi_rte_f"], float(d["fit_nu_shp_f"]),
          float(d["fit_nu_rte_f"]), d["fit_rho_f"])
    eng = _engine_for(d["X"], d["R"], K, st, mut=mut)
    try:
        L, M = d["X"].shape[0], d["X"].shape[3]
        _assert_replicates(eng, d["R"], *_params(np.random.RandomState(7), 2, L, M, (0.01, 0.8, 1.5)), n_trials=2)
    finally:
        eng.close()


def test_replicates_k12_general_kernels():
    g = np.random.RandomState(12)
    L, N, M, K = 2, 23, 70, 12
    X = (g.rand(L, N, N, M) < 0.05).astype(np.uint8)
    R = (g.rand(L, N, N, M) < 0.3).astype(np.uint8)
    eng = _engine_for(X, R, K, _random_state(g, L, N, M, K, sparse_p=False))
    try:
        assert eng.sweep_shape()[1] == 0     # (the general kernels: no LDS levels)
        theta, lam, eta = _params(g, 2, L, M, np.linspace(0.01, 1.5, K))
        lam[1, 1] = lam[1, 1, ::-1]          # the table is per replicate and per layer
        _assert_replicates(eng, R, theta, lam, eta, n_trials=3)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 4. observed statistics
_OBS_WANT = {}


@pytest.mark.parametrize("case", ["A_ones_mut", "B_random_mask_K3", "D_self_mask", "I_karnataka_vil1_money"])
def test_observed_statistics_on_golden_cases(case, vmr_format):
    d = load_case(case)
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    if case not in _OBS_WANT:
        _OBS_WANT[case] = stats_np(d["X"], d["R"])
    want = _OBS_WANT[case]
    st = (d["fit_gamma_shp_f"], d["fit_gamma_rte_f"], d["fit_phi_shp_f"], d["fit_phi_rte_f"], float(d["fit_nu_shp_f"]),
          float(d["fit_nu_rte_f"]), d["fit_rho_f"])
    eng = _engine_for(d["X"], d["R"], K, st, mut=mut)
    try:
        assert eng.data_format()[0] == vmr_format
        counts, by_rep = eng.ppc_observed(by_reporter=True)
        assert np.array_equal(counts, want[0]), (counts, want[0])
        assert np.array_equal(by_rep, want[1])
        assert np.array_equal(eng.ppc_observed(), counts)
        assert counts[:, 0].min() > 0
    finally:
        eng.close()


def test_observed_statistics_coo_counts_above_255():
    from vimure_amd import CaviEngine
    d = np.load(os.path.join(GOLDEN, "N_counts_12000.npz"))
    shape = tuple(int(s) for s in d["X_shape"])
    L, N, _, M = shape
    K = int(d["K"])
    subs = tuple(np.asarray(s, np.int64) for s in d["X_subs"])
    vals = np.asarray(d["X_vals"], np.int64)
    Rs = tuple(np.asarray(s, np.int64) for s in d["R_subs"])
    assert vals.max() > 255
    X, R = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
    X[subs], R[Rs] = vals, 1
    eng = CaviEngine.from_coo(subs, vals, shape, R=Rs, K=K)
    try:
        eng.set_priors(*PRI)
        eng.set_state(*_random_state(np.random.RandomState(1), L, N, M, K))
        counts, by_rep = eng.ppc_observed(by_reporter=True)
        want = stats_np(X, R)
        assert np.array_equal(counts, want[0]) and np.array_equal(by_rep, want[1])
        assert counts[0, 2] > 12000 ** 2
    finally:
        eng.close()


def test_observed_statistics_hand_made_coo():
    """N = M = 30: a partial mask with empty and full rows, reports outside the mask, diagonal entries in S, mutual pairs."""
    g = np.random.RandomState(8)
    L, N, M, K = 2, 30, 30, 2
    R = (g.rand(L, N, N, M) < 0.2).astype(np.uint8)
    R[0, 2], R[1, :, 5], R[0, 7, 7], R[1, 3, 4] = 0, 0, 1, 1
    X = ((g.rand(L, N, N, M) < 0.25) * g.randint(1, 300, (L, N, N, M))).astype(np.int64)
    X[0, 7, 7, :3], X[1, 3, 4, :], X[1, 4, 3, :] = 2, 1, 1
    eng = _engine_for(X, R, K, _random_state(g, L, N, M, K), coo=True)
    try:
        counts, by_rep = eng.ppc_observed(by_reporter=True)
        want = stats_np(X, R)
        assert np.array_equal(counts, want[0]) and np.array_equal(by_rep, want[1])
        assert counts[:, 3].min() > 0 and counts[:, 5].min() > 0
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 5. chunks, launches, seeds
def test_chunk_and_launch_independence(monkeypatch):
    c = _case1()
    g = np.random.RandomState(9)
    L, M = 2, 70
    theta, lam, eta = _params(g, 5, L, M, (0.01, 1.5))
    eta[:] = [0.3, 0.0, 0.5, 0.1, 0.7]
    monkeypatch.delenv("VMR_NETSTATS_CHUNK", raising=False)
    eng = _engine_for(c["X"], c["R"], 2, c["st"])
    try:
        one = eng.ppc_replicates(theta, lam, eta, SEED_Y, SEED_X, n_trials=2, by_reporter=True)
        again = eng.ppc_replicates(theta, lam, eta, SEED_Y, SEED_X, n_trials=2, by_reporter=True)
        assert np.array_equal(one[0], again[0]) and np.array_equal(one[1], again[1])
        for r in range(5):
            single = eng.ppc_replicates(theta[r:r + 1], lam[r:r + 1], eta[r:r + 1], SEED_Y + r, SEED_X + r, n_trials=2, by_reporter=True)
            assert np.array_equal(single[0][0], one[0][r]) and np.array_equal(single[1][0], one[1][r])
        assert len({tuple(one[0][r].ravel()) for r in range(5)}) == 5
        # seed_y = 2^64 - 1 wraps: its second replicate draws Y with seed 0
        top = 2 ** 64 - 1
        w = eng.ppc_replicates(theta[:2], lam[:2], eta[:2], top, SEED_X)
        z = eng.ppc_replicates(theta[1:2], lam[1:2], eta[1:2], 0, SEED_X + 1)
        assert np.array_equal(w[1], z[0])
        want = _want(eng, c["R"], theta[:2], lam[:2], eta[:2], seed_y=top)
        assert np.array_equal(w, want[0])
    finally:
        eng.close()
    monkeypatch.setenv("VMR_NETSTATS_CHUNK", "2")      # 5 = 2 + 2 + 1
    eng = _engine_for(c["X"], c["R"], 2, c["st"])
    try:
        many = eng.ppc_replicates(theta, lam, eta, SEED_Y, SEED_X, n_trials=2, by_reporter=True)
    finally:
        eng.close()
    assert np.array_equal(many[0], one[0]) and np.array_equal(many[1], one[1])


# ---------------------------------------------------------------------------------------------- 6. wide reporter sets
def test_wide_reporters_self_reporter_coo():
    """N = M = 8200: beyond the 8192 reporters of the specialised kernels; 300 reporters (node 8199 among them) with the
    self-reporter mask the edgelist reader builds.  A dense replicate would take 5.5e11 bytes."""
    import torch
    from vimure_amd import CaviEngine
    from vimure_amd._io import self_reporter_coo
    g = np.random.RandomState(10)
    L, N, M, K = 1, 8200, 8200, 2
    reps = np.unique(np.concatenate([g.choice(N - 1, 299, replace=False), [N - 1]]))
    Rs = self_reporter_coo(L, N, reps)
    pick = g.rand(len(Rs[0])) < 0.01
    out = (np.zeros(50, np.int64), g.randint(0, N, 50), g.randint(0, N, 50), g.randint(0, M, 50))      # reports outside the mask
    key = np.unique(np.concatenate([np.ravel_multi_index(tuple(s[pick] for s in Rs), (L, N, N, M)), np.ravel_multi_index(out, (L, N, N, M))]))
    subs = tuple(np.asarray(s, np.int64) for s in np.unravel_index(key, (L, N, N, M)))
    vals = 1 + g.randint(0, 400, len(key))
    eng = CaviEngine.from_coo(subs, vals, (L, N, N, M), R=Rs, K=K)
    try:
        assert eng.data_format()[0] == "sparse" and eng.mask_format() == ("lists", len(Rs[0]))
        assert eng.sweep_shape()[1] == 0      # (the general kernels: no LDS levels)
        eng.set_priors(*PRI)
        pr = torch.empty((L, N, N, K), dtype=torch.float64, device=f"cuda:{eng.device}")
        pr[..., 0], pr[..., 1] = 0.7, 0.3
        eng.set_state(np.ones((L, M)), np.ones((L, M)), np.ones((L, K)), np.ones((L, K)), 1.0, 2.0, pr)
        del pr
        theta, lam, eta = _params(g, 2, L, M, (0.05, 1.5))
        counts, by_rep = eng.ppc_replicates(theta, lam, eta, SEED_Y, SEED_X, by_reporter=True)
        again = eng.ppc_replicates(theta, lam, eta, SEED_Y, SEED_X, by_reporter=True)
        assert np.array_equal(counts, again[0]) and np.array_equal(by_rep, again[1])
        assert np.array_equal(by_rep.sum(axis=2), counts[:, :, :2])
        n_pos, total, sumsq, mutual, reported, agreed = (counts[..., k] for k in range(6))
        assert np.all(agreed <= reported) and np.all(reported <= n_pos) and np.all(n_pos <= total) and np.all(mutual <= n_pos)
        assert np.all(agreed > 0) and np.all(mutual > 0)
        silent = np.setdiff1d(np.arange(M), reps)
        assert not by_rep[:, :, silent].any() and by_rep[:, :, N - 1, 0].min() > 0
        oc, ob = eng.ppc_observed(by_reporter=True)
        want = stats_coo(subs, vals, Rs, (L, N, N, M))
        assert np.array_equal(oc, want[0]) and np.array_equal(ob, want[1])
        assert oc[0, 0] < len(vals)           # (the reports outside the mask are not counted)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 7. the model's own mean
def test_totals_agree_with_the_models_mean():
    """Independent of generate.hip's composition: with first ~ Poisson((a + eta b) / (1 - eta^2)) and second ~ Poisson(b + eta
    first), E[x_ij] = (a + eta b) / (1 - eta^2) in either order, so E[total] = sum_{i != j, m} theta_m (E[lam_ij] + eta E[lam_ji]) /
    (1 - eta^2) with E[lam_ij] = sum_k rho_ijk lambda_k (n_trials = 1).  The mean of 64 totals must lie within 5 standard errors
    (from the replicates' own sample variance)."""
    g = np.random.RandomState(11)
    L, N, M, K, S = 1, 40, 30, 2, 64
    X = (g.rand(L, N, N, M) < 0.1).astype(np.uint8)
    eng = _engine_for(X, None, K, _random_state(g, L, N, M, K))
    try:
        theta1, lam1, eta1 = 0.5 + 1.5 * g.rand(L, M), np.array([[0.01, 1.5]]), 0.3
        theta, lam, eta = np.broadcast_to(theta1, (S, L, M)), np.broadcast_to(lam1, (S, L, K)), np.full(S, eta1)
        counts = eng.ppc_replicates(theta, lam, eta, SEED_Y, SEED_X)
        rho = eng.get_state()["rho"]
    finally:
        eng.close()
    el = (rho[0] * lam1[0]).sum(-1)                      # E[lam_ij]
    pair = (el + eta1 * el.T) / (1.0 - eta1 * eta1)
    np.fill_diagonal(pair, 0.0)
    expected = pair.sum() * theta1[0].sum()
    tot = counts[:, 0, 1].astype(np.float64)
    se = tot.std(ddof=1) / np.sqrt(S)
    print("expected %.3f mean %.3f se %.3f" % (expected, tot.mean(), se))
    assert abs(tot.mean() - expected) <= 5.0 * se


# ---------------------------------------------------------------------------------------------- 8. the model's method
def test_model_posterior_predictive_check():
    from vimure_amd import VimureModel
    from vimure_amd.synthetic import standard_sbm
    net = standard_sbm(N=60, M=60, K=2, seed=0)

    def fit(**kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return VimureModel().fit(net.X, R=net.R, K=2, seed=3, num_realisations=1, max_iter=21, **kw)

    m = fit(keep_engine=True)
    n_rep = 6
    res = m.posterior_predictive_check(n_rep=n_rep, seed=41, by_reporter=True)
    assert res.observed.shape == (m.L, 6) and res.replicated.shape == (n_rep, m.L, 6)
    assert res.observed_by_reporter.shape == (m.L, m.M, 2) and res.replicated_by_reporter.shape == (n_rep, m.L, m.M, 2)
    assert (res.seed_y, res.seed_x) == (41, 41 + 2 ** 32) and res.theta.shape == (n_rep, m.L, m.M) and res.eta.shape == (n_rep,)
    assert res.p_values().shape == (m.L, 6) and res.p_values_by_reporter().shape == (m.L, m.M, 2)
    assert len(res.summary()) == 6 * m.L
    assert res.support.tolist() == [m._engine.mean_poisson_size(layer=l) for l in range(m.L)]
    Xd, Rd = np.asarray(net.X), (np.asarray(net.R) if net.R is not None else None)
    want = stats_np(Xd, Rd)
    assert np.array_equal(res.observed, want[0]) and np.array_equal(res.observed_by_reporter, want[1])
    same = m.posterior_predictive_check(n_rep=n_rep, seed=41, by_reporter=True)
    other = m.posterior_predictive_check(n_rep=n_rep, seed=42)
    assert np.array_equal(same.replicated, res.replicated) and np.array_equal(same.replicated_by_reporter, res.replicated_by_reporter)
    assert not np.array_equal(other.replicated, res.replicated) and np.array_equal(other.observed, res.observed)
    mean = m.posterior_predictive_check(n_rep=2, params="mean")           # seed None: the fit's
    assert mean.seed_y == m.seed and np.array_equal(mean.theta[0], m.gamma_shp_f / m.gamma_rte_f) and mean.eta_redraws == 0
    m.close()
    with pytest.raises(ValueError, match="keep_engine=True"):
        m.posterior_predictive_check(n_rep=2)
    tmp = m.posterior_predictive_check(n_rep=n_rep, seed=41, by_reporter=True, X=net.X, R=net.R)     # a temporary engine
    assert np.array_equal(tmp.replicated, res.replicated) and np.array_equal(tmp.observed, res.observed)
    assert np.array_equal(tmp.replicated_by_reporter, res.replicated_by_reporter)


# ---------------------------------------------------------------------------------------------- 9. errors
def test_errors_on_a_live_handle():
    from vimure_amd import _lib
    from vimure_amd.engine import EngineError
    c = _case1()
    theta, lam, eta = (np.ascontiguousarray(a) for a in c["par"])
    eng = _engine_for(c["X"], c["R"], 2, None)
    try:
        with pytest.raises(EngineError, match="vmr_set_state"):
            eng.ppc_replicates(theta, lam, eta, 1, 2)
        with pytest.raises(EngineError, match="vmr_set_state"):
            eng.ppc_observed()
        counts = np.zeros((3, eng.L, 6), np.uint64)
        args = (theta.ctypes.data, lam.ctypes.data, eta.ctypes.data)
        assert eng.lib.vmr_ppc_replicates(eng._h, 3, 1, 2, 1, *args, counts.ctypes.data, None) == _lib.VMR_ESTATE
        eng.set_state(*c["st"])
        bad = eta.copy()
        bad[1] = 1.0
        with pytest.raises(ValueError, match=r"The mutuality parameter has to be in \[0, 1\)!"):
            eng.ppc_replicates(theta, lam, bad, 1, 2)
        neg = theta.copy()
        neg[2, 1, 69] = -0.5
        with pytest.raises(ValueError, match="theta"):
            eng.ppc_replicates(neg, lam, eta, 1, 2)
        inf = lam.copy()
        inf[0, 0, 1] = np.inf
        with pytest.raises(ValueError, match="lambda"):
            eng.ppc_replicates(theta, inf, eta, 1, 2)
        assert eng.lib.vmr_ppc_replicates(eng._h, 0, 1, 2, 1, *args, counts.ctypes.data, None) == _lib.VMR_EINVAL
        assert b"n_rep" in eng.lib.vmr_last_error(eng._h)
        with pytest.raises(ValueError, match="n_trials"):
            eng.ppc_replicates(theta, lam, eta, 1, 2, n_trials=0)
        assert eng.lib.vmr_ppc_replicates(eng._h, 3, 1, 2, 1, *args, None, None) == _lib.VMR_EINVAL
        assert b"NULL" in eng.lib.vmr_last_error(eng._h)
        assert eng.lib.vmr_ppc_observed(eng._h, None, None) == _lib.VMR_EINVAL
        with pytest.raises(ValueError, match="expected"):
            eng.ppc_replicates(theta[:, :, :5], lam, eta, 1, 2)
        assert eng.ppc_replicates(theta, lam, eta, 1, 2).shape == (3, eng.L, 6)      # the handle still works
        assert eng.ppc_observed().shape == (eng.L, 6)
    finally:
        eng.close()
