"""GPU: expected reports and report AUC on the device (vmr_mean_poisson, vmr_report_auc; the reference's
`_calculate_mean_poisson`, model.py:1220-1293, and `utils.calculate_AUC`, utils.py:40-66).  Held to the reference's recorded
values (tests/golden/P_mean_poisson_*.npz), to the NumPy restatement of the contract (tests/ppc_util.py) and to the exact
rank statistic on the host, over both data layouts, every mask kind, packed and two-word entries and a wide handle."""
import warnings
from fractions import Fraction

import numpy as np
import pytest
import scipy.special as sp

from tests.golden_util import case_config, load_case
from tests.ppc_util import PPC_CASES, dense_of, load_ppc, mean_poisson_np

pytestmark = pytest.mark.gpu


def _geo(shp, rte):
    return np.exp(sp.psi(shp) - np.log(rte))


def _engine_for(X, R, K, mut, st, coo=False):
    """An engine holding X and R, set to the state st = (gamma_shp, gamma_rte, phi_shp, phi_rte, nu_shp, nu_rte, rho)."""
    from vimure_amd import CaviEngine
    if coo:
        xs = np.nonzero(X)
        eng = CaviEngine.from_coo(xs, X[xs], X.shape, R=None if R is None else np.nonzero(R), K=K, mutuality=mut)
    else:
        eng = CaviEngine(X, R, K=K, mutuality=mut)
    L, M = X.shape[0], X.shape[3]
    eng.set_priors(0.1 * np.ones((L, M)), 0.1 * np.ones((L, M)), 10.0 * np.ones((L, K)), 10.0 * np.ones((L, K)), 0.5, 1.0)
    eng.set_state(*st)
    return eng


def _golden_state(d):
    return (d["fit_gamma_shp_f"], d["fit_gamma_rte_f"], d["fit_phi_shp_f"], d["fit_phi_rte_f"], float(d["fit_nu_shp_f"]),
            float(d["fit_nu_rte_f"]), d["fit_rho_f"])


def _check_against_reference(eng, d, p, auc_tol=1e-12):
    """auc_tol: how close the device AUC must come to the reference's.  Without mutuality most ties of these cases carry a
    rho within rounding of one-hot, and their scores tie, or nearly, across ties; G_theta and G_lambda, computed on the device
    to within an ulp of scipy's, then order a few such pairs the other way (1e-7 of the AUC).  The device AUC is held EXACTLY
    to the rank statistic of its own values in every case."""
    from vimure_amd.utils import calculate_AUC
    subs, vals = eng.mean_poisson()
    S = np.stack(subs).astype(np.int64)
    key = np.ravel_multi_index(tuple(S), d["X"].shape)
    assert np.all(np.diff(key) > 0)                                  # lexicographic (l,i,j,m)
    assert np.array_equal(S, p["mp_subs"].astype(np.int64))
    np.testing.assert_allclose(vals, p["mp_vals"], rtol=1e-13, atol=0)
    for l in range(d["X"].shape[0]):
        auc, npos, nneg = eng.report_auc(layer=l)
        assert abs(auc - p["auc_layer"][l]) <= auc_tol
        dense = dense_of(subs, vals, d["X"].shape)
        assert abs(auc - calculate_AUC(dense[l], d["X"][l], mask=d["R"][l])) <= 1e-12
        sl, vl = eng.mean_poisson(layer=l)
        assert np.all(sl[0] == l) and np.array_equal(vl, vals[S[0] == l])
        assert npos + nneg == len(vl)
    auc, npos, nneg = eng.report_auc()
    assert abs(auc - float(p["auc_all"])) <= auc_tol
    assert abs(auc - calculate_AUC(dense_of(subs, vals, d["X"].shape), d["X"], mask=d["R"])) <= 1e-12
    assert npos == int(((d["X"] > 0) & (d["R"] > 0)).sum()) and npos + nneg == len(vals)


@pytest.mark.parametrize("case", [c for c in PPC_CASES if c != "L_default_K12"])
def test_engine_matches_reference(case, vmr_format):
    d, p = load_case(case), load_ppc(case)
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        assert eng.data_format()[0] == vmr_format
        _check_against_reference(eng, d, p, auc_tol=1e-12 if mut else 1e-6)
    finally:
        eng.close()


def test_engine_matches_reference_k12_general_kernels():
    d, p = load_case("L_default_K12"), load_ppc("L_default_K12")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    assert K == 12
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        _check_against_reference(eng, d, p)
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["B_random_mask_K3", "D_self_mask"])
def test_mask_words_instead_of_lists(case, monkeypatch):
    monkeypatch.setenv("VMR_NO_RLISTS", "1")
    d, p = load_case(case), load_ppc(case)
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        assert eng.mask_format()[0] == "words"
        _check_against_reference(eng, d, p)
    finally:
        eng.close()


def test_coo_self_mask_matches_reference():
    d, p = load_case("D_self_mask"), load_ppc("D_self_mask")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d), coo=True)
    try:
        _check_against_reference(eng, d, p)
    finally:
        eng.close()


def _random_state(g, L, N, M, K, rho_values=None):
    gs, gr = g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(2.0, 1.0, (L, M)) + 0.1
    ps, pr = g.gamma(5.0, 1.0, (L, K)) + 0.1, g.gamma(2.0, 1.0, (L, K)) + 0.1
    rho = g.rand(L, N, N, K) if rho_values is None else rho_values
    rho = rho / rho.sum(-1, keepdims=True)
    return gs, gr, ps, pr, 3.0, 2.5, rho


def _check_restatement(eng, X, R, st, mut, layer=None):
    gs, gr, ps, pr, ns, nr, rho = st
    subs, vals = mean_poisson_np(X, R, rho, _geo(gs, gr), _geo(ps, pr), float(_geo(ns, nr)), mut)
    s_dev, v_dev = eng.mean_poisson()
    assert np.array_equal(np.stack(s_dev).astype(np.int64), np.stack(subs))
    np.testing.assert_allclose(v_dev, vals, rtol=1e-13, atol=0)
    # bit for bit where the inputs are the same bits: the restatement's G are scipy's, the device's its own (an ulp apart at
    # most), so the device's score is held to the restatement evaluated at the device's own G
    gth, gla, gnu = eng.get_geometric()[:3]
    vals_dev_g = mean_poisson_np(X, R, eng.get_state()["rho"], gth, gla, float(gnu), mut)[1]
    assert np.array_equal(v_dev, vals_dev_g), int((v_dev != vals_dev_g).sum())
    from vimure_amd.utils import calculate_AUC
    mp = dense_of(subs, vals, X.shape)
    auc = eng.report_auc()[0]
    assert abs(auc - calculate_AUC(mp, X, mask=np.ones(X.shape) if R is None else R)) <= 1e-12
    return s_dev, v_dev


def test_wide_coo_handle_and_two_word_entries():
    """M = 9000 > 8192 (a wide handle: two-word entries, general kernels, mask lists of three reporters per tie), counts up to
    5000, reports outside the mask."""
    g = np.random.RandomState(3)
    L, N, M, K = 1, 36, 9000, 2
    R = np.zeros((L, N, N, M), np.uint8)
    ii, jj = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    R[0, ii, jj, ii] = 1
    R[0, ii, jj, jj] = 1
    R[0, ii, jj, 8200 + (7 * ii + jj) % 700] = 1
    R[0, 3, 5] = 0                                                   # an empty row
    X = np.zeros((L, N, N, M), np.int32)
    sup = np.nonzero(R)
    pick = g.rand(len(sup[0])) < 0.3
    X[tuple(s[pick] for s in sup)] = g.randint(1, 5000, int(pick.sum()))
    out = (g.randint(0, L, 40), g.randint(0, N, 40), g.randint(0, N, 40), g.randint(0, M, 40))
    X[out] = g.randint(1, 4, 40)
    st = _random_state(g, L, N, M, K)
    for mut in (True, False):
        eng = _engine_for(X, R, K, mut, st, coo=True)
        try:
            _check_restatement(eng, X, R, st, mut)
        finally:
            eng.close()


def test_mask_lists_with_m_past_one_group(monkeypatch):
    """M = 70: a group is 64 lanes, so an all-ones row takes a full round and a round of six; the listed rows hold the
    reporters either side of the group's edge (63, 64) and the last one (69); one row is empty.  (Report lists: a handle of
    dense tiles keeps its partial rows as mask words.)"""
    monkeypatch.setenv("VMR_FORMAT", "sparse")
    g = np.random.RandomState(11)
    L, N, M, K = 1, 12, 70, 3
    R = np.zeros((L, N, N, M), np.uint8)
    ii, jj = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    for m in (ii, jj, 63 + 0 * ii, 64 + 0 * ii, 69 + 0 * ii):
        R[0, ii, jj, m] = 1
    R[0, (ii + jj) % 5 == 0] = 1                                     # all-ones rows
    R[0, 2, 7] = 0                                                   # an empty row
    X = np.where(g.rand(L, N, N, M) < 0.2, g.randint(1, 6, (L, N, N, M)), 0).astype(np.int32)   # reports outside the mask too
    st = _random_state(g, L, N, M, K)
    for mut in (True, False):
        eng = _engine_for(X, R, K, mut, st)
        try:
            assert eng.data_format()[0] == "sparse" and eng.mask_format()[0] == "lists"
            _check_restatement(eng, X, R, st, mut)
        finally:
            eng.close()


def _fit_case(name, **kw):
    from vimure_amd import VimureModel
    d = load_case(name)
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VimureModel(mutuality=bool(d["mutuality"]), undirected=und)
        m.fit(d["X"], R=d["R"], K=K, seed=seed, rho_prior=rho_prior, **priors, **fitargs, **kw)
    return d, m


@pytest.mark.parametrize("case", ["A_ones_mut", "B_random_mask_K3"])
def test_model_kept_engine_temporary_engine_and_numpy_agree(case):
    import torch
    from vimure_amd.utils import calculate_AUC
    d, m = _fit_case(case, keep_engine=True)
    mp_kept = m.calculate_mean_poisson()
    mp_dev = m.calculate_mean_poisson(device=True)
    auc_kept = m.report_auc()
    layers = [m.calculate_mean_poisson(layer=l) for l in range(m.L)]
    auc_layers = [m.report_auc(layer=l) for l in range(m.L)]
    m.close()
    with pytest.raises(ValueError, match="keep_engine=True"):
        m.calculate_mean_poisson()
    mp_tmp = m.calculate_mean_poisson(X=d["X"], R=d["R"])
    auc_tmp = m.report_auc(X=d["X"], R=d["R"])
    subs, vals = mean_poisson_np(d["X"], d["R"], m.rho_f, m.G_exp_theta_f, m.G_exp_lambda_f, float(m.G_exp_nu_f), m.mutuality)
    for mp in (mp_kept, mp_tmp):
        assert mp.shape == d["X"].shape
        assert np.array_equal(np.stack(mp.subs), np.stack(subs))
        np.testing.assert_allclose(mp.vals, vals, rtol=1e-13, atol=0)
    assert isinstance(mp_dev.vals, torch.Tensor) and mp_dev.vals.is_cuda
    assert np.array_equal(mp_dev.vals.cpu().numpy(), mp_kept.vals)
    for a, b in zip(mp_dev.subs, mp_kept.subs):
        assert np.array_equal(a.cpu().numpy().astype(np.int64), b)
    dense = dense_of(mp_kept.subs, mp_kept.vals, d["X"].shape)
    ref = calculate_AUC(dense, d["X"], mask=d["R"])
    assert abs(auc_kept - ref) <= 1e-12 and abs(auc_tmp - ref) <= 1e-12
    for l in range(m.L):
        sel = mp_kept.subs[0] == l
        assert np.array_equal(layers[l].vals, mp_kept.vals[sel])
        assert np.array_equal(np.stack(layers[l].subs), np.stack([s[sel] for s in mp_kept.subs]))
        assert abs(auc_layers[l] - calculate_AUC(dense[l], d["X"][l], mask=d["R"][l])) <= 1e-12


@pytest.mark.parametrize("fmt", ["sparse", "dense"])
def test_exact_ties_give_the_rational_auc(fmt, monkeypatch):
    """Equal theta for every reporter, no mutuality, rho one of two vectors per tie: two distinct scores, every other pair a tie."""
    monkeypatch.setenv("VMR_FORMAT", fmt)
    g = np.random.RandomState(11)
    L, N, M, K = 1, 12, 5, 2
    X = (g.rand(L, N, N, M) < 0.3).astype(np.uint8) * g.randint(1, 3, (L, N, N, M)).astype(np.uint8)
    R = (g.rand(L, N, N, M) < 0.6).astype(np.uint8)
    hi = g.rand(L, N, N) < 0.4
    rho = np.where(hi[..., None], np.array([0.25, 0.75]), np.array([0.875, 0.125]))
    st = (np.full((L, M), 2.0), np.full((L, M), 1.5), np.array([[3.0, 9.0]]), np.array([[1.0, 1.0]]), 3.0, 2.5, rho)
    eng = _engine_for(X, R, K, False, st)
    try:
        auc, npos, nneg = eng.report_auc()
    finally:
        eng.close()
    sup = R > 0
    pos, hi4 = sup & (X > 0), np.broadcast_to(hi[..., None], X.shape)
    P, Q = int(pos.sum()), int((sup & ~pos).sum())
    ph, pl = int((pos & hi4).sum()), int((pos & ~hi4).sum())
    nh, nl = int((sup & ~pos & hi4).sum()), int((sup & ~pos & ~hi4).sum())
    want = Fraction(2 * ph * nl + ph * nh + pl * nl, 2 * P * Q)     # high scores beat low ones; equal scores count half
    assert (npos, nneg) == (P, Q)
    assert auc == float(want)


def test_repeat_calls_are_bit_identical(monkeypatch):
    monkeypatch.delenv("VMR_DETERMINISTIC", raising=False)
    from vimure_amd.synthetic import standard_sbm
    net = standard_sbm(N=120, M=20, L=2, K=2, avg_degree=4.0, eta=0.4, seed=5)
    g = np.random.RandomState(2)
    R = (g.rand(*net.X.shape) < 0.7).astype(np.uint8)
    st = _random_state(g, 2, 120, 20, 3)
    eng = _engine_for(net.X, R, 3, True, st)
    try:
        a = eng.mean_poisson()
        b = eng.mean_poisson()
        assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
        assert eng.report_auc() == eng.report_auc()
        assert eng.report_auc(layer=1) == eng.report_auc(layer=1)
    finally:
        eng.close()


def test_restored_handle_reads_the_snapshot():
    g = np.random.RandomState(4)
    L, N, M, K = 1, 20, 6, 2
    X = (g.rand(L, N, N, M) < 0.2).astype(np.uint8)
    st = _random_state(g, L, N, M, K)
    eng = _engine_for(X, None, K, True, st)
    try:
        want = eng.mean_poisson()
        eng.snapshot()
        eng.step(3)
        eng.restore()
        got = eng.mean_poisson()
        assert np.array_equal(got[1], want[1])
        _check_restatement(eng, X, None, st, True)
    finally:
        eng.close()


def test_medium_sbm_fit():
    from vimure_amd import VimureModel
    from vimure_amd.synthetic import standard_sbm
    from vimure_amd.utils import calculate_AUC
    net = standard_sbm(N=500, M=50, L=1, K=2, avg_degree=10.0, eta=0.3, seed=8)
    R = (np.random.RandomState(1).rand(*net.X.shape) < 0.3).astype(np.uint8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VimureModel().fit(net.X, R=R, K=2, seed=3, max_iter=30, keep_engine=True)
    mp = m.calculate_mean_poisson()
    auc = m.report_auc()
    subs, vals = mean_poisson_np(net.X, R, m.rho_f, m.G_exp_theta_f, m.G_exp_lambda_f, float(m.G_exp_nu_f), True)
    m.close()
    assert np.array_equal(np.stack(mp.subs), np.stack(subs))
    np.testing.assert_allclose(mp.vals, vals, rtol=1e-13, atol=0)
    assert abs(auc - calculate_AUC(dense_of(subs, vals, net.X.shape), net.X, mask=R)) <= 1e-12
