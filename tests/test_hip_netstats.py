"""GPU: network statistics of posterior samples and their expectations on the device (vmr_sample_stats, vmr_expected_stats).
Every count is held, integer for integer, to the NumPy restatement (tests/netstats_util.py) of the samples `CaviEngine.sample`
returns for the same seeds, over both data layouts, the general kernels (K = 12, 16), a coordinate-list handle, several chunks;
the expectations to NumPy on the rho read back; sampling to its expectation; the model's method to `sample_inferred_model`."""
import warnings

import numpy as np
import pytest

from tests.golden_util import case_config, load_case
from tests.netstats_util import stats_np

pytestmark = pytest.mark.gpu

KEYS = ("edges", "weight", "mutual", "tp", "deg_out", "deg_in")


def _engine_for(X, R, K, mut, st, coo=False):
    from vimure_amd import CaviEngine
    if coo:
        xs = np.nonzero(X)
        eng = CaviEngine.from_coo(xs, X[xs], X.shape, R=None if R is None else np.nonzero(R), K=K, mutuality=mut)
    else:
        eng = CaviEngine(X, R, K=K, mutuality=mut)
    L, M = X.shape[0], X.shape[3]
    eng.set_priors(0.1 * np.ones((L, M)), 0.1 * np.ones((L, M)), 10.0 * np.ones((L, K)), 10.0 * np.ones((L, K)), 0.5, 1.0)
    if st is not None:
        eng.set_state(*st)
    return eng


def _golden_state(d):
    return (d["fit_gamma_shp_f"], d["fit_gamma_rte_f"], d["fit_phi_shp_f"], d["fit_phi_rte_f"], float(d["fit_nu_shp_f"]),
            float(d["fit_nu_rte_f"]), d["fit_rho_f"])


def _random_state(g, L, N, M, K, sparse_p=False):
    gs, gr = g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(2.0, 1.0, (L, M)) + 0.1
    ps, pr = g.gamma(5.0, 1.0, (L, K)) + 0.1, g.gamma(2.0, 1.0, (L, K)) + 0.1
    rho = g.rand(L, N, N, K)
    if sparse_p:
        rho[..., 0] *= 6.0   # most of the mass on "no edge": a network, not noise
    rho = rho / rho.sum(-1, keepdims=True)
    return gs, gr, ps, pr, 3.0, 2.5, rho


def _assert_equal_stats(got, want):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


def _check_exact(eng, seed, S, Y_ref, trials=(1, 3)):
    for n_trials in trials:
        Ys = [eng.sample(seed + s, n_trials) for s in range(S)]
        _assert_equal_stats(eng.sample_stats(seed, S, n_trials=n_trials, Y_ref=Y_ref, degrees=True), stats_np(Ys, Y_ref))
        plain = eng.sample_stats(seed, S, n_trials=n_trials)
        assert "deg_out" not in plain and not plain["tp"].any()
        assert np.array_equal(plain["mutual"], stats_np(Ys)["mutual"])


@pytest.mark.parametrize("case", ["A_ones_mut", "B_random_mask_K3", "D_self_mask", "E_undirected"])
def test_counts_equal_numpy_on_the_samples(case, vmr_format):
    d = load_case(case)
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        assert eng.data_format()[0] == vmr_format
        _check_exact(eng, 11, 8, np.argmax(d["fit_rho_f"], -1))
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["L_default_K12", "M_K16_nomut"])
def test_counts_equal_numpy_general_kernels(case):
    d = load_case(case)
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    assert K > 8
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        _check_exact(eng, 5, 8, np.argmax(d["fit_rho_f"], -1))
    finally:
        eng.close()


def test_counts_equal_numpy_coo_handle():
    d = load_case("D_self_mask")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d), coo=True)
    try:
        _check_exact(eng, 3, 8, np.argmax(d["fit_rho_f"], -1))
    finally:
        eng.close()


def _medium(g, K=3):
    from vimure_amd.synthetic import standard_sbm
    L, N, M = 2, 300, 12
    net = standard_sbm(N=N, M=M, L=L, K=2, avg_degree=6.0, eta=0.4, seed=9)
    return net.X, _random_state(g, L, N, M, K, sparse_p=True)


def test_medium_case_several_blocks_and_chunks(vmr_format, monkeypatch):
    """L = 2, N = 300, K = 3: five strips of rows (the last one partial), a non-trivial perm on report lists, and chunks of 5
    samples (16 = 5 + 5 + 5 + 1) against one chunk."""
    g = np.random.RandomState(21)
    X, st = _medium(g)
    Y_ref = (g.rand(2, 300, 300) < 0.1).astype(np.uint8)
    monkeypatch.delenv("VMR_NETSTATS_CHUNK", raising=False)
    eng = _engine_for(X, None, 3, True, st)
    try:
        assert eng.data_format()[0] == vmr_format
        _check_exact(eng, 1000, 16, Y_ref)
        one = eng.sample_stats(1000, 16, n_trials=3, Y_ref=Y_ref, degrees=True)
        import torch
        dev = eng.sample_stats(1000, 16, n_trials=3, Y_ref=torch.from_numpy(Y_ref).cuda(), degrees=True)
        _assert_equal_stats(dev, one)
    finally:
        eng.close()
    monkeypatch.setenv("VMR_NETSTATS_CHUNK", "5")
    eng = _engine_for(X, None, 3, True, st)
    try:
        many = eng.sample_stats(1000, 16, n_trials=3, Y_ref=Y_ref, degrees=True)
    finally:
        eng.close()
    _assert_equal_stats(many, one)


def test_repeat_calls_identical_and_seed_wraps():
    d = load_case("B_random_mask_K3")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        a = eng.sample_stats(77, 6, n_trials=2, degrees=True)
        b = eng.sample_stats(77, 6, n_trials=2, degrees=True)
        _assert_equal_stats(a, b)
        top = 2 ** 64 - 1
        w = eng.sample_stats(top, 2, degrees=True)
        Ys = [eng.sample((top + s) % 2 ** 64) for s in range(2)]
        _assert_equal_stats(w, stats_np(Ys))
        assert np.array_equal(Ys[1], eng.sample(0))
    finally:
        eng.close()


def _expected_np(rho):
    L, N, _, K = rho.shape
    p = rho[..., 1:].sum(-1)
    return {"edges": p.sum(axis=(1, 2)), "weight": (rho * np.arange(K)).sum(axis=(1, 2, 3)),
            "mutual": np.einsum("lij,lji->l", p, p), "edges_var": (p * (1.0 - p)).sum(axis=(1, 2))}


def _check_expected(K):
    g = np.random.RandomState(K)
    L, N, M = 2, 70, 6
    X = (g.rand(L, N, N, M) < 0.1).astype(np.uint8)
    st = _random_state(g, L, N, M, K, sparse_p=True)
    eng = _engine_for(X, None, K, True, st)
    try:
        got, again = eng.expected_stats(), eng.expected_stats()
        want = _expected_np(eng.get_state()["rho"])
    finally:
        eng.close()
    terms = {"edges": N * N * K, "weight": N * N * K, "mutual": N * N, "edges_var": N * N}   # terms of each sum
    for k in want:
        assert got[k].shape == (L,) and got[k].dtype == np.float64
        assert np.array_equal(got[k].view(np.uint64), again[k].view(np.uint64)), k
        np.testing.assert_allclose(got[k], want[k], rtol=2 * terms[k] * 2.0 ** -53, atol=0, err_msg=k)


@pytest.mark.parametrize("K", [2, 3])
def test_expected_stats_against_numpy(K, vmr_format):
    _check_expected(K)


def test_expected_stats_against_numpy_k12_general_kernels():
    _check_expected(12)


def test_expected_stats_on_golden_state():
    d = load_case("A_ones_mut")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        got = eng.expected_stats()
        want = _expected_np(eng.get_state()["rho"])
    finally:
        eng.close()
    N = d["X"].shape[1]
    for k in want:
        n = N * N * K if k in ("edges", "weight") else N * N
        np.testing.assert_allclose(got[k], want[k], rtol=2 * n * 2.0 ** -53, atol=0, err_msg=k)


def test_sampling_agrees_with_expectation():
    """S = 2000 samples of the N = 300 case, n_trials = 1: per layer the means of `edges` and `mutual` lie within six standard
    errors of their analytic expectations (pairs are independent under q)."""
    g = np.random.RandomState(33)
    X, st = _medium(g, K=2)
    S = 2000
    eng = _engine_for(X, None, 2, True, st)
    try:
        got = eng.sample_stats(4242, S)
        exp = eng.expected_stats()
        rho = eng.get_state()["rho"]
    finally:
        eng.close()
    p = rho[..., 1:].sum(-1)
    for l in range(p.shape[0]):
        E, V = exp["edges"][l], exp["edges_var"][l]
        assert abs(got["edges"][:, l].mean() - E) <= 6.0 * np.sqrt(V / S)
        pd_ = np.diag(p[l])
        q = p[l] * p[l].T
        Em = q.sum() - (pd_ ** 2).sum() + pd_.sum()
        iu = np.triu_indices(p.shape[1], 1)
        Vm = 4.0 * (q[iu] * (1.0 - q[iu])).sum() + (pd_ * (1.0 - pd_)).sum()
        assert abs(got["mutual"][:, l].mean() - Em) <= 6.0 * np.sqrt(Vm / S)


def test_model_posterior_network_stats():
    from vimure_amd import VimureModel
    from vimure_amd.utils import calculate_overall_reciprocity
    d = load_case("A_ones_mut")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)

    def fit(**kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = VimureModel(mutuality=bool(d["mutuality"]), undirected=und)
            m.fit(d["X"], R=d["R"], K=K, seed=seed, rho_prior=rho_prior, **priors, **fitargs, **kw)
        return m

    m = fit(keep_engine=True)
    Y_true = np.argmax(d["fit_rho_f"], -1)
    S, sd = 6, 123
    res = m.posterior_network_stats(n_samples=S, seed=sd, Y_true=Y_true, degrees=True)
    assert m._rho_f is None                                           # rho has not crossed PCIe
    Ys = [m.sample_inferred_model(N=1, seed=sd + s, device=True)[0] for s in range(S)]
    assert m._rho_f is None
    want = stats_np(Ys, Y_true)
    for k in ("edges", "weight", "mutual", "tp", "deg_out", "deg_in"):
        assert np.array_equal(getattr(res, k), want[k]), k
    for s in range(S):
        for l in range(m.L):
            assert res.reciprocity[s, l] == calculate_overall_reciprocity(Ys[s][l])
    ref_edges = (Y_true > 0).sum(axis=(1, 2))
    assert np.array_equal(res.ref_edges, ref_edges)
    assert np.array_equal(res.f1, 2 * want["tp"] / (want["edges"] + ref_edges[None, :]).astype(float))
    assert res.expected["expected_reciprocity"].shape == (m.L,)
    assert len(res.summary()) == m.L * len(res.statistics())
    dflt = m.posterior_network_stats(n_samples=2)                     # seed None: the fit's
    assert np.array_equal(dflt.edges, stats_np([m.sample_inferred_model(N=1, seed=m.seed + s, device=True)[0] for s in range(2)])["edges"])
    exp_kept = res.expected
    m.close()
    with pytest.raises(ValueError, match="keep_engine=True"):
        m.posterior_network_stats(n_samples=2)
    m2 = fit()
    res2 = m2.posterior_network_stats(n_samples=S, seed=sd, Y_true=Y_true, degrees=True, X=d["X"], R=d["R"])
    for k in ("edges", "weight", "mutual", "tp", "deg_out", "deg_in"):
        assert np.array_equal(getattr(res2, k), getattr(res, k)), k
    assert np.array_equal(res2.reciprocity, res.reciprocity, equal_nan=True)
    for k in exp_kept:
        np.testing.assert_allclose(res2.expected[k], exp_kept[k], rtol=1e-12)
    with pytest.raises(ValueError, match="Y_true"):
        m2.posterior_network_stats(n_samples=2, Y_true=Y_true[:, :-1], X=d["X"], R=d["R"])


def test_errors_on_a_live_handle():
    from vimure_amd import _lib
    from vimure_amd.engine import EngineError
    d = load_case("A_ones_mut")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, None)
    try:
        with pytest.raises(EngineError, match="vmr_set_state"):
            eng.sample_stats(1, 2)
        with pytest.raises(EngineError, match="vmr_set_state"):
            eng.expected_stats()
        counts = np.zeros((2, eng.L, 4), np.uint64)
        assert eng.lib.vmr_sample_stats(eng._h, 1, 2, 1, None, 0, counts.ctypes.data, None, None) == _lib.VMR_ESTATE
        eng.set_state(*_golden_state(d))
        with pytest.raises(ValueError, match="n_samples"):
            eng.sample_stats(1, 0)
        with pytest.raises(ValueError, match="n_trials"):
            eng.sample_stats(1, 2, n_trials=0)
        assert eng.lib.vmr_sample_stats(eng._h, 1, 2, 1, None, 0, None, None, None) == _lib.VMR_EINVAL
        assert b"counts" in eng.lib.vmr_last_error(eng._h)
        assert eng.lib.vmr_expected_stats(eng._h, None) == _lib.VMR_EINVAL
        with pytest.raises(ValueError, match="shape"):
            eng.sample_stats(1, 2, Y_ref=np.zeros((eng.L, eng.N, eng.N + 1), np.uint8))
        assert eng.sample_stats(1, 2)["edges"].shape == (2, eng.L)   # the handle still works
    finally:
        eng.close()
