"""GPU: the K = 2 update passes through the difference of the log prior (SlArgs::lpd).  The passes without ELBO read
lp_1 - lp_0 (8 bytes per tie) instead of the log prior; VMR_NO_LPD=1 makes them read the log prior and form the difference in
registers, as the ELBO passes always do.  Both take the same decisions on the same numbers, so the two runs are bit-identical --
also where the bounds test fails and a wave takes the literal code (large counts below).  Parity with the reference on these
handles is the golden fit tests' (tests/test_hip_fit.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE = ("gamma_shp", "gamma_rte", "phi_shp", "phi_rte", "nu_shp", "nu_rte", "rho")


def _run(case, monkeypatch, no_lpd, scale=1, lazy=False, sweeps=15):
    """A fit of a golden case's network on the sorted report lists, deterministic mode (sums across workgroups in a fixed order:
    runs comparable bit for bit)."""
    from oracle import vimure_oracle as vo
    from tests.golden_util import case_config, load_case
    from vimure_amd import CaviEngine
    monkeypatch.setenv("VMR_FORMAT", "sparse")
    monkeypatch.setenv("VMR_DETERMINISTIC", "1")
    for name, on in (("VMR_NO_LPD", no_lpd), ("VMR_DEBUG_LAZY_RHO", lazy)):
        if on:
            monkeypatch.setenv(name, "1")
        else:
            monkeypatch.delenv(name, raising=False)
    d = load_case(case)
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    assert K == 2
    X = d["X"]
    if scale != 1:   # counts far beyond what |a_k| < 700 allows: the bounds test fails, waves take the literal code
        X = np.minimum(X.astype(np.int64) * scale, 255).astype(X.dtype)
    L, N, _, M = X.shape
    pr = vo.make_priors(L, M, K, **priors)
    pb = vo.Problem(X, d["R"], K, mut, pr, undirected=und)
    st = vo.init_state(pb, np.random.RandomState(seed), rho_prior=rho_prior)
    eng = CaviEngine(X, d["R"], K=K, mutuality=mut)
    assert eng.data_format()[0] == "sparse"
    eng.set_priors(pr.alpha_theta, pr.beta_theta, pr.alpha_lambda, pr.beta_lambda, pr.alpha_eta, pr.beta_eta)
    eng.set_state(st.gamma_shp, st.gamma_rte, st.phi_shp, st.phi_rte, st.nu_shp, st.nu_rte, st.pr_rho)
    elbos = [eng.step(1, want_elbo=True), eng.step(4, want_elbo=False)]
    rows, elbo, its, conv = eng.fit_loop(sweeps, 1e-12, 100)
    elbos += [r[1] for r in rows] + [elbo]
    out = eng.get_state(rho=True)
    eng.close()
    return elbos, out


def _same(a, b):
    ea, sa = a
    eb, sb = b
    assert ea == eb
    for k in STATE:
        assert np.array_equal(np.asarray(sa[k]), np.asarray(sb[k])), k


def _have(case):
    import os
    from tests.golden_util import GOLDEN
    return os.path.exists(os.path.join(GOLDEN, case + ".npz"))


@pytest.mark.parametrize("case", ["A_ones_mut", "C_ones_nomut", "D_self_mask"])
@pytest.mark.parametrize("scale", [1, 10])
def test_lpd_matches_log_prior_bit_for_bit(case, scale, monkeypatch):
    if not _have(case):
        pytest.skip("no such golden case")
    a = _run(case, monkeypatch, False, scale)
    b = _run(case, monkeypatch, True, scale)
    _same(a, b)
    assert all(np.isfinite(e) for e in a[0][:1] + a[0][2:])


@pytest.mark.parametrize("scale", [1, 10])
def test_lazy_rho_stays_bit_identical(scale, monkeypatch):
    """VMR_DEBUG_LAZY_RHO=1: no plain sweep writes rho; ensure_rho's re-run (the stale nu, the stored difference) replays it exactly."""
    _same(_run("A_ones_mut", monkeypatch, False, scale), _run("A_ones_mut", monkeypatch, False, scale, lazy=True))


def test_deterministic_lpd_is_bit_reproducible(monkeypatch):
    _same(_run("D_self_mask", monkeypatch, False, 10), _run("D_self_mask", monkeypatch, False, 10))


def test_config3_shaped_lpd_matches_log_prior(monkeypatch):
    """A network of hundreds of workgroups (L = 2, N = 600, M = 60, K = 2, mutuality on), its steps without reports included."""
    import torch
    from bench import draw_state
    from vimure_amd import CaviEngine
    from vimure_amd.synthetic import standard_sbm
    net = standard_sbm(N=600, M=60, L=2, K=2, avg_degree=6.0, eta=0.5, seed=3, device="cuda:0")
    outs = []
    for no_lpd in (False, True):
        if no_lpd:
            monkeypatch.setenv("VMR_NO_LPD", "1")
        else:
            monkeypatch.delenv("VMR_NO_LPD", raising=False)
        monkeypatch.setenv("VMR_DETERMINISTIC", "1")   # (the sums across workgroups in a fixed order: the two runs comparable bit for bit)
        eng = CaviEngine(net.X, None, K=2, mutuality=True, device=0)
        sum_x, cov = eng.data_stats()
        host, pr = draw_state(dict(L=2, N=600, M=60, K=2, mutuality=True), 5, sum_x, cov)
        eng.set_priors(0.1, 0.1, 10.0, 10.0, 0.5, 1.0)
        eng.set_state(host.gamma_shp, host.gamma_rte, host.phi_shp, host.phi_rte, host.nu_shp, host.nu_rte, pr)
        e = [eng.step(1, want_elbo=True), eng.step(9, want_elbo=True)]
        outs.append((e, eng.get_state(rho=True)))
        eng.close()
    _same(outs[0], outs[1])
    del net
    torch.cuda.empty_cache()
