"""GPU: VMR_DETERMINISTIC=1 on handles that run the general kernels (sweep_gen.hip): K > 8 (the reference's default K = max(X) + 1),
counts beyond a packed entry (two-word entries) and coordinate lists of more than 8192 reporters.  Two runs of the same fit leave
bit-identical states and ELBOs; they agree with the default mode, the NumPy oracle, the coordinate-list oracle and the reference's
golden values.  (tests/test_hip_deterministic.py holds the same checks for the specialised K <= 8 kernels.)"""
import os
import warnings

import numpy as np
import pytest

from oracle import cavi_coo

pytestmark = pytest.mark.gpu
PRI = (0.1, 0.1, 10.0, 10.0, 0.5, 1.0)
STATE = ("gamma_shp", "gamma_rte", "phi_shp", "phi_rte", "nu_shp", "nu_rte", "rho")


def _switch(monkeypatch, det):
    if det:
        monkeypatch.setenv("VMR_DETERMINISTIC", "1")
    else:
        monkeypatch.delenv("VMR_DETERMINISTIC", raising=False)


def _fit(make, sweeps, monkeypatch, det):
    """One ELBO sweep, then `sweeps` more through fit_loop (ELBO every sweep) on the handle `make()` returns; its ELBOs and state."""
    _switch(monkeypatch, det)
    eng = make()
    elbos = [eng.step(1, want_elbo=True)]
    rows, elbo, its, conv = eng.fit_loop(sweeps, 1e-12, 100)
    elbos += [r[1] for r in rows] + [elbo]
    out = eng.get_state(rho=True)
    eng.close()
    return elbos, out


def _golden(case):
    from oracle import vimure_oracle as vo
    from tests.golden_util import case_config, load_case
    from vimure_amd import CaviEngine
    d = load_case(case)
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    L, N, _, M = d["X"].shape
    pr = vo.make_priors(L, M, K, **priors)
    pb = vo.Problem(d["X"], d["R"], K, mut, pr, undirected=und)
    st = vo.init_state(pb, np.random.RandomState(seed), rho_prior=rho_prior)

    def make():   # (as test_hip_deterministic.py::_run)
        eng = CaviEngine(d["X"], d["R"], K=K, mutuality=mut)
        eng.set_priors(pr.alpha_theta, pr.beta_theta, pr.alpha_lambda, pr.beta_lambda, pr.alpha_eta, pr.beta_eta)
        eng.set_state(st.gamma_shp, st.gamma_rte, st.phi_shp, st.phi_rte, st.nu_shp, st.nu_rte, st.pr_rho)
        return eng
    return make, d, pb, st, mut


def _coo_maker(subs, vals, shape, R, K, mut, init, priors=PRI):
    from vimure_amd import CaviEngine

    def make():
        eng = CaviEngine.from_coo(subs, vals, shape, R=R, K=K, mutuality=mut)
        eng.set_priors(*priors)
        eng.set_state(*init)
        return eng
    return make


def _counts_12000():
    """N_counts_12000 (counts to 16990: two-word entries).  The reference's raw exponentials overflow on these counts (its fit
    ends in "ELBO is NaN", test_hip_general.py::test_reference_nans_on_huge_counts_and_so_do_we); priors of 10^7 - 10^9 pseudo-counts
    hold E log theta + E log lambda near -0.02, where a fit of 30 sweeps stays finite (checked against oracle/cavi_coo)."""
    from tests.golden_util import GOLDEN
    d = np.load(os.path.join(GOLDEN, "N_counts_12000.npz"))
    shape = tuple(int(s) for s in d["X_shape"])
    L, N, _, M = shape
    K = int(d["K"])
    subs = tuple(np.asarray(s, np.int64) for s in d["X_subs"])
    vals = np.asarray(d["X_vals"], np.int64)
    R = tuple(np.asarray(s, np.int64) for s in d["R_subs"])
    g = np.random.RandomState(6)
    pr = g.rand(L, N, N, K) + 0.05
    pr /= pr.sum(-1, keepdims=True)
    assert K == 2 and vals.max() > 2047
    init = (np.full((L, M), 4e9), np.full((L, M), 4.002e9), np.full((L, K), 5e7), np.array([[5.1e7, 5.2e7]]), 0.7, 1.0 + float(vals.sum()), pr)
    return _coo_maker(subs, vals, shape, R, K, True, init, priors=(4e9, 4.002e9, 5e7, 5.1e7, 0.5, 1.0))


def _synthetic_k100():
    """K = 100: two categories per lane (NCH = 2 in k_sweep_gen); bit-packed partial mask rows."""
    L, N, M, K = 1, 12, 70, 100
    g = np.random.RandomState(100)
    X = ((g.rand(L, N, N, M) < 0.05) * g.randint(1, 5, size=(L, N, N, M))).astype(np.int64)
    R = (g.rand(L, N, N, M) < 0.9).astype(np.uint8)
    R[:, :2] = 1
    R[:, 2] = 0
    pr = g.rand(L, N, N, K) + 0.05
    pr /= pr.sum(-1, keepdims=True)
    init = (0.5 + g.rand(L, M), 0.5 + g.rand(L, M), 1 + g.rand(L, K), 1 + g.rand(L, K), 0.7, 1.0 + float(X.sum()), pr)
    sx = np.nonzero(X)
    return _coo_maker(sx, X[sx], X.shape, np.nonzero(R), K, True, init)


def _assert_bit_equal(a, b):
    (e1, s1), (e2, s2) = a, b
    assert np.all(np.isfinite(e1)) and e1 == e2
    for k in STATE:
        assert np.array_equal(np.asarray(s1[k]), np.asarray(s2[k])), k


@pytest.mark.parametrize("case", ["L_default_K12", "M_K16_nomut", "N_counts_12000", "K100"])
def test_two_deterministic_runs_are_bit_equal(case, monkeypatch):
    if case == "N_counts_12000":
        make = _counts_12000()
    elif case == "K100":
        make = _synthetic_k100()
    else:
        make = _golden(case)[0]
    probe = make()
    assert probe.sweep_shape()[1] == 0   # (the general kernels: no LDS levels)
    probe.close()
    r1 = _fit(make, 30, monkeypatch, True)
    r2 = _fit(make, 30, monkeypatch, True)
    _assert_bit_equal(r1, r2)
    e0, s0 = _fit(make, 30, monkeypatch, False)
    np.testing.assert_allclose(r1[0], e0, rtol=1e-9)
    for k in STATE:
        if k != "nu_rte":
            np.testing.assert_allclose(np.asarray(r1[1][k]), np.asarray(s0[k]), rtol=1e-8, atol=1e-11, err_msg=k)


@pytest.mark.parametrize("case", ["L_default_K12", "M_K16_nomut"])
def test_deterministic_mode_against_the_oracle_and_the_reference(case, monkeypatch):
    """Every iteration stored in the golden case: the NumPy oracle's sweep from the same state and the reference's own sub-step
    values, to the tolerances of test_hip_deterministic.py."""
    from oracle import vimure_oracle as vo
    make, d, pb, st, mut = _golden(case)
    _switch(monkeypatch, True)
    eng = make()
    for it in range(1, len(d["step_elbo"]) + 1):
        e = eng.step(1, want_elbo=True)
        vo.cavi_step(pb, st)
        eo, er = vo.elbo(pb, st), float(d["step_elbo"][it - 1])
        assert abs(e - eo) <= 1e-9 * max(1.0, abs(eo)) and abs(e - er) <= 1e-9 * max(1.0, abs(er)), (it, e, eo, er)
        g = eng.get_state()
        if f"it{it}_rho" in d:
            np.testing.assert_allclose(g["rho"], d[f"it{it}_rho"], rtol=1e-8, atol=1e-12)
            np.testing.assert_allclose(g["gamma_shp"], d[f"it{it}_gamma_shp"], rtol=1e-9)
            np.testing.assert_allclose(g["phi_rte"], d[f"it{it}_phi_rte"], rtol=1e-9)
            if mut:
                np.testing.assert_allclose(g["nu_shp"], d[f"it{it}_nu_shp"], rtol=1e-9)
    eng.close()


def _big_network():
    """L = 2, N = 600, M = 300, K = 12, counts 1..11, mutuality on: hundreds of workgroups, and rows of H both in LDS (mirror
    counts y < YL, here 4) and only in global memory (y >= 4).  Mask: empty rows, all-ones rows and short partial lists."""
    L, N, M, K = 2, 600, 300, 12
    g = np.random.RandomState(12)
    T = L * N * N
    kinds = g.rand(T)
    full = np.nonzero((kinds >= 0.3) & (kinds < 0.31))[0]
    part = np.nonzero(kinds >= 0.31)[0]
    n = g.randint(1, 4, len(part))
    ties = np.concatenate([np.repeat(part, n), np.repeat(full, M)])
    ms = np.concatenate([g.randint(0, M, int(n.sum())), np.tile(np.arange(M), len(full))])
    rkey = np.unique(ties.astype(np.int64) * M + ms)
    pick = rkey[g.rand(len(rkey)) < 0.15]
    out = g.randint(0, T * M, 2000).astype(np.int64)   # (a few reports outside the mask: the ELBO's eps terms)
    xkey = np.unique(np.concatenate([pick, out]))
    shape = (L, N, N, M)
    R = tuple(np.asarray(s, np.int64) for s in np.unravel_index(rkey, shape))
    subs = tuple(np.asarray(s, np.int64) for s in np.unravel_index(xkey, shape))
    vals = 1 + g.randint(0, 11, len(xkey))
    pr = g.rand(L, N, N, K) + 0.05
    pr /= pr.sum(-1, keepdims=True)
    init = (0.5 + g.rand(L, M), 0.5 + g.rand(L, M), 1 + g.rand(L, K), 1 + g.rand(L, K), 0.7, 1.0 + float(vals.sum()), pr)
    return _coo_maker(subs, vals, shape, R, K, True, init)


@pytest.mark.parametrize("hsum", ["auto", "1"])
def test_network_with_many_workgroups_is_bit_equal(hsum, monkeypatch):
    """The sums that cross workgroups and waves.  auto: H's 43 200 cells per layer are summed by several workgroups (k_gen_hsum,
    nb > 1); 1: by the finalize kernel alone (VMR_GEN_HSUM=1, its sums in LDS)."""
    if hsum == "auto":
        monkeypatch.delenv("VMR_GEN_HSUM", raising=False)
    else:
        monkeypatch.setenv("VMR_GEN_HSUM", hsum)
    make = _big_network()
    outs = []
    for _ in range(2):
        _switch(monkeypatch, True)
        eng = make()
        assert eng.sweep_shape()[1] == 0
        e = [eng.step(1, want_elbo=True) for _ in range(3)] + [eng.step(5, want_elbo=True)]
        outs.append((e, eng.get_state(rho=True)))
        eng.close()
    _assert_bit_equal(outs[0], outs[1])


def _survey_df(N=9000, extra=500, seed=5, weights=False):
    """A self-reporter edgelist: pairs (2r, 2r + 1) reported by one of them, then `extra` edges reported by their ego
    (as test_hip_wide_reporters.py); weights: counts 1..10 instead of ones."""
    import pandas as pd
    g = np.random.RandomState(seed)
    r = np.arange(N // 2)
    ego, alter = 2 * r, 2 * r + 1
    rep = np.where(r % 2 == 0, ego, alter)
    e2 = 2 * np.arange(extra) + 1
    a2 = (e2 + 2 + 2 * g.randint(0, N // 2 - 2, extra)) % N
    ego, alter, rep = np.concatenate([ego, e2]), np.concatenate([alter, a2]), np.concatenate([rep, e2])
    w = 1 + g.randint(0, 10, len(ego)) if weights else 1
    return pd.DataFrame({"reporter": [f"n{v}" for v in rep], "ego": [f"n{v}" for v in ego], "alter": [f"n{v}" for v in alter],
                         "weight": w, "layer": "L0"})


def test_wide_survey_is_bit_equal_and_matches_the_coordinate_oracle(monkeypatch):
    """N = M = 9000 through vmr_create_coo (M > 8192: the general kernels only): two runs bit-equal, and whole sweeps against
    oracle/cavi_coo to the tolerances of test_hip_wide_reporters.py."""
    from vimure_amd._io import read_from_edgelist
    net = read_from_edgelist(_survey_df(), K=2)
    X, R = net.X, net.R
    L, N, M, K = 1, 9000, 9000, 2
    vals = np.asarray(X.vals, np.int64)
    g = np.random.RandomState(3)
    pr = 1.0 + 0.01 * g.rand(L, N, N, K)
    pr /= pr.sum(-1)[..., None]
    init = (0.1 + 0.1 * g.rand(L, M), 0.1 + 0.1 * g.rand(L, M), 10 + 10 * g.rand(L, K), 10 + 10 * g.rand(L, K),
            0.5 + 0.5 * g.rand(), 1.0 + float(vals.sum()), pr)
    make = _coo_maker(X.subs, vals, (L, N, N, M), R.subs, K, True, init)
    outs = []
    for _ in range(2):
        _switch(monkeypatch, True)
        eng = make()
        assert eng.mask_format() == ("lists", len(R.vals)) and eng.sweep_shape()[1] == 0
        e = [eng.step(1, want_elbo=True) for _ in range(2)]
        outs.append((e, eng.get_state(rho=True)))
        eng.close()
    _assert_bit_equal(outs[0], outs[1])
    c = cavi_coo.CooRef((X.subs, vals), R.subs, (L, N, N, M), K, True, PRI, *init)
    for it in range(2):
        c.cavi_step()
        ref = c.elbo()
        assert abs(outs[0][0][it] - ref) <= 1e-9 * max(1.0, abs(ref)), (it, outs[0][0][it], ref)
    st = outs[0][1]
    for k in ("gamma_shp", "gamma_rte", "phi_shp", "phi_rte"):
        np.testing.assert_allclose(st[k], getattr(c, k), rtol=1e-9, err_msg=k)
    np.testing.assert_allclose(st["rho"], c.rho, rtol=1e-9, atol=1e-13)
    assert abs(st["nu_shp"] - c.nu_shp) <= 1e-9 * abs(c.nu_shp)


def test_user_fit_with_default_k_is_reproducible(monkeypatch):
    """The user's route for a count edgelist: read_from_edgelist(df, is_weighted=True), then VimureModel().fit(X, R=R, seed=...)
    without K: K = max(X) + 1 = 11 > 8, the general kernels.  (fit(DataFrame) reads an edgelist as binary, hence K = 2 there.)"""
    from vimure_amd import VimureModel
    from vimure_amd._io import read_from_edgelist
    df = _survey_df(N=120, extra=300, seed=9, weights=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = read_from_edgelist(df, is_weighted=True)
    runs = []
    for _ in range(2):
        _switch(monkeypatch, True)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            m = VimureModel().fit(net.X, R=net.R, seed=4, num_realisations=1, max_iter=60)
        assert any("Defaulting to" in str(x.message) for x in w) and m.K == 11
        runs.append((np.asarray(m.rho_f).copy(), m.trace["elbo"].values.copy(), m.trace["iter"].tolist()))
        m.close()
    (r1, e1, i1), (r2, e2, i2) = runs
    assert np.all(np.isfinite(e1)) and np.array_equal(e1, e2)
    assert i1 == i2
    assert np.array_equal(r1, r2)
