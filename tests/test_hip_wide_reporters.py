"""GPU: coordinate-list handles with more than 8192 reporters (vmr_create_coo with a run-time key width, the general kernels,
the mask lists of a wide handle and their packed two-reporter rows).  Held to a relabelling of the same data on a narrow handle,
to the coordinate-list oracle (oracle/cavi_coo.c) and to the user's own route: a self-reporter edgelist with N = M = 9000."""
import warnings

import numpy as np
import pytest
from scipy.special import gammaln, psi

from oracle import cavi_coo

pytestmark = pytest.mark.gpu
PRI = (0.1, 0.1, 10.0, 10.0, 0.5, 1.0)


def _steps():
    from vimure_amd import _lib
    return (_lib.STEP_GAMMA, _lib.STEP_PHI, _lib.STEP_RHO, _lib.STEP_NU)


def _mask_rows(g, L, N, M, lens, p_empty=0.2, p_full=0.0):
    """Mask coordinates: per tie empty, all ones, or a partial list of a length drawn from `lens` (random reporters in [0, M),
    repeats dropped), sorted by (l, i, j, m)."""
    kinds = g.rand(L * N * N)
    full = np.nonzero((kinds >= p_empty) & (kinds < p_empty + p_full))[0]
    part = np.nonzero(kinds >= p_empty + p_full)[0]
    n = np.asarray(lens)[g.randint(0, len(lens), len(part))]
    ties = np.concatenate([np.repeat(part, n), np.repeat(full, M)])
    ms = np.concatenate([g.randint(0, M, int(n.sum())), np.tile(np.arange(M), len(full))])
    key = np.unique(ties.astype(np.int64) * M + ms)
    t, m = key // M, key % M
    l, rest = t // (N * N), t % (N * N)
    return l, rest // N, rest % N, m


def _reports(g, L, N, M, R, n_out=200, p_in=0.25, vmax=5):
    """Reports: a share of the mask entries (x in R), a few outside it (the ELBO's eps terms); counts 1..vmax."""
    rl, ri, rj, rm = R
    pick = g.rand(len(rl)) < p_in
    key = [np.ravel_multi_index((rl[pick], ri[pick], rj[pick], rm[pick]), (L, N, N, M))]
    key.append(np.ravel_multi_index((g.randint(0, L, n_out), g.randint(0, N, n_out), g.randint(0, N, n_out), g.randint(0, M, n_out)),
                                    (L, N, N, M)))
    key = np.unique(np.concatenate(key))
    subs = np.unravel_index(key, (L, N, N, M))
    return tuple(np.asarray(s, np.int64) for s in subs), 1 + g.randint(0, vmax, len(key))


def _init(g, L, N, M, K, mut, sumx):
    pr = 1.0 + 0.01 * g.rand(L, N, N, K)
    pr /= pr.sum(-1)[..., None]
    nu = (0.5 + 0.5 * g.rand(), 1.0 + float(sumx)) if mut else (1e-6, 1.0)
    return (0.1 + 0.1 * g.rand(L, M), 0.1 + 0.1 * g.rand(L, M), 10 + 10 * g.rand(L, K), 10 + 10 * g.rand(L, K), nu[0], nu[1], pr)


def _gamma_term(pa, pb, qa, qb):
    return gammaln(qa) - pa * np.log(qb) + (pa - qa) * psi(qa) + qa * (1.0 - pb / qb)


@pytest.mark.parametrize("K", [2, 12])
@pytest.mark.parametrize("mut", [True, False])
def test_relabelled_reporters_give_the_same_fit(K, mut):
    """The same data on M = 300 (narrow: K = 2 runs the specialised kernels) and embedded in M' = 20000 by m -> 61 m + c mod M'
    (wide: the general kernels, keys of 15 reporter bits); reporters outside every row only add their prior's ELBO term."""
    from vimure_amd import CaviEngine
    L, N, M, Mw = 2, 300, 300, 20000
    c0 = (Mw - 1) - 61 * (M - 1)   # (m = M - 1 lands on M' - 1)
    emb = (61 * np.arange(M) + c0) % Mw
    assert emb.max() == Mw - 1 and (emb > 8192).sum() > 100 and len(np.unique(emb)) == M
    g = np.random.RandomState(11 + K + 2 * mut)
    R = _mask_rows(g, L, N, M, lens=[1, 1, 2, 2, 2, 3, 5, 17, 64])
    sx, vx = _reports(g, L, N, M, R)
    init = _init(g, L, N, M, K, mut, vx.sum())
    gs_w, gr_w = 0.1 + 0.1 * g.rand(L, Mw), 0.1 + 0.1 * g.rand(L, Mw)
    gs_w[:, emb], gr_w[:, emb] = init[0], init[1]
    init_w = (gs_w, gr_w) + init[2:]
    wide = lambda s: (s[0], s[1], s[2], emb[s[3]])
    en = CaviEngine.from_coo(sx, vx, (L, N, N, M), R=R, K=K, mutuality=mut)
    ew = CaviEngine.from_coo(wide(sx), vx, (L, N, N, Mw), R=wide(R), K=K, mutuality=mut)
    assert ew.data_format() == ("sparse", len(vx)) and ew.mask_format() == en.mask_format() == ("lists", len(R[0]))
    unused = np.setdiff1d(np.arange(Mw), emb)
    for e, ini in ((en, init), (ew, init_w)):
        e.set_priors(*PRI)
        e.set_state(*ini)
    for _ in range(3):
        for s in _steps():
            en.sub_step(s)
            ew.sub_step(s)
        a, b = en.get_state(), ew.get_state()
        np.testing.assert_allclose(b["rho"], a["rho"], rtol=1e-9, atol=1e-13)
        for k in ("phi_shp", "phi_rte"):
            np.testing.assert_allclose(b[k], a[k], rtol=1e-9)
        for k in ("nu_shp", "nu_rte"):
            assert abs(b[k] - a[k]) <= 1e-9 * abs(a[k])
        for k in ("gamma_shp", "gamma_rte"):
            np.testing.assert_allclose(b[k][:, emb], a[k], rtol=1e-9)
        extra = float(_gamma_term(PRI[0], PRI[1], b["gamma_shp"][:, unused], b["gamma_rte"][:, unused]).sum())
        e_n, e_w = en.elbo(), ew.elbo() - extra
        assert abs(e_w - e_n) <= 1e-9 * abs(e_n), (e_w, e_n)
    en.close()
    ew.close()


def _oracle_run(sx, vx, R, shape, K, mut, init, sweeps, check_each=True):
    """Sub-steps of a from_coo handle against CooRef (the tolerances of test_hip_coo.py); the engine is returned open."""
    from vimure_amd import CaviEngine
    eng = CaviEngine.from_coo(sx, vx, shape, R=R, K=K, mutuality=mut)
    c = cavi_coo.CooRef((sx, vx), R, shape, K, mut, PRI, *init)
    eng.set_priors(*PRI)
    eng.set_state(*init)
    ref_steps = (c.update_gamma, c.update_phi, c.update_rho, c.update_nu)
    for it in range(sweeps):
        for s, f in zip(_steps(), ref_steps):
            eng.sub_step(s)
            f()
        if check_each or it == sweeps - 1:
            st = eng.get_state()
            np.testing.assert_allclose(st["gamma_shp"], c.gamma_shp, rtol=1e-9)
            np.testing.assert_allclose(st["gamma_rte"], c.gamma_rte, rtol=1e-9)
            np.testing.assert_allclose(st["phi_shp"], c.phi_shp, rtol=1e-9)
            np.testing.assert_allclose(st["phi_rte"], c.phi_rte, rtol=1e-9)
            np.testing.assert_allclose(st["rho"], c.rho, rtol=1e-9, atol=1e-13)
            assert abs(st["nu_shp"] - c.nu_shp) <= 1e-9 * abs(c.nu_shp)
            ref = c.elbo()
            assert abs(eng.elbo() - ref) <= 1e-9 * max(1.0, abs(ref)), (eng.elbo(), ref)
    return eng


@pytest.mark.parametrize("rows", ["two", "long"])
@pytest.mark.parametrize("K", [2, 12])
@pytest.mark.parametrize("mut", [True, False])
def test_wide_handle_matches_the_coordinate_oracle(rows, K, mut):
    """M = 12000: all-ones rows, empty rows and partial ones -- lists of one or two reporters only (the packed two-reporter
    rows of the general pass) or also longer ones (the list walk)."""
    L, N, M = 1, 300, 12000
    g = np.random.RandomState(23 + K + 2 * mut + (rows == "long"))
    lens = [1, 2] if rows == "two" else [1, 2, 3, 9, 40, 64]
    R = _mask_rows(g, L, N, M, lens=lens, p_empty=0.15, p_full=0.002)
    sx, vx = _reports(g, L, N, M, R, p_in=0.02 if rows == "long" else 0.2)
    init = _init(g, L, N, M, K, mut, vx.sum())
    eng = _oracle_run(sx, vx, R, (L, N, N, M), K, mut, init, sweeps=3)
    assert eng.mask_format()[0] == "lists" and eng.sweep_shape()[1] == 0   # (the general kernels: no LDS levels)
    eng.close()


@pytest.mark.parametrize("M,K", [(8192, 12), (8193, 2), (65535, 2)])
def test_reporter_width_boundaries(M, K):
    """13-bit keys and packed entries up to M = 8192 (K = 12 there: the K <= 8 kernels keep 8192 reporters' tables in LDS and
    refuse them with mutuality on, as before), 14 bits at 8193, 16 at 65535."""
    L, N = 1, 40
    g = np.random.RandomState(M % 97)
    R = _mask_rows(g, L, N, M, lens=[1, 2, 3], p_empty=0.1)
    # the highest reporter is listed and reports
    R = tuple(np.concatenate([a, [v]]) for a, v in zip(R, (0, 5, 7, M - 1)))
    key = np.unique(np.ravel_multi_index(R, (L, N, N, M)))
    R = tuple(np.asarray(s, np.int64) for s in np.unravel_index(key, (L, N, N, M)))
    sx, vx = _reports(g, L, N, M, R, p_in=0.3)
    if not np.any((sx[1] == 5) & (sx[2] == 7) & (sx[3] == M - 1)):
        key = np.unique(np.concatenate([np.ravel_multi_index(sx, (L, N, N, M)), [np.ravel_multi_index((0, 5, 7, M - 1), (L, N, N, M))]]))
        sx = tuple(np.asarray(s, np.int64) for s in np.unravel_index(key, (L, N, N, M)))
        vx = 1 + g.randint(0, 5, len(key))
    init = _init(g, L, N, M, K, True, vx.sum())
    eng = _oracle_run(sx, vx, R, (L, N, N, M), K, True, init, sweeps=1)
    eng.close()


def test_m_beyond_65535_is_refused_before_any_kernel():
    from vimure_amd import CaviEngine
    from vimure_amd.engine import EngineError
    one = tuple(np.zeros(1, np.int64) for _ in range(3))
    with pytest.raises((ValueError, EngineError), match="65535"):
        CaviEngine.from_coo(one + (np.full(1, 65535),), np.ones(1, np.int64), (1, 2, 2, 65536), K=2)


def _survey_df(N=9000, extra=500, seed=5):
    """A self-reporter edgelist: pairs (2r, 2r + 1) reported by one of them, then `extra` edges reported by their ego."""
    import pandas as pd
    g = np.random.RandomState(seed)
    r = np.arange(N // 2)
    ego, alter = 2 * r, 2 * r + 1
    rep = np.where(r % 2 == 0, ego, alter)
    e2 = 2 * np.arange(extra) + 1
    a2 = (e2 + 2 + 2 * g.randint(0, N // 2 - 2, extra)) % N
    ego, alter, rep = np.concatenate([ego, e2]), np.concatenate([alter, a2]), np.concatenate([rep, e2])
    return pd.DataFrame({"reporter": [f"n{v}" for v in rep], "ego": [f"n{v}" for v in ego], "alter": [f"n{v}" for v in alter],
                         "weight": 1, "layer": "L0"})


def test_survey_with_9000_reporters_fits(monkeypatch):
    """The user's case: VimureModel().fit(DataFrame) of a 9000-node self-reporter survey, with no dense tensor anywhere; then the
    same containers through from_coo against the coordinate oracle."""
    import vimure_amd.model as vmm
    import vimure_amd.tensor as vt
    from vimure_amd import VimureModel
    from vimure_amd._io import read_from_edgelist

    def boom(*a, **k):
        raise AssertionError("dense conversion called for a 9000-reporter survey")
    monkeypatch.setattr(vmm, "to_dense_u8", boom)
    monkeypatch.setattr(vt, "to_dense_u8", boom)
    df = _survey_df()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VimureModel().fit(df, K=2, seed=1, num_realisations=1, max_iter=11, keep_engine=True)
        net = read_from_edgelist(df, K=2)
    assert (m.L, m.N, m.M, m.K) == (1, 9000, 9000, 2)
    assert m._engine.data_format() == ("sparse", len(net.X.vals))
    assert len(m.trace) > 0 and np.all(np.isfinite(m.trace["elbo"].values)) and np.isfinite(m.maxL)
    assert m.get_inferred_model().shape == (1, 9000, 9000)
    m.close()
    del m
    X, R = net.X, net.R
    L, N, M, K = 1, 9000, 9000, 2
    g = np.random.RandomState(3)
    init = _init(g, L, N, M, K, True, np.asarray(X.vals).sum())
    eng = _oracle_run(X.subs, np.asarray(X.vals, np.int64), R.subs, (L, N, N, M), K, True, init, sweeps=2, check_each=False)
    assert eng.mask_format() == ("lists", len(R.vals))
    eng.close()
