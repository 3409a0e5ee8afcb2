"""GPU: the initial rho prior drawn on the device (vmr_draw_pr_rho, `fit(init_on_device=True)`).  Every comparison is bit for bit
(np.array_equal): against the reference's own initial priors (tests/golden), the host draw of vimure_amd/csrc/host_init.c, the
NumPy statements of `_set_rho_prior` for K >= 8 and undirected networks, and whole fits under VMR_DETERMINISTIC=1."""
import warnings

import numpy as np
import pytest

from tests.golden_util import case_config, load_case
from vimure_amd import _hostlib, _lib

pytestmark = pytest.mark.gpu

# every golden case with a reference initial prior and no informative rho_prior (F_rho_prior keeps the host draw)
CASES = ["A_ones_mut", "B_random_mask_K3", "C_ones_nomut", "D_self_mask", "E_undirected", "G_config1_sbm", "H_ref_f1_over",
         "H_ref_f1_under", "I_karnataka_vil1_money", "L_default_K12", "M_K16_nomut", "O_wide_rows"]
SMALL = ("gamma_shp_f", "gamma_rte_f", "phi_shp_f", "phi_rte_f", "nu_shp_f", "nu_rte_f")


def _engine(kind, X, R, K, mut):
    from vimure_amd import CaviEngine
    if kind == "dense":
        return CaviEngine(X, R, K=K, mutuality=mut)
    sx = np.nonzero(X)
    return CaviEngine.from_coo(sx, X[sx], X.shape, R=None if R is None else np.nonzero(R), K=K, mutuality=mut)


def _coo_engine(L, N, K, cover, seed=0, M=2):
    """A coordinate-list handle of shape (L, N, N, M) whose coverage is a random `cover` share of the ties."""
    from vimure_amd import CaviEngine
    g = np.random.RandomState(seed)
    ties = L * N * N
    t = np.sort(g.choice(ties, int(cover * ties), replace=False)) if cover < 1 else np.arange(ties)
    l, r = np.divmod(t, N * N)
    i, j = np.divmod(r, N)
    m = g.randint(0, M, len(t))
    return CaviEngine.from_coo((l, i, j, m), 1 + g.randint(0, K - 1, len(t)), (L, N, N, M), K=K, mutuality=True)


def _numpy_prior(prng, L, N, K, bias0, cov, undirected):
    """The statements of `_set_rho_prior` without an informative prior (VimureModel._draw_pr_rho's NumPy branch)."""
    pr = 1.0 + 0.01 * prng.rand(L, N, N, K)
    pr[..., 0] += bias0
    if undirected:
        pr = (pr + pr.transpose(0, 2, 1, 3)) / 2.0
    pr /= pr.sum(axis=-1)[..., None]
    onehot = np.zeros(K)
    onehot[0] = 1.0
    pr[cov == 0] = onehot
    return pr


def _start(kind, seed):
    g = np.random.RandomState(seed)
    if kind == "odd":
        g.randint(1, 500)
    elif kind == "mid":
        g.random_sample(201)
    return g


def _twin(g):
    h = np.random.RandomState()
    h.set_state(g.get_state())
    return h


def _same_state(a, b):
    sa, sb = a.get_state(), b.get_state()
    return sa[2] == sb[2] and np.array_equal(sa[1], sb[1])


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("kind", ["dense", "coo"])
def test_matches_the_reference_initial_prior(name, kind):
    import torch
    d = load_case(name)
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    assert rho_prior is None
    L, N = d["X"].shape[:2]
    eng = _engine(kind, d["X"], d["R"], K, mut)
    try:
        for nblk in (1, 7, None, L * N * N):
            blocks = _hostlib.mt_block_states(np.random.RandomState(seed), L, N, K, nblk)
            host = np.full((L, N, N, K), np.nan)
            eng.draw_pr_rho(blocks, 0.0, und, out=host)
            assert np.array_equal(host, d["init_pr_rho"]), (name, kind, nblk)
        dev = torch.empty((L, N, N, K), dtype=torch.float64, device="cuda")
        eng.draw_pr_rho(_hostlib.mt_block_states(np.random.RandomState(seed), L, N, K), 0.0, und, out=dev)
        assert np.array_equal(dev.cpu().numpy(), d["init_pr_rho"])
    finally:
        eng.close()


@pytest.mark.parametrize("start", ["fresh", "odd", "mid"])
def test_matches_the_host_draw_at_config3_size(start):
    """BASELINE config 3's shape (L = 4, N = 2000, K = 2; 32 M doubles) against the threaded C draw, a quarter of the ties covered."""
    L, N, K = 4, 2000, 2
    eng = _coo_engine(L, N, K, 0.25, seed=1)
    try:
        _, cov = eng.data_stats()
        assert 0.2 < cov.mean() < 0.3
        a = _start(start, 5)
        b = _twin(a)
        got = np.empty((L, N, N, K))
        eng.draw_pr_rho(_hostlib.mt_block_states(a, L, N, K), 0.0, False, out=got)
        ref = _hostlib.draw_pr_rho(b, (L, N, N, K), 0.0, cov)
        assert np.array_equal(got, ref)
        assert _same_state(a, b)
    finally:
        eng.close()


@pytest.mark.parametrize("L,N,K,undirected,bias0,start,cover,nblk", [
    (1, 600, 12, False, 0.0, "fresh", 0.6, None),   # the reference's default K on count data: 8-accumulator sums
    (1, 600, 12, False, 0.4, "odd", 0.6, 333),
    (2, 20, 129, False, 0.0, "mid", 0.7, 5),        # one split of the pairwise sum
    (2, 20, 256, False, 0.3, "odd", 0.7, None),     # K = 256: two levels of splits on the right half of n = 255 .. 256
    (1, 9, 255, False, 0.0, "fresh", 1.0, 81),      # 255: the right half (135) splits again
    (1, 300, 9, True, 0.0, "fresh", 0.5, None),     # undirected: symmetrised, then normalised; each tie's own coverage
    (2, 40, 9, True, 0.2, "mid", 0.5, 17),
    (1, 50, 3, True, 0.0, "odd", 0.5, 2500),        # undirected, one tie per block
])
def test_matches_the_numpy_statements(L, N, K, undirected, bias0, start, cover, nblk):
    eng = _coo_engine(L, N, K, cover, seed=K)
    try:
        _, cov = eng.data_stats()
        assert cover == 1.0 or 0 < cov.mean() < 1
        if undirected:
            assert (cov != cov.transpose(0, 2, 1)).any()   # (each direction's own one-hot)
        a = _start(start, 13)
        b = _twin(a)
        got = np.empty((L, N, N, K))
        eng.draw_pr_rho(_hostlib.mt_block_states(a, L, N, K, nblk), bias0, undirected, out=got)
        ref = _numpy_prior(b, L, N, K, bias0, cov, undirected)
        assert np.array_equal(got, ref)
        assert _same_state(a, b)
    finally:
        eng.close()


def _survey(N, extra, seed, weights):
    """A self-reporter edgelist: pairs (2r, 2r + 1) reported by one of them, then `extra` edges reported by their ego; weights:
    counts 1..weights (K = weights + 1 by the reference's default) or ones."""
    import pandas as pd
    from vimure_amd._io import read_from_edgelist
    g = np.random.RandomState(seed)
    r = np.arange(N // 2)
    ego, alter = 2 * r, 2 * r + 1
    rep = np.where(r % 2 == 0, ego, alter)
    e2 = 2 * np.arange(extra) + 1
    a2 = (e2 + 2 + 2 * g.randint(0, N // 2 - 2, extra)) % N
    ego, alter, rep = np.concatenate([ego, e2]), np.concatenate([alter, a2]), np.concatenate([rep, e2])
    w = 1 + g.randint(0, weights, len(ego)) if weights else 1
    if weights:
        w[0] = weights
    df = pd.DataFrame({"reporter": [f"n{v}" for v in rep], "ego": [f"n{v}" for v in ego], "alter": [f"n{v}" for v in alter],
                       "weight": w, "layer": "L0"})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return read_from_edgelist(df, is_weighted=bool(weights))


def _fit(net, monkeypatch, on_device, **kw):
    from vimure_amd import VimureModel
    monkeypatch.setenv("VMR_DETERMINISTIC", "1")   # (before the fit creates its engine)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VimureModel()
        if on_device is None:
            m.fit(net.X, R=net.R, **kw)
        else:
            m.fit(net.X, R=net.R, init_on_device=on_device, **kw)
    return m


def _assert_fits_equal(a, b):
    cols = ["realisation", "seed", "iter", "elbo", "reached_convergence"]   # (not the wall-clock runtime column)
    assert a.trace[cols].equals(b.trace[cols])
    assert a.maxL == b.maxL
    assert np.array_equal(a.rho_f, b.rho_f)
    for k in SMALL:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.seed == b.seed


@pytest.mark.parametrize("weights,K", [(0, 2), (11, 12)])
def test_fit_is_bit_equal_to_the_host_draw(weights, K, monkeypatch):
    """K = 2 (the specialised kernels) and K = 12 from a count edgelist (the general kernels), three realisations: the producer
    thread walks the generator for realisation r + 1 while r sweeps."""
    net = _survey(160, 400, 9, weights)
    host = _fit(net, monkeypatch, None, K=K, seed=4, num_realisations=3, max_iter=60)
    dev = _fit(net, monkeypatch, True, K=K, seed=4, num_realisations=3, max_iter=60)
    assert host.pr_rho_drawn_on == "host" and dev.pr_rho_drawn_on == "device"
    assert host.K == dev.K == K and dev.trace["realisation"].nunique() == 3
    _assert_fits_equal(host, dev)
    one = _fit(net, monkeypatch, True, K=K, seed=4, num_realisations=1, max_iter=60)   # (the single-realisation path)
    ref = _fit(net, monkeypatch, False, K=K, seed=4, num_realisations=1, max_iter=60)
    assert ref.pr_rho_drawn_on == "host" and one.pr_rho_drawn_on == "device"
    _assert_fits_equal(ref, one)


def test_device_draw_needs_no_host_staging(monkeypatch):
    from vimure_amd import CaviEngine, VimureModel
    net = _survey(160, 400, 9, 0)
    L, N, M = (int(s) for s in (net.X.shape[0], net.X.shape[1], net.X.shape[3]))
    eng = CaviEngine.from_coo(net.X.subs, np.asarray(net.X.vals, np.int64), (L, N, N, M), R=net.R.subs, K=2, mutuality=True)

    def refuse(*a, **k):
        raise AssertionError("host staging used")
    monkeypatch.setattr(eng, "staging", refuse)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = VimureModel().fit(net.X, R=net.R, K=2, seed=2, num_realisations=2, max_iter=30, engine=eng, init_on_device=True)
        assert m.pr_rho_drawn_on == "device" and np.isfinite(m.maxL)
        with pytest.raises(AssertionError, match="host staging"):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                VimureModel().fit(net.X, R=net.R, K=2, seed=2, num_realisations=2, max_iter=30, engine=eng)
    finally:
        eng.close()


def test_both_modes_on_one_engine(monkeypatch):
    """Device-drawn and host-drawn fits alternate on one engine: the device slot of the draw and the host path's upload-ahead
    (pinned staging, its own copy stream: rho of 800 nodes is past the 8 MB pinning threshold) coexist; every fit is equal."""
    from vimure_amd import CaviEngine, VimureModel
    monkeypatch.setenv("VMR_DETERMINISTIC", "1")
    net = _survey(800, 200, 5, 0)
    L, N, M = (int(s) for s in (net.X.shape[0], net.X.shape[1], net.X.shape[3]))
    assert N * N * 2 * 8 >= (8 << 20)
    eng = CaviEngine.from_coo(net.X.subs, np.asarray(net.X.vals, np.int64), (L, N, N, M), R=net.R.subs, K=2, mutuality=True)
    fits = []
    try:
        for on_dev in (True, False, True):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                m = VimureModel().fit(net.X, R=net.R, K=2, seed=5, num_realisations=3, max_iter=30, engine=eng, init_on_device=on_dev)
            assert m.pr_rho_drawn_on == ("device" if on_dev else "host")
            fits.append(m)
        assert eng.can_upload_ahead()
    finally:
        eng.close()
    _assert_fits_equal(fits[0], fits[1])
    _assert_fits_equal(fits[0], fits[2])


def test_informative_prior_keeps_the_host_draw(monkeypatch):
    net = _survey(160, 400, 9, 11)
    L, N = net.X.shape[0], net.X.shape[1]
    g = np.random.RandomState(8)
    rho_prior = np.where(g.rand(L, N, N) < 0.05, g.rand(L, N, N) * 4, 0.0)
    host = _fit(net, monkeypatch, None, K=12, seed=3, num_realisations=2, max_iter=40, rho_prior=rho_prior)
    dev = _fit(net, monkeypatch, True, K=12, seed=3, num_realisations=2, max_iter=40, rho_prior=rho_prior)
    assert host.pr_rho_drawn_on == "host" and dev.pr_rho_drawn_on == "host"
    _assert_fits_equal(host, dev)


def test_invalid_descriptors_are_refused_before_any_launch():
    L, N, K = 1, 6, 3
    eng = _coo_engine(L, N, K, 0.5)
    lib = eng.lib
    try:
        cuts, keys, pos = _hostlib.mt_block_states(np.random.RandomState(1), L, N, K, 3)
        out = np.full((L, N, N, K), -7.0)

        def call(nblk, c, k, p):
            c = np.ascontiguousarray(c, np.int64)
            k = np.ascontiguousarray(k, np.uint32)
            p = np.ascontiguousarray(p, np.int32)
            return lib.vmr_draw_pr_rho(eng._h, nblk, c.ctypes.data, k.ctypes.data, p.ctypes.data, 0.0, 0, out.ctypes.data, 0)

        bad = [
            (0, cuts, keys, pos, "nblk"),
            (-2, cuts, keys, pos, "nblk"),
            (3, [0, 20, 20, 36], keys, pos, "increasing"),
            (3, [0, 25, 12, 36], keys, pos, "increasing"),
            (3, [0, 12, 24, 35], keys, pos, "span"),
            (3, [1, 12, 24, 36], keys, pos, "span"),
            (3, cuts, keys, [624, 625, 3], "position"),
            (3, cuts, keys, [-1, 5, 3], "position"),
        ]
        for nblk, c, k, p, msg in bad:
            assert call(nblk, c, k, p) == _lib.VMR_EINVAL, msg
            assert msg in lib.vmr_last_error(eng._h).decode()
            assert np.all(out == -7.0)   # nothing was launched or copied
        assert lib.vmr_draw_pr_rho(None, 3, cuts.ctypes.data, keys.ctypes.data, pos.ctypes.data, 0.0, 0, out.ctypes.data, 0) == _lib.VMR_EINVAL
        assert lib.vmr_draw_pr_rho(eng._h, 3, None, keys.ctypes.data, pos.ctypes.data, 0.0, 0, out.ctypes.data, 0) == _lib.VMR_EINVAL
        assert np.all(out == -7.0)
        with pytest.raises(ValueError, match="blocks"):
            eng.draw_pr_rho((cuts[:-1], keys, pos), 0.0, False, out=out)
        assert call(3, cuts, keys, pos) == _lib.VMR_OK   # (the handle is still usable)
        _, cov = eng.data_stats()
        assert np.array_equal(out, _numpy_prior(np.random.RandomState(1), L, N, K, 0.0, cov, False))
    finally:
        eng.close()
