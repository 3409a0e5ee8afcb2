"""GPU: connectivity of posterior samples on the device (vmr_sample_connectivity).  Every output is held, integer for integer, to
the scipy restatement (tests/connectivity_util.py) of the samples `CaviEngine.sample` returns for the same seeds: both data
layouts, the general kernels (K = 12, 16), a coordinate-list handle, every word and source-block boundary at the percolation
threshold, designed graphs with closed forms, several chunks, every optional output on its own, the argument errors, and the
model's method against `sample_inferred_model`."""
import warnings

import numpy as np
import pytest

from tests.connectivity_util import CONN_KEYS, NDIST, NODE_KEYS, check_designed, connectivity_np, designed_graphs
from tests.golden_util import case_config, load_case
from tests.test_hip_netstats import _engine_for, _golden_state, _random_state

pytestmark = pytest.mark.gpu

ALL_KEYS = CONN_KEYS + ("dist_hist",) + NODE_KEYS


def _assert_equal_conn(got, want, keys=ALL_KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


def _check_exact(eng, seed, S, trials=(1, 3)):
    """`sample_connectivity` against scipy on the samples of the same seeds; returns the last reference."""
    want = None
    for n_trials in trials:
        want = connectivity_np([eng.sample(seed + s, n_trials) for s in range(S)])
        got = eng.sample_connectivity(seed, S, n_trials=n_trials, nodes=True)
        assert sorted(got) == sorted(ALL_KEYS)
        _assert_equal_conn(got, want)
    return want


@pytest.mark.parametrize("case", ["A_ones_mut", "B_random_mask_K3", "D_self_mask", "E_undirected"])
def test_counts_equal_scipy_on_the_samples(case, vmr_format):
    d = load_case(case)
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        assert eng.data_format()[0] == vmr_format
        _check_exact(eng, 11, 8)
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["L_default_K12", "M_K16_nomut"])
def test_counts_equal_scipy_general_kernels(case):
    d = load_case(case)
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    assert K > 8
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        _check_exact(eng, 5, 8)
    finally:
        eng.close()


def test_counts_equal_scipy_coo_handle():
    d = load_case("D_self_mask")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d), coo=True)
    try:
        _check_exact(eng, 3, 8)
    finally:
        eng.close()


def _engine_with_rho(rho, seed, M=4):
    """An engine on random reports whose state holds the given rho [L, N, N, K]."""
    L, N, _, K = rho.shape
    g = np.random.RandomState(seed)
    X = (g.rand(L, N, N, M) < 0.1).astype(np.uint8)
    st = _random_state(g, L, N, M, K)
    return _engine_for(X, None, K, True, st[:6] + (rho,))


@pytest.mark.parametrize("N", [5, 63, 64, 65, 129])
def test_word_and_source_block_boundaries(N):
    """L = 2, K = 3 and W = ceil(N / 64) = 1, 1, 1, 2, 3 words per bit row and source blocks per layer; rho puts 1 - 1.5 / N on
    "no tie" and splits the rest: the percolation threshold, where components, reach and path lengths all vary.  These are the
    boundaries of the first three words only: one or two lanes per row, one node per thread.  The wider shapes -- 8, 16 and 32
    lanes, a second trip of the word stride, three to eight nodes per thread, the node bound -- are held in
    tests/test_hip_graph_shapes.py."""
    L, K, S = 2, 3, 8
    rho = np.empty((L, N, N, K))
    rho[..., 0] = 1.0 - 1.5 / N
    rho[..., 1:] = 0.75 / N
    eng = _engine_with_rho(rho, 100 + N)
    try:
        Ys = np.asarray([eng.sample(7 + s) for s in range(S)])
        assert Ys[:, :, np.arange(N), np.arange(N)].any()             # clearing the diagonal is exercised
        want = _check_exact(eng, 7, S, trials=(1,))
        if N >= 63:                                                    # the comparison cannot pass on trivial graphs
            assert (want["components_w"] >= 2).any() and (want["giant_s"] >= 2).any()
            assert (want["diameter"] >= 3).all()
            assert (want["reach_pairs"] > 0).all() and (want["reach_pairs"] < N * (N - 1)).all()
    finally:
        eng.close()


def test_designed_graphs():
    """One-hot rho, N = 129, L = 4, K = 2: every sample is the design whatever the seed -- the directed path (diameter 128, 2145
    pairs beyond the histogram's bins), the directed cycle, two cycles that fill the two source blocks beside a node with a
    self-loop, and the empty graph."""
    Y = designed_graphs()
    rho = np.stack([1.0 - Y, Y], axis=-1).astype(np.float64)
    eng = _engine_with_rho(rho, 3)
    try:
        for s in (40, 41):
            assert np.array_equal(eng.sample(s), Y)
        want = connectivity_np([Y, Y])
        check_designed(want)
        got = eng.sample_connectivity(40, 2, nodes=True)
        check_designed(got)
        _assert_equal_conn(got, want)
    finally:
        eng.close()


def test_medium_case_several_chunks(monkeypatch):
    """L = 2, N = 300, K = 3 on report lists, five words per bit row and five source blocks, S = 16: one chunk against chunks of
    5 samples (16 = 5 + 5 + 5 + 1), both against scipy; `sample_stats` and `sample_triads` of the same engine are what they were
    before the call."""
    from tests.test_hip_netstats import _medium
    g = np.random.RandomState(21)
    X, st = _medium(g)
    seed, S = 1000, 16
    monkeypatch.setenv("VMR_FORMAT", "sparse")
    monkeypatch.delenv("VMR_NETSTATS_CHUNK", raising=False)
    eng = _engine_for(X, None, 3, True, st)
    try:
        assert eng.data_format()[0] == "sparse"
        before = dict(eng.sample_stats(seed, S, degrees=True), **eng.sample_triads(seed, S, nodes=True))
        one = eng.sample_connectivity(seed, S, nodes=True)
        after = dict(eng.sample_stats(seed, S, degrees=True), **eng.sample_triads(seed, S, nodes=True))
        want = connectivity_np([eng.sample(seed + s) for s in range(S)])
    finally:
        eng.close()
    _assert_equal_conn(one, want)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    monkeypatch.setenv("VMR_NETSTATS_CHUNK", "5")
    eng = _engine_for(X, None, 3, True, st)
    try:
        many = eng.sample_connectivity(seed, S, nodes=True)
    finally:
        eng.close()
    _assert_equal_conn(many, one)


def test_optional_outputs():
    """counts alone, counts with the histogram, and counts with each node array alone (the raw call, the others NULL)."""
    from vimure_amd import _lib
    d = load_case("B_random_mask_K3")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        S = 4
        full = eng.sample_connectivity(9, S, nodes=True)
        plain = eng.sample_connectivity(9, S, hist=False)
        assert sorted(plain) == sorted(CONN_KEYS)
        _assert_equal_conn(plain, full, keys=CONN_KEYS)
        with_hist = eng.sample_connectivity(9, S)
        assert sorted(with_hist) == sorted(CONN_KEYS + ("dist_hist",))
        _assert_equal_conn(with_hist, full, keys=CONN_KEYS + ("dist_hist",))
        for q, k in enumerate(NODE_KEYS):
            counts = np.zeros((S, eng.L, _lib.CONN_NSTAT), np.uint64)
            arr = np.full((S, eng.L, eng.N), -1, np.int32)
            ptrs = [None] * len(NODE_KEYS)
            ptrs[q] = arr.ctypes.data
            assert eng.lib.vmr_sample_connectivity(eng._h, 9, S, 1, counts.ctypes.data, None, *ptrs) == _lib.VMR_OK
            assert np.array_equal(arr, full[k]), k
            for c, name in enumerate(_lib.CONN_NAMES):
                assert np.array_equal(counts[..., c].astype(np.int64), full[name]), (k, name)
    finally:
        eng.close()


def test_argument_errors_on_a_live_handle():
    from vimure_amd import _lib
    from vimure_amd.engine import ConnectivityArgumentError, EngineError
    d = load_case("A_ones_mut")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, None)
    try:
        with pytest.raises(EngineError, match="vmr_set_state") as ei:
            eng.sample_connectivity(1, 2)
        assert not isinstance(ei.value, ConnectivityArgumentError)
        counts = np.zeros((2, eng.L, _lib.CONN_NSTAT), np.uint64)
        nul = [None] * 7
        assert eng.lib.vmr_sample_connectivity(eng._h, 1, 2, 1, counts.ctypes.data, *nul) == _lib.VMR_ESTATE
        eng.set_state(*_golden_state(d))
        with pytest.raises(ConnectivityArgumentError, match="n_samples"):
            eng.sample_connectivity(1, 0)
        with pytest.raises(ConnectivityArgumentError, match="n_trials"):
            eng.sample_connectivity(1, 2, n_trials=0)
        assert eng.lib.vmr_sample_connectivity(eng._h, 1, 0, 1, counts.ctypes.data, *nul) == _lib.VMR_EINVAL
        assert b"n_samples" in eng.lib.vmr_last_error(eng._h)
        assert eng.lib.vmr_sample_connectivity(eng._h, 1, 2, 0, counts.ctypes.data, *nul) == _lib.VMR_EINVAL
        assert b"n_trials" in eng.lib.vmr_last_error(eng._h)
        assert eng.lib.vmr_sample_connectivity(eng._h, 1, 2, 1, None, *nul) == _lib.VMR_EINVAL
        assert b"counts" in eng.lib.vmr_last_error(eng._h)
        assert eng.sample_connectivity(1, 2)["components_w"].shape == (2, eng.L)   # the handle still works
    finally:
        eng.close()


def test_more_nodes_than_the_bound_are_refused():
    """A coordinate-list handle of VMR_CONN_NMAX + 1 nodes with a handful of entries and no state: refused for its N, not for
    its state."""
    from vimure_amd import CaviEngine, _lib
    from vimure_amd.engine import ConnectivityArgumentError
    N = _lib.CONN_NMAX + 1
    subs = tuple(np.array(a, np.int64) for a in ([0, 0, 0], [0, 5, N - 1], [1, N - 1, 0], [0, 1, 0]))
    eng = CaviEngine.from_coo(subs, np.array([1, 2, 1], np.int64), (1, N, N, 2), K=2)
    try:
        with pytest.raises(ConnectivityArgumentError, match=str(_lib.CONN_NMAX)):
            eng.sample_connectivity(1, 2)
        counts = np.zeros((2, 1, _lib.CONN_NSTAT), np.uint64)
        assert eng.lib.vmr_sample_connectivity(eng._h, 1, 2, 1, counts.ctypes.data, *[None] * 7) == _lib.VMR_EINVAL
        assert b"N <= %d" % _lib.CONN_NMAX in eng.lib.vmr_last_error(eng._h)
    finally:
        eng.close()


def test_model_posterior_connectivity():
    from vimure_amd import VimureModel
    from vimure_amd.synthetic import standard_sbm
    net = standard_sbm(N=60, M=8, L=1, K=2, avg_degree=6.0, eta=0.4, seed=4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VimureModel(mutuality=True)
        m.fit(net.X, K=2, seed=1, max_iter=30, num_realisations=1, keep_engine=True)
    try:
        S, sd = 8, 321
        res = m.posterior_connectivity(n_samples=S, seed=sd, nodes=True)
        assert m._rho_f is None                                           # rho has not crossed PCIe
        Ys = [m.sample_inferred_model(N=1, seed=sd + s, device=True)[0] for s in range(S)]
        want = connectivity_np(Ys)
        assert want["reach_pairs"].min() > 0
        for k in ALL_KEYS:
            assert np.array_equal(getattr(res, k), want[k]), k
        with np.errstate(divide="ignore", invalid="ignore"):
            assert np.array_equal(res.avg_path_length, want["dist_sum"] / want["reach_pairs"].astype(float), equal_nan=True)
        assert np.array_equal(res.connectedness, want["pairs_w"] / float(m.N * (m.N - 1)))
        assert res.closeness_out.shape == (S, m.L, m.N) and res.global_efficiency.shape == (S, m.L)
        assert np.array_equal(res.same_component(0, 1), (want["node_comp_w"][:, :, 0] == want["node_comp_w"][:, :, 1]).mean(axis=0))
        assert len(res.summary()) == m.L * len(res.statistics())
        assert set(CONN_KEYS) <= set(res.summary()["statistic"])
        plain = m.posterior_connectivity(n_samples=S, seed=sd)
        assert plain.node_comp_w is None and np.array_equal(plain.dist_hist, want["dist_hist"])
        # the dyad read-out is what it was
        base = m.posterior_network_stats(n_samples=S, seed=sd)
        assert tuple(base.statistics()) == ("edges", "weight", "mutual", "reciprocity", "density")
    finally:
        m.close()
