"""GPU: triad statistics of posterior samples and their expectations on the device (vmr_sample_triads, vmr_expected_triads).
Every count is held, integer for integer, to the NumPy restatement (tests/triads_util.py) of the samples `CaviEngine.sample`
returns for the same seeds: both data layouts, the general kernels (K = 12, 16), a coordinate-list handle, every word boundary of
the bit rows, several chunks; the expectations to NumPy on the rho read back; sampling to its expectation; the model's method to
`sample_inferred_model`."""
import warnings

import numpy as np
import pytest

from tests.golden_util import case_config, load_case
from tests.netstats_util import stats_np
from tests.test_hip_netstats import _engine_for, _golden_state, _random_state
from tests.triads_util import TRIAD_KEYS, expected_triads_np, triads_np

pytestmark = pytest.mark.gpu

NODE_KEYS = ("node_tri", "node_deg")


def _assert_equal_triads(got, want, keys=TRIAD_KEYS + NODE_KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


def _check_exact(eng, seed, S, trials=(1, 3)):
    """`sample_triads` against NumPy on the samples of the same seeds; returns the last reference."""
    want = None
    for n_trials in trials:
        want = triads_np([eng.sample(seed + s, n_trials) for s in range(S)])
        _assert_equal_triads(eng.sample_triads(seed, S, n_trials=n_trials, nodes=True), want)
    return want


@pytest.mark.parametrize("case", ["A_ones_mut", "B_random_mask_K3", "D_self_mask", "E_undirected"])
def test_counts_equal_numpy_on_the_samples(case, vmr_format):
    d = load_case(case)
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        assert eng.data_format()[0] == vmr_format
        _check_exact(eng, 11, 8)
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["L_default_K12", "M_K16_nomut"])
def test_counts_equal_numpy_general_kernels(case):
    d = load_case(case)
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    assert K > 8
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        _check_exact(eng, 5, 8)
    finally:
        eng.close()


def test_counts_equal_numpy_coo_handle():
    d = load_case("D_self_mask")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d), coo=True)
    try:
        _check_exact(eng, 3, 8)
    finally:
        eng.close()


def _random_engine(N, seed, L=2, M=4, K=3):
    g = np.random.RandomState(seed)
    X = (g.rand(L, N, N, M) < 0.1).astype(np.uint8)
    return _engine_for(X, None, K, True, _random_state(g, L, N, M, K, sparse_p=True))


@pytest.mark.parametrize("N", [5, 63, 64, 65, 129])
def test_word_boundaries(N):
    """L = 2, K = 3 and W = ceil(N / 64) = 1, 1, 1, 2, 3 words per bit row: one partial word, one short of a word, an exact
    word, one spare bit, a third word holding one bit.  The samples of a random state carry edges on their diagonal.  These are
    the boundaries of the first three words only: the register path with one and two words, two lanes striding three.  The
    register path with 4 to 32 words, 8 to 64 lanes with a second trip, more than one block of 32 words and the second trip of
    the degree loop are held in tests/test_hip_graph_shapes.py."""
    eng = _random_engine(N, 100 + N)
    try:
        Ys = np.asarray([eng.sample(7 + s) for s in range(8)])
        assert all(Ys[:, l, np.arange(N), np.arange(N)].any() for l in range(2))   # clearing the diagonal is exercised
        want = _check_exact(eng, 7, 8, trials=(1,))
        if N >= 63:
            assert want["triangles_u"].min() > 0 and want["cyclic"].min() > 0    # the comparison cannot pass on zeros
            assert want["transitive"].min() > 0 and want["node_tri"].max() > 0
    finally:
        eng.close()


def test_medium_case_several_chunks(monkeypatch):
    """L = 2, N = 300, K = 3 on report lists (a non-trivial perm), five words per bit row (the last one partial), S = 16: one
    chunk against chunks of 5 samples (16 = 5 + 5 + 5 + 1), both against NumPy; the counts without the node arrays; and
    `sample_stats` of the same engine is what it was before the call."""
    from tests.test_hip_netstats import _medium
    g = np.random.RandomState(21)
    X, st = _medium(g)
    seed, S = 1000, 16
    monkeypatch.setenv("VMR_FORMAT", "sparse")
    monkeypatch.delenv("VMR_NETSTATS_CHUNK", raising=False)
    eng = _engine_for(X, None, 3, True, st)
    try:
        assert eng.data_format()[0] == "sparse"
        before = eng.sample_stats(seed, S, degrees=True)
        one = eng.sample_triads(seed, S, nodes=True)
        plain = eng.sample_triads(seed, S)
        after = eng.sample_stats(seed, S, degrees=True)
        want = triads_np([eng.sample(seed + s) for s in range(S)])
    finally:
        eng.close()
    _assert_equal_triads(one, want)
    assert sorted(plain) == sorted(TRIAD_KEYS)
    _assert_equal_triads(plain, want, keys=TRIAD_KEYS)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    monkeypatch.setenv("VMR_NETSTATS_CHUNK", "5")
    eng = _engine_for(X, None, 3, True, st)
    try:
        many = eng.sample_triads(seed, S, nodes=True)
    finally:
        eng.close()
    _assert_equal_triads(many, one)


def _check_expected(eng, N):
    got, again = eng.expected_triads(), eng.expected_triads()
    want = expected_triads_np(eng.get_state()["rho"])
    # every term of every sum is non-negative: any summation order of n terms is within (n + 2) 2^-53 relative; one such
    # bound for the device and one for NumPy
    rtol = 2 * (N ** 3 + 3) * 2.0 ** -53
    for k in TRIAD_KEYS:
        assert got[k].shape == (eng.L,) and got[k].dtype == np.float64, k
        assert np.array_equal(got[k].view(np.uint64), again[k].view(np.uint64)), k
        assert (want[k] > 0).all(), k
        print(k, got[k], want[k], np.abs(got[k] - want[k]) / want[k], rtol)
        np.testing.assert_allclose(got[k], want[k], rtol=rtol, atol=0, err_msg=k)


@pytest.mark.parametrize("N", [5, 65, 129])
def test_expected_triads_against_numpy(N):
    eng = _random_engine(N, 200 + N)
    try:
        _check_expected(eng, N)
    finally:
        eng.close()


def test_expected_triads_on_golden_state():
    d = load_case("B_random_mask_K3")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        _check_expected(eng, d["X"].shape[1])
    finally:
        eng.close()


def test_sampling_agrees_with_expectation():
    """N = 129, S = 256: the mean of each count over the samples lies within 5 standard errors of its expectation; the standard
    error is that of the NumPy counts of the same samples."""
    S, seed = 256, 4242
    eng = _random_engine(129, 329)
    try:
        got = eng.sample_triads(seed, S)
        exp = eng.expected_triads()
        ref = triads_np([eng.sample(seed + s) for s in range(S)])
    finally:
        eng.close()
    for k in TRIAD_KEYS:
        for l in range(2):
            se = ref[k][:, l].std(ddof=1) / np.sqrt(S)
            assert se > 0
            assert abs(got[k][:, l].mean() - exp[k][l]) <= 5.0 * se, (k, l, got[k][:, l].mean(), exp[k][l], se)


def test_argument_errors_on_a_live_handle():
    from vimure_amd import _lib
    from vimure_amd.engine import EngineError
    d = load_case("A_ones_mut")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, None)
    try:
        with pytest.raises(EngineError, match="vmr_set_state"):
            eng.sample_triads(1, 2)
        with pytest.raises(EngineError, match="vmr_set_state"):
            eng.expected_triads()
        counts = np.zeros((2, eng.L, _lib.TRIAD_NSTAT), np.uint64)
        assert eng.lib.vmr_sample_triads(eng._h, 1, 2, 1, counts.ctypes.data, None, None) == _lib.VMR_ESTATE
        assert eng.lib.vmr_expected_triads(eng._h, np.zeros((eng.L, 6)).ctypes.data) == _lib.VMR_ESTATE
        eng.set_state(*_golden_state(d))
        with pytest.raises(EngineError, match="n_samples"):
            eng.sample_triads(1, 0)
        with pytest.raises(EngineError, match="n_trials"):
            eng.sample_triads(1, 2, n_trials=0)
        assert eng.lib.vmr_sample_triads(eng._h, 1, 0, 1, counts.ctypes.data, None, None) == _lib.VMR_EINVAL
        assert eng.lib.vmr_sample_triads(eng._h, 1, 2, 0, counts.ctypes.data, None, None) == _lib.VMR_EINVAL
        assert eng.lib.vmr_sample_triads(eng._h, 1, 2, 1, None, None, None) == _lib.VMR_EINVAL
        assert b"counts" in eng.lib.vmr_last_error(eng._h)
        assert eng.lib.vmr_expected_triads(eng._h, None) == _lib.VMR_EINVAL
        assert eng.sample_triads(1, 2)["transitive"].shape == (2, eng.L)   # the handle still works
    finally:
        eng.close()


def test_model_posterior_network_stats_with_triads():
    from vimure_amd import VimureModel
    from vimure_amd.synthetic import standard_sbm
    net = standard_sbm(N=60, M=8, L=1, K=2, avg_degree=6.0, eta=0.4, seed=4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VimureModel(mutuality=True)
        m.fit(net.X, K=2, seed=1, max_iter=30, num_realisations=1, keep_engine=True)
    try:
        S, sd = 8, 321
        res = m.posterior_network_stats(n_samples=S, seed=sd, triads=True, local_clustering=True)
        assert m._rho_f is None                                           # rho has not crossed PCIe
        Ys = [m.sample_inferred_model(N=1, seed=sd + s, device=True)[0] for s in range(S)]
        want = triads_np(Ys)
        assert want["two_paths"].min() > 0
        for k in TRIAD_KEYS + NODE_KEYS:
            assert np.array_equal(getattr(res, k), want[k]), k
        with np.errstate(divide="ignore", invalid="ignore"):
            assert np.array_equal(res.transitivity_directed, want["transitive"] / want["two_paths"].astype(float), equal_nan=True)
            assert np.array_equal(res.cyclicity, want["cyclic"] / want["two_paths"].astype(float), equal_nan=True)
            wd = want["wedges_u"].astype(float)
            assert np.array_equal(res.transitivity, np.where(wd > 0, 3 * want["triangles_u"] / wd, np.nan), equal_nan=True)
            dg = want["node_deg"].astype(np.int64)
            cl = np.where(dg >= 2, 2.0 * want["node_tri"] / (dg * (dg - 1)), np.nan)
        assert res.local_clustering.shape == (S, m.L, m.N)
        assert np.array_equal(res.local_clustering, cl, equal_nan=True)
        for s in range(S):
            for l in range(m.L):
                v = cl[s, l][~np.isnan(cl[s, l])]
                assert v.size and np.isclose(res.avg_clustering[s, l], v.mean(), rtol=1e-14, atol=0)
        exp = m._engine.expected_triads()
        for k in TRIAD_KEYS:
            assert np.array_equal(res.expected["exp_" + k], exp[k]), k
        names = set(res.summary()["statistic"])
        assert set(TRIAD_KEYS) | {"transitivity_directed", "cyclicity", "transitivity", "avg_clustering"} <= names
        assert len(res.summary()) == m.L * len(res.statistics())
        # without the new keywords: the keys and the values of the dyad statistics alone, as before
        base = m.posterior_network_stats(n_samples=S, seed=sd)
        assert tuple(base.statistics()) == ("edges", "weight", "mutual", "reciprocity", "density")
        assert tuple(base.expected) == ("edges", "weight", "mutual", "edges_var", "expected_reciprocity")
        dy = stats_np(Ys)
        for k in ("edges", "weight", "mutual"):
            assert np.array_equal(getattr(base, k), dy[k]) and np.array_equal(getattr(res, k), dy[k]), k
        assert np.array_equal(base.reciprocity, dy["mutual"] / dy["weight"].astype(float))
        assert base.deg_out is None and base.f1 is None
        assert set(base.summary()["statistic"]) == {"edges", "weight", "mutual", "reciprocity", "density"}
    finally:
        m.close()
